"""Inputs of tests/test_gpu_seg_probe.py: k = 1 calls whose segment-index sub-buckets are decided by bitmap
lookups (options seg_probe / seg_probe_min) or, where part 0 leaves more than six bases outside its bins,
by the tile walk.  Each Batch holds its arrays and the oracle's answer per percentage (computed
once, read-only); tests/test_seg_probe_inputs_cpu.py checks on the CPU that every input has the geometry
its test is about.

Plain Python / numpy over helpers and the oracle."""
import functools

import numpy as np

import oracle as orc
from helpers import canonical, random_bucket

SEG_MIN = 512        # buckets from this many entries up go through the segment index
PROBE_MAX_REST = 6   # most bases outside a part's bins that the lookups take


def geometry(n, L, k=1):
    """[(first base, bases that index the bins, bases outside the bins)] of the k + 1 parts of a bucket
    of n entries, as plan_segment cuts it."""
    P = k + 1
    nb_cap = max(2, min(12, (int(n).bit_length() - 1 - 4) // 2))
    out = []
    for j in range(P):
        b0, b1 = j * L // P, (j + 1) * L // P
        nb = min(b1 - b0, nb_cap)
        out.append((b0, nb, L - nb))
    return out


class Batch:
    """One call of one-word keys: buckets [(umis, freq)] in rank order."""

    def __init__(self, L, buckets, with_n=False):
        self.L = L
        self.buckets = buckets
        self.umis = [u for b in buckets for u in b[0]]
        self.fr = np.array([f for b in buckets for f in b[1]], np.int32)
        self.off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
        self.keys, self.nm = orc.encode_keys(self.umis)
        assert with_n == bool(self.nm.any())
        self.nmask = self.nm if with_n else None
        self._ref = {}

    def sizes(self):
        return [len(b[0]) for b in self.buckets]

    def reference(self, p):
        """The oracle's (kept, root) at k = 1."""
        if p not in self._ref:
            okept, oroot, _ = orc.dedup_batch(self.keys, self.nm, self.fr, self.off, self.L, 1, p, 0, 0)
            okept, oroot = np.asarray(okept).copy(), np.asarray(oroot).copy()
            okept.setflags(write=False)
            oroot.setflags(write=False)
            self._ref[p] = (okept, oroot)
        return self._ref[p]


def unique_bucket(rng, n_raw, L, n_frac=0.0):
    """The distinct UMIs among n_raw uniform ones, geometric freqs capped at 40 (one-way and symmetric pairs
    both occur), in rank order."""
    raw = rng.integers(0, 4, (n_raw, L))
    if n_frac:
        raw = np.where(rng.random(raw.shape) < n_frac, 4, raw)
    umis = sorted({"".join("ACGTN"[c] for c in r) for r in raw})
    rng.shuffle(umis)
    freq = np.minimum(rng.geometric(0.5, len(umis)), 40).tolist()
    return canonical(umis, freq)[:2]


def small_buckets(rng, L, sizes=(20, 35, 12)):
    """Buckets of the fused kernel's size (molecule model)."""
    return [canonical(*random_bucket(rng, n_mol, L, err=0.05))[:2] for n_mol in sizes]


@functools.lru_cache(maxsize=None)
def first_eligible():
    """L = 8, one bucket of ~600: two bases per bin, six outside -- the first bucket the segment index takes."""
    return Batch(8, [unique_bucket(np.random.default_rng(7101), 620, 8)])


@functools.lru_cache(maxsize=None)
def dense():
    """L = 6, ~2,000 of the 4,096 possible UMIs: about nine partners per entry, one giant component."""
    return Batch(6, [unique_bucket(np.random.default_rng(7102), 2745, 6)])


@functools.lru_cache(maxsize=None)
def uneven(n_raw=3300):
    """L = 7: parts of 3 and 4 bases; part 1's bins are indexed by fewer bases than the part has (3,300 raw:
    ~3,000 unique, three bases per bin in both parts; 6,000 raw: ~5,000 unique, three and four)."""
    return Batch(7, [unique_bucket(np.random.default_rng(7103 + n_raw), n_raw, 7)])


@functools.lru_cache(maxsize=None)
def mixed():
    """L = 9: buckets of ~600 and ~900 (seven bases outside the bins: tiles) and of ~5,000 and ~20,000 (five
    or four: lookups) in one call, fused-size buckets in between."""
    rng = np.random.default_rng(7104)
    small = small_buckets(rng, 9)
    buckets = []
    for n_raw in (610, 5050, 915, 20800):
        buckets.append(unique_bucket(rng, n_raw, 9))
        if small:
            buckets.append(small.pop())
    return Batch(9, buckets)


@functools.lru_cache(maxsize=None)
def deep(L):
    """~70,000 unique UMIs in one bucket: six bases per bin -- at L = 12 six outside (the geometry of a
    position of a million reads, at the smallest n that has it), at L = 13 seven (tiles)."""
    return Batch(L, [unique_bucket(np.random.default_rng(7105), 70000, L)])


@functools.lru_cache(maxsize=None)
def duplicated():
    """The L = 8 bucket with one key there twice and another three times, in rank order: legal input (the
    contract asks for rank order and freq >= 1), and two entries of one bin with the same bases outside it."""
    umis, freq = first_eligible().buckets[0]
    umis, freq = list(umis), list(freq)
    n = len(umis)
    extra = [(umis[n // 3], 2), (umis[n // 2], 1), (umis[n // 2], 1)]
    if freq[0] > 1:
        extra[0] = (umis[n // 3], freq[0])
    umis += [u for u, _ in extra]
    freq += [f for _, f in extra]
    return Batch(8, [canonical(umis, freq)[:2]])


@functools.lru_cache(maxsize=None)
def with_n():
    """The L = 8 shape with 0.5 % N bases and an N mask: not taken by lookups."""
    return Batch(8, [unique_bucket(np.random.default_rng(7101), 620, 8, n_frac=0.005)], with_n=True)
