"""Inputs of tests/test_gpu_kept_only.py: calls that ask for the kept mask alone (want_root = False), where
the batched directional collapse leaves the union-find forest unflattened and follows only the endpoints
of the one-way pairs to their roots.  Each Batch holds its arrays and the oracle's answer (computed once,
read-only); tests/test_kept_only_inputs_cpu.py checks on the CPU that every input has the structure its
test is about.

Plain Python / numpy over chain_inputs, helpers and the oracle."""
import functools

import numpy as np

import chain_inputs as ci
import oracle as orc
from helpers import canonical, random_bucket


class Batch:
    """One call: buckets [(umis, freq)] in rank order, keys of one word (form "one") or several ("wide")."""

    def __init__(self, form, L, k, p, buckets):
        self.form, self.L, self.k, self.p = form, L, k, p
        self.is_chain = [len(b) > 2 and b[2] for b in buckets]  # (everything falls to a chain's rank 0)
        self.buckets = buckets = [tuple(b[:2]) for b in buckets]
        self.umis, self.fr, self.off = ci.assemble(buckets)
        self.keys, self.nm = (orc.encode_keys if form == "one" else orc.encode_keys_wide)(self.umis)
        assert not self.nm.any()
        self._ref = None

    def reference(self):
        """The oracle's kept mask."""
        if self._ref is None:
            run = orc.dedup_batch if self.form == "one" else orc.dedup_batch_wide
            okept, _, _ = run(self.keys, None, self.fr, self.off, self.L, self.k, self.p)
            okept = np.asarray(okept).astype(np.uint8)
            okept.setflags(write=False)
            self._ref = okept
        return self._ref

    def sizes(self):
        return np.diff(self.off.astype(np.int64)).tolist()

    def run(self, ctx, want_root):
        run = ctx.dedup_batch if self.form == "one" else ctx.dedup_batch_wide
        return run(self.keys, None, self.fr, self.off, self.L, self.k, self.p, want_root=want_root)


def randoms(seed, L, sizes=(25, 10, 35)):
    """Small random buckets (molecule model) to stand between the chains."""
    rng = np.random.default_rng(61000 + seed)
    return [canonical(*random_bucket(rng, n_mol, L, err=0.06))[:2] for n_mol in sizes]


def interleave(chains, rnd):
    """chain, random, chain, random, ...: (umis, freq, is a chain) per bucket"""
    out, rnd = [], list(rnd)
    for c in chains:
        out.append((c.umis, c.freq, True))
        if rnd:
            out.append(rnd.pop(0) + (False,))
    return out + [b + (False,) for b in rnd]


SYM4 = [("sym", o) for o in ci.ORDERS]
HALF = SYM4 + [("halving", "forward")]                                        # p = 0.5
ONE = [("step2", "forward"), ("comb", "forward"), ("sym", "zigzag")]          # p = 1.0
PATHS = [(21, 1), (8, 1), (21, 4)]  # 64, 25 and 16 nodes


@functools.lru_cache(maxsize=None)
def chain_batches(L, stride, form="one"):
    """The two calls of one path: sym in four orders and halving at p = 0.5; step2, comb and sym zig-zag at
    p = 1.0.  The reverse and zig-zag orders make the union-find trees deep (read-only climbs of up to
    n - 1 hops); comb is sets of two chained by one-way pairs; step2 is n - 1 one-way pairs in a row."""
    half = [ci.chain(lad, L, stride, o) for lad, o in HALF]
    one = [ci.chain(lad, L, stride, o) for lad, o in ONE]
    return (Batch(form, L, stride, 0.5, interleave(half, randoms(L + stride, L))),
            Batch(form, L, stride, 1.0, interleave(one, randoms(100 + L + stride, L))))


SELF_EDGE_TAIL = "CGTACGTTGCA"
SELF_EDGE_TRIO = ["A" + SELF_EDGE_TAIL, "C" + SELF_EDGE_TAIL, "G" + SELF_EDGE_TAIL]


@functools.lru_cache(maxsize=None)
def self_edge_batch():
    """Three UMIs that differ in one position, freq 3, 2, 1, p = 1.0 (thr(f) = f + 1): 3 ~ 2 and 2 ~ 1 are
    permitted both ways, 3 -> 1 one way only -- a one-way pair inside one symmetric set, which resolves to
    (root, root).  In one bucket with 20 random entries."""
    rng = np.random.default_rng(62001)
    umis, freq = list(SELF_EDGE_TRIO), [3, 2, 1]
    while len(umis) < 23:
        u = rng.choice(np.frombuffer(b"ACGT", np.uint8), 12).tobytes().decode()
        if u not in umis:
            umis.append(u)
            freq.append(int(rng.integers(1, 6)))
    return Batch("one", 12, 1, 1.0, [canonical(umis, freq)[:2]])


MIXED_MOLECULES = (30, 12, 40, 115, 260)  # three fused buckets, one for the chunk kernel, one for the segment index


@functools.lru_cache(maxsize=None)
def mixed_batch():
    """Default options: buckets of at most 128 entries (the fused kernel's: the collapse gets ranges), one
    of 129..511 (the chunk kernel: flagged and plain pairs appended to the list, united by the list's union
    pass) and one of 512 or more (the segment index: one-way pairs in private slots, moved to the list)."""
    rng = np.random.default_rng(62002)
    return Batch("one", 12, 1, 0.5, [canonical(*random_bucket(rng, n_mol, 12, err=0.05))[:2]
                                     for n_mol in MIXED_MOLECULES])


@functools.lru_cache(maxsize=None)
def overflow_batch():
    """40 buckets of the 64-node step2 ladder: about 2,500 one-way pairs against the list's floor of 1,024."""
    ch = ci.chain("step2", 21, 1)
    return Batch("one", 21, 1, 1.0, interleave([ch] * 40, randoms(700, 21, sizes=(30, 12))))
