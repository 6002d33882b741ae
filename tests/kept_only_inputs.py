"""Inputs of tests/test_gpu_kept_only.py and tests/test_gpu_kept_only_matrix.py: calls that ask for the
kept mask alone (want_root = False), where the batched directional collapse leaves the union-find forest
unflattened and follows only the endpoints of the one-way pairs to their roots.  Each Batch holds its
arrays and the oracle's answer (computed once, read-only); tests/test_kept_only_inputs_cpu.py checks on
the CPU that every input has the structure its test is about.

Plain Python / numpy over chain_inputs, helpers and the oracle."""
import functools

import numpy as np

import chain_inputs as ci
import edit_model as em
import oracle as orc
import seq_model as sm
from helpers import canonical, clustered_bucket, random_bucket, seq_buckets


class Batch:
    """One call: buckets [(umis, freq)] in rank order, keys of one word (form "one") or several ("wide").
    with_n: the UMIs may hold N bases, and the N masks go to the oracle and to the library (where there is one)."""

    def __init__(self, form, L, k, p, buckets, with_n=False):
        self.form, self.L, self.k, self.p = form, L, k, p
        self.is_chain = [len(b) > 2 and b[2] for b in buckets]  # (everything falls to a chain's rank 0)
        self.buckets = buckets = [tuple(b[:2]) for b in buckets]
        self.umis, self.fr, self.off = ci.assemble(buckets)
        self.keys, self.nm = (orc.encode_keys if form == "one" else orc.encode_keys_wide)(self.umis)
        assert with_n or not self.nm.any()
        self.nmask = self.nm if with_n and self.nm.any() else None
        self._ref = {}

    def reference(self, algo=0, amf=0):
        """The oracle's kept mask."""
        if (algo, amf) not in self._ref:
            run = orc.dedup_batch if self.form == "one" else orc.dedup_batch_wide
            okept, _, _ = run(self.keys, self.nmask, self.fr, self.off, self.L, self.k, self.p, algo, amf)
            okept = np.asarray(okept).astype(np.uint8)
            okept.setflags(write=False)
            self._ref[(algo, amf)] = okept
        return self._ref[(algo, amf)]

    def sizes(self):
        return np.diff(self.off.astype(np.int64)).tolist()

    def run(self, ctx, want_root, algo=0, amf=0):
        run = ctx.dedup_batch if self.form == "one" else ctx.dedup_batch_wide
        return run(self.keys, self.nmask, self.fr, self.off, self.L, self.k, self.p, algo, amf, want_root=want_root)


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


# ---- tests/test_gpu_kept_only_matrix.py ------------------------------------------------------------------

N_SIZES = (40, 300, 600)  # the fused kernel, the chunk kernel (129..511), the segment index (512 or more)
N_FRACS = (0.02, 0.2)


@functools.lru_cache(maxsize=None)
def n_buckets(n_frac):
    rng = np.random.default_rng(63000 + int(1000 * n_frac))
    return tuple(clustered_bucket(rng, n, 12, n_frac) for n in N_SIZES)


@functools.lru_cache(maxsize=None)
def n_batch(n_frac, k, p):
    """12-base UMIs of which a share n_frac carries an N, one bucket per size class."""
    return Batch("one", 12, k, p, list(n_buckets(n_frac)), with_n=True)


FUZZ_SEEDS = tuple(range(12))
FUZZ_SIZES = (0, 1, 2, 63, 64, 65, 128, 129, 300, 511, 512, 513, 1024, 1025, 2000)


@functools.lru_cache(maxsize=None)
def fuzz_batch(seed):
    """The generator of tests/test_gpu_fuzz.py, directional only, over the sizes around every kernel boundary."""
    rng = np.random.default_rng(64000 + seed)
    L = int(rng.choice([6, 9, 12, 13, 17, 21]))
    k = int(rng.choice([0, 1, 2, 3, 4, 5]))
    p = float(rng.choice([0.0, 0.3, 0.5, 0.75, 1.0]))
    n_frac = float(rng.choice([0.0, 0.02]))
    sizes = [int(x) for x in rng.choice(FUZZ_SIZES, size=int(rng.integers(3, 7)))]
    cap = 4 ** L // 2
    buckets = [clustered_bucket(rng, min(n, cap), L, n_frac) if n else ([], []) for n in sizes]
    return Batch("one", L, k, p, buckets, with_n=True)


class EditBatch:
    """A call of dedup_batch_edit over the buckets of edit_model.batch / same_composition_bucket; the reference
    is edit_model.model_batch."""

    def __init__(self, L, buckets, mats, packed, with_n):
        self.L, self.buckets, self.mats = L, buckets, mats
        self.keys, self.nm, self.fr, self.off = packed
        self.nmask = self.nm if with_n else None
        self._ref = {}

    def reference(self, k, p):
        if (k, p) not in self._ref:
            ekept, _ = em.model_batch(self.buckets, k, p, mats=self.mats)
            ekept.setflags(write=False)
            self._ref[(k, p)] = ekept
        return self._ref[(k, p)]

    def run(self, ctx, want_root, k, p):
        return ctx.dedup_batch_edit(self.keys, self.nmask, self.fr, self.off, self.L, k=k, percentage=p,
                                    want_root=want_root)


EDIT_INPUTS = ((12, 0.05), (21, 0.0))


@functools.lru_cache(maxsize=None)
def edit_batch(L, n_frac):
    buckets, mats, packed = em.batch(L, n_frac)
    return EditBatch(L, buckets, mats, packed, bool(n_frac))


@functools.lru_cache(maxsize=None)
def edit_dense_batch():
    """600 arrangements of one multiset of letters: every pair passes the count filter."""
    umis, freq = em.same_composition_bucket(12, 600)
    return EditBatch(12, [(umis, freq)], [em.edit_matrix(umis)], em.pack([(umis, freq)]), False)


class SeqBatch:
    """A call of dedup_seqs: buckets [(reads as bytes, freq)] in rank order, one length per bucket; the reference
    is seq_model.dedup."""

    def __init__(self, k, p, buckets):
        self.k, self.p, self.buckets = k, p, buckets
        self.blen = [len(b[0][0]) for b in buckets]
        w = max(sm.words(x) for x in self.blen)
        enc = [sm.encode(list(b[0]), w) for b in buckets]
        self.keys = np.concatenate([e[0] for e in enc])
        self.nm = np.concatenate([e[1] for e in enc])
        self.fr = np.array([f for b in buckets for f in b[1]], np.int32)
        self.off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
        self._ref = None

    def reference(self):
        if self._ref is None:
            ent = [(s, int(f), 0) for b in self.buckets for s, f in zip(*b)]
            kept, _ = sm.dedup(ent, [int(x) for x in self.off], self.blen, self.k, 0, self.p)
            kept = kept.astype(np.uint8)
            kept.setflags(write=False)
            self._ref = kept
        return self._ref

    def run(self, ctx, want_root):
        return ctx.dedup_seqs(self.keys, self.nm, self.fr, self.off, self.blen, k=self.k, percentage=self.p,
                              want_root=want_root)


SEQ_LENGTHS = (30, 100)


@functools.lru_cache(maxsize=None)
def seq_batch(k):
    """Reads of 30 and of 100 bases in one call: per length a pair, a bucket below 512 entries and one above."""
    return SeqBatch(k, 0.5, [b for L in SEQ_LENGTHS for b in seq_buckets(L, k, sizes=(2, 200, 600))])


DEEP_L = 256  # 769 nodes: the whole-read paths of tests/test_gpu_deep_chains.py


@functools.lru_cache(maxsize=None)
def deep_batch(which):
    """"sym": the all-symmetric path in reverse and in zig-zag order at p = 0.5 (the reverse order leaves a
    union-find tree n - 1 deep); "step2": 768 one-way pairs in a row at p = 1.0."""
    if which == "sym":
        chains, p = [ci.chain("sym", DEEP_L, 1, o) for o in ("reverse", "zigzag")], 0.5
    else:
        chains, p = [ci.chain("step2", DEEP_L, 1)], 1.0
    return SeqBatch(1, p, [([u.encode() for u in c.umis], c.freq) for c in chains])


GIANT_N = 20000


@functools.lru_cache(maxsize=None)
def giant_batch():
    """The benchmark's one-position shape at small size: 20,000 distinct uniform 8-base UMIs out of 65,536,
    geometric freq (three in four are 1) in rank order.  At k = 1 and p = 0.5 the freq-1 entries are joined
    by symmetric pairs into one set that holds most of them, and every entry of freq 2 or more sends one-way
    pairs into it."""
    rng = np.random.default_rng(65001)
    codes = rng.choice(4 ** 8, GIANT_N, replace=False)
    freq = np.sort(rng.geometric(0.75, GIANT_N))[::-1]
    umis = ["".join("ACGT"[(int(c) >> (2 * i)) & 3] for i in range(8)) for c in codes]
    return Batch("one", 8, 1, 0.5, [(umis, freq.tolist())])


@functools.lru_cache(maxsize=None)
def mixed_n_batch():
    """The buckets of mixed_batch and one of 300 entries of which a fifth carries an N."""
    rng = np.random.default_rng(62003)
    return Batch("one", 12, 1, 0.5, list(mixed_batch().buckets) + [clustered_bucket(rng, 300, 12, 0.2)], with_n=True)


@functools.lru_cache(maxsize=None)
def step2_batch():
    """The 64-node step2 ladder alone: 63 one-way pairs in a row."""
    ch = ci.chain("step2", 21, 1)
    return Batch("one", 21, 1, 1.0, [(ch.umis, ch.freq, True)])


@functools.lru_cache(maxsize=None)
def small_batch():
    """One bucket of 300 entries."""
    rng = np.random.default_rng(62004)
    return Batch("one", 12, 1, 0.5, [clustered_bucket(rng, 300, 12, 0.0)])


EXTENT_SIZES = (0, 1, 2, 3, 255, 257, 1025)


@functools.lru_cache(maxsize=None)
def extent_bucket(n, L=12):
    """(umis, freq) of one bucket of n entries in rank order, without N."""
    rng = np.random.default_rng(66000 + 100 * n + L)
    return clustered_bucket(rng, n, L, 0.0) if n else ([], [])


LATE_FEED, LATE_SET = 12, 26


@functools.lru_cache(maxsize=None)
def late_label_batch():
    """A label that reaches a set late, through a pair that ends below the set's root.  Along the 21-base path at
    p = 1.0: x0 -> x1 -> ... -> x11 -> u one-way (freq 27, 25, ..., 5, then u = 3), u -> v one-way (v = 1), and
    v ~ ... ~ a symmetric (freq 1, 2, ..., 26).  In rank order a stands right behind x0 and before every other x,
    so a is the root of its set and root(a's set) < u: the pair (u, v) resolves to (u, a), moves nothing in the
    first round (lab[u] > a until x0's label has come down the twelve pairs), and must find a again in a later
    one.  Everything falls to x0."""
    nodes = ci.hamming_path(21)[:LATE_FEED + 1 + LATE_SET]
    freq = [3 + 2 * (LATE_FEED - i) for i in range(LATE_FEED)] + [3] + list(range(1, LATE_SET + 1))
    umis, freq, _ = canonical(nodes, freq)
    return Batch("one", 21, 1, 1.0, [(umis, freq)] + randoms(900, 21))


@functools.lru_cache(maxsize=None)
def split_batch():
    """The buckets of mixed_n_batch (three of them the fused kernel's, one with N) and behind them the bucket of
    giant_batch, which dominates the call: what a multi-device context splits over its devices."""
    return Batch("one", 8, 1, 0.5, [b for b in split_small_buckets()] + list(giant_batch().buckets), with_n=True)


@functools.lru_cache(maxsize=None)
def split_small_buckets():
    rng = np.random.default_rng(62005)
    return tuple([canonical(*random_bucket(rng, n_mol, 8, err=0.05))[:2] for n_mol in MIXED_MOLECULES]
                 + [clustered_bucket(rng, 300, 8, 0.2)])
