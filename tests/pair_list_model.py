"""The pair lists from their definition, on the CPU: what umi_pairs_partial_device must list over all its
parts and what a neighbour store (umi_data_new[_wide]) must hold, plus the named inputs that the GPU tests
of those lists run (tests/test_gpu_pair_lists.py, tests/test_gpu_neighbour_lists.py) and the conditions
that make them worth running (checked without a GPU in tests/test_pair_list_model_cpu.py).

Written from the reference's definitions (distance: bitset.rs:77-91 word by word, utils/mod.rs:25; the
directional test: directional.rs:38-39 over naive.rs:31; adjacency.rs:56), not from the kernels."""
import functools

import numpy as np

from helpers import (ALPHA, WIDE_STRADDLE, clustered_bucket, dense_clusters, dist_blocks, merged_bucket, part_bounds,
                     planted_bucket, seg_bin_bases, seg_index_applies, seg_probe_entries, thr_f32)

BATCH_MAX_K = 128  # the batched calls and the stores clamp k to this (umihip_host.hpp)
EDGE_BUF = 512     # edges a block stages in LDS before it appends them (umihip_device.h)
FIRST_LIST = 1024  # the library's own list is never shorter (Pipeline::pair_stage)
GROWN = FIRST_LIST + FIRST_LIST // 16  # ... and this many entries are past any first list of a context told 1

ALGO_DIRECTIONAL, ALGO_ADJACENCY, ALGO_CLUSTER = 0, 1, 2
# the lists (p, algo, amf) a growth input is run for on a context of its own each: long enough that one part's
# share outgrows the first list whichever way the tasks are dealt to two or three parts
GROWTH_LISTS = ((1.0, ALGO_DIRECTIONAL, 0), (0.5, ALGO_CLUSTER, 0))


# ---- the model ---------------------------------------------------------------------------------------

def pair_distances(keys, nm, off):
    """Per bucket (first entry, int32 [n, n]): the reference's distance of every pair of the bucket
    (symmetric, 0 on the diagonal; the pairs i < j are its upper triangle).  keys / nm: uint64 [N] or
    [N, words]; every word goes through bitset.rs:77-91 on its own, the sum is halved once."""
    keys = np.ascontiguousarray(keys, np.uint64)
    nm = np.zeros_like(keys) if nm is None else np.ascontiguousarray(nm, np.uint64)
    out = []
    for b in range(len(off) - 1):
        s, e = int(off[b]), int(off[b + 1])
        d = np.zeros((e - s, e - s), np.int32)
        for r0, blk in dist_blocks(keys[s:e], nm[s:e]):
            d[r0:r0 + len(blk)] = blk
        out.append((s, d))
    return out


def neighbour_rows(dist, k):
    """Per entry (call-wide index) the ascending list of (other, distance) with distance <= k, the entry
    itself left out."""
    rows = []
    for s, d in dist:
        for i in range(len(d)):
            js = np.flatnonzero(d[i] <= k)
            rows.append([(s + int(j), int(d[i, j])) for j in js if j != i])
    return rows


def expected_edges(dist, freq, k, p, algo, amf):
    """The multiset of (src, dst, flag) a list call must produce over all its parts, as int64 [m, 3] in
    lexicographic order (call-wide entry indices).  k is clamped to BATCH_MAX_K as the library does."""
    k = min(int(k), BATCH_MAX_K)
    freq = np.asarray(freq, np.int64)
    out = []
    for s, d in dist:
        n = len(d)
        if n < 2 or (algo == ALGO_ADJACENCY and amf < 1):
            continue
        i, j = np.nonzero(np.triu(d <= k, 1))
        f = freq[s:s + n]
        if algo == ALGO_CLUSTER:
            src, dst, flag = i, j, np.ones(len(i), np.int64)
        elif algo == ALGO_ADJACENCY:
            keep = f[j] <= amf
            src, dst, flag = i[keep], j[keep], np.zeros(int(keep.sum()), np.int64)
        else:
            thr = np.array([thr_f32(p, int(x)) for x in f], np.int64)
            fwd, bwd = f[j] <= thr[i], f[i] <= thr[j]
            both, only_f, only_b = fwd & bwd, fwd & ~bwd, bwd & ~fwd
            src = np.concatenate([i[both], i[only_f], j[only_b]])
            dst = np.concatenate([j[both], j[only_f], i[only_b]])
            flag = np.concatenate([np.ones(int(both.sum()), np.int64), np.zeros(int(only_f.sum() + only_b.sum()), np.int64)])
        out.append(np.stack([src + s, dst + s, flag], axis=1).astype(np.int64))
    return sort_edges(np.concatenate(out) if out else np.zeros((0, 3), np.int64))


def sort_edges(e):
    e = np.asarray(e, np.int64).reshape(-1, 3)
    return e[np.lexsort((e[:, 2], e[:, 1], e[:, 0]))]


def decode_edges(u64):
    """uint64 words as umi_pairs_partial_device hands them out -> int64 [m, 3] of (src, dst, flag).
    The library copies its list of uint2 {x = src | flag << 31, y = dst} to the caller's buffer byte for
    byte (umihip_batch.cpp: hipMemcpyAsync of found * sizeof(uint2)); on this little-endian machine x is
    the low and y the high half of the 64-bit word."""
    w = np.ascontiguousarray(u64).view(np.uint64).reshape(-1)
    lo = (w & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return np.stack([lo & 0x7FFFFFFF, (w >> np.uint64(32)).astype(np.int64), lo >> 31], axis=1)


def collapse_of(edges, n, algo=ALGO_DIRECTIONAL):
    """(kept uint8 [n], root uint32 [n]) of a list over n entries, by plain min-label propagation: every
    entry ends with the smallest index that reaches it along src -> dst, flagged entries followed both ways,
    and is kept iff that is itself.  (Directional: the smallest entry that reaches v is a survivor -- whatever
    removed it would reach v too and be smaller -- and the first survivor in rank order to reach v, so this is
    the reference's root loop.  Cluster: every entry is flagged, the labels are the components' minima.)
    Adjacency (algo 1) is no closure: a root takes its direct neighbours only and an entry that was taken
    takes nothing, so there the entries are walked in rank order, one hop from every survivor."""
    edges = np.asarray(edges, np.int64).reshape(-1, 3)
    label = np.arange(n, dtype=np.int64)
    if algo == ALGO_ADJACENCY:
        order = np.argsort(edges[:, 0], kind="stable")
        src, dst = edges[order, 0], edges[order, 1]
        first = np.searchsorted(src, np.arange(n + 1))
        gone = np.zeros(n, bool)
        for r in range(n):
            if gone[r]:
                continue
            for v in dst[first[r]:first[r + 1]]:
                if not gone[v] and v != r:
                    gone[v] = True
                    label[v] = r
        return (~gone).astype(np.uint8), label.astype(np.uint32)
    sym = edges[:, 2] != 0
    src = np.concatenate([edges[:, 0], edges[sym, 1]])
    dst = np.concatenate([edges[:, 1], edges[sym, 0]])
    while True:
        new = label.copy()
        np.minimum.at(new, dst, label[src])
        if np.array_equal(new, label):
            break
        label = new
    return (label == np.arange(n)).astype(np.uint8), label.astype(np.uint32)


def replay_remove_near(rows, freq, present, q, k, max_freq):
    """naive.rs:26-40 over neighbour_rows: what remove_near(q, k, max_freq) removes from `present` (in
    place), ascending.  The query goes whatever its freq (distance 0), k < 0 removes nothing."""
    out = []
    if k >= 0 and present[q]:
        out.append(q)
    for o, d in rows[q]:
        if present[o] and d <= k and (d == 0 or freq[o] <= max_freq):
            out.append(o)
    for o in out:
        present[o] = False
    return sorted(out)


# ---- the named inputs --------------------------------------------------------------------------------

class Input:
    """One call's buckets: umis (call-wide list), L, k, keys / nm (uint64 [N] or [N, words]), fr, off, and
    opts, the context options the case is run under."""

    def __init__(self, name, L, k, buckets, opts=None, seg=False, dense=False, growth=False):
        import oracle as orc
        self.name, self.L, self.k, self.opts = name, L, k, dict(opts or {})
        self.seg, self.dense, self.growth = seg, dense, growth
        self.wide = L > 21
        self.umis, fr, off = [], [], [0]
        for umis, freq in buckets:
            self.umis += list(umis)
            fr += list(freq)
            off.append(len(self.umis))
        enc = orc.encode_keys_wide if self.wide else orc.encode_keys
        if self.umis:
            self.keys, self.nm = enc(self.umis)
        else:
            self.keys, self.nm = np.zeros(0, np.uint64), np.zeros(0, np.uint64)
        self.fr, self.off = np.array(fr, np.int32), np.array(off, np.uint64)

    @functools.cached_property
    def dist(self):
        return pair_distances(self.keys, self.nm, self.off)

    def edges(self, p, algo, amf):
        return expected_edges(self.dist, self.fr, self.k, p, algo, amf)


def _seed(name):
    return [ord(c) for c in name]


def _closed(rng, bucket):
    """The bucket (rank order) and one more entry of freq 1, so the last in rank order, one substitution from the
    first: the pair of a bucket's first row and last column, the last column of every task of its first rows."""
    umis, freq = list(bucket[0]), list(bucket[1])
    if len(umis) < 2:
        return umis, freq
    first = np.frombuffer(umis[0].encode(), np.uint8)
    while True:
        u = first.copy()
        i = int(rng.integers(len(u)))
        if u[i] == ord("N"):
            continue
        u[i] = rng.choice(ALPHA[ALPHA != u[i]])
        if u.tobytes().decode() not in umis:
            return umis + [u.tobytes().decode()], freq + [1]


def _planted(rng, n, L, k, n_frac, part_len=None):
    """planted_bucket of exactly n entries, closed (_closed) from three entries up."""
    sites = WIDE_STRADDLE if L > 21 else ()
    if n < 3:
        return planted_bucket(rng, n, L, k, n_frac, sites, part_len)
    return _closed(rng, planted_bucket(rng, n - 1, L, k, n_frac, sites, part_len))


def _seg_bucket(rng, n, L, k, n_frac, part_len=None):
    """About n entries for the segment index: planted copies at k - 1 .. k + 2, and from 400 entries up a
    clustered half (sub-buckets of more than a few entries), with the probe pairs of every part."""
    parts = [seg_probe_entries(rng, L, k, part_len)]
    if n >= 400 and L <= 21:
        parts.append(clustered_bucket(rng, n // 2, L, n_frac))
        n -= n // 2
    parts.append(_planted(rng, n, L, k, n_frac, part_len))
    return _closed(rng, merged_bucket(*parts))


def _with_opposite(rng, bucket):
    """The bucket and two more entries that differ in every base: a pair at the largest distance there is."""
    L = len(bucket[0][0])
    c = rng.choice(ALPHA, L)
    u = np.array([rng.choice(ALPHA[ALPHA != x]) for x in c], np.uint8)
    return merged_bucket(bucket, {c.tobytes().decode(): 3, u.tobytes().decode(): 1})


CHUNK_SIZES = (1, 2, 33, 64, 65, 129, 300)
CHUNK_LK = ((12, 2), (20, 3))
SEG_LK = ((12, 1), (12, 2), (12, 3), (18, 5), (20, 2))
SEG_MIN = {"seg_min": 129}
BIG = {"small_max": 0, "seg_index": 0}
SECOND_TILE = {"seg_index": 0, "small_max": 2048}  # a bucket of 1,100 entries as small tasks of the chunk kernel


def _tag(L, k, n_frac):
    return "L%d_k%d%s" % (L, k, "_N" if n_frac else "")


def _pair_builders():
    b = {}
    for L, k in CHUNK_LK:
        for nf in (0.0, 0.02):
            b["chunk_sizes_" + _tag(L, k, nf)] = lambda rng, L=L, k=k, nf=nf: Input(
                "", L, k, [_planted(rng, n, L, k, nf) for n in CHUNK_SIZES])
            b["chunk_1100_" + _tag(L, k, nf)] = lambda rng, L=L, k=k, nf=nf: Input(
                "", L, k, [_planted(rng, 1100, L, k, nf)])
    b["big_300_2100"] = lambda rng: Input("", 12, 2, [_planted(rng, 300, 12, 2, 0.01), _planted(rng, 2100, 12, 2, 0.01)],
                                          BIG)
    for L, k in SEG_LK:
        for nf in (0.0, 0.02):
            b["seg_" + _tag(L, k, nf)] = lambda rng, L=L, k=k, nf=nf: Input(
                "", L, k, [_seg_bucket(rng, 300, L, k, nf), _seg_bucket(rng, 600, L, k, nf)], SEG_MIN, seg=True)
    b["dense_L8_k8"] = lambda rng: Input("", 8, 8, [_closed(rng, clustered_bucket(rng, 299, 8, 0.0))], dense=True)
    b["growth_chunk"] = lambda rng: Input(
        "", 10, 4, [_closed(rng, merged_bucket(dense_clusters(rng, 5, 45, 10, 4), _planted(rng, 60, 10, 4, 0.1)))], growth=True)
    b["growth_seg"] = lambda rng: Input(
        "", 12, 3, [_closed(rng, merged_bucket(dense_clusters(rng, 12, 50, 12, 3), _seg_bucket(rng, 200, 12, 3, 0.05)))],
        SEG_MIN, seg=True, growth=True)
    return b


_PAIR_BUILDERS = _pair_builders()
PAIR_INPUTS = tuple(_PAIR_BUILDERS)


@functools.lru_cache(maxsize=None)
def pair_input(name):
    inp = _PAIR_BUILDERS[name](np.random.default_rng(_seed(name)))
    inp.name = name
    return inp


# ---- neighbour stores: one bucket each, as a map in shuffled order with the freq that came with it ----

class Store:
    """One store's map: umis in shuffled order (a map has no rank order), freq, L, max_edits, opts; ctx is
    "single", "multi" (a context over devices [0, 0]) or "grow" (edge_capacity = 1 before every build)."""

    def __init__(self, name, L, max_edits, bucket, opts=None, seg=False, dense=False, growth=False, ctx="single"):
        rng = np.random.default_rng(_seed("shuffle" + name))
        umis, freq = bucket
        order = rng.permutation(len(umis)).tolist()
        inp = Input(name, L, max_edits, [([umis[i] for i in order], [freq[i] for i in order])], opts, seg, dense, growth)
        d = inp.dist[0][1]
        if len(order) > 2 and d[0, -1] > max_edits:  # a neighbouring pair first and last: a task's last column is tried
            i, j = [int(x[0]) for x in np.nonzero(np.triu(d <= max_edits, 1))]
            order[0], order[i] = order[i], order[0]
            j = i if j == 0 else j  # (what stood first has moved to i)
            order[-1], order[j] = order[j], order[-1]
            inp = Input(name, L, max_edits, [([umis[i] for i in order], [freq[i] for i in order])], opts, seg, dense, growth)
        self.inp, self.name, self.L, self.max_edits, self.opts, self.ctx = inp, name, L, max_edits, inp.opts, ctx
        self.umis, self.freq = inp.umis, inp.fr.tolist()
        self.seg, self.dense, self.growth = seg, dense, growth
        self.part_len = min(L, 21)  # (the index looks at the first word's 21 bases)

    @functools.cached_property
    def rows(self):
        return neighbour_rows(self.inp.dist, min(self.max_edits, BATCH_MAX_K))


def _store_builders():
    b = {}
    for L, me in CHUNK_LK:
        for nf in (0.0, 0.02):
            for n in (2, 64, 65, 129, 300):
                b["chunk_n%d_%s" % (n, _tag(L, me, nf))] = lambda rng, L=L, me=me, nf=nf, n=n: Store(
                    "", L, me, _planted(rng, n, L, me, nf))
    b["big_n300_L12_k2"] = lambda rng: Store("", 12, 2, _planted(rng, 300, 12, 2, 0.01), BIG)
    for L, me, nf, opts in ((12, 1, 0.0, {}), (12, 3, 0.0, {}), (18, 5, 0.0, {}), (20, 2, 0.02, {}),
                            (12, 3, 0.02, {"seg_blocks": 1})):
        name = "seg_n300_" + _tag(L, me, nf) + ("_1block" if opts else "")
        b[name] = lambda rng, L=L, me=me, nf=nf, opts=opts: Store(
            "", L, me, _seg_bucket(rng, 300, L, me, nf), dict(SEG_MIN, **opts), seg=True)
    for L in (22, 43, 85):
        # (n = 129: all pairs at one edit, the index at two; n = 200: the other way round)
        for n, seg, me in ((129, False, 1), (129, True, 2), (200, False, 2), (200, True, 1)):
            name = "wide_%s_n%d_L%d_k%d_N" % ("seg" if seg else "pairs", n, L, me)
            b[name] = lambda rng, L=L, n=n, seg=seg, me=me: Store(
                "", L, me, _seg_bucket(rng, n, L, me, 0.02, 21) if seg else _planted(rng, n, L, me, 0.02, 21),
                SEG_MIN if seg else {"seg_index": 0}, seg=seg)
    b["dense_n200_L8_k8"] = lambda rng: Store("", 8, 8, clustered_bucket(rng, 200, 8, 0.0), dense=True)
    b["dense_n129_L43_k43"] = lambda rng: Store("", 43, 43, _with_opposite(rng, clustered_bucket(rng, 127, 43, 0.02)),
                                                {"seg_index": 0}, dense=True)
    b["growth_seg_n300_L12_k3"] = lambda rng: Store(
        "", 12, 3, merged_bucket(dense_clusters(rng, 4, 50, 12, 3), _seg_bucket(rng, 150, 12, 3, 0.05)), SEG_MIN, seg=True,
        growth=True, ctx="grow")
    b["multi_n129_L12_k2_N"] = lambda rng: Store("", 12, 2, _planted(rng, 129, 12, 2, 0.02), ctx="multi")
    return b


_STORE_BUILDERS = _store_builders()
STORES = tuple(_STORE_BUILDERS)


@functools.lru_cache(maxsize=None)
def store(name):
    st = _STORE_BUILDERS[name](np.random.default_rng(_seed(name)))
    st.name = st.inp.name = name
    return st


# ---- the conditions that make an input worth running ---------------------------------------------------

def limit_pairs(inp):
    """Pairs of the input at distance exactly k and exactly k + 1."""
    at_k = sum(int((np.triu(d, 1) == inp.k).sum()) for _, d in inp.dist) if inp.k > 0 else 0
    at_k1 = sum(int((np.triu(d, 1) == inp.k + 1).sum()) for _, d in inp.dist)
    return at_k, at_k1


def direction_census(inp, p=0.5):
    """(symmetric, one-way, not permitted either way) among the input's pairs within k."""
    e = inp.edges(p, ALGO_DIRECTIONAL, 0)
    within = len(inp.edges(p, ALGO_CLUSTER, 0))
    sym = int((e[:, 2] == 1).sum())
    return sym, len(e) - sym, within - len(e)


def shared_bins(umis, i, j, L, k, n):
    """The parts of a bucket of n entries in whose bin entries i and j meet (the filter keys fold N onto A)
    and the parts on which they agree base for base."""
    a, b = umis[i].replace("N", "A"), umis[j].replace("N", "A")
    bins = frozenset(p for p, (b0, nb) in enumerate(seg_bin_bases(n, L, k)) if a[b0:b0 + nb] == b[b0:b0 + nb])
    pb = part_bounds(L, k + 1)
    whole = frozenset(p for p in range(k + 1) if umis[i][pb[p]:pb[p + 1]] == umis[j][pb[p]:pb[p + 1]])
    return bins, whole


def seg_census(inp, part_len=None, seg_min=129):
    """Per bucket that the segment index takes: (parts j with a pair within k that agrees on part j and meets in
    no other part's bin, pairs within k that meet in two bins or more, pairs that agree on two whole parts or more)."""
    L = min(part_len or inp.L, inp.L)
    out = []
    for s, d in inp.dist:
        n = len(d)
        if n < seg_min:
            continue
        alone, two_bins, two_parts = set(), 0, 0
        for i, j in zip(*np.nonzero(np.triu(d <= inp.k, 1))):
            bins, whole = shared_bins(inp.umis[s:s + n], int(i), int(j), L, inp.k, n)
            if len(bins) == 1 and bins <= whole:
                alone |= bins
            two_bins += len(bins) >= 2
            two_parts += len(whole) >= 2
        out.append((alone, two_bins, two_parts))
    return out


def most_edges_of_a_row_task(inp, rows=64):
    """The most pairs within k that one task of `rows` rows against every later column holds."""
    best = 0
    for _, d in inp.dist:
        per_row = np.triu(d <= inp.k, 1).sum(1)
        best = max([best] + [int(per_row[r:r + rows].sum()) for r in range(0, len(d), rows)])
    return best
