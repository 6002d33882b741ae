"""The inputs of tests/test_gpu_kept_only.py and tests/test_gpu_kept_only_matrix.py (tests/kept_only_inputs.py),
checked without a GPU: the oracle agrees with the chains' closed form, and every input holds the pairs its
test is about."""
import numpy as np
import pytest

import chain_inputs as ci
import edit_model as em
import helpers as h
import kept_only_inputs as ko


def pair_census(umis, freq, k, p):
    """(symmetric pairs, one-way pairs (u, v)) of one bucket from the definition."""
    adj = ci.permitted_pairs(umis, freq, k, p)
    sym = np.argwhere(np.triu(adj & adj.T, 1))
    one = np.argwhere(adj & ~adj.T)
    return sym, one


def components(n, sym):
    comp = list(range(n))

    def find(x):
        while comp[x] != x:
            x = comp[x]
        return x
    for u, v in sym:
        a, b = find(int(u)), find(int(v))
        if a != b:
            comp[max(a, b)] = min(a, b)
    return [find(i) for i in range(n)]


@pytest.mark.parametrize("form,L,stride", [("one",) + p for p in ko.PATHS] + [("wide", 85, 1)])
def test_chain_batches_fall_to_rank_0(form, L, stride):
    for b in ko.chain_batches(L, stride, form):
        okept = b.reference()
        lo = 0
        for i, (umis, freq) in enumerate(b.buckets):
            if b.is_chain[i]:  # only its rank 0 stays
                assert okept[lo] == 1 and not okept[lo + 1:lo + len(umis)].any(), (b.p, i)
            lo += len(umis)
        assert lo == len(b.keys) and sum(b.is_chain) == (len(ko.HALF) if b.p == 0.5 else len(ko.ONE))


def test_chain_batches_hold_deep_trees_and_chained_sets():
    half, one = ko.chain_batches(21, 1)
    assert half.sizes()[0] == 64 and one.sizes()[0] == 64 and max(half.sizes() + one.sizes()) <= 128
    # comb: symmetric and one-way pairs alternate
    comb = ci.chain("comb", 21, 1)
    sym, ow = pair_census(comb.umis, comb.freq, 1, 1.0)
    assert len(sym) == 32 and len(ow) == 31
    # step2: every pair one-way
    s2 = ci.chain("step2", 21, 1)
    sym, ow = pair_census(s2.umis, s2.freq, 1, 1.0)
    assert len(sym) == 0 and len(ow) == 63


def test_self_edge_trio():
    b = ko.self_edge_batch()
    assert b.sizes() == [23]
    umis, freq = b.buckets[0]
    at = [umis.index(u) for u in ko.SELF_EDGE_TRIO]
    assert [freq[i] for i in at] == [3, 2, 1]
    adj = ci.permitted_pairs(umis, freq, 1, 1.0)
    a, c, g = at
    assert adj[a, c] and adj[c, a] and adj[c, g] and adj[g, c]  # 3 ~ 2, 2 ~ 1
    assert adj[a, g] and not adj[g, a]                            # 3 -> 1 only
    sym, _ = pair_census(umis, freq, 1, 1.0)
    comp = components(len(umis), sym)
    assert comp[a] == comp[c] == comp[g]  # the one-way pair lies inside one symmetric set
    okept = b.reference()
    assert okept[a] == 1 and okept[c] == 0 and okept[g] == 0


def test_mixed_batch_reaches_every_kernel():
    b = ko.mixed_batch()
    sizes = b.sizes()
    assert sum(1 for s in sizes if s <= 128) >= 3
    chunk = [i for i, s in enumerate(sizes) if 129 <= s <= 511]
    deep = [i for i, s in enumerate(sizes) if s >= 512]
    assert len(chunk) == 1 and len(deep) == 1, sizes
    for i in chunk + deep:
        umis, freq = b.buckets[i]
        sym, ow = pair_census(umis, freq, 1, 0.5)
        assert len(sym) > 0 and len(ow) > 0, (i, len(sym), len(ow))
        # some one-way pair ends inside a set of more than one entry: its endpoint is not its own root
        comp = components(len(umis), sym)
        assert any(comp[int(u)] != int(u) or comp[int(v)] != int(v) for u, v in ow)
    okept = b.reference()
    assert 0 < int(okept.sum()) < len(okept)


def test_overflow_batch_is_longer_than_the_lists_floor():
    b = ko.overflow_batch()
    n_one_way = 0
    for umis, freq in b.buckets[:1]:
        _, ow = pair_census(umis, freq, 1, 1.0)
        n_one_way = len(ow)
    assert n_one_way == 63 and 40 * n_one_way > 1024
    okept = b.reference()
    assert okept[0] == 1 and not okept[1:64].any()


# ---- the inputs of tests/test_gpu_kept_only_matrix.py -----------------------------------------------------

def permitted_by_keys(batch, b):
    """bool [n, n] of bucket b: u -> v permitted, by the reference's distance over keys and N masks."""
    lo, hi = int(batch.off[b]), int(batch.off[b + 1])
    f = batch.fr[lo:hi].astype(np.int64)
    thr = np.array([h.thr_f32(batch.p, int(x)) for x in f])
    adj = np.zeros((hi - lo, hi - lo), bool)
    for r0, d in h.dist_blocks(batch.keys[lo:hi], batch.nm[lo:hi]):
        adj[r0:r0 + len(d)] = (d <= batch.k) & (f[None, :] <= thr[r0:r0 + len(d), None])
    np.fill_diagonal(adj, False)
    return adj


@pytest.mark.parametrize("p", [0.5, 1.0])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n_frac", ko.N_FRACS)
def test_n_batches_hold_n_in_every_size_class(n_frac, k, p):
    b = ko.n_batch(n_frac, k, p)
    assert b.sizes() == list(ko.N_SIZES) and b.nmask is not None
    assert b.sizes()[0] <= 128 and 129 <= b.sizes()[1] <= 511 and b.sizes()[2] >= 512
    with_n_pair = 0
    for i in range(3):
        lo, hi = int(b.off[i]), int(b.off[i + 1])
        has_n = b.nm[lo:hi] != 0
        assert has_n.any(), (n_frac, i)
        adj = permitted_by_keys(b, i)
        with_n_pair += int((adj & (has_n[:, None] | has_n[None, :])).sum())
    assert with_n_pair > 0
    assert 0 < int(b.reference().sum()) < len(b.keys)


def test_fuzz_batches_hold_one_way_pairs_and_deep_buckets():
    deep = large_k = 0
    for seed in ko.FUZZ_SEEDS:
        b = ko.fuzz_batch(seed)
        assert 3 <= len(b.sizes()) <= 6
        deep += max(b.sizes()) >= 512
        large_k += b.k >= 4
        if b.k >= 1 and b.p > 0:
            one_way = 0
            for i in [i for i, n in enumerate(b.sizes()) if n >= 2]:
                adj = permitted_by_keys(b, i)
                one_way += int((adj & ~adj.T).sum())
            assert one_way > 0, seed
    assert deep >= 8 and large_k >= 3, (deep, large_k)


def test_edit_batches_hold_one_way_pairs_that_only_a_shift_joins():
    """At k = 2 some permitted one-way pairs are within 2 by edit distance and farther by Hamming distance."""
    for L, n_frac in ko.EDIT_INPUTS:
        b = ko.edit_batch(L, n_frac)
        shift_only = 0
        for (umis, freq), d in zip(b.buckets, b.mats):
            if len(umis) < 2:
                continue
            thr = np.array([h.thr_f32(0.5, f) for f in freq])
            adj = (d <= 2) & (np.array(freq)[None, :] <= thr[:, None])
            np.fill_diagonal(adj, False)
            shift_only += int((adj & ~adj.T & (em.hamming_matrix(umis) > 2)).sum())
        assert shift_only > 0, (L, n_frac)
        assert (b.nm.any()) == bool(n_frac)
    d = ko.edit_dense_batch()
    assert len(d.buckets[0][0]) == 600 and 0 < int(d.reference(2, 0.5).sum()) < 600


def test_seq_batches_have_both_lengths_and_a_partitioned_bucket():
    for k in (1, 2):
        b = ko.seq_batch(k)
        assert b.blen == [30] * 3 + [100] * 3 and np.diff(b.off.astype(np.int64)).tolist() == [2, 200, 600] * 2
        assert h.seq_partitioned(100, k) and b.nm.any()
        assert 0 < int(b.reference().sum()) < len(b.fr)


def test_deep_batches_are_768_hops_deep():
    rev = ci.chain("sym", ko.DEEP_L, 1, "reverse")
    assert rev.n == 769 and rev.depth == rev.n - 1
    for which, n_buckets in (("sym", 2), ("step2", 1)):
        b = ko.deep_batch(which)
        assert np.diff(b.off.astype(np.int64)).tolist() == [769] * n_buckets
        exp = np.zeros(len(b.fr), np.uint8)
        exp[::769] = 1  # everything falls to rank 0
        assert np.array_equal(b.reference(), exp)
    s2 = ci.chain("step2", ko.DEEP_L, 1)
    adj = ci.permitted_pairs(s2.umis, s2.freq, 1, 1.0)
    assert int((adj & adj.T).sum()) == 0 and int(adj.sum()) == 768


def test_giant_batch_is_one_giant_component():
    b = ko.giant_batch()
    n = ko.GIANT_N
    assert b.sizes() == [n] and len(set(b.buckets[0][0])) == n
    assert (np.diff(b.fr) <= 0).all() and b.fr[0] > 2 and b.fr[-1] == 1
    # the distance-1 neighbours of every entry through a table over the 4^8 codes (no N here)
    code = np.zeros(n, np.int64)
    for i in range(8):
        code |= np.array(["ACGT".index(u[i]) for u in b.buckets[0][0]], np.int64) << (2 * i)
    at = np.full(4 ** 8, -1, np.int64)
    at[code] = np.arange(n)
    thr = np.array([h.thr_f32(0.5, int(f)) for f in b.fr])
    sym, one_way = [], []
    for i in range(8):
        for x in (1, 2, 3):
            v = at[code ^ (x << (2 * i))]
            u = np.nonzero(v >= 0)[0]
            v = v[u]
            fwd, bwd = b.fr[v] <= thr[u], b.fr[u] <= thr[v]
            sym.append(np.stack([u, v], 1)[fwd & bwd & (u < v)])
            one_way.append(np.stack([u, v], 1)[fwd & ~bwd])
    sym, one_way = np.concatenate(sym), np.concatenate(one_way)
    comp = np.array(components(n, sym))
    ids, counts = np.unique(comp, return_counts=True)
    giant = ids[np.argmax(counts)]
    assert counts.max() > n // 2, counts.max()
    assert int((comp[one_way[:, 1]] == giant).sum()) > 1024
    assert 0 < int(b.reference().sum()) < n


def test_mixed_n_batch_and_small_inputs():
    b = ko.mixed_n_batch()
    assert b.nmask is not None and b.sizes()[:-1] == ko.mixed_batch().sizes() and b.sizes()[-1] == 300
    lo = int(b.off[-2])
    assert (b.nm[lo:] != 0).any() and not (b.nm[:lo] != 0).any()
    for algo, amf in ((0, 0), (1, 0), (1, 3)):
        assert int(b.reference(algo, amf).sum()) > 0
    assert int(b.reference(1, 0).sum()) == len(b.keys)            # adj_max_freq = 0 removes nothing
    assert int(b.reference(1, 3).sum()) < len(b.keys)
    s2 = ko.step2_batch()
    assert s2.sizes() == [64] and s2.reference().tolist() == [1] + [0] * 63
    assert ko.small_batch().sizes() == [300]
    for n in ko.EXTENT_SIZES:
        for L in (12, 30):
            umis, freq = ko.extent_bucket(n, L)
            assert len(umis) == n and all(len(u) == L and "N" not in u for u in umis)
            assert all(a >= c for a, c in zip(freq, freq[1:]))


def test_late_label_batch_ends_below_a_root_that_stands_before_the_source():
    b = ko.late_label_batch()
    umis, freq = b.buckets[0]
    n = len(umis)
    assert n == ko.LATE_FEED + 1 + ko.LATE_SET
    sym, ow = pair_census(umis, freq, 1, 1.0)
    comp = components(n, sym)
    assert len(sym) == ko.LATE_SET - 1 and len(ow) == ko.LATE_FEED + 1
    # the one one-way pair into the set of 26: its target is not the set's root, the root stands before its source
    into = [(int(u), int(v)) for u, v in ow if comp[int(v)] != int(v)]
    assert len(into) == 1
    u, v = into[0]
    a = comp[v]
    assert a == 1 and comp[u] == u and a < u and sum(1 for c in comp if c == a) == ko.LATE_SET
    # x0's label needs every pair of the feed to reach u, and u's own label never moves a
    hops = ci.hops_from_rank0(ci.permitted_pairs(umis, freq, 1, 1.0))
    assert hops[u] == ko.LATE_FEED and min(hops) >= 0
    okept = b.reference()
    assert okept[0] == 1 and not okept[1:n].any()


def test_split_batch_is_dominated_by_one_bucket_and_holds_fused_buckets_with_pairs():
    b = ko.split_batch()
    sizes = np.array(b.sizes(), np.float64)
    assert sizes[-1] == ko.GIANT_N and 2 * sizes.max() ** 2 > (sizes ** 2).sum()  # the planner's test of "dominates"
    assert b.nmask is not None and not (b.nm[int(b.off[-2]):] != 0).any()
    fused = [i for i, s in enumerate(b.sizes()) if 2 <= s <= 128]
    assert len(fused) == 3 and all(permitted_by_keys(b, i).any() for i in fused)
    assert 0 < int(b.reference().sum()) < len(b.keys)
