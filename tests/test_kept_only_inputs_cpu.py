"""The inputs of tests/test_gpu_kept_only.py (tests/kept_only_inputs.py), checked without a GPU: the oracle
agrees with the chains' closed form, and every input holds the pairs its test is about."""
import numpy as np
import pytest

import chain_inputs as ci
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
