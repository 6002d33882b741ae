"""The deep-chain buckets of tests/chain_inputs.py, checked on the CPU before a kernel sees them: the
keys are distinct, the entries are in rank order, the chain of permitted pairs is as deep as claimed
(a model of dist <= k and freq[v] <= threshold(p, freq[u]) written here), and the oracle -- the
restated reference for keys of up to 85 bases, the numpy model of whole reads beyond -- gives the
closed-form answer."""
import numpy as np
import pytest

import chain_inputs as ci
import oracle as orc
import seq_model as sm

# (ladder, L, stride, order) of every chain tests/test_gpu_deep_chains.py uses
ONE_WORD = [(lad, L, s, o) for L, s in ((21, 1), (8, 1), (21, 4), (8, 4)) for lad, o in
            [("sym", o) for o in ci.ORDERS] + [("halving", "forward"), ("step2", "forward"), ("comb", "forward")]]
WIDE = [(lad, L, 1, o) for L in (85, 30) for lad, o in
        [("sym", o) for o in ci.ORDERS] + [("halving", "forward"), ("step2", "forward"), ("comb", "forward")]]
SEQ = [(lad, L, 1, o) for L in (256, 100) for lad, o in
       (("sym", "forward"), ("sym", "zigzag"), ("step2", "forward"), ("comb", "forward"))]


@pytest.mark.parametrize("L", [2, 3, 8, 21, 85, 256])
def test_path_distances(L):
    nodes = ci.hamming_path(L)
    assert len(nodes) == 3 * L + 1 == ci.n_nodes(L) and len(set(nodes)) == len(nodes)
    i = np.arange(len(nodes))
    assert np.array_equal(ci.distances(nodes), np.minimum(np.abs(i[:, None] - i[None, :]), L))


@pytest.mark.parametrize("L,k,n", [(21, 1, 64), (85, 1, 256), (256, 1, 769), (21, 4, 16), (8, 1, 25), (8, 4, 7),
                                   (30, 1, 91), (100, 1, 301)])
def test_strided_path_is_induced(L, k, n):
    nodes = ci.hamming_path(L, k)
    assert len(nodes) == n == ci.n_nodes(L, k)
    d = ci.distances(nodes)
    i = np.arange(n)
    gap = np.abs(i[:, None] - i[None, :])
    assert (d[gap == 1] == k).all() and (d[gap >= 2] >= min(2 * k, L)).all() and 2 * k <= L


@pytest.mark.parametrize("order", ci.ORDERS)
@pytest.mark.parametrize("n", [1, 2, 7, 16, 25, 64, 256])
def test_orders_are_permutations(order, n):
    pos = ci.order_positions(n, order)
    assert sorted(pos) == list(range(n))
    if order == "zigzag" and n >= 4:
        assert pos[:4] == [0, n - 1, 1, n - 2]


def _check_chain(c, k):
    assert len(set(c.umis)) == c.n == len(c.freq)
    assert all(a >= b for a, b in zip(c.freq, c.freq[1:])) and min(c.freq) >= 1 and max(c.freq) < 2 ** 31
    adj = ci.permitted_pairs(c.umis, c.freq, k, c.p)
    hop = ci.hops_from_rank0(adj)
    assert min(hop) >= 0 and max(hop) == c.depth, (c.name, max(hop), c.depth)
    # the pairs are the path's own, and of the kind the ladder promises
    pos = np.array(c.pos)
    near = np.abs(pos[:, None] - pos[None, :]) == 1
    assert not (adj & ~near).any()
    both, one = adj & adj.T, adj ^ adj.T
    assert ((both | one) == near).all()
    ladder = c.name.split("/")[0]
    if ladder == "sym":
        assert not one.any()
    elif ladder in ("halving", "step2"):
        assert not both.any()
    else:
        assert both.sum() // 2 == c.n // 2 and one.sum() // 2 == (c.n - 1) // 2
    return adj


@pytest.mark.parametrize("ladder,L,stride,order", ONE_WORD)
def test_one_word_chains(ladder, L, stride, order):
    c = ci.chain(ladder, L, stride, order)
    _check_chain(c, stride)
    keys, nm = orc.encode_keys(c.umis)
    off = np.array([0, c.n], np.uint64)
    fr = np.array(c.freq, np.int32)
    kept, root, _ = orc.dedup_batch(keys, nm, fr, off, L, stride, c.p)
    ek, er = c.directional()
    assert np.array_equal(kept, ek) and np.array_equal(root, er), c.name
    if stride > 1:  # one edit less and nothing is near anything
        kept, _, _ = orc.dedup_batch(keys, nm, fr, off, L, stride - 1, c.p)
        assert kept.all()
    if ladder == "sym":
        for amf in (0, 1):
            kept, root, _ = orc.dedup_batch(keys, nm, fr, off, L, stride, c.p, 1, amf)
            ek, er, _ = ci.expected([(c.umis, c.freq)], [c], 1, amf)
            assert np.array_equal(kept, ek) and np.array_equal(root, er), (c.name, amf)
        if order == "forward":
            assert np.array_equal(c.adjacency(1)[0], (np.arange(c.n) % 2 == 0).astype(np.uint8))


@pytest.mark.parametrize("ladder,L,stride,order", WIDE)
def test_wide_chains(ladder, L, stride, order):
    c = ci.chain(ladder, L, stride, order)
    _check_chain(c, stride)
    keys, nm = orc.encode_keys_wide(c.umis)
    off = np.array([0, c.n], np.uint64)
    fr = np.array(c.freq, np.int32)
    kept, root, _ = orc.dedup_batch_wide(keys, nm, fr, off, L, stride, c.p)
    ek, er = c.directional()
    assert np.array_equal(kept, ek) and np.array_equal(root, er), c.name
    if ladder == "sym":
        for amf in (0, 1):
            kept, root, _ = orc.dedup_batch_wide(keys, nm, fr, off, L, stride, c.p, 1, amf)
            ek, er, _ = ci.expected([(c.umis, c.freq)], [c], 1, amf)
            assert np.array_equal(kept, ek) and np.array_equal(root, er), (c.name, amf)


@pytest.mark.parametrize("ladder,L,stride,order", SEQ)
def test_seq_chains(ladder, L, stride, order):
    c = ci.chain(ladder, L, stride, order)
    _check_chain(c, stride)
    ent = [(u.encode(), f, 0) for u, f in zip(c.umis, c.freq)]
    kept, root = sm.dedup(ent, [0, c.n], [L], stride, 0, c.p)
    ek, er = c.directional()
    assert np.array_equal(kept, ek.astype(bool)) and np.array_equal(root, er), c.name
