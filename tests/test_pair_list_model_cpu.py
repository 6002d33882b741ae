"""The CPU model of the pair lists (tests/pair_list_model.py) against the oracle, and the conditions that make
the inputs of tests/test_gpu_pair_lists.py and tests/test_gpu_neighbour_lists.py worth running.  No GPU."""
import ctypes as C
import functools

import numpy as np
import pytest

import cluster_model
import oracle as orc
import pair_list_model as plm
from pair_list_model import ALGO_ADJACENCY, ALGO_CLUSTER, ALGO_DIRECTIONAL, EDGE_BUF, GROWN

SMALL = 340  # buckets up to this many entries are compared with orc.umi_dist pair by pair

ALL_INPUTS = [("pair", n) for n in plm.PAIR_INPUTS] + [("store", n) for n in plm.STORES]
SEG_INPUTS = [(kind, n) for kind, n in ALL_INPUTS if (plm.pair_input(n) if kind == "pair" else plm.store(n)).seg]


def get(kind, name):
    return plm.pair_input(name) if kind == "pair" else plm.store(name).inp


@functools.lru_cache(maxsize=None)
def wide_ranked(L):
    """A wide bucket in rank order (the stores' maps are shuffled: nothing the batched oracle takes)."""
    return plm.Input("wide_ranked_L%d" % L, L, 2, [plm._planted(np.random.default_rng(L), 200, L, 2, 0.02, 21)])


@pytest.mark.parametrize("kind,name", ALL_INPUTS)
def test_distances_equal_the_oracle_pair_by_pair(kind, name):
    inp = get(kind, name)
    dist_fn = orc.lib().orc_umi_dist
    checked = 0
    for s, d in inp.dist:
        n = len(d)
        assert (d == d.T).all() and (np.diag(d) == 0).all()
        if n > SMALL:
            continue
        sets = [orc.to_bitset(u) for u in inp.umis[s:s + n]]
        refs = [C.byref(b) for b in sets]
        want = np.zeros((n, n), np.int32)
        for i in range(n):
            ri = refs[i]
            want[i, i + 1:] = [dist_fn(ri, refs[j]) for j in range(i + 1, n)]
        assert np.array_equal(np.triu(d, 1), want)
        checked += n * (n - 1) // 2
    assert checked or all(len(d) > SMALL or len(d) < 2 for _, d in inp.dist)


def test_straddling_bases_are_among_the_wide_inputs():
    """N at bases 21 and 42, the ones that straddle two key words, in the wide stores."""
    for L, sites in ((22, (21,)), (43, (21, 42)), (85, (21, 42))):
        names = [n for n in plm.STORES if n.startswith("wide_") and "_L%d_" % L in n]
        assert len(names) == 4
        for site in sites:
            assert any(u[site] == "N" for n in names for u in plm.store(n).umis), (L, site)
        for n in names:
            st = plm.store(n)
            assert st.inp.nm.any() and st.inp.keys.shape[1] == (3 * L + 63) // 64


@pytest.mark.parametrize("name", ["chunk_n65_L12_k2_N", "chunk_n129_L20_k3_N", "seg_n300_L18_k5", "wide_pairs_n129_L43_k1_N",
                                  "wide_seg_n200_L85_k1_N", "dense_n200_L8_k8", "dense_n129_L43_k43"])
def test_rows_replayed_equal_naive(name):
    st = plm.store(name)
    rng = np.random.default_rng(5)
    n = len(st.umis)
    for _ in range(3):
        o = orc.Naive(st.umis, st.freq)
        present = np.ones(n, bool)
        for q in rng.integers(0, n, 100):
            k = int(rng.integers(-1, st.max_edits + 1))
            mf = int(rng.choice([0, 1, 2, 3, 5, 2 ** 31 - 1]))
            got = plm.replay_remove_near(st.rows, st.freq, present, int(q), k, mf)
            assert got == sorted(o.remove_near(int(q), k, mf))
        assert all(o.contains(i) == bool(present[i]) for i in range(n))


@pytest.mark.parametrize("name", list(plm.PAIR_INPUTS) + ["wide_ranked_L22", "wide_ranked_L43", "wide_ranked_L85"])
def test_collapse_of_the_expected_list_equals_the_oracle(name):
    """The direction rule, tied to the restated reference: the list's closure is the oracle's result."""
    inp = wide_ranked(int(name.rsplit("L", 1)[1])) if name.startswith("wide_ranked") else plm.pair_input(name)
    fn = orc.dedup_batch_wide if inp.wide else orc.dedup_batch
    n = len(inp.umis)
    for p, algo, amf in ((0.3, ALGO_DIRECTIONAL, 0), (0.5, ALGO_DIRECTIONAL, 0), (1.0, ALGO_DIRECTIONAL, 0),
                         (0.5, ALGO_ADJACENCY, 2)):
        okept, oroot, _ = fn(inp.keys, inp.nm, inp.fr, inp.off, inp.L, inp.k, p, algo, amf)
        kept, root = plm.collapse_of(inp.edges(p, algo, amf), n, algo)
        assert np.array_equal(kept, okept) and np.array_equal(root, oroot), (p, algo, amf)
    assert len(inp.edges(0.5, ALGO_ADJACENCY, 0)) == 0  # adjacency.rs as written: only the query goes
    e = inp.edges(0.5, ALGO_CLUSTER, 0)
    assert (e[:, 2] == 1).all() and (e[:, 0] < e[:, 1]).all()
    ckept, croot = cluster_model.batch([d for _, d in inp.dist], inp.off, inp.k)
    kept, root = plm.collapse_of(e, n, ALGO_CLUSTER)
    assert np.array_equal(kept, ckept) and np.array_equal(root, croot)


def test_decode_edges_layout():
    src, dst = np.array([0, 5, 2 ** 31 - 17], np.uint64), np.array([1, 2 ** 31 - 2, 7], np.uint64)
    flag = np.array([0, 1, 1], np.uint64)
    w = np.zeros(3, [("x", "<u4"), ("y", "<u4")])  # a uint2 in memory
    w["x"], w["y"] = src | (flag << np.uint64(31)), dst
    got = plm.decode_edges(w.view(np.uint64))
    assert got.tolist() == [[0, 1, 0], [5, 2 ** 31 - 2, 1], [2 ** 31 - 17, 7, 1]]
    assert plm.decode_edges(np.zeros(0, np.int64)).shape == (0, 3)


def test_collapse_of_small_lists():
    # 0 -> 1 -> 2 one-way, 3 = 4 symmetric, 4 -> 2: the smallest entry that reaches 2 is 0
    e = [(0, 1, 0), (1, 2, 0), (3, 4, 1), (4, 2, 0)]
    kept, root = plm.collapse_of(e, 6)
    assert kept.tolist() == [1, 0, 0, 1, 0, 1] and root.tolist() == [0, 0, 0, 3, 3, 5]
    # a one-way pair against the rank order removes nothing (3 was a root before 4 came), unless 4 is reached first
    kept, root = plm.collapse_of([(4, 3, 0)], 5)
    assert kept.tolist() == [1, 1, 1, 1, 1] and root.tolist() == [0, 1, 2, 3, 4]
    kept, root = plm.collapse_of([(4, 3, 0), (1, 4, 0)], 5)
    assert kept.tolist() == [1, 1, 1, 0, 0] and root.tolist() == [0, 1, 2, 1, 1]
    # adjacency: 1 was taken by 0 and takes nothing
    kept, root = plm.collapse_of([(0, 1, 0), (1, 2, 0)], 3, ALGO_ADJACENCY)
    assert kept.tolist() == [1, 0, 1] and root.tolist() == [0, 0, 2]


# ---- conditions, not measurements ----------------------------------------------------------------------

@pytest.mark.parametrize("kind,name", ALL_INPUTS)
def test_every_input_has_pairs_at_k_and_just_beyond(kind, name):
    inp = get(kind, name)
    at_k, at_k1 = plm.limit_pairs(inp)
    assert at_k > 0, "no pair at exactly k"
    if len(inp.umis) == 2:  # a store of two entries is one pair: at exactly k
        return
    if inp.k + 1 <= inp.L:
        assert at_k1 > 0, "no pair at exactly k + 1"
    else:  # every pair is within k: the largest distance there is stands in
        assert max(int(d.max()) for _, d in inp.dist) == inp.L
    if "_N" in name or name.startswith(("big", "growth")):
        assert inp.nm.any(), "an input with N holds none"
    else:
        assert not inp.nm.any() or name.startswith("dense_n129")


@pytest.mark.parametrize("kind,name", ALL_INPUTS)
def test_every_bucket_pairs_its_first_row_with_its_last_column(kind, name):
    """The last column of a task is a bucket's last entry: the first entry is within k of it."""
    inp = get(kind, name)
    for _, d in inp.dist:
        assert len(d) < 2 or d[0, -1] <= inp.k


@pytest.mark.parametrize("name", plm.PAIR_INPUTS)
def test_every_directional_input_has_all_three_kinds_of_pair(name):
    sym, one_way, neither = plm.direction_census(plm.pair_input(name), 0.5)
    assert sym > 0 and one_way > 0 and neither > 0, (sym, one_way, neither)


@pytest.mark.parametrize("kind,name", SEG_INPUTS)
def test_every_part_of_the_segment_index_finds_a_pair_alone(kind, name):
    if kind == "pair":
        inp, part_len = plm.pair_input(name), None
    else:
        inp, part_len = plm.store(name).inp, plm.store(name).part_len
    assert plm.seg_index_applies(min(inp.L, 21), inp.k)
    census = plm.seg_census(inp, part_len)
    assert len(census) == len(inp.off) - 1, "a bucket below seg_min"
    for alone, two_bins, two_parts in census:
        assert alone == set(range(inp.k + 1)), "parts that find a pair alone: %s" % sorted(alone)
        assert two_bins > 0, "no pair for the dedupe rule"
        if inp.k >= 2:  # (at k = 1 a pair that agrees on both parts is one UMI twice)
            assert two_parts > 0


@pytest.mark.parametrize("kind,name", [(k, n) for k, n in ALL_INPUTS if n.startswith("dense")])
def test_dense_inputs_overrun_the_stage(kind, name):
    inp = get(kind, name)
    assert (plm.pair_input(name) if kind == "pair" else plm.store(name)).dense
    assert plm.most_edges_of_a_row_task(inp) > EDGE_BUF
    if inp.L == 43:  # one 64 x 64 block of the wide kernel
        assert all((d <= inp.k).all() for _, d in inp.dist) and len(inp.umis) >= 128
    if kind == "store":
        got = set(np.unique(np.concatenate([np.triu(d, 1)[np.triu_indices(len(d), 1)] for _, d in inp.dist])).tolist())
        assert got >= (set(range(1, 9)) if inp.L == 8 else {1, 2, 30})


@pytest.mark.parametrize("kind,name", [(k, n) for k, n in ALL_INPUTS if n.startswith("growth")])
def test_growth_inputs_outgrow_the_first_list(kind, name):
    inp = get(kind, name)
    within = len(inp.edges(0.5, ALGO_CLUSTER, 0))
    assert within > GROWN
    if kind == "pair":  # ... in one part's share of every list that a context of its own is made for, whatever the split into three
        for p, algo, amf in plm.GROWTH_LISTS:
            assert len(inp.edges(p, algo, amf)) > 3 * GROWN, (p, algo, amf)


def test_shapes_of_the_cases():
    """The sizes and options the cases were chosen for."""
    for name in plm.PAIR_INPUTS:
        inp = plm.pair_input(name)
        sizes = np.diff(inp.off.astype(np.int64)).tolist()
        if name.startswith("chunk_sizes"):
            assert sizes == list(plm.CHUNK_SIZES) and not inp.opts
        elif name.startswith("chunk_1100"):
            assert sizes == [1100] and not inp.opts
        elif name.startswith("big"):
            assert sizes == [300, 2100] and inp.opts == plm.BIG
        elif name.startswith("seg"):
            assert 300 <= sizes[0] <= 380 and 600 <= sizes[1] <= 680 and inp.opts == plm.SEG_MIN, sizes
    for name in plm.STORES:
        st = plm.store(name)
        n = len(st.umis)
        assert n <= 380
        if "_n" in name and not name.startswith(("seg", "growth", "wide_seg")):
            assert n == int(name.split("_n")[1].split("_")[0]), (name, n)
        if st.seg:
            assert n >= 129 and st.opts["seg_min"] == 129
        if st.growth:
            assert sum(len(r) for r in st.rows) // 2 > GROWN
