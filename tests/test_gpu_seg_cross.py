"""The pairs between super-bins read off the super-bins' rest-code maps (seg_cross_kernel, options seg_cross and
seg_cross_map_mb): every case three ways -- seg_cross 1, seg_cross 0, seg_super 0 -- against the oracle, kept and root
bit for bit, with root and without, directional at p = 0.5 and p = 1.0 and as connected components; the counted
statistics equal across the three, and n_candidates what the model of tests/seg_cross_inputs.py says (every pair at
distance 1, once).  The inputs are checked on the CPU in tests/test_seg_cross_inputs_cpu.py."""
import numpy as np
import pytest

import oracle as orc
import seg_cross_inputs as sci
from test_gpu_seg_local import deep_bucket, join, mid_buckets

pytestmark = pytest.mark.gpu

CLUSTER = 2  # UMI_ALGO_CLUSTER
MODES = [(0.5, 0), (1.0, 0), (0.5, CLUSTER)]
DEFAULTS = dict(seg_super=1, seg_super_bases=0, seg_super_cap=5632, seg_super_min=1024, grid_cus=0, seg_cross_map_mb=8,
                seg_cross=1)
WAYS = (dict(seg_cross=1, seg_super=1), dict(seg_cross=0, seg_super=1), dict(seg_cross=1, seg_super=0))
COUNTED = ("n_edges", "n_candidates", "n_pairs_evaluated", "n_kept")
SAME = COUNTED + ("n_pair_launches", "kernel_id")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


@pytest.fixture()
def fresh():
    """a context of its own, with the options a case wants from its first call on"""
    import umi_collapse_rs_amd as umi
    made = []

    def make(**opts):
        c = umi.Context(0)
        made.append(c)
        for name, v in opts.items():
            c.set_option(name, v)
        return c
    yield make
    for c in made:
        c.close()


_oracle = {}


def oracle_of(name, batch, L, k, p, algo):
    key = (name, L, k, p, algo)
    if key not in _oracle:
        keys, nm, fr, off = batch
        _oracle[key] = orc.dedup_batch(keys, nm, fr, off, L, k, float("inf") if algo == CLUSTER else p, 0, 0)[:2]
    return _oracle[key]


def call(c, batch, L, k, p, algo, want_root=True, **opts):
    keys, nm, fr, off = batch
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        return c.dedup_batch(keys, nm if nm.any() else None, fr, off, L, k, p, algo, 0, want_root=want_root)
    finally:
        for name, v in DEFAULTS.items():  # ("seg_cross" last: armed again whatever the call met)
            c.set_option(name, v)


def check(what, got, okept, oroot):
    kept, root, st = got
    assert (kept == okept).all(), "%s: kept differs at %s" % (what, np.nonzero(kept != okept)[0][:10])
    assert root is None or (root == oroot).all(), "%s: root differs at %s" % (what, np.nonzero(root != oroot)[0][:10])
    assert st["n_kept"] == int(okept.sum()), what
    return st


def counters(c):
    return c.counter("seg_cross_launches"), c.counter("seg_cross_abandoned")


def three_ways(c, name, batch, L, k=1, modes=MODES, candidates=None, path="runs", **opts):
    """Returns the statistics of the seg_cross = 1 runs with root, one per mode.  path: what the context's counters must
    say of the seg_cross = 1 call -- "runs": seg_cross_kernel launched (once per attempt), nothing abandoned;
    "abandoned": launched once and the call fell back; "not planned": neither.  The other two ways never launch it."""
    out = []
    for p, algo in modes:
        okept, oroot = oracle_of(name, batch, L, k, p, algo)
        for want_root in (True, False):
            sts = []
            for i, way in enumerate(WAYS):
                before = counters(c)
                sts.append(check("%s p=%g algo=%d root=%d %s %s" % (name, p, algo, want_root, way, opts),
                                 call(c, batch, L, k, p, algo, want_root, **dict(opts, **way)), okept, oroot))
                launched, abandoned = (x - y for x, y in zip(counters(c), before))
                what = (name, p, algo, want_root, way, path, launched, abandoned)
                if i or path == "not planned":
                    assert (launched, abandoned) == (0, 0), what
                elif path == "abandoned":
                    assert (launched, abandoned) == (1, 1), what
                else:
                    assert 1 <= launched <= sts[0]["n_pair_launches"] and abandoned == 0, what
            for f in COUNTED:
                assert sts[0][f] == sts[1][f] == sts[2][f], (name, p, algo, want_root, opts, f, [s[f] for s in sts])
            for f in SAME:  # (seg_super = 0 walks its part 0 by another kernel: the launches may differ there)
                assert sts[0][f] == sts[1][f], (name, p, algo, want_root, opts, f, sts[0][f], sts[1][f])
            if candidates is not None:
                assert sts[0]["n_candidates"] == candidates, (name, sts[0]["n_candidates"], candidates)
            if want_root:
                out.append(sts[0])
    return out


def model_counts(batch, shape):
    """(cross pairs, all pairs at distance 1) of a one-bucket input"""
    return len(sci.cross_pairs(batch[0], shape["L"], shape["nb0"], shape["g"])), sci.neighbours(batch[0], shape["L"])


@pytest.mark.parametrize("partners", [None, [4, 13]])
def test_lone_entry_and_its_partners(ctx, partners):
    """super-bins of one entry at both ends of a pair, empty super-bins among the partners', partners above and below
    the entry's code in both shared bases at d = 1, 2, 3: found once each (n_candidates is the model's count)"""
    batch, shape, n_partners = sci.lone_entry_with_all_partners(partners=partners)
    n_cross, n_all = model_counts(batch, shape)
    assert n_cross >= n_partners
    three_ways(ctx, "lone%s" % (partners,), batch, 10, candidates=n_all)


def test_first_and_last_bits_of_the_map(ctx):
    """hits at bit 0 and bit 31 of the first and of the last word, ranks behind every other entry; with one CU's 16
    blocks as well, so that every block takes a whole super-bin's 32 chunks and its queue lives across them"""
    batch, shape = sci.map_edges()
    n_all = model_counts(batch, shape)[1]
    three_ways(ctx, "map_edges", batch, 10, candidates=n_all)
    three_ways(ctx, "map_edges", batch, 10, candidates=n_all, modes=MODES[:1], grid_cus=1)


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 128, 200])
def test_queue_of_one_wave(ctx, m):
    """m hits from one 64-word chunk of one pair of maps: the queue at 0, 1, one short of a drain, a drain exactly,
    one and many beyond"""
    batch, shape = sci.queue_fill(m)
    three_ways(ctx, "queue%d" % m, batch, 10, candidates=model_counts(batch, shape)[1], modes=MODES[:1] + MODES[2:])


def test_maps_of_fewer_than_2048_words(ctx):
    """L = 10 at g = 2: rest-codes of 7 bases, 64 super-bins, three shared bases, maps of 512 words"""
    batch = sci.uniform(20000, 10, seed=1)
    assert sci.shape_of(len(batch[0]), 10, g=2, smin=64) == (5, 2)
    three_ways(ctx, "l10_g2", batch, 10, candidates=sci.neighbours(batch[0], 10), seg_super_bases=2, seg_super_min=64)


def test_l12_many_super_bins(ctx):
    """L = 12, ~40,000: g = 1, 256 super-bins of ~156 entries with four shared bases, rest-codes of 8 bases"""
    batch = sci.uniform(40000, 12, seed=2)
    assert sci.shape_of(len(batch[0]), 12, smin=64) == (5, 1)
    sts = three_ways(ctx, "l12", batch, 12, candidates=sci.neighbours(batch[0], 12), seg_super_min=64)
    assert sts[0]["n_edges"] > 0


def test_one_super_bin_for_the_segment(ctx):
    """g = nb0: no shared base, no cross pair, no part 1 filed -- still right"""
    batch = sci.uniform(5400, 8, seed=3)
    assert sci.shape_of(len(batch[0]), 8, cap=8192) == (4, 4)
    three_ways(ctx, "l8_one", batch, 8, candidates=sci.neighbours(batch[0], 8), seg_super_cap=8192)


def test_one_way_pairs_beyond_a_blocks_slot(ctx):
    """three classes of freq, one CU's 16 blocks, a super-bin each: more one-way pairs than the 512 of a private slot"""
    batch, shape = sci.dense_one_way()
    sts = three_ways(ctx, "l8_dense", batch, 8, candidates=model_counts(batch, shape)[1], modes=MODES[:2], grid_cus=1,
                     seg_super_cap=2048)
    # (n_edges counts the united pairs too: that one block's one-way pairs pass its slot of 512 is shown on the CPU,
    # tests/test_seg_cross_inputs_cpu.py::test_dense_one_way; here only that the call is the dense one)
    assert sts[0]["n_edges"] > 16 * 512


def test_edge_list_runs_over_with_the_path_on(fresh):
    """edge_capacity = 1: the first attempt's list of 1,024 runs over, the pair work is done again with the path on
    and nothing is counted twice"""
    batch, shape = sci.dense_one_way()
    okept, oroot = oracle_of("l8_dense", batch, 8, 1, 0.5, 0)
    sts = []
    for way in WAYS[:2]:
        c = fresh(edge_capacity=1, **way)
        keys, nm, fr, off = batch
        sts.append(check("overflow %s" % way, c.dedup_batch(keys, None, fr, off, 8, 1, 0.5, 0, 0), okept, oroot))
    assert sts[0]["n_edges"] > 1024 and sts[0]["n_candidates"] == model_counts(batch, shape)[1]
    for f in SAME:
        assert sts[0][f] == sts[1][f], (f, sts[0][f], sts[1][f])


def test_segments_with_and_without_the_path_in_one_call(ctx):
    """a deep bucket planned with the path, one without super-bins (~3,000 entries: three bin bases leave ten outside),
    mid-size segments and small buckets for the fused kernel: seg_pair_kernel and seg_cross_kernel in one call"""
    rng = np.random.default_rng(1270)
    batch = join(mid_buckets(rng, 3, 10, 40), sci.uniform(20000, 10, seed=4), mid_buckets(rng, 2, 10, 900),
                 sci.uniform(3000, 10, seed=5), mid_buckets(rng, 3, 10, 30))
    assert sci.shape_of(3000, 10)[1] == 0
    sts = three_ways(ctx, "l10_mixed_call", batch, 10)
    assert sts[0]["n_edges"] > 0


def fallback_case(fresh, name, batch, L, overflow=False, **opts):
    """a call the path is abandoned in: results as the oracle's, statistics as those of a context with seg_cross = 0
    that makes the same calls in the same order -- the first call of a context, its next calls (planned without the
    path), and calls after the option has armed the path again; once with root in the first call, once without.
    overflow: edge_capacity = 1 -- the edge list of 1,024 runs over in the first call's attempts (a context keeps the
    list it grew: only its first call meets the short one)."""
    keys, nm, fr, off = batch
    first = dict(opts, edge_capacity=1) if overflow else opts
    for p, algo in MODES:
        okept, oroot = oracle_of(name, batch, L, 1, p, algo)
        for root_first in (True, False):
            ref, c = fresh(seg_cross=0, **first), fresh(**first)
            tried = 0
            for turn, want_root in (("first", root_first), ("next", True), ("next", False), ("armed again", True),
                                    ("armed again", False)):
                if (turn, want_root) == ("armed again", True):  # (once: the call behind it finds the path off again)
                    c.set_option("seg_cross", 1)
                what = "%s %s p=%g algo=%d root=%d/%d" % (name, turn, p, algo, root_first, want_root)
                want = check(what + " seg_cross=0", ref.dedup_batch(keys, None, fr, off, L, 1, p, algo, 0, want_root=want_root),
                             okept, oroot)
                st = check(what, c.dedup_batch(keys, None, fr, off, L, 1, p, algo, 0, want_root=want_root), okept, oroot)
                for f in SAME:
                    assert st[f] == want[f], (what, f, st[f], want[f])
                # one wasted attempt per context and arming: the first call tries the path and falls back, the next
                # calls do not try it, the first call after the option is set again does, the one behind it does not
                tried += 1 if (turn, want_root) in (("first", root_first), ("armed again", True)) else 0
                assert counters(c) == (tried, tried) and counters(ref) == (0, 0), (what, counters(c), tried)
                if overflow and turn == "first" and algo != CLUSTER:  # (connected components list no one-way pair)
                    assert want["n_edges"] > 1024 and want["n_pair_launches"] >= 2, (what, want)
            ref.close()
            c.close()


def test_fallback_key_twice(fresh):
    fallback_case(fresh, "l10_twice", sci.with_key_twice(sci.uniform(20000, 10, seed=6)), 10)


def test_fallback_super_bin_above_the_cap(fresh):
    batch, _ = sci.crowded_super_bin()
    fallback_case(fresh, "l10_crowded", batch, 10, seg_super_cap=2048)


def test_fallback_with_an_overflowing_edge_list(fresh):
    """a key twice, a super-bin above the cap and a list that runs over, all in the first attempt"""
    batch, _ = sci.crowded_super_bin(freq=sci.three_classes)
    fallback_case(fresh, "l10_crowded_twice", sci.with_key_twice(batch, seed=1), 10, overflow=True, seg_super_cap=2048)


def test_fallback_in_a_call_with_mid_size_buckets(fresh):
    """buckets of ~300 entries (above the fused kernel's 128, below the segment index's 512: pair_kernel chunks, a
    launch of their own in every attempt) beside the deep bucket that falls back: the abandoned attempt's launches, all
    of them, are not the call's"""
    mids = [sci.uniform(300, 10, seed=20 + i) for i in range(3)]
    assert all(129 <= len(m[0]) <= 511 for m in mids)
    batch = join(mids[0], sci.with_key_twice(sci.uniform(20000, 10, seed=6)), mids[1], mids[2])
    fallback_case(fresh, "l10_twice_mids", batch, 10)


def test_a_good_call_behind_a_fallback(ctx):
    """the module's context: abandoned, then (armed by call()'s defaults) the path again on a call it serves"""
    twice = sci.with_key_twice(sci.uniform(20000, 10, seed=6))
    three_ways(ctx, "l10_twice", twice, 10, modes=MODES[:1], path="abandoned")
    batch, shape = sci.map_edges()
    three_ways(ctx, "map_edges", batch, 10, candidates=model_counts(batch, shape)[1], modes=MODES[:1])


def test_calls_the_path_is_not_planned_for(ctx):
    """an N mask; 14 bases (no super-bins at this size, and maps of 32 MB if there were); seg_cross_map_mb = 0"""
    rng = np.random.default_rng(1280)
    with_n = deep_bucket(rng, 20000, 10, 0.005)
    assert with_n[1].any()
    three_ways(ctx, "l10_n", with_n, 10, modes=MODES[:1], path="not planned")
    three_ways(ctx, "l14", sci.uniform(20000, 14, seed=7), 14, modes=MODES[:1], path="not planned")
    three_ways(ctx, "l10_no_maps", sci.uniform(20000, 10, seed=1), 10, modes=MODES[:1], seg_cross_map_mb=0, path="not planned")


def test_option_bounds(ctx):
    import umi_collapse_rs_amd as umi
    for name, values in {"seg_cross": (-1, 2), "seg_cross_map_mb": (-1, 65)}.items():
        for v in values:
            with pytest.raises(umi.UmiHipError):
                ctx.set_option(name, v)
    for name, v in list(dict(seg_cross_map_mb=64, seg_cross=0).items()) + list(DEFAULTS.items()):
        ctx.set_option(name, v)
