"""Coarse filing of part 0 (option seg_super_coarse): in a segment with super-bins the counting sort files an entry
under the first bin of its run, seg_super_kernel counts the pairs inside the fine bins, and a run above the cap is one
sub-bucket for the tiles, whose drain keeps a hit only inside a fine bin.  None of this shows from outside except in
the results, so every case runs three ways -- seg_super_coarse 1, seg_super_coarse 0, seg_super 0 -- each against the
oracle bit for bit (kept, and root where the call has one), and n_edges, n_candidates, n_pairs_evaluated and n_kept
must be equal across the three.  Directional at p = 0.5 and p = 1.0, and connected components."""
import numpy as np
import pytest

import oracle as orc
from helpers import canonical
from test_gpu_seg_local import deep_bucket, join, mid_buckets
from test_gpu_seg_super import CLUSTER, COUNTED, MODES, base_of, bucket_of, oracle_of, super_sizes

pytestmark = pytest.mark.gpu

DEFAULTS = dict(seg_super=1, seg_super_coarse=1, seg_super_bases=0, seg_super_cap=5632, seg_super_min=1024)
WAYS = (dict(seg_super=1, seg_super_coarse=1), dict(seg_super=1, seg_super_coarse=0), dict(seg_super=0, seg_super_coarse=1))


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def call(c, batch, L, k, p, algo, want_root=True, **opts):
    keys, nm, fr, off = batch
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        return c.dedup_batch(keys, nm if nm.any() else None, fr, off, L, k, p, algo, 0, want_root=want_root)
    finally:
        for name, v in DEFAULTS.items():
            c.set_option(name, v)


def three_ways(c, name, batch, L, k=1, modes=MODES, want_root=True, **opts):
    """the three ways against the oracle; the counted statistics equal.  Returns the coarse runs' statistics."""
    out = []
    for p, algo in modes:
        okept, oroot = oracle_of(name, batch, L, k, p, algo)
        sts = []
        for way in WAYS:
            kept, root, st = call(c, batch, L, k, p, algo, want_root, **dict(opts, **way))
            what = "%s p=%g algo=%d %s %s" % (name, p, algo, way, opts)
            assert (kept == okept).all(), "%s: kept differs at %s" % (what, np.nonzero(kept != okept)[0][:10])
            if want_root:
                assert (root == oroot).all(), "%s: root differs at %s" % (what, np.nonzero(root != oroot)[0][:10])
            else:
                assert root is None, what
            assert st["n_kept"] == int(okept.sum()), what
            sts.append(st)
        for f in COUNTED:
            assert sts[0][f] == sts[1][f] == sts[2][f], (name, p, algo, opts, f, [st[f] for st in sts])
        out.append(sts[0])
    return out


def codes2(keys, L):
    """2 bits per base, base b at bits 2b (the filter key of a key without N)"""
    c = np.zeros(len(keys), np.int64)
    for b in range(L):
        c |= base_of(keys, b) << (2 * b)
    return c


def near_pairs(code, bases_a, bases_b=None):
    """ordered pairs of entries that differ in exactly one base of bases_a (and, if given, in exactly one of bases_b
    as well) and in nothing else"""
    n = 0
    for ba in bases_a:
        for da in (1, 2, 3):
            va = code ^ (da << (2 * ba))
            if bases_b is None:
                n += int(np.isin(va, code).sum())
                continue
            for bb in bases_b:
                for db in (1, 2, 3):
                    n += int(np.isin(va ^ (db << (2 * bb)), code).sum())
    return n


@pytest.fixture(scope="module")
def l10():
    return deep_bucket(np.random.default_rng(700), 40000, 10)


def test_l10_one_bucket_of_16_super_bins(ctx, l10):
    """~39,000 distinct UMIs of 10 bases: g = 3, 16 super-bins of ~2,450 entries in 64 fine bins each"""
    sizes = super_sizes(l10[0], 5, 3)
    assert sizes.min() >= 2 and sizes.max() <= 5632 * 3 // 4
    sts = three_ways(ctx, "l10", l10, 10)
    assert sts[0]["n_edges"] > 0


def test_l12_many_small_super_bins_per_block(ctx):
    """positions of ~40,000 and ~20,000 at L = 12 with seg_super_min = 64: g = 1, super-bins of ~156 and ~78 entries in
    4 fine bins, many of them per index block and per block of seg_super_kernel"""
    rng = np.random.default_rng(701)
    l12 = join(deep_bucket(rng, 40000, 12), deep_bucket(rng, 20000, 12))
    three_ways(ctx, "l12", l12, 12, seg_super_min=64)


def test_super_bins_above_and_below_the_cap(ctx):
    """L = 10 with one crowded super-bin (bases 3 and 4 = AA, ~4,600 entries) above a cap of 2,048 among fifteen below
    it.  The crowded one is a single sub-bucket of 64 fine bins for the tiles, whose compare keys leave out bases
    0..4.  It holds pairs that differ in one base of 0..2 alone -- two fine bins, one part-1 bin: the tile queues them,
    the drain's mask[0] test drops them, part 1 reports them (the flag word is set: today's dedupe rule) -- and pairs
    that differ in one base of 0..2 and one of 5..9: distance 2, queued by the tile and rejected."""
    rng = np.random.default_rng(702)
    raw = rng.integers(0, 4, (21600, 10))
    raw[18000:, 3:5] = 0
    batch = bucket_of(raw, rng)
    cap = 2048
    sizes = super_sizes(batch[0], 5, 3)
    assert (sizes > cap).sum() == 1 and (sizes <= cap).sum() == 15 and sizes[0] > cap
    code = codes2(batch[0], 10)
    crowded = code[(code >> 6) & 15 == 0]
    assert len(crowded) == sizes[0]
    assert near_pairs(crowded, (0, 1, 2)) > 100          # other fine bin, same part-1 bin: distance 1
    assert near_pairs(crowded, (0, 1, 2), (5, 6, 7, 8, 9)) > 100  # other fine bin, distance 2
    assert near_pairs(crowded, (5, 6, 7, 8, 9)) > 100    # same fine bin: part 0's own pairs
    sts = three_ways(ctx, "l10_mixed", batch, 10, seg_super_cap=cap)
    assert sts[0]["n_edges"] > 0


def test_no_super_bin_taken(ctx):
    """L = 10 with base 3 fixed: four super-bins of ~4,800 entries, all above a cap of 4,096, twelve empty"""
    rng = np.random.default_rng(703)
    raw = rng.integers(0, 4, (20000, 10))
    raw[:, 3] = 0
    batch = bucket_of(raw, rng)
    sizes = super_sizes(batch[0], 5, 3)
    assert ((sizes == 0) | (sizes > 4096)).all() and 1024 <= len(batch[0]) // 16 <= 4096 // 4 * 3
    three_ways(ctx, "l10_none", batch, 10, seg_super_cap=4096)


def test_empty_single_and_last_fine_bin_runs(ctx):
    """L = 10, g = 3: a super-bin without entries, one with a single entry, and one whose entries all have GGG at bases
    0..2 -- the last of the run's 64 fine bins, filed under the first; the other thirteen as they come"""
    rng = np.random.default_rng(707)
    raw = rng.integers(0, 4, (24000, 10))
    sb = raw[:, 3] + 4 * raw[:, 4]
    raw = np.concatenate([raw[(sb != 5) & (sb != 9)], raw[sb == 9][:1]])
    sb = raw[:, 3] + 4 * raw[:, 4]
    raw[sb == 14, 0:3] = 2  # 'G': code 3
    batch = bucket_of(raw, rng)
    keys = batch[0]
    sizes = super_sizes(keys, 5, 3)
    assert sorted(sizes)[:2] == [0, 1] and 1024 <= len(keys) // 16 <= 5632 // 4 * 3
    code = codes2(keys, 10)
    runs = (code >> 6) & 15  # (bases 3 and 4)
    all_last = [r for r in range(16) if (runs == r).sum() > 1 and ((code[runs == r] & 63) == 63).all()]
    assert len(all_last) == 1 and (runs == all_last[0]).sum() > 500, all_last
    three_ways(ctx, "l10_edges_of_a_run", batch, 10)


def test_key_twice_in_a_super_bin(ctx):
    """a key twice in the input: its super-bin is walked pair by pair; the fine bins' pairs count the equal keys too"""
    rng = np.random.default_rng(704)
    keys, nm, fr, off = deep_bucket(rng, 20000, 10)
    again = rng.choice(np.nonzero(fr == 1)[0], 40, replace=False)
    k2 = np.concatenate([keys, keys[again]])
    f2 = np.concatenate([fr, np.ones(len(again), np.int32)])
    order = np.lexsort((np.arange(len(k2)), -f2))
    batch = (k2[order], np.zeros_like(k2), f2[order], np.array([0, len(k2)], np.uint64))
    assert len(np.unique(batch[0])) < len(batch[0])
    three_ways(ctx, "l10_twice", batch, 10)


def test_call_without_root(ctx, l10):
    """the mask-only tail"""
    three_ways(ctx, "l10", l10, 10, want_root=False)


def test_planned_and_unplanned_segments_in_one_batch(ctx):
    """a deep position with super-bins (g = 1 at seg_super_min = 64) between segments of ~900 and ~700 entries that
    leave 9 bases outside their bins -- no super-bins there: filed by fine bin as before, by the same blocks' kernels;
    then a call at k = 2 and a call with an N mask, neither planned at all"""
    rng = np.random.default_rng(706)
    batch = join(mid_buckets(rng, 4, 12, 900), deep_bucket(rng, 20000, 12), mid_buckets(rng, 2, 12, 700))
    three_ways(ctx, "l12_mixed_segments", batch, 12, seg_super_min=64)
    with_n = deep_bucket(rng, 20000, 10, 0.005)
    assert with_n[1].any()
    three_ways(ctx, "l10_n", with_n, 10, modes=MODES[:1])
    three_ways(ctx, "l12_k2", deep_bucket(rng, 20000, 12), 12, k=2, modes=MODES[:1])


def test_segment_of_two_index_blocks_and_three_entries(ctx):
    """8,192 x 2 + 3 entries: three blocks of the counting sort, the last with three entries"""
    rng = np.random.default_rng(708)
    umis = sorted({"".join("ACGT"[c] for c in r) for r in rng.integers(0, 4, (17500, 10))})
    rng.shuffle(umis)
    umis = umis[:8192 * 2 + 3]
    assert len(umis) == 8192 * 2 + 3
    fr = np.minimum(rng.geometric(0.5, len(umis)), 40).tolist()
    umis, fr, _ = canonical(umis, fr)
    keys, nm = orc.encode_keys(umis)
    batch = (keys, nm, np.array(fr, np.int32), np.array([0, len(umis)], np.uint64))
    assert 1024 <= len(umis) // 16
    sts = three_ways(ctx, "l10_16387", batch, 10)
    assert sts[0]["n_edges"] > 0


def test_64_bit_keys_are_not_planned(ctx):
    """L = 20: 64-bit filter keys, no super-bins -- result and counters as they were, whatever the option says"""
    rng = np.random.default_rng(709)
    batch = join(mid_buckets(rng, 3, 20, 700), deep_bucket(rng, 20000, 20))
    three_ways(ctx, "l20", batch, 20)
    three_ways(ctx, "l20", batch, 20, k=2, modes=MODES[:1])


def test_option_bounds(ctx):
    import umi_collapse_rs_amd as umi
    for v in (-1, 2):
        with pytest.raises(umi.UmiHipError):
            ctx.set_option("seg_super_coarse", v)
    for v in (0, 1):
        ctx.set_option("seg_super_coarse", v)
