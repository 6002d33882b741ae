"""The mask-only collapse's round 0 in the launch that gathers the private slots (gather_resolve_hook_kernel).

A call without root on the batched directional path has no flatten pass: lab[] = identity is stored by the entry
kernels beside label[], and one launch behind the unions takes every one-way pair -- those the pair kernels left in
their blocks' private slots (gather blocks: a pair is resolved to (root, root), stored at its place in the list and
hooked by the thread that finds that place) and those they appended to the list themselves (list blocks: resolved in
place, flagged entries skipped).  The rounds from 1 on, the check beside finalize and the host's continuation read
what that launch stored.

Every case asserts what tests/test_gpu_kept_only.py asserts (check / check_mask there): the mask and n_kept equal
the CPU oracle's, the same context's call with want_root = True and a context with collapse_kept_only = 0, and all
three calls report the same n_edges and n_candidates.  What an input is meant to hold (one-way pairs, symmetric
pairs, a chain's depth) is counted on the CPU from the UMIs and freqs before the GPU is asked.

n_rounds = 1 (the unions) + the rounds that ran: 2 says that round 0 ran and left changed[0] at 0."""
import functools

import numpy as np
import pytest

import chain_inputs as ci
import kept_only_inputs as ko
from helpers import canonical, clustered_bucket
from test_gpu_kept_only import check, context

pytestmark = pytest.mark.gpu

SEG_PRIV_CAP = 512  # edges of a private slot (umihip_internal.h)
SEG_MIN = 512       # smallest bucket of the segment index at default options
# a pair kernel grid of exactly seg_blocks one-wave blocks and nobody else's slots: the local and the super-bin
# kernel (which bring slots of their own) off
SLOTS = dict(seg_local=0, seg_super=0)


def pair_counts(umis, freq, k, p):
    """(one-way, symmetric) permitted pairs of one bucket, unordered"""
    adj = ci.permitted_pairs(umis, freq, k, p)
    return int((adj & ~adj.T).sum()), int((adj & adj.T).sum()) // 2


@functools.lru_cache(maxsize=None)
def segment_600():
    """One bucket of 600 clustered 12-base UMIs, just above seg_min: (umis, freq) in rank order"""
    return clustered_bucket(np.random.default_rng(68001), 600, 12, 0.0)


def test_one_way_pairs_only_in_private_slots():
    """One segment of 600 entries with a few dozen one-way pairs: no wave's edge stage fills (384 edges), so every
    pair is in a private slot and the list blocks find an empty list.  The same UMIs with all freqs equal have no
    one-way pair at all: round 0 must leave changed[0] at 0 (n_rounds = 2) and the mask is the sets' roots."""
    umis, freq = segment_600()
    assert SEG_MIN <= len(umis) <= 640
    one_way, sym = pair_counts(umis, freq, 1, 0.5)
    assert 24 <= one_way < 384 and sym > 0, (one_way, sym)
    st = check(ko.Batch("one", 12, 1, 0.5, [(umis, freq)]), {}, "segment of 600")
    assert st["n_edges"] == one_way + sym and st["n_rounds"] >= 3, st
    flat = ko.Batch("one", 12, 1, 0.5, [(umis, [1] * len(umis))])
    one_way, sym = pair_counts(umis, [1] * len(umis), 1, 0.5)
    assert one_way == 0 and sym > 0
    st = check(flat, {}, "segment of 600, freqs equal")
    assert st["n_edges"] == sym and st["n_rounds"] == 2, st


def three_classes(n):
    """7 / 3 / 1 in thirds of the rank order: at p = 0.5 two of three pairs are one-way, one in nine symmetric
    (tests/test_gpu_seg_super.py)"""
    return [7] * (n // 3) + [3] * (n // 3) + [1] * (n - 2 * (n // 3))


@functools.lru_cache(maxsize=None)
def clustered_one_way(n_reads):
    """The clustered one-way input of tests/test_gpu_seg_super.py at n_reads reads: (keys, freq, bucket_off, umis)"""
    from umi_collapse_rs_amd import synth
    st = synth.config2m(seed=31, n_reads=n_reads, umi_len=12, n_molecules=n_reads // 10, err=0.02)
    keys = st["keys"]
    umis = ["".join("ACGT"[(int(x) >> (3 * b)) & 3] for b in range(12)) for x in keys]
    return keys, np.array(three_classes(len(keys)), np.int32), st["bucket_off"], umis


class KeysBatch:
    """the interface of kept_only_inputs.Batch over staged keys"""

    def __init__(self, keys, fr, off, L, k, p):
        self.keys, self.fr, self.off, self.L, self.k, self.p = keys, fr, off, L, k, p
        self._ref = None

    def reference(self):
        import oracle as orc
        if self._ref is None:
            self._ref = np.asarray(orc.dedup_batch(self.keys, None, self.fr, self.off, self.L, self.k, self.p, 0, 0)[0]).astype(np.uint8)
            self._ref.setflags(write=False)
        return self._ref

    def run(self, ctx, want_root):
        return ctx.dedup_batch(self.keys, None, self.fr, self.off, self.L, self.k, self.p, 0, 0, want_root=want_root)


ONE_WAY_READS = 6000  # the fewest thousands of reads whose one-way pairs exceed two slots (asserted below)


@pytest.mark.parametrize("opts", [dict(SLOTS, seg_blocks=2), dict(seg_blocks=2, seg_local=0, seg_super_min=16)],
                         ids=["two-slots", "super-bins-too"])
def test_slots_and_list_at_once(opts):
    """The clustered one-way input, sized so that its one-way pairs do not fit the slots: with two pair-kernel blocks
    and no other kernel there are two slots of 512, the blocks flush their stages to the list on the way and leave
    the rest in their slots -- list blocks and gather blocks both have pairs.  (Second case: the super-bin kernel on
    as in test_gpu_seg_super.py, seg_super_min = 16; its waves bring slots of their own, so that case only has the
    pair kernel's share to say for itself.)"""
    keys, fr, off, umis = clustered_one_way(ONE_WAY_READS)
    one_way, sym = pair_counts(umis, fr.tolist(), 1, 0.5)
    assert one_way > 2 * SEG_PRIV_CAP and sym > 0, (one_way, sym)
    fewer = clustered_one_way(ONE_WAY_READS - 1000)
    assert pair_counts(fewer[3], fewer[1].tolist(), 1, 0.5)[0] <= 2 * SEG_PRIV_CAP
    st = check(KeysBatch(keys, fr, off, 12, 1, 0.5), opts, "clustered one-way %s" % opts)
    assert st["n_edges"] == one_way + sym and st["n_edges"] - sym > 2 * SEG_PRIV_CAP, st


def test_flagged_pairs_in_the_list():
    """A bucket of 300 (the tile kernel: its symmetric pairs go to the list flagged, its one-way pairs plain) next to
    a segment of 600 (one-way pairs in private slots): the list blocks skip the flagged entries and resolve the rest
    while the gather blocks work behind them."""
    mid = clustered_bucket(np.random.default_rng(68002), 300, 12, 0.0)
    assert 129 <= len(mid[0]) <= 511
    mid_one_way, mid_sym = pair_counts(mid[0], mid[1], 1, 0.5)
    seg_one_way, seg_sym = pair_counts(*segment_600(), 1, 0.5)
    assert mid_one_way > 0 and mid_sym > 0 and seg_one_way > 0
    st = check(ko.Batch("one", 12, 1, 0.5, [mid, segment_600()]), {}, "tile bucket and segment")
    assert st["n_edges"] == mid_one_way + mid_sym + seg_one_way + seg_sym, st


@functools.lru_cache(maxsize=None)
def six_bases():
    """~2,100 UMIs over 6 free bases (the shape of test_gpu_parity.py::test_edge_list_overflow_in_adjacency_mode) with
    freqs 7 / 3 / 1 at p = 0.5: two of three pairs are one-way, some 6,500 of them.  (batch, one-way, symmetric)"""
    from umi_collapse_rs_amd import synth
    bases = synth.uniform_reads(seed=8, n_reads=3000, umi_len=12)
    bases[:, 6:] = 0
    s = synth.stage(np.zeros(len(bases), dtype=np.int64), synth.bases_to_keys(bases))
    keys, off = s["keys"], s["bucket_off"]
    fr = np.array(three_classes(len(keys)), np.int32)
    assert 2000 <= len(keys) <= 2200
    umis = ["".join("ACGT"[(int(x) >> (3 * b)) & 3] for b in range(12)) for x in keys]
    return (KeysBatch(keys, fr, off, 12, 1, 0.5),) + pair_counts(umis, fr.tolist(), 1, 0.5)


@pytest.mark.parametrize("opts", [dict(edge_capacity=1), dict(SLOTS, seg_blocks=2, edge_capacity=1)],
                         ids=["default-grid", "two-slots"])
def test_retry_starts_from_an_identity_lab(opts):
    """six_bases, directional, against the list's floor of 1,024: the first attempt's round 0 hooks the pairs that
    fit (labels fall: most entries sit in one set that the freq-7 entries reach) and the host then sees the count.
    The second attempt's lab[] must be the identity again.  Then the same call once more on the grown list."""
    batch, one_way, _ = six_bases()
    assert one_way > 4 * 1024
    with context(opts) as ctx, context(dict(opts, collapse_kept_only=0)) as old:
        st = check(batch, opts, "overflow, first call", ctx, old)
        assert st["n_edges"] > 4 * 1024 and st["n_rounds"] >= 3, st
        st2 = check(batch, opts, "overflow, second call", ctx, old)
        assert st2["n_edges"] == st["n_edges"] and st2["n_rounds"] == st["n_rounds"]


LADDER = 64  # nodes of the step2 ladder over 21 bases


@functools.lru_cache(maxsize=None)
def forest_and_ladder():
    """p = 1.0, one bucket.  The 64-node step2 ladder (freq 128, 126, ..., 2: 63 one-way pairs in a row, its last
    node T * 21) and some 1,400 UMIs of freq 1 and 3 that are T * 15 and six uniform bases: the freq-1 entries are one
    set (every pair among them is symmetric; the unions of a set that size leave parent chains tens deep), the
    freq-3 entries reach it by one-way pairs that end anywhere in that forest, and the ladder's end is in it."""
    rng = np.random.default_rng(68003)
    ladder = ci.chain("step2", 21, 1)
    assert ladder.n == LADDER and ladder.umis[-1] == "T" * 21
    tails = {"".join("ACGT"[c] for c in r) for r in rng.integers(0, 4, (1700, 6))}
    crowd = sorted("T" * 15 + t for t in tails if "T" * 15 + t not in ladder.umis)[:1500]
    rng.shuffle(crowd)
    freq = [3 if i % 8 == 0 else 1 for i in range(len(crowd))]
    umis, freq, _ = canonical(list(ladder.umis) + crowd, list(ladder.freq) + freq)
    return umis, freq


def test_deep_forest_and_deep_chain():
    """The continuation rounds run over pairs that round 0 resolved in a forest it had to climb: more rounds than the
    host enqueues ahead (n_rounds > 17, the threshold of test_gpu_kept_only.py::test_continuation_after_the_first_look)."""
    umis, freq = forest_and_ladder()
    adj = ci.permitted_pairs(umis, freq, 1, 1.0)
    hops = ci.hops_from_rank0(adj)
    assert max(hops) >= 20 and int((adj & ~adj.T).sum()) >= 20 + 100
    low = np.array(freq) == 1
    assert (adj & adj.T)[np.ix_(low, low)].sum() // 2 > low.sum()  # (the freq-1 entries: more pairs than a tree has)
    st = check(ko.Batch("one", 21, 1, 1.0, [(umis, freq)]), {}, "forest and ladder")
    assert st["n_rounds"] > 17, st


SEG_SMALL = dict(fused_max=0, seg_min=2)  # every bucket a segment, whatever its size


def test_roots_above_and_below():
    """late_label_batch: a pair u -> v whose source's root has the larger index -- round 0 resolves it to (u, a) with
    a < u and moves nothing, the label comes down to u later and the resolved pair must carry it on.
    self_edge_batch: a one-way pair whose endpoints share a root resolves to (root, root) and moves nothing.  Both in
    segments (seg_min = 2), so the pairs sit in private slots."""
    st = check(ko.late_label_batch(), SEG_SMALL, "late label")
    assert st["n_rounds"] >= 4, st
    assert ko.late_label_batch().reference()[:1 + ko.LATE_FEED + ko.LATE_SET].sum() == 1
    st = check(ko.self_edge_batch(), SEG_SMALL, "self edge")
    assert st["n_edges"] > 0


def test_state_on_the_context():
    """mask-only, with root (whose flatten pass writes lab[] itself and leaves it lowered), mask-only again, then a
    different, smaller input: lab[] of the call before must not show."""
    first = ko.Batch("one", 12, 1, 0.5, [segment_600(), clustered_bucket(np.random.default_rng(68004), 300, 12, 0.0)])
    small = ko.Batch("one", 12, 1, 0.5, [clustered_bucket(np.random.default_rng(68005), 520, 12, 0.0)])
    with context({}) as ctx, context(dict(collapse_kept_only=0)) as old:
        st = check(first, {}, "first input", ctx, old)           # mask-only, then with root
        st_b = check(first, {}, "first input again", ctx, old)   # mask-only behind the call with root
        assert st_b["n_edges"] == st["n_edges"] and st_b["n_rounds"] == st["n_rounds"]
        check(small, {}, "smaller input", ctx, old)
        check(ko.late_label_batch(), {}, "another, fused buckets", ctx, old)
        check(first, {}, "first input, third time", ctx, old)


@pytest.mark.parametrize("slots", [1, 63, 65, 129])
def test_group_edges(slots):
    """The gather blocks take 64 slots each; at the default grid the slot count is a multiple of 64.  seg_blocks pair
    kernel blocks and no other kernel's slots: one group of 1, one of 63, a full one and one of 1, two full ones and
    one of 1, the clustered one-way input's pairs spread over them."""
    keys, fr, off, umis = clustered_one_way(3000)
    one_way, sym = pair_counts(umis, fr.tolist(), 1, 0.5)
    assert one_way > 129 and len(keys) // 7 + 64 >= 129  # (the planner's bound of the pair kernel's tasks caps its grid)
    st = check(KeysBatch(keys, fr, off, 12, 1, 0.5), dict(SLOTS, seg_blocks=slots), "%d slots" % slots)
    assert st["n_edges"] == one_way + sym, st


@pytest.mark.parametrize("slots", [24, 65])
def test_many_pairs_in_one_group(slots):
    """A group's pairs are dealt to eight blocks in chunks of 512.  six_bases over 24 slots: some 270 pairs per slot on average
    (below the 384 at which a wave's stage goes to the list) and 6,500 in the one group -- more than eight chunks, so
    the blocks come round to a second chunk, the last one ragged.  Over 65 slots: 100 per slot, a first group of
    6,400 and a second of one slot."""
    batch, one_way, sym = six_bases()
    assert one_way > 8 * 512 + 512 and one_way // slots < 384 * 3 // 4
    st = check(batch, dict(SLOTS, seg_blocks=slots), "six bases over %d slots" % slots)
    assert st["n_edges"] == one_way + sym, st


def test_no_segment_at_all():
    """Only tile-kernel buckets (129..511 entries) and fused ones: no private slot, no gather block; lab[] comes from
    prep_kernel, and the list blocks do all of round 0."""
    rng = np.random.default_rng(68006)
    buckets = [clustered_bucket(rng, n, 12, 0.0) for n in (300, 40, 500, 129)]
    one_way = sum(pair_counts(u, f, 1, 0.5)[0] for u, f in buckets if len(u) > 128)
    assert one_way > 0 and all(len(u) < SEG_MIN for u, _ in buckets)
    st = check(ko.Batch("one", 12, 1, 0.5, buckets), {}, "tile buckets only")
    assert st["n_edges"] >= one_way and st["n_rounds"] >= 3, st
