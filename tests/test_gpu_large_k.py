"""k > 3 on every pair kernel, and the edge-list retry away from the one-word path.

Every bucket is built from centres with copies at planted distances k-1 .. k+2 (helpers.planted_bucket),
and every case is checked on the CPU to hold pairs at exactly k and k + 1 (tests/test_large_k_inputs_cpu.py
runs those checks for all cases without a GPU; the cases here repeat them before they call the library).

What covers what (code that depends on k -> tests here):
  fused kernel, sliced body for k <= 3 / column-walking body above, lim = 2k + 1
      test_one_word_boundary, test_one_word_huge_k: the buckets of 2..128 entries under {} and fused_sliced = 0
  tile / chunk kernel, lim = 2k
      the same tests: buckets of 129..1024 entries, and all of them under fused_max = 0 / seg_index = 0
  segment index applies or falls back (k + 1 <= 8, L / (k + 1) >= 3)
      test_one_word_boundary: (21,6) (20,6) (18,5) (15,4) (12,3) on, (21,7) (17,5) (14,4) (11,3) off, asserted
      through n_pairs_evaluated
  segment pair and local kernels, broadcast body for k > 3, lim2 = 2k
      test_one_word_boundary under {}, seg_sliced / seg_ckey / seg_unite / seg_local / seg_lds = 0, seg_min = 129
  wide keys: k > 3 switches the wide fused kernel off
      test_wide_keys
  whole reads: clamp at 400, partition while L / (k + 1) >= 8, exactly-once over up to 32 parts
      test_whole_reads (n_candidates / n_edges against the model: a pair decided in two bins counts twice)
  DataStruct path, max_edits > 3
      test_hipnaive_large_max_edits
  edge-list overflow and redo away from the one-word path
      test_edge_list_overflow_wide, test_edge_list_overflow_whole_reads
  k >= 2^30 (2k wraps in an int)
      test_one_word_huge_k, test_wide_keys, test_whole_reads, test_hipnaive_large_max_edits

Mutation check (each change made alone on a scratch copy, the first test here that turned red):
  umihip_kernels.hip tile kernel  lim = 2k -> 2k - 1        test_one_word_boundary[21-7-0.0]
  umihip_kernels.hip fused kernel lim = 2k + 1 -> 2k + 2    test_one_word_boundary[21-7-0.0]  (and -> 2k - 1)
  umihip_seg.hip pair kernel      lim2 = 2k -> 2k - 1       test_one_word_boundary[12-3-0.0], {"seg_sliced": 0}
  umihip_seg.hip local kernel     lim2 = 2k -> 2k - 1       test_one_word_boundary[12-3-0.0], {"seg_sliced": 0}
  umihip_seg.hip within_k (64 bit) <= 2k -> <= 2k - 1       test_one_word_boundary[21-6-0.0]
  umihip_seq.hip lim = 2k + 2 -> 2k + 1 and -> 2k + 3       test_whole_reads[100-8]
  seq_pair_kernel earlier = 0                               test_whole_reads[150-16]  (n_candidates 1178, model 464)
  seg_index_applies >= 3 -> >= 2                            test_one_word_boundary[17-5-0.0]  (n_pairs_evaluated)
  the k > 3 term of the wide fused kernel's switch removed  test_wide_keys[22-4]
The tile kernel's lim, lim2 and within_k are filters over keys whose codes differ in exactly two bits or in
none, and every hit is decided again by the exact distance: 2k + 1 admits nothing that 2k does not, so the
step up changes no result and no counter, and the step down is the mutant that counts.  lim2 is only read
where compare keys are in use, which the planner allows for parts that leave 10 bases or fewer: with k > 3
that never holds, so k = 3 under seg_sliced = 0 is where it is reached.
"""
import numpy as np
import pytest

import helpers as h
import oracle as orc
import seq_model as sm

pytestmark = pytest.mark.gpu

LEGACY_SETS = [{"prune": 1}, {"bitslice": 0, "fused_max": 0}, {"bs_unit": 1, "small_max": 200, "seg_index": 0},
               {"seg_min": 129, "two_phase": 1}]
OPTION_SETS = [{}, {"seg_index": 0}, {"fused_max": 0}, {"fused_sliced": 0}, {"seg_sliced": 0}, {"seg_ckey": 0},
               {"seg_unite": 0}, {"seg_local": 0}, {"seg_lds": 0}, {"seg_min": 129}] + LEGACY_SETS
# k >= L - 1: every pair of a bucket is (nearly) an edge candidate and the segment index never applies, so
# the options that only steer the index (seg_*) are left out (the list of (L, k) cases is not shortened)
OPTION_SETS_HUGE = [{}, {"seg_index": 0}, {"fused_max": 0}, {"fused_sliced": 0}] + LEGACY_SETS
MODES = [(0, 0), (1, 0), (1, 2)]  # (algo, adj_max_freq)


def run_one_word(keys, nm, fr, off, L, k, option_sets):
    import umi_collapse_rs_amd as umi
    kk = min(k, L)
    census = h.limit_census(keys, nm, fr, off, kk)
    nmask = nm if nm.any() else None
    for algo, amf in MODES:
        okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, k, 0.5, algo, amf)
        if algo == 0:
            h.assert_k_decides(census, L, k, okept, orc.dedup_batch(keys, nm, fr, off, L, kk - 1)[0])
        for opts in option_sets:
            if not h.usable(opts):
                continue
            ctx = umi.Context(0)
            try:
                for name, v in opts.items():
                    ctx.set_option(name, v)
                kept, root, st = ctx.dedup_batch(keys, nmask, fr, off, L, k, 0.5, algo, amf)
            finally:
                ctx.close()
            assert (kept == okept).all(), (L, k, algo, amf, opts, np.nonzero(kept != okept)[0][:5])
            assert (root == oroot).all(), (L, k, algo, amf, opts)
            if algo == 1 and amf < 1:
                continue  # (the reference's adjacency needs no pairs: nothing is evaluated)
            index_on = h.seg_index_applies(L, k) and opts.get("seg_index", 1) and not (set(opts) & h.LEGACY_OPTS)
            if index_on:
                assert st["n_pairs_evaluated"] < st["n_pairs"], (L, k, opts, st)
            elif not set(opts) & h.LEGACY_OPTS:
                # all pairs, tile padding included (umihip.h): never fewer than the pairs there are
                assert st["n_pairs_evaluated"] >= st["n_pairs"], (L, k, opts, st)


@pytest.mark.parametrize("n_frac", [0.0, 0.01])
@pytest.mark.parametrize("L,k", h.ONE_WORD_BOUNDARY)
def test_one_word_boundary(L, k, n_frac):
    """(L, k) on both sides of seg_index_applies, every bucket size of the fused / chunk / deep kernels in one
    call, both algorithms, under every option set; which path ran is asserted through n_pairs_evaluated."""
    keys, nm, fr, off = h.one_word_batch(L, k, n_frac)
    run_one_word(keys, nm, fr, off, L, k, OPTION_SETS)


@pytest.mark.parametrize("n_frac", [0.0, 0.01])
@pytest.mark.parametrize("L,k", h.ONE_WORD_HUGE)
def test_one_word_huge_k(L, k, n_frac):
    """k = L - 1, L, L + 1 and the values around which 2 k and 2 k + 1 leave an int: the reference only
    ever asks dist <= k, so all of these are legal and from k = L on mean every pair of a bucket."""
    keys, nm, fr, off = h.one_word_batch(L, k, n_frac)
    assert np.diff(off.astype(np.int64)).max() <= 2000 or k < L  # (an edge list in the low millions at most)
    run_one_word(keys, nm, fr, off, L, k, OPTION_SETS_HUGE)


@pytest.mark.parametrize("L,k", h.WIDE_CASES)
def test_wide_keys(L, k):
    """umi_dedup_batch_wide at k > 3: positions of up to 128 entries, which the wide fused kernel no longer
    takes, one for the chunk kernel and a deep one (segment index on the first word for k <= 6, all pairs
    from k = 7 on, asserted); also all-pairs everywhere and sharded over three workers."""
    import umi_collapse_rs_amd as umi
    keys, nm, fr, off = h.wide_batch(L, k)
    kk = min(k, L)
    census = h.limit_census(keys, nm, fr, off, kk)
    assert np.diff(off.astype(np.int64)).max() >= 2000
    ctx, c2, multi = umi.Context(0), umi.Context(0), umi.Context([0, 0, 0])
    try:
        c2.set_option("seg_index", 0)
        c2.set_option("fused_max", 0)
        for algo, amf in MODES:
            okept, oroot, _ = orc.dedup_batch_wide(keys, nm, fr, off, L, k, 0.5, algo, amf)
            if algo == 0:
                h.assert_k_decides(census, L, k, okept, orc.dedup_batch_wide(keys, nm, fr, off, L, kk - 1)[0])
            kept, root, st = ctx.dedup_batch_wide(keys, nm, fr, off, L, k, 0.5, algo, amf)
            assert (kept == okept).all(), (algo, amf, np.nonzero(kept != okept)[0][:10])
            assert (root == oroot).all(), (algo, amf)
            kept2, root2, st2 = c2.dedup_batch_wide(keys, nm, fr, off, L, k, 0.5, algo, amf)
            assert (kept2 == okept).all() and (root2 == oroot).all(), (algo, amf)
            mk, mr, _ = multi.dedup_batch_wide(keys, nm, fr, off, L, k, 0.5, algo, amf)
            assert (mk == okept).all() and (mr == oroot).all(), (algo, amf)
            if algo == 1 and amf < 1:
                continue
            if h.seg_index_applies(21, k):  # the index looks at the first word's 21 bases
                assert st["n_pairs_evaluated"] < st["n_pairs"], st
            else:
                assert st["n_pairs_evaluated"] >= st["n_pairs"], st
            assert st2["n_pairs_evaluated"] >= st2["n_pairs"], st2
    finally:
        ctx.close(); c2.close(); multi.close()


# ---- whole reads -------------------------------------------------------------------------------------

def seq_pairs(buckets, k, join=False):
    """The pairs within k of every bucket, from the model (the same for every algorithm)."""
    out = []
    for seqs, _ in buckets:
        keys, nm = sm.encode(seqs, max(1, sm.words(len(seqs[0]))))
        out.append(sm.pairs_join(seqs, keys, nm, k) if join else sm.pairs_brute(keys, nm, k))
    return out


def seq_reference(buckets, all_pairs, k, algo, adj):
    """kept, root and the three counters of umi_dedup_seqs from the model: the pairs within k
    (n_candidates), those the algorithm permits in at least one direction (n_edges), and the pairs inside
    the bins of equal parts of the partitioned buckets / all pairs of the others (n_pairs_evaluated)."""
    kept, root, n_cand, n_edges, n_eval = [], [], 0, 0, 0
    base = 0
    for (seqs, freq), pairs in zip(buckets, all_pairs):
        n, L = len(seqs), len(seqs[0])
        kb, rb = sm.collapse(n, pairs, freq, algo, k, 0.5, adj)
        kept.append(kb); root.append(rb + base); base += n
        n_cand += len(pairs)
        f = np.array(freq)
        thr = np.array([sm.thr_f32(0.5, int(x)) for x in freq])
        for i, j in pairs:
            if algo == 0:
                n_edges += bool(f[j] <= thr[i] or f[i] <= thr[j])
            else:
                n_edges += bool(f[j] <= adj)
        if n >= 512 and h.seq_partitioned(L, k):
            P = min(k, 400) + 1
            arr = np.frombuffer(b"".join(seqs), np.uint8).reshape(n, L)
            for j in range(P):
                lo, hi = j * L // P, (j + 1) * L // P
                _, cnt = np.unique(np.ascontiguousarray(arr[:, lo:hi]).view(np.dtype((np.void, hi - lo))).ravel(),
                                   return_counts=True)
                n_eval += int((cnt * (cnt - 1) // 2).sum())
        else:
            n_eval += n * (n - 1) // 2
    return np.concatenate(kept), np.concatenate(root), n_cand, n_edges, n_eval


def call_seqs(ctx, buckets, k, algo, adj):
    from umi_collapse_rs_amd import to_bitset_seq
    seqs = [s for b in buckets for s in b[0]]
    freq = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    blen = [len(b[0][0]) for b in buckets]
    keys, nm = to_bitset_seq(seqs, max(sm.words(L) for L in blen))
    return ctx.dedup_seqs(keys, nm, freq, off, blen, k=k, percentage=0.5, algo=algo, adj_max_freq=adj)


def check_seqs(ctx, buckets, all_pairs, k, algo, adj):
    mk, mr, n_cand, n_edges, n_eval = seq_reference(buckets, all_pairs, k, algo, adj)
    kept, root, st = call_seqs(ctx, buckets, k, algo, adj)
    assert np.array_equal(kept.astype(bool), mk)
    assert np.array_equal(root, mr)
    if algo == 1 and adj < 1:
        return st  # (no pair work at all)
    assert st["n_candidates"] == n_cand  # a pair decided in two bins would count twice
    assert st["n_edges"] == n_edges
    assert st["n_pairs_evaluated"] == n_eval
    return st


@pytest.mark.parametrize("L,k", h.SEQ_CASES)
def test_whole_reads(L, k):
    """umi_dedup_seqs against seq_model: a pair, a bucket below 512 entries (all pairs) and one above (k + 1
    parts while a part has 8 bases: 150 / 18 and 256 / 32 still do, 150 / 19 and 256 / 33 do not; k = 31 at
    L = 256 uses all 32 bits of the exactly-once masks, with planted pairs equal in part 31 only and in part
    0 only).  kept / root bit-identical, and n_candidates, n_edges and n_pairs_evaluated equal to the model."""
    from umi_collapse_rs_amd import Context
    buckets = h.seq_buckets(L, k)
    kk = min(k, L)
    seqs = [s for b in buckets for s in b[0]]
    fr = [f for b in buckets for f in b[1]]
    off = np.cumsum([0] + [len(b[0]) for b in buckets])
    keys, nm = sm.encode(seqs, sm.words(L))
    ent = [(s, f, 0) for s, f in zip(seqs, fr)]
    h.assert_k_decides(h.limit_census(keys[2:], nm[2:], fr[2:], off[1:] - 2, kk), L, k, sm.dedup(ent, list(off), [L] * 3, kk)[0],
                       sm.dedup(ent, list(off), [L] * 3, kk - 1)[0])
    all_pairs = seq_pairs(buckets, k)
    if h.seq_partitioned(L, k):  # pairs equal in the last part only and in part 0 only are really there
        h.assert_tight_pigeonhole(buckets[2][0], all_pairs[2], k + 1)
    ctx = Context(0)
    try:
        for algo, adj in MODES:
            check_seqs(ctx, buckets, all_pairs, k, algo, adj)
    finally:
        ctx.close()


# ---- DataStruct path ---------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [12, 21, 24, 50])
def test_hipnaive_large_max_edits(L):
    import umi_collapse_rs_amd as umi
    rng = np.random.default_rng(40 + L)
    for max_edits in (4, 6, 8, L, 2 ** 31 - 1):
        umis, freq = h.planted_bucket(rng, 150, L, min(max_edits, L), 0.01, (21, 42))
        order = rng.permutation(len(umis))  # (a map has no rank order)
        umis, freq = [umis[i] for i in order], [freq[i] for i in order]
        d = umi.HipNaive.new(dict(zip(umis, freq)), L, max_edits)
        o = orc.Naive(umis, freq)
        ks = [max_edits, min(max_edits, L) - 1, min(max_edits, L), min(max_edits, L + 1)]
        for t, q in enumerate(rng.permutation(len(umis))[:60]):
            kk = ks[t % 4] if t < 16 else int(rng.integers(0, min(max_edits, L + 2) + 1))
            mf = int(rng.integers(0, 6))
            got = d.remove_near(umis[q], kk, mf)
            exp = {umis[i] for i in o.remove_near(int(q), kk, mf)}
            assert got == exp, (L, max_edits, kk, mf)
        assert all(d.contains(u) == o.contains(i) for i, u in enumerate(umis))


# ---- edge-list overflow and redo ---------------------------------------------------------------------

def test_edge_list_overflow_wide():
    """A wide call whose edge list starts at 8 entries: grown, the pair work redone, the result the oracle's;
    the context keeps the grown list for its next call."""
    import umi_collapse_rs_amd as umi
    L, k = 43, 8
    rng = np.random.default_rng(77)
    parts = [h.dense_clusters(rng, 12, 120, L, k), h.dense_clusters(rng, 3, 30, L, k)]
    keys, nm, fr, off = [], [], [], [0]
    for umis, freq in parts:
        kk, mm = orc.encode_keys_wide(umis)
        keys.append(kk); nm.append(mm); fr.extend(freq); off.append(off[-1] + len(umis))
    keys, nm, fr, off = np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)
    okept, oroot, _ = orc.dedup_batch_wide(keys, nm, fr, off, L, k)
    ctx = umi.Context(0)
    try:
        ctx.set_option("edge_capacity", 8)
        kept, root, st = ctx.dedup_batch_wide(keys, None, fr, off, L, k)
        assert (kept == okept).all() and (root == oroot).all()
        assert st["n_pair_launches"] >= 2 and st["n_edges"] > 10000, st
        kept, root, st2 = ctx.dedup_batch_wide(keys, None, fr, off, L, k)
        assert (kept == okept).all() and (root == oroot).all()
        assert st2["n_pair_launches"] == 1 and st2["n_edges"] == st["n_edges"], st2
    finally:
        ctx.close()


@pytest.mark.parametrize("L,k,partitioned", [(256, 16, True), (100, 100, False)])
def test_edge_list_overflow_whole_reads(L, k, partitioned):
    """umi_dedup_seqs with an edge list of 8 entries and a few 10^5 edges to hold: the redo must leave
    n_edges, n_candidates and n_pairs_evaluated at the model's values (not doubled), and the second call
    on the context must find its list large enough."""
    from umi_collapse_rs_amd import Context
    rng = np.random.default_rng(5 * L + k)
    if partitioned:
        umis, freq = h.dense_clusters(rng, 30, 160, L, k)  # ~4,800 entries: pairs_join is the reference
    else:
        umis, freq = h.planted_bucket(rng, 900, L, L)      # every pair is within k
    buckets = [([u.encode() for u in umis], freq)]
    assert h.seq_partitioned(L, k) == partitioned and (len(umis) > 3000) == partitioned
    ctx = Context(0)
    try:
        ctx.set_option("edge_capacity", 8)
        all_pairs = seq_pairs(buckets, k, join=partitioned)
        st = check_seqs(ctx, buckets, all_pairs, k, 0, 0)
        assert st["n_pair_launches"] >= 2 and st["n_edges"] >= 100000, st
        st2 = check_seqs(ctx, buckets, all_pairs, k, 0, 0)
        assert st2["n_pair_launches"] == 1, st2
    finally:
        ctx.close()
