"""Mask-only calls (want_root = False / d_root = 0) on every batched entry point and option.

tests/test_gpu_kept_only.py runs the path that leaves the union-find forest unflattened on hand-made chains
and a few small buckets of dedup_batch / dedup_batch_wide.  That path is taken by everything that goes through
the pipeline's run_one_sync -- the one-word, wide and edit-distance calls, every shard of a multi-device context
-- and it is what the command-line program runs unless clusters are asked for.  This file takes it through N
bases, a seeded fuzz over every kernel boundary, edit distance, deep trees, one giant component (the benchmark's
shape), the extent of the writes to d_kept and the state a mask-only call leaves on its context.  The whole-read
call, umi_collapse_edges_device and the giant-bucket split of a multi-device context collapse a finished edge
list instead (EdgeCollapse: directional_labels, where a null root only leaves a store out); they are called with
a null root here as well, against the same references.

Every case goes through check_mask of tests/test_gpu_kept_only.py: kept and n_kept of the mask-only call equal the CPU reference (the oracle,
tests/edit_model.py or tests/seq_model.py), the same context's call with root, and a context with
collapse_kept_only = 0; the three calls report the same n_edges and n_candidates.  Everything is integer and
bit-exact.  Inputs: tests/kept_only_inputs.py, checked on the CPU in tests/test_kept_only_inputs_cpu.py."""
import contextlib
import ctypes as C
import functools

import numpy as np
import pytest

import edit_model as em
import kept_only_inputs as ko
import oracle as orc
import test_gpu_deferred as df
from helpers import legacy_mark, usable
from test_gpu_deep_chains import model_edges
from test_gpu_kept_only import LIST_OPTS, _ident, check_mask, context, same_mask

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def contexts(opts, device=0):
    """(ctx, old): two contexts with these options, collapse_kept_only as shipped (1) and 0."""
    import umi_collapse_rs_amd as umi
    made = []
    try:
        for extra in ({}, dict(collapse_kept_only=0)):
            made.append(umi.Context(device))
            for name, v in dict(opts, **extra).items():
                made[-1].set_option(name, v)
        yield tuple(made)
    finally:
        for c in made:
            c.close()


def dev(a):
    """the array on the device (one zero where it is empty: a buffer to point at)"""
    a = np.ascontiguousarray(a)
    return df.dev_t(a if a.size else np.zeros(1, a.dtype))


def back(t, n):
    return t.cpu().numpy().reshape(-1)[:n]


# ---- 1. N bases ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}] + LIST_OPTS, ids=["default"] + [_ident(o) for o in LIST_OPTS])
@pytest.mark.parametrize("p", [0.5, 1.0])
@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n_frac", ko.N_FRACS)
def test_n_bases(n_frac, k, p, opts):
    """UMIs with N, nmask passed: a fused bucket (40), one of the chunk kernel (300) and one of the segment index
    (600) in one call."""
    batch = ko.n_batch(n_frac, k, p)
    assert batch.nmask is not None
    with contexts(opts) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "N %g k=%d p=%g %s" % (n_frac, k, p, opts), ctx, old)
        assert st["n_edges"] > 0


# ---- 2. fuzz -------------------------------------------------------------------------------------------------
FUZZ_OPTS = ({}, {"prune": 1}, {"bitslice": 0, "fused_max": 0}, {"bs_unit": 1, "small_max": 200, "seg_index": 0},
             {"seg_index": 0}, {"seg_min": 129, "two_phase": 1}, {"seg_min": 129, "fused_max": 0})


@pytest.mark.parametrize("seed", ko.FUZZ_SEEDS)
def test_fuzz(seed):
    """The fuzz of tests/test_gpu_fuzz.py through the mask-only call (k = 4 and 5: the kernels' bodies for k > 3)."""
    batch = ko.fuzz_batch(seed)
    for opts in FUZZ_OPTS:
        if not usable(opts):
            continue
        with contexts(opts) as (ctx, old):
            check_mask(batch.run, batch.reference(), "fuzz %d L=%d k=%d p=%g %s %s" % (
                seed, batch.L, batch.k, batch.p, batch.sizes(), opts), ctx, old)


# ---- 3. edit distance ----------------------------------------------------------------------------------------
def edit_device_run(b, k, p):
    def run(ctx, want_root):
        import torch
        n = len(b.keys)
        t_keys, t_fr = dev(b.keys), dev(b.fr)
        t_nm = dev(b.nm) if b.nmask is not None else None
        kept = df.zeros(n, torch.uint8)
        root = df.zeros(n, torch.int32) if want_root else None
        st = ctx.dedup_batch_edit_device(t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0, t_fr.data_ptr(),
                                         b.off, b.L, kept.data_ptr(), root.data_ptr() if want_root else 0, k=k,
                                         percentage=p)
        torch.cuda.synchronize()
        return back(kept, n), (back(root, n) if want_root else None), st
    return run


@pytest.mark.parametrize("p", [0.5, 1.0])
@pytest.mark.parametrize("k", [1, 2, 3, "L"])
@pytest.mark.parametrize("L,n_frac", ko.EDIT_INPUTS)
def test_edit_distance(L, n_frac, k, p):
    """dedup_batch_edit with want_root = False and dedup_batch_edit_device with d_root = 0 against the model."""
    b = ko.edit_batch(L, n_frac)
    k = L if k == "L" else k
    with contexts({}) as (ctx, old):
        what = "edit L=%d k=%d p=%g" % (L, k, p)
        st = check_mask(lambda c, wr: b.run(c, wr, k, p), b.reference(k, p), what + " host", ctx, old)
        assert st["n_edges"] > 0
        check_mask(edit_device_run(b, k, p), b.reference(k, p), what + " device", ctx, old)


def test_edit_distance_behind_the_overflow_retry():
    """edge_capacity = 64 on 600 UMIs of one composition at k = 2: the list runs over behind a resolving round."""
    b = ko.edit_dense_batch()
    with contexts(dict(edge_capacity=64)) as (ctx, old):
        st = check_mask(lambda c, wr: b.run(c, wr, 2, 0.5), b.reference(2, 0.5), "edit, edge_capacity 64", ctx, old)
        assert st["n_edges"] > 1024
    with contexts(dict(edge_capacity=64)) as (ctx, old):
        check_mask(edit_device_run(b, 2, 0.5), b.reference(2, 0.5), "edit device, edge_capacity 64", ctx, old)


# ---- 4. whole reads ------------------------------------------------------------------------------------------
def seqs_device_run(b):
    def run(ctx, want_root):
        import torch
        from umi_collapse_rs_amd import _lib
        n = len(b.fr)
        t_keys, t_nm, t_fr = dev(b.keys), dev(b.nm), dev(b.fr)
        kept = df.zeros(n, torch.uint8)
        root = df.zeros(n, torch.int32) if want_root else None
        blen = np.array(b.blen, np.int32)
        stats = _lib.Stats()
        _lib.check(_lib.load().umi_dedup_seqs_device(
            ctx._h, t_keys.data_ptr(), t_nm.data_ptr(), b.keys.shape[1], t_fr.data_ptr(), _lib.ptr(b.off, C.c_uint64),
            _lib.ptr(blen, C.c_int32), len(blen), b.k, b.p, 0, 0, kept.data_ptr(),
            root.data_ptr() if want_root else None, None, C.byref(stats)))
        torch.cuda.synchronize()
        return back(kept, n), (back(root, n) if want_root else None), stats.as_dict()
    return run


@pytest.mark.parametrize("k", [1, 2])
def test_whole_reads(k):
    """dedup_seqs with want_root = False and umi_dedup_seqs_device with a null root: reads of 30 and of 100 bases
    in one call, per length a pair, 200 entries (all pairs) and 600 (partitioned)."""
    b = ko.seq_batch(k)
    with contexts({}) as (ctx, old):
        st = check_mask(b.run, b.reference(), "whole reads k=%d host" % k, ctx, old)
        assert st["n_edges"] > 0
        check_mask(seqs_device_run(b), b.reference(), "whole reads k=%d device" % k, ctx, old)


# ---- 5. deep trees -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [dict(fused_max=0), dict(fused_max=0, seg_min=2)], ids=_ident)
@pytest.mark.parametrize("which", ["sym", "step2"])
def test_deep_trees(which, opts):
    """769-entry paths of 256 bases, which only the whole-read call takes: all pairs symmetric in reverse and
    zig-zag order (union-find trees up to 768 deep) and 768 one-way pairs in a row.  The whole-read call collapses
    its list by directional_labels, whose first look covers the union pass and 3 rounds (then 6, 12, 16, ...):
    n_rounds beyond 4 means its continuation ran.  (Measured on the MI355X: 11 = 1 + 3 + 6 + 1, every call.  The
    17 of test_gpu_deep_chains.py::test_step2_rounds_beyond_the_first_look belongs to run_one_sync, which this
    call does not go through; test_deep_trees_wide_keys asserts it on the deepest paths that do.)"""
    b = ko.deep_batch(which)
    with contexts(opts) as (ctx, old):
        st = check_mask(b.run, b.reference(), "deep %s %s" % (which, opts), ctx, old)
        assert st["n_edges"] > 0
        if which == "step2":
            assert st["n_rounds"] > 4


@pytest.mark.parametrize("opts", [dict(fused_max=0), dict(fused_max=0, seg_min=2)], ids=_ident)
@pytest.mark.parametrize("which", [0, 1], ids=["p0.5-sym-halving", "p1-step2-comb"])
def test_deep_trees_wide_keys(which, opts):
    """256-entry paths of 85 bases, the deepest that go through run_one_sync: sym in four orders (trees up to 255
    deep, climbed read-only by the resolving round) and halving at p = 0.5; step2 (255 one-way pairs in a row: the
    host's continuation over the resolved pairs), comb and sym zig-zag at p = 1.0."""
    batch = ko.chain_batches(85, 1, "wide")[which]
    with contexts(opts) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "deep wide p=%g %s" % (batch.p, opts), ctx, old)
        assert st["n_edges"] > 0
        if which == 1:  # (the threshold: test_gpu_deep_chains.py::test_step2_rounds_beyond_the_first_look)
            assert st["n_rounds"] > 17


@pytest.mark.parametrize("opts", LIST_OPTS, ids=_ident)
def test_label_that_reaches_a_set_late(opts):
    """A one-way pair that ends below its set's root, the root before the pair's source in rank order, and a label
    that comes down to the source only after twelve rounds: the rounds behind the resolving one must find the
    set's root at the pair's stored endpoint."""
    batch = ko.late_label_batch()
    with contexts(opts) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "late label %s" % opts, ctx, old)
        assert st["n_edges"] > 0 and st["n_rounds"] > 4


# ---- 6. one giant component ----------------------------------------------------------------------------------
@pytest.mark.parametrize("opts", [{}, dict(seg_index=0)], ids=["default", "seg_index0"])
def test_one_giant_component(opts):
    """One position of 20,000 uniform 8-base UMIs: the symmetric pairs form one set of most entries, thousands of
    one-way pairs end in it (one word of lab[] takes all their atomics)."""
    batch = ko.giant_batch()
    with contexts(opts) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "giant component %s" % opts, ctx, old)
        assert st["n_edges"] > 1024 and st["max_bucket"] == ko.GIANT_N


# ---- 7. other collapse routes with a null root ---------------------------------------------------------------
@pytest.mark.parametrize("amf", [0, 3])
def test_adjacency_mask_only(amf):
    batch = ko.mixed_n_batch()
    with contexts({}) as (ctx, old):
        check_mask(lambda c, wr: batch.run(c, wr, 1, amf), batch.reference(1, amf), "adjacency amf=%d" % amf, ctx, old)


@legacy_mark()
def test_two_phase_1_mask_only():
    """The hook / jump rounds of the development build, directional."""
    batch = ko.mixed_n_batch()
    with contexts(dict(two_phase=1)) as (ctx, old):
        check_mask(batch.run, batch.reference(), "two_phase=1", ctx, old)


def edges_run(n, edges):
    def run(ctx, want_root):
        import torch
        t_e = dev(edges)
        kept = df.zeros(n, torch.uint8)
        root = df.zeros(n, torch.int32) if want_root else None
        st = ctx.collapse_edges_device(n, t_e.data_ptr() if len(edges) else 0, len(edges), kept.data_ptr(),
                                       root.data_ptr() if want_root else 0)
        torch.cuda.synchronize()
        return back(kept, n), (back(root, n) if want_root else None), st
    return run


def test_collapse_edges_device_with_a_null_root():
    """umi_collapse_edges_device with d_root = 0: the edges of the 64-node step2 ladder written from the
    definition, and those of the mixed batch (with its N-bearing bucket) from pairs_partial_device in two parts."""
    import torch
    s2 = ko.step2_batch()
    mixed = ko.mixed_n_batch()
    with contexts({}) as (ctx, old):
        edges = model_edges(s2, 0, 0)
        assert len(edges) == 63
        check_mask(edges_run(64, edges), s2.reference(), "edge list of the step2 ladder", ctx, old)
        t_keys, t_nm, t_fr = dev(mixed.keys), dev(mixed.nm), dev(mixed.fr)
        parts = []
        for part in range(2):
            buf = df.zeros(1 << 18, torch.int64)
            ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(), mixed.off, mixed.L, part,
                                             2, buf.data_ptr(), 1 << 18, k=mixed.k, percentage=mixed.p)
            assert ne > 0
            parts.append(buf[:ne].cpu().numpy().view(np.uint64))
        check_mask(edges_run(len(mixed.keys), np.concatenate(parts)), mixed.reference(), "edge list of the mixed batch",
                   ctx, old)


def test_multi_device_context_default_options():
    """Context([0, 0]) as it comes (test_gpu_multi.py's mask-only call sets seg_index = 0 first)."""
    batch = ko.mixed_n_batch()
    with contexts({}, device=[0, 0]) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "Context([0, 0])", ctx, old)
        assert st["n_edges"] > 0


def test_multi_device_giant_bucket_split():
    """One bucket above split_min that dominates the call, behind small buckets of which one holds N: the pairs of
    the whole call are split over the devices, the lists gathered on the first one, one collapse there.  That the
    split route ran shows in n_edges: it switches the fused kernel off, so the pairs of the three buckets of at most
    128 entries are in its lists, while the same call sharded by buckets (split_min out of reach) leaves them to
    the fused kernel, which lists nothing."""
    batch = ko.split_batch()
    assert batch.nmask is not None
    with contexts(dict(split_min=10000), device=[0, 0]) as (ctx, old):
        st = check_mask(batch.run, batch.reference(), "giant bucket split over two devices", ctx, old)
        assert st["n_edges"] > 1024
        ctx.set_option("split_min", 10 ** 9)
        kept, root, st_sharded = batch.run(ctx, False)
        assert root is None
        same_mask("the same call sharded by buckets", kept, st_sharded["n_kept"], batch.reference())
        print("n_edges: split %d, sharded by buckets %d" % (st["n_edges"], st_sharded["n_edges"]))
        assert st["n_edges"] > st_sharded["n_edges"] > 1024


# ---- 8. extent of the writes ---------------------------------------------------------------------------------
GUARD = 64


def guarded(n, offset):
    """n bytes for d_kept, `offset` bytes past a 64-byte guard band, another band behind; everything 0x5A."""
    import torch
    buf = torch.full((GUARD + offset + n + GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    return buf, buf.data_ptr() + GUARD + offset


def check_guarded(buf, n, offset, exp, what):
    import torch
    torch.cuda.synchronize()
    got = buf.cpu().numpy()
    lo = GUARD + offset
    assert (got[:lo] == 0x5A).all() and (got[lo + n:] == 0x5A).all(), what + ": a write outside [0, n)"
    assert np.array_equal(got[lo:lo + n], np.asarray(exp).astype(np.uint8)), what


@pytest.mark.parametrize("n", ko.EXTENT_SIZES)
def test_extent_of_the_writes(n):
    """The device forms with d_root = 0 under fused_max = 0 (map_finalize_kernel's four-at-a-time branch) on a
    d_kept between guard bands, 0, 1 and 3 bytes off its allocation's alignment: nothing outside [0, n) changes,
    and the inputs are as they were."""
    from umi_collapse_rs_amd import _lib
    one = ko.Batch("one", 12, 1, 0.5, [ko.extent_bucket(n)])
    umis30, freq30 = ko.extent_bucket(n, 30)
    if n:
        wide = ko.Batch("wide", 30, 1, 0.5, [(umis30, freq30)])
        wkeys, wref = wide.keys, wide.reference()
    else:
        wkeys, wref = np.zeros((0, 2), np.uint64), np.zeros(0, np.uint8)
    edges = model_edges(one, 0, 0)
    ekept, _ = em.model_batch(one.buckets, 2)
    if n:
        seq = ko.SeqBatch(1, 0.5, [([u.encode() for u in umis30], freq30)])
        skeys, sref = seq.keys, seq.reference()
    else:
        skeys, sref = np.zeros((0, 2), np.uint64), np.zeros(0, np.uint8)
    blen = np.array([30], np.int32)
    ins = dict(keys=one.keys, fr=one.fr, off=one.off, wkeys=wkeys, wfr=np.array(freq30, np.int32), edges=edges,
               skeys=skeys)

    def seqs_device(t, p):
        stats = _lib.Stats()
        _lib.check(_lib.load().umi_dedup_seqs_device(
            ctx._h, t["skeys"].data_ptr(), None, 2, t["wfr"].data_ptr(), _lib.ptr(one.off, C.c_uint64),
            _lib.ptr(blen, C.c_int32), 1, 1, 0.5, 0, 0, p, None, None, C.byref(stats)))
        return stats.as_dict()
    with context(dict(fused_max=0)) as ctx:
        for offset in (0, 1, 3):
            t = {name: dev(a) for name, a in ins.items()}
            forms = {
                "dedup_batch_device": (one.reference(), lambda p: ctx.dedup_batch_device(
                    t["keys"].data_ptr(), 0, t["fr"].data_ptr(), one.off, 12, p, 0, k=1)),
                "dedup_batch_device_table": (one.reference(), lambda p: ctx.dedup_batch_device(
                    t["keys"].data_ptr(), 0, t["fr"].data_ptr(), one.off, 12, p, 0, k=1,
                    d_bucket_off=t["off"].data_ptr())),
                "begin / end": (one.reference(), lambda p: (ctx.dedup_batch_device_begin(
                    t["keys"].data_ptr(), 0, t["fr"].data_ptr(), one.off, 12, p, 0, k=1), ctx.dedup_batch_end())[1]),
                "dedup_batch_edit_device": (ekept, lambda p: ctx.dedup_batch_edit_device(
                    t["keys"].data_ptr(), 0, t["fr"].data_ptr(), one.off, 12, p, 0, k=2)),
                "dedup_batch_wide_device": (wref, lambda p: ctx.dedup_batch_wide_device(
                    t["wkeys"].data_ptr(), 0, 2, t["wfr"].data_ptr(), one.off, 30, p, 0, k=1)),
                "collapse_edges_device": (one.reference(), lambda p: ctx.collapse_edges_device(
                    n, t["edges"].data_ptr() if len(edges) else 0, len(edges), p, 0)),
                "umi_dedup_seqs_device": (sref, lambda p: seqs_device(t, p)),
            }
            for form, (exp, call) in forms.items():
                buf, ptr = guarded(n, offset)
                st = call(ptr)
                what = "%s n=%d offset %d" % (form, n, offset)
                check_guarded(buf, n, offset, exp, what)
                assert st["n_kept"] == int(np.asarray(exp).sum()), what
            for name, a in ins.items():
                assert np.array_equal(back(t[name], a.size).view(a.dtype), a.reshape(-1)), (name, n, offset)


# ---- 9. state left on the context ----------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def x_batches():
    rng = np.random.default_rng(2612)
    return dict(x=df.with_deep(df.staged(rng, 8000, 800), rng, 1500))


def x_adjacency(ctx, b, s):
    keys, nm, fr, off = b["x"]
    kept, root, st = ctx.dedup_batch(keys, nm, fr, off, df.L, k=1, algo=1, adj_max_freq=2)
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, df.L, 1, 0.5, 1, 2)
    assert (kept == okept).all() and (root == oroot).all() and st["n_kept"] == int(okept.sum())


def x_edit(ctx, b, s):
    eb = ko.edit_batch(12, 0.05)
    ekept, eroot = em.model_batch(eb.buckets, 2, mats=eb.mats)
    kept, root, st = ctx.dedup_batch_edit(eb.keys, eb.nm, eb.fr, eb.off, 12, k=2)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist() and st["n_kept"] == int(ekept.sum())


X_AFTER = {"root": df.x_dedup_batch, "adjacency": x_adjacency, "edit": x_edit, "seqs": df.x_dedup_seqs,
           "wide": df.x_dedup_batch_wide_22, "pairs_partial_then_collapse": df.x_pairs_partial_then_collapse,
           "hipnaive": df.x_hipnaive}


@pytest.mark.parametrize("x", list(X_AFTER))
def test_other_entry_points_after_a_mask_only_call(x):
    """label[] holds an unflattened forest and lab[] what the rounds left when a mask-only call ends: every other
    entry point on that context still gives its own reference's result, and so does the next mask-only call."""
    mixed, deep = ko.mixed_batch(), ko.chain_batches(85, 1, "wide")[1]  # (255 one-way pairs in a row)
    with context({}) as ctx:
        for batch in (mixed, deep):
            kept, root, st = batch.run(ctx, False)
            assert root is None
            same_mask("mask-only call ahead of %s" % x, kept, st["n_kept"], batch.reference())
        assert st["n_rounds"] > 17
        X_AFTER[x](ctx, x_batches(), None)
        kept, _, st = mixed.run(ctx, False)
        same_mask("mask-only call behind %s" % x, kept, st["n_kept"], mixed.reference())


def test_small_call_after_a_large_one():
    """20,000 entries mask-only and straight behind them 300, mask-only, on the same context: the unflattened
    forest the large call left beyond n must not be seen.  The full checks of both follow."""
    giant, small = ko.giant_batch(), ko.small_batch()
    with contexts(dict(fused_max=0)) as (ctx, old):
        for batch in (giant, small, giant, small):
            kept, root, st = batch.run(ctx, False)
            assert root is None
            same_mask("large / small / large / small, mask-only", kept, st["n_kept"], batch.reference())
        assert st["n_edges"] > 0
        check_mask(giant.run, giant.reference(), "the large call", ctx, old)
        check_mask(small.run, small.reference(), "the small call behind it", ctx, old)


def test_rounds_ahead_carried_between_calls():
    """A call's rounds beyond the first look set how many the next call on the context enqueues ahead
    (dag_rounds_ahead), whichever path either takes: deep then shallow, shallow then deep, want_root False / True /
    False, and collapse_kept_only 1 / 0 / 1 between calls on one context."""
    deep, mixed = ko.chain_batches(21, 1)[1], ko.mixed_batch()
    opts = dict(fused_max=0)
    for order in ((deep, mixed), (mixed, deep)):
        with contexts(opts) as (ctx, old):
            for batch in order + order:  # mask-only calls back to back, nothing in between
                kept, root, st = batch.run(ctx, False)
                assert root is None
                same_mask("mask-only calls back to back", kept, st["n_kept"], batch.reference())
                if batch is deep:
                    assert st["n_rounds"] > 17
            for i, batch in enumerate(order):
                st = check_mask(batch.run, batch.reference(), "call %d of %s" % (i, "deep / shallow" if order[0] is deep
                                                                                 else "shallow / deep"), ctx, old)
                if batch is deep:
                    assert st["n_rounds"] > 17
    with context(opts) as ctx:
        for want_root in (False, True, False):
            for batch in (deep, mixed):
                kept, root, st = batch.run(ctx, want_root)
                assert (root is not None) == want_root
                same_mask("want_root %s" % want_root, kept, st["n_kept"], batch.reference())
    with context(opts) as ctx:
        for v in (1, 0, 1):
            ctx.set_option("collapse_kept_only", v)
            for batch in (deep, mixed):
                kept, _, st = batch.run(ctx, False)
                same_mask("collapse_kept_only %d" % v, kept, st["n_kept"], batch.reference())
