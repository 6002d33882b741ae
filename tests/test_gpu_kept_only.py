"""Calls that ask for the kept mask alone (want_root = False / d_root = 0) on the batched directional path.

With option collapse_kept_only (default 1) such a call skips the flatten of the union-find forest: the
first round follows the endpoints of the one-way pairs to their roots and rewrites the pairs in place, the
rounds after it, the check beside finalize and the host's continuation read the rewritten pairs, and the
mask is parent[i] == i && lab[i] == i.  This file runs that path on hand-made chains and a few small
buckets; tests/test_gpu_kept_only_matrix.py takes it through the other entry points, options and kinds
of input with the same assertions (the rest of the suite asks for root and runs the flattening path).
Every case asserts that kept and n_kept equal the CPU oracle's, the same context's call with
want_root = True, and a context with collapse_kept_only = 0; all three calls must report the same
n_edges and n_candidates.  Inputs: tests/kept_only_inputs.py (checked on the CPU in
tests/test_kept_only_inputs_cpu.py)."""
import contextlib

import numpy as np
import pytest

import kept_only_inputs as ko

pytestmark = pytest.mark.gpu


@contextlib.contextmanager
def context(opts):
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        yield c
    finally:
        c.close()


def same_mask(what, got, n_kept, exp):
    got, exp = np.asarray(got).astype(np.uint8), np.asarray(exp).astype(np.uint8)
    bad = np.nonzero(got != exp)[0]
    assert bad.size == 0, "%s: kept differs at %d entries, first %d (%d, expected %d)" % (
        what, bad.size, bad[0], got[bad[0]], exp[bad[0]])
    assert n_kept == int(exp.sum()), (what, n_kept, int(exp.sum()))


def check_mask(run, ref, what, ctx, old):
    """The common assertions on run(ctx, want_root) -> (kept, root or None, stats) against the reference mask ref;
    ctx / old: contexts with collapse_kept_only on / off.  Returns the stats of the want_root = False call."""
    kept, root, st = run(ctx, False)
    assert root is None
    same_mask(what + ": against the reference", kept, st["n_kept"], ref)
    kept_r, root_r, st_r = run(ctx, True)
    assert root_r is not None
    same_mask(what + ": the call with root", kept_r, st_r["n_kept"], kept)
    kept_o, _, st_o = run(old, False)
    same_mask(what + ": collapse_kept_only=0", kept_o, st_o["n_kept"], kept)
    for other in (st_r, st_o):
        assert other["n_edges"] == st["n_edges"] and other["n_candidates"] == st["n_candidates"], (what, st, other)
    return st


def check(batch, opts, what, ctx=None, old=None):
    """check_mask on a Batch against the oracle.  ctx / old: contexts to go on with (kept-only on / off); made and
    closed here otherwise."""
    with contextlib.ExitStack() as es:
        ctx = ctx or es.enter_context(context(opts))
        old = old or es.enter_context(context(dict(opts, collapse_kept_only=0)))
        return check_mask(batch.run, batch.reference(), what, ctx, old)


LIST_OPTS = [dict(fused_max=0)] + [dict(fused_max=0, seg_min=2, seg_unite=a, seg_local=b) for a in (0, 1) for b in (0, 1)]


def _ident(o):
    return "-".join("%s%d" % (k.replace("fused_max", "fm").replace("seg_", ""), v) for k, v in o.items())


@pytest.mark.parametrize("opts", LIST_OPTS, ids=_ident)
@pytest.mark.parametrize("L,stride", ko.PATHS)
def test_chains_on_the_list_path(L, stride, opts):
    """The fused kernel off: every bucket through the chunk kernel or the segment index, the chains' pairs in
    the list.  sym in reverse and zig-zag order: trees up to 63 deep, climbed read-only; comb: sets of two
    chained by one-way pairs; step2: one-way pairs only (every endpoint its own root)."""
    for batch in ko.chain_batches(L, stride):
        st = check(batch, opts, "chains L=%d k=%d %s p=%g" % (L, stride, opts, batch.p))
        assert st["n_edges"] > 0 and st["n_rounds"] >= 2


def test_one_way_pair_inside_one_set():
    """3 ~ 2 ~ 1 symmetric, 3 -> 1 one-way: the pair resolves to (root, root) and must move nothing."""
    st = check(ko.self_edge_batch(), dict(fused_max=0), "self edge after resolve")
    assert st["n_edges"] > 0


def test_continuation_after_the_first_look():
    """The 64-node step2 ladder, twice on one context: more rounds than the host enqueues ahead (the
    threshold and its reason: test_gpu_deep_chains.py::test_step2_rounds_beyond_the_first_look), so
    run_rounds goes on over the resolved pairs -- its round index restarts at 0 and must not skip or
    resolve -- and the second finalize runs."""
    batch = ko.chain_batches(21, 1)[1]
    opts = dict(fused_max=0)
    with context(opts) as ctx, context(dict(opts, collapse_kept_only=0)) as old:
        for i in range(2):
            st = check(batch, opts, "step2 continuation, call %d" % i, ctx, old)
            assert st["n_rounds"] > 17


def test_mixed_call_default_options():
    """Fused buckets (ranges non-null), a chunk-kernel bucket (flagged and plain pairs appended directly,
    united by the list's union pass) and a segment-index bucket (private slots gathered) in one list."""
    batch = ko.mixed_batch()
    st = check(batch, {}, "mixed call")
    assert st["n_edges"] > 0


@pytest.mark.parametrize("which", [0, 1], ids=["p0.5-sym-halving", "p1-step2-comb"])
def test_wide_keys(which):
    """256 nodes of 85 bases, the segment index over the first key word (seg_min = 129)."""
    batch = ko.chain_batches(85, 1, "wide")[which]
    st = check(batch, dict(seg_min=129), "wide p=%g" % batch.p)
    assert st["n_edges"] > 0 and st["n_rounds"] >= 2


def test_device_entry_points():
    """The mixed input through dedup_batch_device with d_root = 0 and through begin / end: the masks of the
    host-buffer call."""
    import torch
    batch = ko.mixed_batch()
    dev = torch.device("cuda:0")
    t_keys = torch.from_numpy(batch.keys.view(np.int64)).to(dev)
    t_fr = torch.from_numpy(batch.fr).to(dev)
    t_kept = torch.zeros(len(batch.keys), dtype=torch.uint8, device=dev)
    for opts in ({}, dict(collapse_kept_only=0)):
        with context(opts) as ctx:
            kept_h, _, st_h = batch.run(ctx, want_root=False)
            same_mask("host-buffer call %s" % opts, kept_h, st_h["n_kept"], batch.reference())
            t_kept.zero_()
            st = ctx.dedup_batch_device(t_keys.data_ptr(), 0, t_fr.data_ptr(), batch.off, batch.L, t_kept.data_ptr(), 0,
                                        k=batch.k, percentage=batch.p)
            torch.cuda.synchronize()
            same_mask("dedup_batch_device %s" % opts, t_kept.cpu().numpy(), st["n_kept"], kept_h)
            assert st["n_edges"] == st_h["n_edges"]
            t_kept.zero_()
            ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_fr.data_ptr(), batch.off, batch.L, t_kept.data_ptr(), 0,
                                         k=batch.k, percentage=batch.p)
            st = ctx.dedup_batch_end()
            torch.cuda.synchronize()
            same_mask("begin / end %s" % opts, t_kept.cpu().numpy(), st["n_kept"], kept_h)
            assert st["n_edges"] == st_h["n_edges"]


def test_behind_the_overflow_retry():
    """edge_capacity = 1 (as test_gpu_deep_chains.py::test_deep_chains_behind_the_overflow_retry): the first
    attempt's list runs over after its resolving round has rewritten what fitted; the pair kernels rebuild
    the list for the second attempt, with a deep chain behind it."""
    batch = ko.overflow_batch()
    opts = dict(fused_max=0, edge_capacity=1)
    with context(opts) as ctx, context(dict(opts, collapse_kept_only=0)) as old:
        st = check(batch, opts, "40 step2 ladders, edge_capacity 1", ctx, old)
        assert st["n_edges"] > 1024
        check(ko.mixed_batch(), opts, "mixed call after the overflow", ctx, old)
