"""k = 1 part-0 sub-buckets decided by bitmap lookups (seg_local_kernel's probe path, options seg_probe and
seg_probe_min): every case runs lookups from two entries up (the small bins of these inputs), lookups from
the default size up, and the tile walk alone; the kept mask and the roots equal the oracle's in each, and
n_edges, n_candidates, n_pairs_evaluated and n_kept do not move between them.  Inputs:
tests/seg_probe_inputs.py (their geometry is checked in tests/test_seg_probe_inputs_cpu.py).
The L = 12 and L = 13 buckets of ~70,000 are compared with the run without lookups instead (the oracle
takes 23 s on them)."""
import numpy as np
import pytest

import seg_probe_inputs as sp

pytestmark = pytest.mark.gpu

PROBE_MIN = 129  # the library's default
COMBOS = [(1, 2), (1, PROBE_MIN), (0, PROBE_MIN)]  # (seg_probe, seg_probe_min); the last is the reference run
STATS = ("n_edges", "n_candidates", "n_pairs_evaluated", "n_kept")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def defaults(c):
    c.set_option("seg_probe", 1)
    c.set_option("seg_probe_min", PROBE_MIN)
    c.set_option("seg_local_cap", 512)


def every_way(c, batch, p, oracle=True, want_root=True, **opts):
    """The combinations, each against the oracle (or the run without lookups) bit for bit, equal statistics."""
    res = []
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        for probe, least in COMBOS:
            c.set_option("seg_probe", probe)
            c.set_option("seg_probe_min", least)
            res.append(c.dedup_batch(batch.keys, batch.nmask, batch.fr, batch.off, batch.L, 1, p, want_root=want_root))
    finally:
        defaults(c)
    ref_kept, ref_root = batch.reference(p) if oracle else res[-1][:2]
    for (probe, least), (kept, root, st) in zip(COMBOS, res):
        what = "seg_probe=%d seg_probe_min=%d p=%g %s" % (probe, least, p, opts)
        assert (kept == ref_kept).all(), "%s: kept differs at %s" % (what, np.nonzero(kept != ref_kept)[0][:10])
        if want_root:
            assert (root == ref_root).all(), "%s: root differs at %s" % (what, np.nonzero(root != ref_root)[0][:10])
        else:
            assert root is None
        assert st["n_kept"] == int(np.asarray(ref_kept).sum()), what
        for f in STATS:
            assert st[f] == res[-1][2][f], (what, f, st[f], res[-1][2][f])
    return res[0][2]


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_first_eligible(ctx, p):
    st = every_way(ctx, sp.first_eligible(), p)
    assert st["n_edges"] > 0 and st["n_candidates"] > 0


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_dense(ctx, p):
    st = every_way(ctx, sp.dense(), p)
    assert st["n_candidates"] > 4 * 2000  # several drains per bin


@pytest.mark.parametrize("p", [0.5, 1.0])
@pytest.mark.parametrize("n_raw", [3300, 6000])
def test_uneven_parts(ctx, n_raw, p):
    every_way(ctx, sp.uneven(n_raw), p)


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_mixed_call(ctx, p):
    every_way(ctx, sp.mixed(), p)


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_config2_geometry(ctx, p):
    """Six bases per bin and six outside, in both parts: against the run without lookups, and the
    structure of a directional result."""
    b = sp.deep(12)
    every_way(ctx, b, p, oracle=False)
    kept, root, _ = ctx.dedup_batch(b.keys, None, b.fr, b.off, 12, 1, p)
    idx = np.arange(len(b.keys), dtype=np.uint32)
    assert ((kept == 1) == (root == idx)).all() and (root[root] == root).all() and (root <= idx).all()


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_stays_on_tiles(ctx, p):
    """Seven bases outside the bins: the options change nothing."""
    every_way(ctx, sp.deep(13), p, oracle=False)


@pytest.mark.parametrize("cap", [2, 40, 64])
@pytest.mark.parametrize("shape", ["first_eligible", "dense"])
def test_caps(ctx, shape, cap):
    """Bins above the cap go to the pair kernel's tiles in the same call as the bins decided by lookups."""
    batch = getattr(sp, shape)()
    every_way(ctx, batch, 0.5, seg_local_cap=cap)
    every_way(ctx, batch, 1.0, seg_local_cap=cap)


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_duplicated_key(ctx, p):
    """Two entries of a bin with one rest-code: the bin is walked by tiles.  (Should the library reject a
    key that is there twice, it does so with the options on as well.)"""
    import umi_collapse_rs_amd as umi
    b = sp.duplicated()
    try:
        ctx.set_option("seg_probe", 0)
        try:
            ctx.dedup_batch(b.keys, None, b.fr, b.off, b.L, 1, p)
            rejected = False
        except umi.UmiHipError:
            rejected = True
    finally:
        defaults(ctx)
    if rejected:
        with pytest.raises(umi.UmiHipError):
            ctx.dedup_batch(b.keys, None, b.fr, b.off, b.L, 1, p)
        return
    every_way(ctx, b, p)
    every_way(ctx, b, p, oracle=False)


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_n_present(ctx, p):
    every_way(ctx, sp.with_n(), p)


@pytest.mark.parametrize("p", [0.5, 1.0])
def test_mask_only(ctx, p):
    every_way(ctx, sp.dense(), p, want_root=False)


def test_deferred(ctx):
    import torch
    b = sp.dense()
    dev = torch.device("cuda:0")
    t_keys = torch.from_numpy(b.keys.view(np.int64)).to(dev)
    t_fr = torch.from_numpy(b.fr).to(dev)
    t_kept = torch.zeros(len(b.keys), dtype=torch.uint8, device=dev)
    t_root = torch.zeros(len(b.keys), dtype=torch.int32, device=dev)
    try:
        ctx.set_option("seg_probe_min", 2)  # (bins of ~31 entries)
        ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_fr.data_ptr(), b.off, b.L, t_kept.data_ptr(),
                                     t_root.data_ptr(), k=1, percentage=0.5)
        st = ctx.dedup_batch_end()
    finally:
        defaults(ctx)
    torch.cuda.synchronize()
    okept, oroot = b.reference(0.5)
    assert (t_kept.cpu().numpy() == okept).all() and (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert st["n_kept"] == int(okept.sum())


def test_option_validation(ctx):
    import umi_collapse_rs_amd as umi
    for bad in (-1, 2, 512, 1 << 20):
        with pytest.raises(umi.UmiHipError):
            ctx.set_option("seg_probe", bad)
    ctx.set_option("seg_probe", 0)
    ctx.set_option("seg_probe", 1)
    for bad in (0, 1, 2049, 1 << 20):
        with pytest.raises(umi.UmiHipError):
            ctx.set_option("seg_probe_min", bad)
    ctx.set_option("seg_probe_min", 2)
    ctx.set_option("seg_probe_min", PROBE_MIN)
