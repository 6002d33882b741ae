"""umi_dedup_batch_cr on the device against tests/cr_model.py, byte for byte: kept, root, target and stats.n_edges,
for the host and the device form, on the small buckets' kernel and on the neighbour list, whichever pair path of
the pipeline fills that list."""
import contextlib

import numpy as np
import pytest

import cr_model as cm

pytestmark = pytest.mark.gpu

SMALL_MAX = (0, None, 1024)   # everything through the neighbour list, the default, the kernel's largest


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


@contextlib.contextmanager
def options(ctx, **opts):
    """options set for one block and put back (their defaults: include/umihip.h)"""
    defaults = dict(cr_small_max=128, seg_min=512, seg_index=1, grid_cus=0)
    for k, v in opts.items():
        if v is not None:
            ctx.set_option(k, v)
    try:
        yield
    finally:
        for k in opts:
            ctx.set_option(k, defaults[k])


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype).copy()).to("cuda:0")


GUARD = 64


def call_device(ctx, keys, nm, fr, off, L, want_root=True, want_target=True):
    """the device form; kept, root and target lie in buffers with GUARD bytes of 0xA5 behind their n entries"""
    import torch
    n = len(keys)
    t_keys, t_fr = dev(keys), dev(fr)
    t_nm = dev(nm) if nm is not None else None
    kept = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    root = torch.full((4 * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    target = torch.full((4 * n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda:0")
    st = ctx.dedup_batch_cr_device(t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0, t_fr.data_ptr(), off, L,
                                   kept.data_ptr(), root.data_ptr() if want_root else 0,
                                   target.data_ptr() if want_target else 0)
    torch.cuda.synchronize()
    k, r, t = kept.cpu().numpy(), root.cpu().numpy(), target.cpu().numpy()
    assert (k[n:] == 0xA5).all() and (r[4 * n:] == 0xA5).all() and (t[4 * n:] == 0xA5).all()
    if not want_root:
        assert (r == 0xA5).all()
    if not want_target:
        assert (t == 0xA5).all()
    return k[:n], r[:4 * n].view(np.uint32), t[:4 * n].view(np.uint32), st


def check(ctx, packed, model, L, with_nmask=False, where=""):
    keys, nm, fr, off = packed
    ekept, eroot, etarget, epairs = model
    kept, root, target, st = ctx.dedup_batch_cr(keys, nm if with_nmask else None, fr, off, L, want_target=True)
    assert kept.tolist() == ekept.tolist(), (where, "host kept")
    assert root.tolist() == eroot.tolist(), (where, "host root")
    assert target.tolist() == etarget.tolist(), (where, "host target")
    assert st["n_edges"] == epairs, (where, "host n_edges")
    assert st["n_kept"] == int(ekept.sum()) and st["n_umis"] == len(keys) and st["n_buckets"] == len(off) - 1
    sizes = np.diff(off.astype(np.int64))
    assert st["max_bucket"] == int(sizes.max()) and st["n_pairs"] == int((sizes * (sizes - 1) // 2).sum())
    kept, root, target, st = call_device(ctx, keys, nm if with_nmask else None, fr, off, L)
    assert kept.tolist() == ekept.tolist(), (where, "device kept")
    assert root.tolist() == eroot.tolist(), (where, "device root")
    assert target.tolist() == etarget.tolist(), (where, "device target")
    assert st["n_edges"] == epairs, (where, "device n_edges")
    return kept, root, target


@pytest.mark.parametrize("small_max", SMALL_MAX)
@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("L", cm.LENGTHS)
def test_parity_with_the_model(ctx, L, n_frac, small_max):
    """buckets of 1, 2, 3, 63, 64, 65, 129 and 600 entries in one call, empty ones between them"""
    buckets, packed, model = cm.batch(L, n_frac)
    if L >= 6:
        assert [len(u) for u, _ in buckets][::2] == list(cm.SIZES)
    with options(ctx, cr_small_max=small_max):
        check(ctx, packed, model, L, with_nmask=bool(n_frac) and L % 2 == 0, where=(L, n_frac, small_max))


@pytest.mark.parametrize("small_max", SMALL_MAX)
@pytest.mark.parametrize("seed", [0, 1])
@pytest.mark.parametrize("lead", [0, 1, 2, 3])
def test_runs_of_tiny_buckets(ctx, lead, seed, small_max):
    """one- to three-entry buckets whose boundaries fall on, before and after multiples of 64 entries"""
    buckets, packed, model = cm.tiny_runs(12, lead, seed)
    ends = set(np.cumsum([len(u) for u, _ in buckets]).tolist())
    if lead == 0:
        assert 64 in ends and 63 in ends and 129 not in ends and 130 in ends   # on a multiple, before one, across one
    with options(ctx, cr_small_max=small_max):
        check(ctx, packed, model, 12, where=(lead, seed, small_max))


@pytest.mark.parametrize("small_max", SMALL_MAX)
@pytest.mark.parametrize("L,letters", [(1, cm.LETTERS), (2, cm.LETTERS), (3, cm.LETTERS), (4, cm.LETTERS), (6, cm.NUCS)])
def test_every_string_in_one_bucket(ctx, L, letters, small_max):
    """all 5^L strings (L <= 4) and all 4^6: every neighbour is present, ties everywhere"""
    buckets, packed, model = cm.all_strings(L, letters)
    assert len(buckets[0][0]) == len(letters) ** L
    assert model[3] == len(letters) ** L * L * (len(letters) - 1) // 2
    with options(ctx, cr_small_max=small_max):
        check(ctx, packed, model, L, where=(L, small_max))


@pytest.mark.parametrize("name", ["600", "4096"])
def test_the_list_does_not_depend_on_the_pair_path(ctx, name):
    """the segment index supplies the pairs ("seg_min" lowered), the tile kernels do ("seg_index" 0): same bytes"""
    if name == "600":
        _, packed, model = cm.batch(12, 0.0)
        L = 12
    else:
        _, packed, model = cm.all_strings(6, cm.NUCS)
        L = 6
    seen = []
    for opts in (dict(), dict(seg_min=64), dict(seg_index=0), dict(cr_small_max=0, seg_min=2), dict(cr_small_max=0, seg_index=0)):
        with options(ctx, **opts):
            seen.append(check(ctx, packed, model, L, where=(name, opts)))
    for other in seen[1:]:
        assert all(a.tobytes() == b.tobytes() for a, b in zip(seen[0], other))


@pytest.mark.parametrize("n", [127, 128, 129])
def test_the_edges_of_cr_small_max(ctx, n):
    """a bucket at cr_small_max - 1, at it and above it, under the default and with the option moved to the bucket"""
    buckets, packed, model = cm.sized(n)
    check(ctx, packed, model, 12, where=(n, "default"))
    for small_max in (n - 1, n, n + 1):
        with options(ctx, cr_small_max=small_max):
            check(ctx, packed, model, 12, where=(n, small_max))


def test_the_same_call_twice(ctx):
    _, packed, model = cm.batch(12, 0.05)
    a = check(ctx, packed, model, 12)
    b = check(ctx, packed, model, 12)
    assert all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


@pytest.mark.parametrize("cus", [1, 3])
def test_grid_cus(ctx, cus):
    """every kernel of the call goes round its grid-stride loop several times"""
    for small_max in (0, None):
        for packed, model, L in (cm.batch(12, 0.05)[1:] + (12,), cm.tiny_runs(12, 1, 1)[1:] + (12,), cm.all_strings(6, cm.NUCS)[1:] + (6,)):
            with options(ctx, grid_cus=cus, cr_small_max=small_max):
                check(ctx, packed, model, L, where=(cus, small_max))


@pytest.mark.parametrize("small_max", SMALL_MAX)
def test_null_root_and_target(ctx, small_max):
    _, (keys, nm, fr, off), (ekept, eroot, etarget, _) = cm.batch(12, 0.05)
    with options(ctx, cr_small_max=small_max):
        for want_root, want_target in ((False, True), (True, False), (False, False)):
            kept, root, target, st = call_device(ctx, keys, None, fr, off, 12, want_root, want_target)
            assert kept.tolist() == ekept.tolist()
            assert not want_root or root.tolist() == eroot.tolist()
            assert not want_target or target.tolist() == etarget.tolist()
            assert st["n_kept"] == int(ekept.sum())
        kept, root, st = ctx.dedup_batch_cr(keys, None, fr, off, 12, want_root=False)
        assert root is None and kept.tolist() == ekept.tolist()
        kept, root, st = ctx.dedup_batch_cr(keys, None, fr, off, 12)
        assert root.tolist() == eroot.tolist()


def test_profile_fills_the_times():
    import umi_collapse_rs_amd as umi
    _, (keys, nm, fr, off), model = cm.batch(12, 0.0)
    c = umi.Context(0, profile=True)
    try:
        kept, root, st = c.dedup_batch_cr(keys, None, fr, off, 12)
        assert kept.tolist() == model[0].tolist()
        assert st["ms_total"] > 0 and st["ms_pairs"] > 0 and st["ms_prep"] > 0 and st["ms_finalize"] > 0
    finally:
        c.close()


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd._lib import UMI_ERR_ARG, UMI_ERR_ORDER

    def fails(code, f):
        with pytest.raises(umi.UmiHipError) as e:
            f()
        assert e.value.code == code

    _, (keys, nm, fr, off), (ekept, eroot, _, _) = cm.batch(12, 0.05)
    fails(UMI_ERR_ARG, lambda: ctx.dedup_batch_cr(keys, None, fr, off, 22))
    fails(UMI_ERR_ARG, lambda: call_device(ctx, keys, None, fr, off, 22))
    fails(UMI_ERR_ARG, lambda: ctx.dedup_batch_cr(keys, None, fr, off, 0))
    multi = umi.Context([0, 0])
    try:
        fails(UMI_ERR_ARG, lambda: multi.dedup_batch_cr(keys, None, fr, off, 12))
        fails(UMI_ERR_ARG, lambda: call_device(multi, keys, None, fr, off, 12))
    finally:
        multi.close()
    # a rise inside a bucket: in the 600 (the list's path) and in a bucket of three (the small kernel's)
    sizes = np.diff(off.astype(np.int64)).tolist()
    for size in (600, 3):
        s = int(off[sizes.index(size)])
        rising = fr.copy()
        rising[s + 1] = rising[s] + 1
        fails(UMI_ERR_ORDER, lambda: ctx.dedup_batch_cr(keys, None, rising, off, 12))
        fails(UMI_ERR_ORDER, lambda: call_device(ctx, keys, None, rising, off, 12))
    zero = fr.copy()
    zero[-1] = 0
    fails(UMI_ERR_ORDER, lambda: ctx.dedup_batch_cr(keys, None, zero, off, 12))
    # an N code that a given nmask does not cover; without any nmask the same keys are fine: code 100 is N
    assert nm.any()
    fails(UMI_ERR_ORDER, lambda: ctx.dedup_batch_cr(keys, np.zeros_like(nm), fr, off, 12))
    kept, root, _ = ctx.dedup_batch_cr(keys, nm, fr, off, 12)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
    # no entries
    for table in (np.zeros(1, np.uint64), np.zeros(4, np.uint64)):
        kept, root, st = ctx.dedup_batch_cr(np.zeros(0, np.uint64), None, np.zeros(0, np.int32), table, 12)
        assert len(kept) == 0 and st["n_umis"] == 0 and st["n_kept"] == 0 and st["n_edges"] == 0 and st["n_pairs"] == 0
    for bad in (-1, 1025):
        fails(UMI_ERR_ARG, lambda: ctx.set_option("cr_small_max", bad))
    # the other calls' algo keeps its three values
    fails(UMI_ERR_ARG, lambda: ctx.dedup_batch(keys, nm, fr, off, 12, k=1, algo=3))


def test_with_a_deferred_call_out(ctx):
    """the call lets a deferred umi_dedup_batch_device_begin end first; its result still waits"""
    import torch
    rng = np.random.default_rng(5)
    small = [cm.dense_bucket(rng, 40, 12) for _ in range(300)]   # every position the fused kernel's
    skeys, snm, sfr, soff = cm.pack(small)
    t = [dev(skeys), dev(sfr)]
    dkept = torch.zeros(len(skeys), dtype=torch.uint8, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t[0].data_ptr(), 0, t[1].data_ptr(), soff, 12, dkept.data_ptr(), 0, k=1, stream=stream.cuda_stream)
    _, packed, model = cm.batch(12, 0.0)
    check(ctx, packed, model, 12)
    st = ctx.dedup_batch_end()
    stream.synchronize()
    hkept, _, hst = ctx.dedup_batch(skeys, None, sfr, soff, 12, k=1)
    assert st["n_kept"] == hst["n_kept"] == int(hkept.sum())
    assert dkept.cpu().numpy().tolist() == hkept.tolist()
