"""umi_saturation_curve / umi_saturation_curve_device on the GPU against tests/saturation_model.py: all eight columns of
every depth equal, both forms, both values of option "saturation_skip", at the smallest shapes where the kernels can go
wrong.  Every call goes through the C interface with a curve buffer that is filled with a pattern and has guard rows
before and behind; the device form's input arrays are read back and compared.  tests/test_saturation_model_cpu.py
checks the model itself."""
import ctypes as C

import numpy as np
import pytest

import saturation_model as sm

pytestmark = pytest.mark.gpu
GUARD, FILL = 4, 0x5A5A5A5A5A5A5A5A  # guard rows of 8 words; what the curve buffer holds before a call


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def call(ctx, m, n_rows, n_cols, L=10, seed=0, mask=None, form="host", stream=0, n_reads=None):
    """(status, curve [L, 8] or None where the status is not OK): one call through the C interface; the guard rows
    are checked, on an error every row of the curve too, and for the device form the inputs"""
    import torch
    import umi_collapse_rs_amd as umi
    lib, p = umi.load(), umi._lib.ptr
    rows = max(1, min(L, 32))
    buf = np.full((rows + 2 * GUARD, 8), FILL, np.uint64)
    curve = buf[GUARD:GUARD + rows]
    entry, kept, root, off = (np.ascontiguousarray(m["read_entry"], np.uint32), np.ascontiguousarray(m["kept"], np.uint8),
                              np.ascontiguousarray(m["root"], np.uint32), np.ascontiguousarray(m["off"], np.uint64))
    row, col = np.ascontiguousarray(m["row"], np.uint32), np.ascontiguousarray(m["col"], np.uint32)
    mask = None if mask is None else np.ascontiguousarray(mask, np.uint8)
    n_reads = len(entry) if n_reads is None else n_reads
    out = curve.ctypes.data_as(C.POINTER(C.c_uint64))
    if form == "host":
        rc = lib.umi_saturation_curve(ctx._h, p(entry, C.c_uint32), n_reads, p(kept, C.c_uint8), p(root, C.c_uint32), p(off, C.c_uint64),
                                      len(off) - 1, p(row, C.c_uint32), p(col, C.c_uint32), n_rows, n_cols, seed, L,
                                      None if mask is None else p(mask, C.c_uint8), out)
    else:
        host = [entry.view(np.int32), kept, root.view(np.int32), row.view(np.int32), col.view(np.int32)] + ([] if mask is None else [mask])
        d = [dev(a) for a in host]
        torch.cuda.synchronize()
        ptr = lambda t: t.data_ptr() if t.numel() else None
        rc = lib.umi_saturation_curve_device(ctx._h, ptr(d[0]), n_reads, ptr(d[1]), ptr(d[2]), p(off, C.c_uint64), len(off) - 1, ptr(d[3]),
                                             ptr(d[4]), n_rows, n_cols, seed, L, None if mask is None else ptr(d[5]), out, stream or None)
        torch.cuda.synchronize()
        for a, t in zip(host, d):
            assert (t.cpu().numpy() == a).all()  # (the device form writes nothing the caller can see except the curve)
    assert (buf[:GUARD] == FILL).all() and (buf[GUARD + rows:] == FILL).all()
    if rc != umi._lib.UMI_OK:
        assert (curve == FILL).all()  # (nothing is written to the curve)
        return rc, None
    return rc, curve.copy()


def same(got, exp, what=""):
    assert got.shape == exp.shape, (what, got.shape, exp.shape)
    bad = np.argwhere(got != exp)
    assert not len(bad), (what, [(int(j), sm.COLUMNS[k], int(got[j, k]), int(exp[j, k])) for j, k in bad[:8]])


def both(ctx, m, n_rows, n_cols, L=10, seed=0, mask=None, skips=(0, 1)):
    """both forms and both values of the option against the model"""
    exp = sm.model_of(m, n_cols, L, seed, mask)
    try:
        for skip in skips:
            ctx.set_option("saturation_skip", skip)
            for form in ("host", "device"):
                rc, got = call(ctx, m, n_rows, n_cols, L, seed, mask, form)
                assert rc == 0, ctx_error()
                same(got, exp, (form, skip))
    finally:
        ctx.set_option("saturation_skip", 0)
    return exp


def ctx_error():
    import umi_collapse_rs_amd as umi
    return umi.load().umi_last_error().decode()


def with_reads(m, n_reads, seed=0, unstaged=0.1):
    """m with n_reads reads drawn over its entries, about a tenth of them unstaged"""
    rng = np.random.default_rng(seed)
    entry = rng.integers(0, len(m["kept"]), n_reads).astype(np.uint32)
    entry[rng.random(n_reads) < unstaged] = sm.UNSTAGED
    return dict(m, read_entry=entry)


def test_fuzz_against_the_model(ctx):
    m = sm.fuzz()
    exp = both(ctx, m, 50, 30)
    assert exp[-1, 1] > 20000 and exp[0, 1] < exp[-1, 1] and exp[-1, 2] > 1000 and exp[-1, 6] > 0
    staged = m["read_entry"][m["read_entry"] != sm.UNSTAGED]
    with_read = np.zeros(len(m["kept"]), bool)
    with_read[m["root"][staged]] = True
    assert int(np.count_nonzero((m["kept"] != 0) & ~with_read)) > 500  # molecules without any read
    assert int(np.count_nonzero(m["kept"][m["root"][staged]] == 0)) > 500  # reads under roots that are not kept
    both(ctx, m, 50, 30, mask=(np.arange(30) % 3 != 0).astype(np.uint8))
    through_the_wrappers = ctx.saturation_curve(m["read_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], 50, 30)
    same(through_the_wrappers, exp)


# 63 .. 65 and 255 .. 257: a wave's and a block's edge in the scatter
@pytest.mark.parametrize("n_reads", [0, 1, 63, 64, 65, 255, 256, 257])
def test_numbers_of_reads(ctx, n_reads):
    m = with_reads(sm.make(5, [3, 1, 40, 0, 2, 33, 7], 4, 3), n_reads, seed=n_reads)
    exp = both(ctx, m, 4, 3)
    if n_reads == 0:
        assert not exp.any()


def test_later_grid_stride_trips(ctx):
    """5,000 reads, 7,000 buckets and 2,500 columns under option "grid_cus" 1 and 3: every kernel's loop makes later
    trips; the curve is the default grid's, value for value"""
    rng = np.random.default_rng(8)
    sizes = [int(x) for x in rng.choice([1, 2, 3], 7000)] + [40, 700]
    m = with_reads(sm.make(9, sizes, 60, 2500), 5000, seed=3)
    mask = (rng.random(2500) < 0.5).astype(np.uint8)
    first = {cm is None: both(ctx, m, 60, 2500, 4, 1, cm) for cm in (None, mask)}
    assert first[True][-1, 3] > 1000
    try:
        for cus in (1, 3):
            ctx.set_option("grid_cus", cus)
            for cm in (None, mask):
                same(both(ctx, m, 60, 2500, 4, 1, cm), first[cm is None])
    finally:
        ctx.set_option("grid_cus", 0)
    # ... and the same reads over few columns (the blocks' own tables in LDS)
    few = dict(m, col=(m["col"] % 7).astype(np.uint32))
    first = both(ctx, few, 60, 7)
    try:
        for cus in (1, 3):
            ctx.set_option("grid_cus", cus)
            same(both(ctx, few, 60, 7), first)
    finally:
        ctx.set_option("grid_cus", 0)


@pytest.mark.parametrize("L", [1, 2, 10, 31, 32])
def test_numbers_of_levels(ctx, L):
    exp = both(ctx, sm.fuzz(), 50, 30, L, seed=4)
    assert len(exp) == L
    if L == 1:  # every read on one level
        assert exp[0, 1] > 20000


def test_most_levels_empty(ctx):
    m = with_reads(sm.make(2, [3, 1, 40, 2], 3, 2), 40, seed=1, unstaged=0.0)
    exp = both(ctx, m, 3, 2, 32)
    assert int(np.count_nonzero(np.diff(exp[:, 0].astype(np.int64)) == 0)) >= 8 and exp[-1, 0] > 20


@pytest.mark.parametrize("seed", [0, 1, sm.M64])
def test_seeds(ctx, seed):
    both(ctx, sm.fuzz(), 50, 30, 10, seed)


def test_ten_levels_are_every_second_of_twenty(ctx):
    m = sm.fuzz()
    for seed in (0, 6):
        ten = call(ctx, m, 50, 30, 10, seed, form="device")[1]
        twenty = call(ctx, m, 50, 30, 20, seed, form="device")[1]
        same(ten, twenty[1::2])
        same(twenty, sm.model_of(m, 30, 20, seed))


def test_one_molecule_of_many_reads(ctx):
    m = sm.make(11, [40, 3, 33, 1], 5, 3)
    deep = int(m["root"][int(m["off"][2]) + 5])
    rng = np.random.default_rng(5)
    entry = np.concatenate([m["read_entry"], np.full(5000, deep, np.uint32)])
    big = dict(m, read_entry=entry[rng.permutation(len(entry))], kept=m["kept"].copy())
    big["kept"][deep] = 1
    exp = both(ctx, big, 5, 3)
    assert exp[-1, 0] > 5000 and exp[0, 0] > 400


# 32 and 33: a lane's bucket and a wave's; 257 and 5,000: more than a wave's one pass
@pytest.mark.parametrize("sizes", [[1], [32], [33], [257], [5000], [0, 1, 0, 32, 33, 0, 257, 5000, 0], [33] * 300 + [1] * 300,
                                   [3, 5, 34, 35, 36, 37, 38, 39, 63, 64, 65, 127, 128, 129]])
def test_bucket_sizes(ctx, sizes):
    for seed, (n_rows, n_cols) in enumerate([(7, 5), (1, 1)]):
        m = sm.make(100 + seed + len(sizes), sizes, n_rows, n_cols, readless=0.1)
        both(ctx, m, n_rows, n_cols, 10, seed)


def test_roots_far_away_and_a_filtered_mask(ctx):
    m = sm.make(7, [5000, 33, 4000, 1], 4, 4, removed=0.6, far_roots=True)
    assert int((m["root"] != np.arange(len(m["root"]))).sum()) > 4000
    both(ctx, m, 4, 4)
    m = sm.make(3, [40] * 50 + [3] * 200, 9, 6, filtered=0.5)
    exp = both(ctx, m, 9, 6)
    assert 0 < exp[-1, 1] <= int(np.count_nonzero(m["kept"])) < int(np.count_nonzero(m["root"] == np.arange(len(m["root"])))) * 2 // 3
    nothing = dict(m, kept=np.zeros(len(m["kept"]), np.uint8))
    assert not both(ctx, nothing, 9, 6).any()
    unstaged = dict(m, read_entry=np.full(len(m["read_entry"]), sm.UNSTAGED, np.uint32))
    assert not both(ctx, unstaged, 9, 6).any()


# a pair's run of k buckets behind a run of 30 and before one of 300: runs that end inside a wave, cross a wave's edge
# (64, 128, ...) and a block's (256) in the segmented minimum
@pytest.mark.parametrize("k", [1, 63, 64, 65, 200])
def test_one_pair_in_many_buckets(ctx, k):
    rng = np.random.default_rng(k)
    nb = 30 + k + 300
    row = np.concatenate([np.zeros(30), np.ones(k), np.zeros(300)]).astype(np.uint32)
    col = np.concatenate([np.zeros(30), np.zeros(k), np.ones(300)]).astype(np.uint32)
    order = rng.permutation(nb)
    m = sm.make(k, [int(x) for x in rng.choice([1, 2, 3, 34], nb)], 2, 2, readless=0.5, unstaged=0.0)
    m = dict(m, row=row[order], col=col[order])
    # (few reads, so that a pair's level is decided by one bucket somewhere in its run)
    m = with_reads(m, 60, seed=k)
    for seed in range(4):
        exp = both(ctx, m, 2, 2, 32, seed, skips=(0,))
        assert 1 <= exp[-1, 2] <= 3


def test_one_column(ctx):
    m = sm.make(21, [3] * 200 + [40, 100], 9, 1)
    exp = both(ctx, m, 9, 1)
    assert exp[-1, 3] == 1 and exp[-1, 6] == exp[-1, 1] and exp[-1, 7] == exp[-1, 2] == 9
    both(ctx, m, 9, 1, mask=np.zeros(1, np.uint8))
    both(ctx, m, 9, 1, mask=np.ones(1, np.uint8))


# L n_cols: 3,000 words (a block's table in LDS), 9,600 (global adds), and 4,096 / 4,128, either side of the threshold
@pytest.mark.parametrize("n_cols,L", [(300, 10), (300, 32), (128, 32), (129, 32)])
def test_selected_columns(ctx, n_cols, L):
    rng = np.random.default_rng(n_cols + L)
    sizes = [int(x) for x in rng.choice([1, 2, 5, 33], 1500)]
    m = sm.make(n_cols, sizes, 20, n_cols - 40)  # (the last 40 columns hold nothing)
    null = both(ctx, m, 20, n_cols, L)
    assert 200 < null[-1, 3] <= n_cols - 40 if n_cols == 300 else 50 < null[-1, 3] <= n_cols - 40
    zero = both(ctx, m, 20, n_cols, L, mask=np.zeros(n_cols, np.uint8))
    assert not zero[:, 3:].any() and (zero[:, :3] == null[:, :3]).all()
    odd = np.zeros(n_cols, np.uint8)
    odd[rng.choice(n_cols - 40, 51, replace=False)] = 1
    even = odd.copy()
    even[np.flatnonzero(odd)[0]] = 0
    empty_ones = odd.copy()
    empty_ones[n_cols - 40:] = 1  # columns selected that hold no molecule
    for mask, n_sel in ((odd, 51), (even, 50), (empty_ones, 91), (np.ones(n_cols, np.uint8), n_cols)):
        assert int(np.count_nonzero(mask)) == n_sel
        exp = both(ctx, m, 20, n_cols, L, 3, mask, skips=(0,))
        assert exp[-1, 3] <= min(n_sel, n_cols - 40)


def test_no_buckets_and_empty_buckets(ctx):
    e32, e8 = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    for off in ([0], [0, 0, 0]):
        nb = len(off) - 1
        m = dict(read_entry=e32, kept=e8, root=e32, off=np.array(off, np.uint64), row=np.zeros(nb, np.uint32), col=np.zeros(nb, np.uint32))
        for form in ("host", "device"):
            rc, got = call(ctx, m, 0, 0, 5, form=form)
            assert rc == 0 and got.shape == (5, 8) and not got.any()
            rc, got = call(ctx, m, 3, 4, 5, mask=np.ones(4, np.uint8), form=form)
            assert rc == 0 and not got.any()


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    m = sm.fuzz()
    n = len(m["kept"])

    def refused(word, L=10, n_rows=50, n_cols=30, n_reads=None, **changed):
        c = dict(m, **changed)
        for form in ("host", "device"):
            rc, got = call(ctx, c, n_rows, n_cols, L, form=form, n_reads=n_reads)
            assert rc == umi._lib.UMI_ERR_ARG and got is None and word in ctx_error(), (form, rc, ctx_error())

    refused("n_levels 0 outside 1..32", L=0)
    refused("n_levels 33 outside 1..32", L=33)
    refused("n_levels -1 outside 1..32", L=-1)
    refused("4294967296 reads exceed", n_reads=1 << 32)  # (refused before any read is looked at)
    staged = np.flatnonzero(m["read_entry"] != sm.UNSTAGED)
    a, c = int(staged[len(staged) // 3]), int(staged[-5])
    for value in (n, n + 7, 0xFFFFFFFE):
        bad = m["read_entry"].copy()
        bad[[a, c]] = value
        refused("read %d: its read_entry" % a, read_entry=bad)
    bad = m["root"].copy()
    bad[m["read_entry"][a]] = n
    first = int(np.flatnonzero(m["read_entry"] == m["read_entry"][a])[0])
    refused("read %d: the root" % first, root=bad)
    # the smallest read of either kind is told
    entry, root = m["read_entry"].copy(), m["root"].copy()
    entry[c] = n
    root[m["read_entry"][a]] = n + 1
    refused("read %d: the root" % first, read_entry=entry, root=root)
    nonempty = np.flatnonzero(np.diff(m["off"].astype(np.int64)))
    for name, top in (("row", 50), ("col", 30)):
        bad = m[name].copy()
        bad[nonempty[:3]] = top
        refused("3 non-empty buckets", **{name: bad})
    off = m["off"].copy()
    off[5] = off[6] + 1
    refused("monotone", off=off)
    refused("a matrix of 0 rows", n_rows=0)
    refused("a matrix of 50 rows and 0 columns", n_cols=0)
    refused("33554432 columns at 32 levels exceed the 30-bit index space of the call's sort", L=32, n_cols=1 << 25)
    # a null pointer, through the C interface
    lib, p = umi.load(), umi._lib.ptr
    nb = len(m["off"]) - 1
    curve = np.full((10, 8), 7, np.uint64)
    args = [p(m["read_entry"], C.c_uint32), len(m["read_entry"]), p(m["kept"], C.c_uint8), p(m["root"], C.c_uint32), p(m["off"], C.c_uint64),
            nb, p(m["row"], C.c_uint32), p(m["col"], C.c_uint32), 50, 30, 0, 10, None, p(curve, C.c_uint64)]
    for i in (0, 2, 3, 4, 6, 7, 13):
        x = list(args)
        x[i] = None
        assert lib.umi_saturation_curve(ctx._h, *x) == umi._lib.UMI_ERR_ARG, i
    assert lib.umi_saturation_curve(None, *args) == umi._lib.UMI_ERR_ARG
    assert (curve == 7).all()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.saturation_curve(m["read_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], 50, 30, n_levels=40)
    assert e.value.code == umi._lib.UMI_ERR_ARG
    with pytest.raises(umi.UmiHipError):
        ctx.set_option("saturation_skip", 2)
    # the context is as good as before
    both(ctx, m, 50, 30)


def test_device_form_on_a_stream_and_a_multi_device_context(ctx):
    import torch
    import umi_collapse_rs_amd as umi
    m = sm.fuzz()
    exp = sm.model_of(m, 30)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(call(ctx, m, 50, 30, form="device", stream=s.cuda_stream)[1], exp)
    d = [dev(a) for a in (m["read_entry"].view(np.int32), m["kept"], m["root"].view(np.int32), m["row"].view(np.int32), m["col"].view(np.int32))]
    torch.cuda.synchronize()
    same(ctx.saturation_curve_device(d[0].data_ptr(), len(m["read_entry"]), d[1].data_ptr(), d[2].data_ptr(), m["off"], d[3].data_ptr(),
                                     d[4].data_ptr(), 50, 30), exp)
    c = umi.Context([0, 0])
    try:
        for form in ("host", "device"):
            same(call(c, m, 50, 30, form=form)[1], exp)
    finally:
        c.close()


def test_while_a_deferred_call_is_out(ctx):
    import torch
    import oracle as orc
    from umi_collapse_rs_amd import synth
    pos, bases = synth.molecule_reads(seed=31, n_positions=2000, reads_per_position=25, umi_len=12, err=0.02)
    st = synth.stage(pos, synth.bases_to_keys(bases))
    keys, freq, off = (np.ascontiguousarray(st["keys"], np.uint64), np.ascontiguousarray(st["freq"], np.int32),
                       np.ascontiguousarray(st["bucket_off"], np.uint64))
    okept, oroot, _ = orc.dedup_batch(keys, None, freq, off, 12, 1)
    t_keys, t_freq = dev(keys.view(np.int64)), dev(freq)
    t_kept = torch.zeros(len(keys), dtype=torch.uint8, device="cuda:0")
    t_root = torch.zeros(len(keys), dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_freq.data_ptr(), off, 12, t_kept.data_ptr(), t_root.data_ptr(),
                                 k=1, stream=s.cuda_stream)
    both(ctx, sm.fuzz(), 50, 30, skips=(0,))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all() and stats["n_kept"] == int(okept.sum())
    # ... and the curve of that call's own result: three reads per entry
    n = len(keys)
    nb = len(off) - 1
    m = dict(read_entry=np.repeat(np.arange(n, dtype=np.uint32), 3), kept=okept, root=oroot.astype(np.uint32), off=off,
             row=(np.arange(nb) % 40).astype(np.uint32), col=(np.arange(nb) % 13).astype(np.uint32))
    exp = both(ctx, m, 40, 13, skips=(0,))
    assert exp[-1, 1] == int(okept.sum())
