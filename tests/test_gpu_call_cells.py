"""umi_call_cells / umi_call_cells_device on the GPU against cells_model.call_model: the five per-column arrays, the
filtered triplets, nnz_out and the ten counts by exact equality, on both call forms.  The shapes walk
csrc/umihip_cells.hip: triplet counts around a wave (64), the column kernels' block (256) and the sum kernel's block
(1,024), column runs inside a wave, across a wave's edge, across a block's edge and over several blocks, one column
that holds everything, columns of one triplet, gaps and empty columns, totals above 2^32, ties at the threshold."""
import ctypes as C

import numpy as np
import pytest

import cells_model as cm

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 1500, 70000]
PER = ("cell_molecules", "cell_reads", "cell_genes", "called", "new_col")
GUARD = 8  # elements behind every device array that must keep their pattern


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def host_call(c, case, **rule):
    return c.call_cells(case.row, case.col, case.molecules, case.reads, case.n_rows, case.n_cols, **rule)


def device_call(c, case, stream=None, **rule):
    """the _device form on tensors of its own, every output with a guard pattern behind it: behind n_cols, and from
    nnz_out on, nothing may be written"""
    import torch
    nnz, nc = len(case.row), case.n_cols
    t_in = [dev(np.asarray(a, np.uint32).view(np.int32)) for a in (case.row, case.col, case.molecules)]
    t_reads = dev(np.asarray(case.reads, np.uint64).view(np.int64))
    full = lambda n, dt: torch.full((n + GUARD,), 0x5A, dtype=dt, device="cuda:0")
    t_per = [full(nc, torch.int64), full(nc, torch.int64), full(nc, torch.int32), full(nc, torch.uint8), full(nc, torch.int32)]
    t_out = [full(nnz, torch.int32), full(nnz, torch.int32), full(nnz, torch.int32), full(nnz, torch.int64)]
    torch.cuda.synchronize()
    p = lambda t, n: t.data_ptr() if n else 0
    nnz_out, counts = c.call_cells_device(p(t_in[0], nnz), p(t_in[1], nnz), p(t_in[2], nnz), p(t_reads, nnz), nnz, case.n_rows, nc,
                                          *(t.data_ptr() for t in t_per), *(t.data_ptr() for t in t_out),
                                          stream=stream.cuda_stream if stream is not None else 0, **rule)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    views = (np.uint64, np.uint64, np.uint32, np.uint8, np.uint32)
    per = {}
    for name, t, v in zip(PER, t_per, views):
        a = t.cpu().numpy().view(v)
        assert (a[nc:] == 0x5A).all(), name
        per[name] = a[:nc]
    trip = []
    for t, v in zip(t_out, (np.uint32, np.uint32, np.uint32, np.uint64)):
        a = t.cpu().numpy().view(v)
        assert (a[nnz_out:] == 0x5A).all()
        trip.append(a[:nnz_out])
    return per, tuple(trip), counts


def same(got, exp):
    (per, trip, counts), (eper, etrip, ecounts) = got, exp
    assert counts == ecounts, (counts, ecounts)
    for name in PER:
        a, b = per[name], eper[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (name, bad[:10], a[bad[:10]], b[bad[:10]])
    assert len(trip) == len(etrip) == 4
    for name, a, b in zip(("row", "col", "molecules", "reads"), trip, etrip):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (name, bad[:10], a[bad[:10]], b[bad[:10]])


def check(c, case, forms=("host", "device"), **rule):
    exp = cm.call_model(case, **rule)
    if "host" in forms:
        same(host_call(c, case, **rule), exp)
    if "device" in forms:
        same(device_call(c, case, **rule), exp)
    return exp


def run(c, case, form, **rule):
    return (host_call if form == "host" else device_call)(c, case, **rule)


def rules_for(case):
    """every rule, expect_cells of 1, n, n + 1 and 3000, the percentile at 0, 990 and 1000, the ratio at 1 and 10"""
    n = int(np.count_nonzero(cm.call_model(case, rule=cm.MIN)[0]["cell_molecules"]))
    out = [dict(rule=cm.CR22), dict(rule=cm.CR22, percentile_permille=1000, max_min_ratio=1),
           dict(rule=cm.CR22, expect_cells=max(n, 1), percentile_permille=0, max_min_ratio=1), dict(rule=cm.MIN, min_molecules=6),
           dict(rule=cm.CR22, expect_cells=20, percentile_permille=900, max_min_ratio=2)]
    out += [dict(rule=cm.TOP, expect_cells=e) for e in sorted({1, max(n, 1), n + 1, 3000, max(1, n // 3)})]
    return out


@pytest.mark.parametrize("nnz", SIZES)
def test_triplet_counts_around_every_bound(ctx, nnz):
    case = cm.random_case(100 + nnz, nnz)
    rules = rules_for(case)
    called = set()
    for k, rule in enumerate(rules if nnz < 70000 else rules[::3]):
        _, trip, counts = check(ctx, case, forms=("host", "device") if k < 3 else (("device", "host")[k % 2],), **rule)
        called.add(counts["called"])
    assert nnz < 1500 or len(called) > 1  # (the rules draw different lines)


def test_runs_inside_a_wave_across_waves_and_across_blocks(ctx):
    runs = [5, 64, 65, 130, 1030, 2500, 1, 1, 3, 700, 64, 300, 2]
    case = cm.runs_case(5, runs)
    for rule in rules_for(case)[::2]:
        per, _, _ = check(ctx, case, **rule)
    assert sorted(np.unique(case.col, return_counts=True)[1].tolist()) == sorted(runs)
    assert int(per["cell_molecules"][-1]) == 0 and (per["cell_molecules"] == 0).sum() >= 5  # gaps and the empty tail


@pytest.mark.parametrize("nnz", [1, 64, 1025, 70000])
def test_one_column_holds_everything(ctx, nnz):
    case = cm.one_column(7, nnz)
    for rule in (dict(rule=cm.CR22), dict(rule=cm.TOP, expect_cells=1), dict(rule=cm.MIN, min_molecules=10 ** 7)):
        per, trip, counts = check(ctx, case, **rule)
    assert counts["called"] == 0 and len(trip[0]) == 0 and int(per["cell_molecules"][0]) == int(case.molecules.sum())


@pytest.mark.parametrize("nnz", [65, 1500])
def test_every_column_one_triplet(ctx, nnz):
    case = cm.one_each(8, nnz)
    for rule in rules_for(case):
        check(ctx, case, **rule)


def test_totals_above_32_bits_reads_near_40_and_a_column_of_zeros(ctx):
    case = cm.big_case()
    for rule in (dict(rule=cm.TOP, expect_cells=1), dict(rule=cm.MIN, min_molecules=1), dict(rule=cm.CR22, max_min_ratio=1),
                 dict(rule=cm.CR22, expect_cells=1, percentile_permille=1000, max_min_ratio=10), dict(rule=cm.MIN, min_molecules=2 ** 33)):
        per, _, counts = check(ctx, case, **rule)
        assert int(per["cell_molecules"][1]) == 3 * 0xFFFFFFFF and int(per["cell_reads"][3]) == 10 and not per["called"][3]
    assert counts["called"] == 1 and counts["threshold"] == 2 ** 33


def test_ties_at_the_threshold_under_every_rule(ctx):
    for seed in (6, 7):
        case = cm.tied_case(seed)
        for rule, t in zip(cm.TIED_RULES, (40, 4, 40)):
            per, _, counts = check(ctx, case, **rule)
            assert counts["threshold"] == t and int((per["cell_molecules"] == np.uint64(t)).sum()) == 3
            assert counts["called"] == int((per["cell_molecules"] >= np.uint64(t)).sum())


def test_no_triplets(ctx):
    z32, z64 = np.zeros(0, np.uint32), np.zeros(0, np.uint64)
    for n_rows, n_cols in ((3, 9), (0, 0), (0, 4)):
        per, trip, counts = check(ctx, cm.Case(z32, z32, z32, z64, n_rows, n_cols), rule=cm.TOP, expect_cells=2)
        assert (per["new_col"] == cm.NOT_CALLED).all() and not any(counts.values()) and len(trip[0]) == 0


def fails(code, call):
    import umi_collapse_rs_amd as umi
    with pytest.raises(umi.UmiHipError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def test_host_side_argument_errors(ctx):
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    L = umi.load()
    case = cm.random_case(9, 300)
    good = dict(rule=cm.CR22)
    check(ctx, case, **good)
    empty = cm.Case(case.row, case.col, case.molecules, case.reads, 0, case.n_cols)
    for form in ("host", "device"):
        for bad in (dict(rule=3), dict(rule=-1), dict(rule=cm.CR22, expect_cells=0), dict(rule=cm.TOP, expect_cells=0),
                    dict(rule=cm.TOP, expect_cells=-5), dict(rule=cm.CR22, percentile_permille=-1),
                    dict(rule=cm.CR22, percentile_permille=1001), dict(rule=cm.CR22, max_min_ratio=0)):
            fails(_lib.UMI_ERR_ARG, lambda: run(ctx, case, form, **bad))
        fails(_lib.UMI_ERR_ARG, lambda: run(ctx, empty, form, **good))
        fails(_lib.UMI_ERR_ARG, lambda: run(ctx, empty._replace(n_rows=5, n_cols=0), form, **good))
        # a rule does not look at what it does not read
        check(ctx, case, forms=(form,), rule=cm.MIN, min_molecules=3, expect_cells=0, percentile_permille=-7, max_min_ratio=0)
        check(ctx, case, forms=(form,), rule=cm.TOP, expect_cells=3, percentile_permille=5000, max_min_ratio=-1, min_molecules=-9)
        check(ctx, case, forms=(form,), **good)  # (and the context still works)
    # NULLs, and a count beyond the index space, before anything is read
    nnz_out, counts = C.c_uint64(5), np.zeros(10, np.uint64)
    pc = _lib.ptr(counts, C.c_uint64)
    a = [np.ones(4, np.uint64) for _ in range(13)]
    p32, p64, p8 = (lambda x: _lib.ptr(x.view(np.uint32), C.c_uint32)), (lambda x: _lib.ptr(x, C.c_uint64)), \
        (lambda x: _lib.ptr(x.view(np.uint8), C.c_uint8))
    args = [p32(a[0]), p32(a[1]), p32(a[2]), p64(a[3]), 1, 2, 2, cm.CR22, 3000, 990, 10, 1, p64(a[4]), p64(a[5]), p32(a[6]), p8(a[7]),
            p32(a[8]), p32(a[9]), p32(a[10]), p32(a[11]), p64(a[12])]
    a[0].view(np.uint32)[0] = a[1].view(np.uint32)[0] = 0
    assert L.umi_call_cells(ctx._h, *args, C.byref(nnz_out), pc) == _lib.UMI_OK and nnz_out.value == 1
    for at in list(range(4)) + list(range(12, 21)):
        holed = list(args)
        holed[at] = None
        assert L.umi_call_cells(ctx._h, *holed, C.byref(nnz_out), pc) == _lib.UMI_ERR_ARG, at
    assert L.umi_call_cells(ctx._h, *args, None, pc) == _lib.UMI_ERR_ARG
    assert L.umi_call_cells(ctx._h, *args, C.byref(nnz_out), None) == _lib.UMI_ERR_ARG
    assert L.umi_call_cells(None, *args, C.byref(nnz_out), pc) == _lib.UMI_ERR_ARG
    nothing = [None] * 4 + [1 << 30, 1, 1, cm.CR22, 3000, 990, 10, 1] + [None] * 9
    assert L.umi_call_cells_device(ctx._h, *nothing, C.byref(nnz_out), pc, None) == _lib.UMI_ERR_ARG
    assert "30-bit" in L.umi_last_error().decode()
    assert L.umi_call_cells(ctx._h, *nothing, C.byref(nnz_out), pc) == _lib.UMI_ERR_ARG


def broken(case, kind, at):
    """the case with one fault of `kind` at element `at` (0, 64 or the last)"""
    row, col = case.row.copy(), case.col.copy()
    n = len(row)
    p = n - 1 if at == "last" else at
    q = p + 1 if p == 0 else p - 1  # the neighbour the fault shows against
    n_rows, n_cols = case.n_rows, case.n_cols
    if kind == "duplicate pair":
        row[p], col[p] = row[q], col[q]
    elif kind == "fallen column":
        col[p] = col[q] + 1 if p == 0 else col[q] - 1
    elif kind == "fallen row":
        assert col[p] == col[q]
        row[p] = row[q] + 1 if p == 0 else row[q] - 1
    elif kind == "row == n_rows":
        row[p] = n_rows
    else:
        assert kind == "col == n_cols"
        col[p] = n_cols
    return case._replace(row=row, col=col)


@pytest.mark.parametrize("kind", ["duplicate pair", "fallen column", "fallen row", "row == n_rows", "col == n_cols"])
def test_errors_found_on_the_device(ctx, kind):
    """(an id out of range is told as such whatever it does to the order)"""
    from umi_collapse_rs_amd import _lib
    case = cm.runs_case(11, [40, 60, 157], empty_tail=0)
    assert len(case.row) == 257 and case.col[64] == 1 and case.col[63] == 1 and case.col[0] == case.col[1] == 0
    code = _lib.UMI_ERR_ARG if "==" in kind else _lib.UMI_ERR_ORDER
    for at in (0, 64, "last"):
        bad = broken(case, kind, at)
        for form in ("host", "device"):
            text = fails(code, lambda: run(ctx, bad, form, rule=cm.CR22))
            assert "1 triplets" in text, text
    check(ctx, case, rule=cm.CR22)  # (and the context still works)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        check(c, cm.random_case(12, 1500), rule=cm.TOP, expect_cells=5)
    finally:
        c.close()


def test_on_a_stream(ctx):
    import torch
    case = cm.random_case(13, 1500)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    rule = dict(rule=cm.CR22, expect_cells=20, percentile_permille=900, max_min_ratio=2)
    same(device_call(ctx, case, stream=s, **rule), cm.call_model(case, **rule))


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the cell call lets it end first, and its result is still handed
    out, and right, afterwards"""
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
    check(ctx, cm.random_case(14, 1500), rule=cm.TOP, expect_cells=5)
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_a_smaller_then_a_larger_input_on_one_context():
    """the workspace grows and is used again"""
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        check(c, cm.random_case(15, 65), rule=cm.CR22)
        check(c, cm.random_case(16, 20000), rule=cm.CR22, expect_cells=50)
        check(c, cm.random_case(15, 65), rule=cm.CR22)
    finally:
        c.close()
