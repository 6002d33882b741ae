"""The four users of the shared run scan (csrc/umihip_pair_table.h) on one layout of runs -- at every lane, wave and
block edge a run can begin, end or cross (tests/pair_run_inputs.py; tests/test_pair_run_inputs_cpu.py checks the
layout) -- against their models, exactly, in host and device forms, the buckets in the given and in a permuted order."""
import numpy as np
import pytest

import gene_model
import pair_run_inputs as pri
import saturation_model
import stats_model
import velocity_model as vm

pytestmark = pytest.mark.gpu
ORDERS = pytest.mark.parametrize("permuted", [False, True])
FILL32, FILL64 = 0x5A5A5A5A, 0x5A5A5A5A5A5A5A5A
TABLE = ("umi_entry", "times_pre", "reads_pre", "times_post", "reads_post")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    signed = {np.dtype(np.uint32): np.int32, np.dtype(np.uint64): np.int64}.get(a.dtype)
    return torch.from_numpy((a.view(signed) if signed else a).copy()).to("cuda:0")


def filled(n, wide=False):
    import torch
    return torch.full((n,), FILL64 if wide else FILL32, dtype=torch.int64 if wide else torch.int32, device="cuda:0")


def back(t, n):
    a = t.cpu().numpy()
    return a.view(np.uint64 if a.dtype == np.int64 else np.uint32)[:n]


def same(got, exp, names):
    assert len(got) == len(exp) == len(names)
    for name, a, b in zip(names, got, exp):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert not len(bad), (name, bad[:10].tolist(), a[a != b][:10], b[a != b][:10])


@ORDERS
def test_count_matrix(ctx, permuted):
    import torch
    m = pri.matrix_case(permuted)
    names = ("row", "col", "molecules", "reads")
    exp = gene_model.count_model(m["kept"], m["freq"], m["off"], m["row"], m["col"])
    assert len(exp[0]) == len(pri.RUNS)
    same(ctx.count_matrix(m["kept"], m["freq"], m["off"], m["row"], m["col"], pri.N_ROWS, pri.N_COLS), exp, names)
    ins = [dev(m[k]) for k in ("kept", "freq", "row", "col")]
    outs = [filled(pri.N_ELEMENTS), filled(pri.N_ELEMENTS), filled(pri.N_ELEMENTS), filled(pri.N_ELEMENTS, wide=True)]
    torch.cuda.synchronize()
    nnz = ctx.count_matrix_device(ins[0].data_ptr(), ins[1].data_ptr(), m["off"], ins[2].data_ptr(), ins[3].data_ptr(), pri.N_ROWS,
                                  pri.N_COLS, *(t.data_ptr() for t in outs))
    torch.cuda.synchronize()
    same([back(t, nnz) for t in outs], exp, names)


@ORDERS
def test_velocity_matrix(ctx, permuted):
    import torch
    m = pri.matrix_case(permuted)
    names = ("row", "col", "spliced", "unspliced", "ambiguous")
    exp = vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])
    assert len(exp[0]) == len(pri.RUNS)
    same(ctx.velocity_matrix(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"], pri.N_ROWS,
                             pri.N_COLS), exp, names)
    ins = [dev(m[k]) for k in ("read_entry", "read_class", "kept", "root", "row", "col")]
    outs = [filled(pri.N_ELEMENTS) for _ in range(5)]
    torch.cuda.synchronize()
    nnz = ctx.velocity_matrix_device(ins[0].data_ptr(), ins[1].data_ptr(), len(m["read_entry"]), ins[2].data_ptr(), ins[3].data_ptr(),
                                     m["off"], ins[4].data_ptr(), ins[5].data_ptr(), pri.N_ROWS, pri.N_COLS,
                                     *(t.data_ptr() for t in outs))
    torch.cuda.synchronize()
    same([back(t, nnz) for t in outs], exp, names)


@ORDERS
def test_saturation_curve(ctx, permuted):
    """(the pairs columns are what the minimum over a run feeds)"""
    import torch
    m = pri.matrix_case(permuted)
    mask = np.ones(pri.N_COLS, np.uint8)
    exp = saturation_model.saturation_model(m["sat_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], pri.N_COLS,
                                            pri.SAT_LEVELS, 0, mask)
    assert int(exp[-1, 2]) > int(exp[0, 2]) > 0
    got = ctx.saturation_curve(m["sat_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], pri.N_ROWS, pri.N_COLS,
                               n_levels=pri.SAT_LEVELS, seed=0, cell_mask=mask)
    same([got], [exp], ["curve"])
    ins = [dev(m[k]) for k in ("sat_entry", "kept", "root", "row", "col")] + [dev(mask)]
    torch.cuda.synchronize()
    got = ctx.saturation_curve_device(ins[0].data_ptr(), len(m["sat_entry"]), ins[1].data_ptr(), ins[2].data_ptr(), m["off"],
                                      ins[3].data_ptr(), ins[4].data_ptr(), pri.N_ROWS, pri.N_COLS, n_levels=pri.SAT_LEVELS, seed=0,
                                      d_cell_mask=ins[5].data_ptr())
    torch.cuda.synchronize()
    same([got], [exp], ["curve"])


@ORDERS
def test_dedup_stats_per_umi_table(ctx, permuted):
    import torch
    keys, freq, kept, root, off, L = pri.stats_case(permuted)
    bins = 64
    names = ("count_pre", "count_post", "dist") + TABLE
    model = stats_model.stats_model(keys, freq, kept, root, off, L, hist_bins=bins)
    exp = [model[k] for k in names]
    assert tuple(int(x) for x in model["times_pre"]) == pri.RUNS
    got = ctx.dedup_stats(keys, freq, kept, root, off, L, n_words=1, hist_bins=bins, per_umi=True)
    same([got[k] for k in names], exp, names)
    n = len(freq)
    ins = [dev(keys), dev(freq), dev(kept), dev(root)]
    outs = [filled(bins, wide=True), filled(bins, wide=True), filled(4 * (L + 2), wide=True), filled(n), filled(n),
            filled(n, wide=True), filled(n), filled(n, wide=True)]
    torch.cuda.synchronize()
    rows = ctx.dedup_stats_device(ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr(), off, L,
                                  outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), n_words=1, hist_bins=bins,
                                  **{"d_" + k: t.data_ptr() for k, t in zip(TABLE, outs[3:])})
    torch.cuda.synchronize()
    assert rows == len(pri.RUNS)
    got = [back(outs[0], bins), back(outs[1], bins), back(outs[2], 4 * (L + 2)).reshape(4, L + 2)] + [back(t, rows) for t in outs[3:]]
    same(got, exp, names)
