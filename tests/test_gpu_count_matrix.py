"""umi_count_matrix / umi_count_matrix_device on the GPU against gene_model.count_model: the four output arrays and
nnz by exact equality, on both call forms.  The shapes walk every path of csrc/umihip_count.hip: buckets on both
sides of the 32-entry bound between a lane's and a wave's, kept[] starting at every alignment, runs of equal pairs
inside one wave, across waves and across blocks, sort keys of one to five digits, empty buckets left out on the
host."""
import numpy as np
import pytest

import gene_model as gm

pytestmark = pytest.mark.gpu
SIZES = [0, 1, 2, 31, 32, 33, 63, 64, 65, 257, 1500]


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_call(c, kept, freq, off, row, col, n_rows, n_cols, stream=None):
    """the _device form on tensors of its own, kept[] one byte off alignment; the arrays behind nnz are not looked at"""
    import torch
    nb = len(off) - 1
    t_kept = torch.zeros(len(kept) + 1, dtype=torch.uint8, device="cuda:0")
    t_kept[1:] = dev(np.asarray(kept, np.uint8))
    t_freq, t_row, t_col = dev(np.asarray(freq, np.int32)), dev(np.asarray(row, np.uint32).view(np.int32)), \
        dev(np.asarray(col, np.uint32).view(np.int32))
    outs = [torch.full((max(nb, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0") for _ in range(3)]
    o_reads = torch.full((max(nb, 1),), 0x5A5A5A5A, dtype=torch.int64, device="cuda:0")
    torch.cuda.synchronize()
    nnz = c.count_matrix_device(t_kept.data_ptr() + 1, t_freq.data_ptr(), off, t_row.data_ptr(), t_col.data_ptr(), n_rows,
                                n_cols, outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), o_reads.data_ptr(),
                                stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    return tuple(t.cpu().numpy().view(np.uint32)[:nnz] for t in outs) + (o_reads.cpu().numpy().view(np.uint64)[:nnz],)


def same(got, exp):
    assert len(got) == len(exp) == 4
    for name, a, b in zip(("row", "col", "molecules", "reads"), got, exp):
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (name, bad[:10], a[bad[:10]], b[bad[:10]])


def check(c, case, forms=("host", "device")):
    kept, freq, off, row, col, n_rows, n_cols = case
    exp = gm.count_model(kept, freq, off, row, col)
    if "host" in forms:
        same(c.count_matrix(kept, freq, off, row, col, n_rows, n_cols), exp)
    if "device" in forms:
        same(device_call(c, kept, freq, off, row, col, n_rows, n_cols), exp)
    return exp


def entries(rng, sizes):
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    kept = (rng.integers(1, 256, n) * (rng.random(n) < 0.6)).astype(np.uint8)  # (values other than 1 count as kept)
    freq = rng.integers(1, 1000, n).astype(np.int32)
    return kept, freq, off


def sized_case(seed, n_rows, n_cols, repeats=3):
    """every size of SIZES `repeats` times in random order, empty buckets between them and at both ends; some
    buckets with kept all zero; ids over the whole range, the largest included"""
    rng = np.random.default_rng(seed)
    sizes = [0, 0] + list(rng.permutation(np.repeat(SIZES, repeats))) + [0]
    kept, freq, off = entries(rng, sizes)
    for b in range(0, len(sizes), 4):
        kept[int(off[b]):int(off[b + 1])] = 0
    nb = len(sizes)
    row = rng.integers(0, n_rows, nb).astype(np.uint32)
    col = rng.integers(0, n_cols, nb).astype(np.uint32)
    row[3], col[3], row[5], col[5] = n_rows - 1, n_cols - 1, 0, 0
    return kept, freq, off, row, col, n_rows, n_cols


@pytest.mark.parametrize("n_rows,n_cols", [(70_000, 300), (2 ** 20 + 3, 2 ** 13 + 1), (5, 1), (1, 1), (1, 9), (2 ** 32 - 1, 2 ** 32 - 1)],
                         ids=["26 bits", "35 bits", "one column", "one pair", "one row", "64 bits"])
def test_bucket_sizes_around_every_bound(ctx, n_rows, n_cols):
    case = sized_case(n_rows % 1000, n_rows, n_cols)
    assert case[2][1] == 0 and case[2][-1] == case[2][-2]  # empty buckets at both ends
    r, c, m, _ = check(ctx, case)
    assert len(r) > 1 or n_rows * n_cols == 1
    assert (m == 0).any() or n_rows * n_cols < 1000  # a triplet without a molecule


def test_runs_of_equal_pairs(ctx):
    """runs of 1, 2, 64, 65 and 1000 buckets that share one pair, scattered over the call"""
    rng = np.random.default_rng(5)
    runs = [1, 2, 64, 65, 1000, 1, 65, 64, 2, 1000]
    pair = np.repeat(np.arange(len(runs)), runs)
    pair = pair[rng.permutation(len(pair))]
    nb = len(pair)
    kept, freq, off = entries(rng, rng.integers(1, 4, nb))
    row, col = (pair * 7919 % 70_000).astype(np.uint32), (pair % 3).astype(np.uint32)
    r, c, m, rd = check(ctx, (kept, freq, off, row, col, 70_000, 300))
    assert len(r) == len(runs) and int(rd.sum()) == int(freq.astype(np.int64).sum())


def test_every_bucket_shares_one_pair(ctx):
    rng = np.random.default_rng(6)
    nb = 20_000
    kept, freq, off = entries(rng, rng.integers(1, 4, nb))
    row, col = np.full(nb, 69_999, np.uint32), np.full(nb, 299, np.uint32)
    r, c, m, rd = check(ctx, (kept, freq, off, row, col, 70_000, 300))
    assert (r.tolist(), c.tolist()) == ([69_999], [299]) and int(m[0]) == int(np.count_nonzero(kept))


def test_sorted_input_of_distinct_pairs(ctx):
    """what the program gives: every bucket a pair of its own, 10^5 of them, none empty"""
    rng = np.random.default_rng(7)
    nb = 100_000
    kept, freq, off = entries(rng, rng.integers(1, 4, nb))
    pair = rng.permutation(300 * 1000)[:nb]
    r, c, m, rd = check(ctx, (kept, freq, off, (pair % 1000).astype(np.uint32), (pair // 1000).astype(np.uint32), 1000, 300))
    assert len(r) == nb


def test_reads_pass_32_bits(ctx):
    big = 2 ** 31 - 1
    kept, freq = np.array([1, 0, 7, 1], np.uint8), np.array([big, big, big, 5], np.int32)
    r, c, m, rd = check(ctx, (kept, freq, np.array([0, 3, 4], np.uint64), [2, 1], [0, 0], 3, 1))
    assert rd.tolist() == [5, 3 * big] and m.tolist() == [1, 2] and 3 * big > 2 ** 32


def test_no_buckets_and_all_buckets_empty(ctx):
    z8, z32 = np.zeros(0, np.uint8), np.zeros(0, np.int32)
    for off, ids in (([0], []), ([0, 0, 0, 0], [4_000_000_000, 7, 9])):
        exp = check(ctx, (z8, z32, np.array(off, np.uint64), np.array(ids, np.uint32), np.array(ids, np.uint32), 3, 3))
        assert all(len(a) == 0 for a in exp)
    # (no rows or columns at all is fine where no bucket holds anything)
    check(ctx, (z8, z32, np.array([0, 0], np.uint64), np.zeros(1, np.uint32), np.zeros(1, np.uint32), 0, 0))


def fails(code, call):
    import umi_collapse_rs_amd as umi
    with pytest.raises(umi.UmiHipError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def test_argument_errors(ctx):
    from umi_collapse_rs_amd import _lib
    rng = np.random.default_rng(8)
    kept, freq, off = entries(rng, [2, 0, 3, 1])
    row, col = np.array([1, 9, 2, 0], np.uint32), np.array([0, 9, 1, 1], np.uint32)
    good = (kept, freq, off, row, col, 3, 2)
    check(ctx, good)  # (the ids of the empty bucket are out of range, and not looked at)
    for form in ("host", "device"):
        for bad_row, bad_col, n_rows, n_cols in ((3, 0, 3, 2), (0, 2, 3, 2), (0, 0, 0, 2), (0, 0, 3, 0)):
            r2, c2 = row.copy(), col.copy()
            r2[2], c2[2] = max(r2[2], bad_row), max(c2[2], bad_col)
            fails(_lib.UMI_ERR_ARG, lambda: check(ctx, (kept, freq, off, r2, c2, n_rows, n_cols), forms=(form,)))
        falling = np.array([0, 5, 3, 6], np.uint64)
        text = fails(_lib.UMI_ERR_ARG, lambda: check(ctx, (kept, freq, falling, row[:3], col[:3], 3, 2), forms=(form,)))
        assert "monotone" in text
        check(ctx, good, forms=(form,))  # (and the context still works)


def test_too_many_buckets_is_refused_before_anything_is_read(ctx):
    import ctypes as C
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    nnz = C.c_uint64(5)
    off = np.zeros(2, np.uint64)
    rc = umi.load().umi_count_matrix_device(ctx._h, None, None, _lib.ptr(off, C.c_uint64), 1 << 30, None, None, 1, 1, None,
                                            None, None, None, C.byref(nnz), None)
    assert rc == _lib.UMI_ERR_ARG and "30-bit" in umi.load().umi_last_error().decode()


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        check(c, sized_case(11, 70_000, 300, repeats=1))
    finally:
        c.close()


def test_on_a_stream(ctx):
    import torch
    case = sized_case(12, 70_000, 300, repeats=1)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, *case, stream=s), gm.count_model(*case[:5]))


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the count lets it end first, and its result is still handed
    out, and right, afterwards -- and is what the count of that very call's kept[] takes as input"""
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
    check(ctx, sized_case(13, 70_000, 300, repeats=1))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)
    # the molecules of that call per (position % 40, position % 7)
    nb = len(off) - 1
    row, col = (np.arange(nb) % 40).astype(np.uint32), (np.arange(nb) % 7).astype(np.uint32)
    r, c, m, rd = check(ctx, (okept, freq, off, row, col, 40, 7))
    assert int(m.sum()) == stats["n_kept"]


def test_a_smaller_then_a_larger_input_on_one_context():
    """the workspace grows and is used again"""
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        check(c, sized_case(14, 5, 1, repeats=1))
        check(c, sized_case(15, 70_000, 300, repeats=6))
        check(c, sized_case(14, 5, 1, repeats=1))
    finally:
        c.close()
