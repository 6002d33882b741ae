"""umi_velocity_matrix / umi_velocity_matrix_device on the GPU against tests/velocity_model.py (velocity_model), and
against umi_count_matrix on the same buckets: the same triplets in the same order, the three layers summing to its
molecules.  tests/test_velocity_model_cpu.py checks what the fuzz input holds."""
import numpy as np
import pytest

import velocity_model as vm

pytestmark = pytest.mark.gpu
GUARD, FILL32 = 16, 0x5A5A5A5A
NAMES = ("row", "col", "spliced", "unspliced", "ambiguous")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def same(got, exp):
    assert len(got) == len(exp) == 5
    for name, a, b in zip(NAMES, got, exp):
        a, b = np.asarray(a), np.asarray(b)
        assert a.shape == b.shape, (name, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (name, bad[:10], a[bad[:10]], b[bad[:10]])


def device_call(ctx, m, n_rows, n_cols, stream=0):
    """the device form on outputs of n_buckets elements with guard words before and behind"""
    import torch
    nb = len(m["off"]) - 1
    ins = [dev(m["read_entry"].view(np.int32)), dev(m["read_class"]), dev(m["kept"]), dev(m["root"].view(np.int32)),
           dev(m["row"].view(np.int32)), dev(m["col"].view(np.int32))]
    outs = [torch.full((nb + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(5)]
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t.numel() else 0
    nnz = ctx.velocity_matrix_device(ptr(ins[0]), ptr(ins[1]), len(m["read_entry"]), ptr(ins[2]), ptr(ins[3]), m["off"], ptr(ins[4]),
                                     ptr(ins[5]), n_rows, n_cols, *(t.data_ptr() + 4 * GUARD for t in outs), stream=stream)
    torch.cuda.synchronize()
    got = []
    for t in outs:
        h = t.cpu().numpy()
        assert (h[:GUARD] == FILL32).all() and (h[GUARD + nb:] == FILL32).all()
        got.append(h[GUARD:GUARD + nnz].view(np.uint32))
    return tuple(got)


def both(ctx, m, n_rows, n_cols):
    """both forms against the model and against umi_count_matrix"""
    exp = vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])
    got = ctx.velocity_matrix(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"], n_rows, n_cols)
    same(got, exp)
    same(device_call(ctx, m, n_rows, n_cols), exp)
    row, col, mol, _ = ctx.count_matrix(m["kept"], np.ones(len(m["kept"]), np.int32), m["off"], m["row"], m["col"], n_rows, n_cols)
    assert (got[0] == row).all() and (got[1] == col).all()
    assert (got[2].astype(np.int64) + got[3] + got[4] == mol).all()
    return got


def test_fuzz_against_the_model(ctx):
    got = both(ctx, vm.fuzz_molecules(), 50, 30)
    assert len(got[0]) > 1000 and min(int(got[k].sum()) for k in (2, 3, 4)) > 300


# 32 and 33: a lane's bucket and a wave's; 257 and 5,000: more than a wave's one pass over its words
@pytest.mark.parametrize("sizes", [[1], [32], [33], [257], [5000], [0, 1, 0, 32, 33, 0, 257, 5000, 0], [33] * 300 + [1] * 300,
                                   [3, 5, 34, 35, 36, 37, 38, 39]])
def test_bucket_sizes(ctx, sizes):
    for seed, (n_rows, n_cols) in enumerate([(7, 5), (1, 1), (3, 1 << 20)]):
        m = vm.make_molecules(100 + seed + len(sizes), sizes, n_rows, n_cols)
        got = both(ctx, m, n_rows, n_cols)
        if n_rows * n_cols < len([s for s in sizes if s]):
            assert len(got[0]) < len([s for s in sizes if s])  # several buckets of one pair


def test_roots_far_away_in_the_bucket(ctx):
    m = vm.make_molecules(7, [5000, 33, 4000, 1], 4, 4, removed=0.6, far_roots=True)
    assert int((m["root"] != np.arange(len(m["root"]))).sum()) > 4000
    got = both(ctx, m, 4, 4)
    assert int(sum(g.sum() for g in got[2:])) == int(np.count_nonzero(m["kept"]))


def test_one_molecule_of_many_reads(ctx):
    """2^17 reads of one molecule, of all three kinds of evidence, among ordinary buckets: ambiguous; with the junction
    reads taken out: unspliced; with and without the load before the atomic (option "velocity_skip")"""
    m = vm.make_molecules(11, [40, 3, 33, 1], 5, 3)
    deep = int(m["off"][2]) + 5
    deep = int(m["root"][deep])
    rng = np.random.default_rng(5)
    n = 1 << 17
    entry = np.concatenate([m["read_entry"], np.full(n, deep, np.uint32)])
    cls = np.concatenate([m["read_class"], rng.choice([vm.EXONIC, vm.JUNCTION, vm.SPANNING, vm.INTRONIC], n).astype(np.uint8)])
    order = rng.permutation(len(entry))
    big = dict(m, read_entry=entry[order], read_class=cls[order], kept=m["kept"].copy())
    big["kept"][deep] = 1
    layer = vm.molecule_layers(big["read_entry"], big["read_class"], big["kept"], big["root"])
    assert layer[deep] == vm.AMBIGUOUS
    try:
        for skip in (1, 0):
            ctx.set_option("velocity_skip", skip)
            both(ctx, big, 5, 3)
            no_junction = dict(big, read_class=np.where((big["read_entry"] == deep) & (big["read_class"] == vm.JUNCTION), vm.EXONIC,
                                                        big["read_class"]).astype(np.uint8))
            assert vm.molecule_layers(no_junction["read_entry"], no_junction["read_class"], big["kept"], big["root"])[deep] == vm.UNSPLICED
            both(ctx, no_junction, 5, 3)
    finally:
        ctx.set_option("velocity_skip", 0)


def test_reads_in_any_order(ctx):
    m = vm.fuzz_molecules()
    first = both(ctx, m, 50, 30)
    order = np.argsort(m["read_entry"], kind="stable")
    for o in (order, order[::-1]):
        same(ctx.velocity_matrix(m["read_entry"][o], m["read_class"][o], m["kept"], m["root"], m["off"], m["row"], m["col"], 50, 30), first)


def test_no_reads_and_no_staged_reads(ctx):
    m = vm.fuzz_molecules()
    row, col, mol, _ = ctx.count_matrix(m["kept"], np.ones(len(m["kept"]), np.int32), m["off"], m["row"], m["col"], 50, 30)
    none = dict(m, read_entry=np.zeros(0, np.uint32), read_class=np.zeros(0, np.uint8))
    unstaged = dict(m, read_entry=np.full(len(m["read_entry"]), vm.UNSTAGED, np.uint32))
    for case in (none, unstaged):
        got = both(ctx, case, 50, 30)
        assert not got[2].any() and not got[3].any() and (got[4] == mol).all()


def test_a_filtered_mask(ctx):
    """molecules removed as the multi-gene filter leaves them: roots with kept == 0 count nowhere, their reads too"""
    m = vm.make_molecules(3, [40] * 50 + [3] * 200, 9, 6, filtered=0.5)
    own = m["root"] == np.arange(len(m["root"]))
    assert int((own & (m["kept"] == 0)).sum()) > 500
    got = both(ctx, m, 9, 6)
    assert int(sum(g.sum() for g in got[2:])) == int(np.count_nonzero(m["kept"]))
    nothing = dict(m, kept=np.zeros(len(m["kept"]), np.uint8))
    got = both(ctx, nothing, 9, 6)
    assert len(got[0]) > 0 and not any(g.any() for g in got[2:])  # the triplets stay, with nothing in them


def test_no_buckets_and_empty_buckets(ctx):
    e32, e8 = np.zeros(0, np.uint32), np.zeros(0, np.uint8)
    for off in ([0], [0, 0, 0]):
        nb = len(off) - 1
        got = ctx.velocity_matrix(e32, e8, e8, e32, off, np.zeros(nb, np.uint32), np.zeros(nb, np.uint32), 0, 0)
        assert all(len(g) == 0 for g in got)
    assert ctx.velocity_matrix_device(0, 0, 0, 0, 0, [0], 0, 0, 3, 3, 0, 0, 0, 0, 0) == 0  # (no bucket: no pointer is looked at)


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    m = vm.fuzz_molecules()
    n = len(m["kept"])

    def raises(word, **changed):
        c = dict(m, **changed)
        for call in ("host", "device"):
            with pytest.raises(umi.UmiHipError) as e:
                if call == "host":
                    ctx.velocity_matrix(c["read_entry"], c["read_class"], c["kept"], c["root"], c["off"], c["row"], c["col"], 50, 30)
                else:
                    device_call(ctx, c, 50, 30)
            assert e.value.code == umi._lib.UMI_ERR_ARG and word in str(e.value), str(e.value)

    staged = np.flatnonzero(m["read_entry"] != vm.UNSTAGED)
    a, b, c = int(staged[len(staged) // 3]), int(staged[len(staged) // 2]), int(staged[-5])
    for value in (n, n + 7, 0xFFFFFFFE):
        bad = m["read_entry"].copy()
        bad[[a, c]] = value
        raises("read %d: its read_entry" % a, read_entry=bad)
    bad = m["read_class"].copy()
    bad[[b, c]] = (5, 255)
    raises("read %d: a read_class" % b, read_class=bad)
    bad = m["root"].copy()
    bad[m["read_entry"][a]] = n
    first = int(np.flatnonzero(m["read_entry"] == m["read_entry"][a])[0])
    raises("read %d: the root" % first, root=bad)
    # the smallest read of any kind is told
    entry, cls = m["read_entry"].copy(), m["read_class"].copy()
    entry[c], cls[a] = n, 9
    raises("read %d: a read_class" % a, read_entry=entry, read_class=cls)
    entry, cls = m["read_entry"].copy(), m["read_class"].copy()
    entry[a], cls[c] = n, 9
    raises("read %d: its read_entry" % a, read_entry=entry, read_class=cls)
    # umi_count_matrix's own
    bad = m["row"].copy()
    bad[np.flatnonzero(np.diff(m["off"].astype(np.int64)))[:3]] = 50
    raises("3 non-empty buckets", row=bad)
    off = m["off"].copy()
    off[5] = off[6] + 1
    raises("monotone", off=off)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.velocity_matrix(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"], 0, 30)
    assert e.value.code == umi._lib.UMI_ERR_ARG
    # a null pointer, through the C interface: nothing is touched
    import ctypes as C
    lib, p = umi.load(), umi._lib.ptr
    nb = len(m["off"]) - 1
    outs = [np.full(nb, 7, np.uint32) for _ in range(5)]
    args = [p(m["read_entry"], C.c_uint32), p(m["read_class"], C.c_uint8), len(m["read_entry"]), p(m["kept"], C.c_uint8),
            p(m["root"], C.c_uint32), p(m["off"], C.c_uint64), nb, p(m["row"], C.c_uint32), p(m["col"], C.c_uint32), 50, 30] + \
           [p(o, C.c_uint32) for o in outs]
    nnz = C.c_uint64(99)
    for i in (0, 1, 3, 4, 5, 7, 8, 11, 12, 13, 14, 15):
        x = list(args)
        x[i] = None
        assert lib.umi_velocity_matrix(ctx._h, *x, C.byref(nnz)) == umi._lib.UMI_ERR_ARG, i
    assert lib.umi_velocity_matrix(ctx._h, *args, None) == umi._lib.UMI_ERR_ARG
    assert lib.umi_velocity_matrix(None, *args, C.byref(nnz)) == umi._lib.UMI_ERR_ARG
    assert all((o == 7).all() for o in outs)
    # the context is as good as before
    both(ctx, m, 50, 30)


def test_device_form_on_a_stream_and_a_multi_device_context(ctx):
    import torch
    import umi_collapse_rs_amd as umi
    m = vm.fuzz_molecules()
    exp = vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, m, 50, 30, stream=s.cuda_stream), exp)
    c = umi.Context([0, 0])
    try:
        same(c.velocity_matrix(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"], 50, 30), exp)
        same(device_call(c, m, 50, 30), exp)
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
    both(ctx, vm.fuzz_molecules(), 50, 30)
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all() and stats["n_kept"] == int(okept.sum())
    # ... and the layers of that call's own result: three reads per entry, classes by the read's number
    n = len(keys)
    entry = np.repeat(np.arange(n, dtype=np.uint32), 3)
    cls = ((np.arange(3 * n) * 7 // 3) % 5).astype(np.uint8)
    nb = len(off) - 1
    m = dict(read_entry=entry, read_class=cls, kept=okept, root=oroot.astype(np.uint32), off=off,
             row=(np.arange(nb) % 40).astype(np.uint32), col=(np.arange(nb) % 13).astype(np.uint32))
    both(ctx, m, 40, 13)
