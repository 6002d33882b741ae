"""umi_junction_matrix / umi_junction_matrix_device on the GPU, bit for bit against tests/junction_model.py: the junction
table, the (column, junction) triplets and the four counts, at the edges of the library's scan and sort tiles, with keys
that need both words, with every error and its named read, and with guard words around every output."""
import ctypes as C

import numpy as np
import pytest

import junction_model as jm

pytestmark = pytest.mark.gpu
GUARD, FILL32 = 16, 0x5A5A5A5A
NAMES = ("jn_ref", "jn_start", "jn_end", "out_jn", "out_col", "molecules", "reads")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    a = np.ascontiguousarray(a)
    a = a.view(np.int64) if a.dtype == np.uint64 else a.view(np.int32) if a.dtype == np.uint32 else a
    return torch.from_numpy(a.copy()).to("cuda:0")


def same(got, exp):
    flat_g = list(got[0]) + list(got[1])
    flat_e = list(exp[0]) + list(exp[1])
    for name, a, b in zip(NAMES, flat_g, flat_e):
        a, b = np.asarray(a), np.asarray(b)
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (name, bad[:10], a[bad[:10]], b[bad[:10]])
    assert [int(x) for x in got[2]] == [int(x) for x in exp[2]], (got[2], exp[2])


def n_words_N(m):
    return int(np.count_nonzero((m["cigar"] & 15) == 3))


def host_call(ctx, m, n_cols, capacity=None):
    return ctx.junction_matrix(m["read_ref"], m["read_pos"], m["cigar"], m["cigar_off"], m["read_entry"], m["kept"], m["root"], m["off"],
                               m["col"], n_cols, capacity)


def device_call(ctx, m, n_cols, capacity=None, stream=0, untouched=False):
    """the device form on outputs of `capacity` elements with guard words before and behind; untouched: the call is
    expected to fail, and nothing at all may have been written"""
    import torch
    cap = n_words_N(m) if capacity is None else capacity
    cigar = m["cigar"] if len(m["cigar"]) else np.zeros(1, np.uint32)
    ins = [dev(m["read_ref"]), dev(m["read_pos"]), dev(cigar), dev(m["cigar_off"]), dev(m["read_entry"]), dev(m["kept"]), dev(m["root"]),
           dev(m["col"])]
    outs = [torch.full((cap + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0") for _ in range(6)]
    outs.append(torch.full((cap + 2 * GUARD,), FILL32, dtype=torch.int64, device="cuda:0"))
    torch.cuda.synchronize()
    ptr = lambda t: t.data_ptr() if t.numel() else 0
    try:
        counts = ctx.junction_matrix_device(ptr(ins[0]), ptr(ins[1]), ptr(ins[2]), ptr(ins[3]), ptr(ins[4]), len(m["read_ref"]),
                                            ptr(ins[5]), ptr(ins[6]), m["off"], ptr(ins[7]), n_cols, cap,
                                            *(t.data_ptr() + t.element_size() * GUARD for t in outs), stream=stream)
    finally:
        torch.cuda.synchronize()
        hs = [t.cpu().numpy() for t in outs]
        for h in hs:
            assert (h[:GUARD] == FILL32).all() and (h[GUARD + cap:] == FILL32).all()
            if untouched:
                assert (h == FILL32).all()
    j, z = int(counts[2]), int(counts[3])
    assert j <= cap and z <= cap
    for h in hs[:3]:
        assert (h[GUARD + j:] == FILL32).all()  # (nothing behind the junctions, nothing behind the triplets)
    for h in hs[3:]:
        assert (h[GUARD + z:] == FILL32).all()
    jn = tuple(h[GUARD:GUARD + j] for h in hs[:3])
    trip = tuple(h[GUARD:GUARD + z].view(np.uint32) for h in hs[3:6]) + (hs[6][GUARD:GUARD + z].view(np.uint64),)
    return jn, trip, counts


def both(ctx, m, n_cols, exp=None):
    exp = exp or jm.model_of(m)
    same(host_call(ctx, m, n_cols), exp)
    same(device_call(ctx, m, n_cols), exp)
    same(device_call(ctx, m, n_cols, capacity=max(1, int(exp[2][1]))), exp)  # (a capacity that just holds them)
    return exp


def test_fuzz_against_the_model(ctx):
    m = jm.make_inputs(5, [0, 1, 1, 2, 3, 5, 8, 32, 33, 40] * 12 + [257, 0, 1], 9)
    exp = both(ctx, m, 9)
    c = [int(x) for x in exp[2]]
    assert c[0] > 500 and c[1] > c[0] and c[2] > 60 and c[3] > c[2]
    assert int(exp[1][3].sum()) == c[1] and (exp[1][2] <= exp[1][3]).all() and (exp[1][2] < exp[1][3]).any()


# the scan's tile is 2,048 elements and the sort's 4,096 (tests/test_gpu_primitives.py): on them and beside them
@pytest.mark.parametrize("total", [0, 1, 2, 2047, 2048, 2049, 4095, 4096, 4097, 8193])
def test_occurrence_totals(ctx, total):
    m = jm.make_inputs(total, [3, 40, 1, 33, 7] * 40, 5, total=total)
    exp = both(ctx, m, 5)
    assert int(exp[2][1]) == total
    if total == 0:
        assert not any(int(x) for x in exp[2]) and all(len(a) == 0 for a in exp[0] + exp[1])


def one_bucket(reads, n_entries=1, kept=None, root=None, entry=None, col=0):
    """reads (ref, pos, cigar text or words) of a single bucket's entries"""
    words, off = [], [0]
    for _, _, c in reads:
        words += jm.cigar_words(c) if isinstance(c, str) else list(c)
        off.append(len(words))
    n = len(reads)
    return dict(read_ref=np.array([r[0] for r in reads], np.int32), read_pos=np.array([r[1] for r in reads], np.int32),
                cigar=np.array(words, np.uint32), cigar_off=np.array(off, np.uint64),
                read_entry=np.zeros(n, np.uint32) if entry is None else np.array(entry, np.uint32),
                kept=np.ones(n_entries, np.uint8) if kept is None else np.array(kept, np.uint8),
                root=np.arange(n_entries, dtype=np.uint32) if root is None else np.array(root, np.uint32),
                off=np.array([0, n_entries], np.uint64), col=np.array([col], np.uint32))


def chain(k, gap=3):
    return "5M" + ("%dN5M" % gap) * k


def test_reads_of_0_1_64_65_and_300_junctions_in_one_wave(ctx):
    ks = [0, 1, 64, 65, 300] + [2, 0, 1] * 19 + [300, 65]
    assert len(ks) == 64
    m = one_bucket([(0, 10 + i, chain(k)) for i, k in enumerate(ks)], n_entries=4, entry=[i % 4 for i in range(64)])
    exp = both(ctx, m, 1)
    assert int(exp[2][1]) == sum(ks) and int(exp[2][0]) == sum(1 for k in ks if k)


def test_keys_that_need_both_words(ctx):
    top = 2 ** 31 - 1
    reads = [(0, 10, "5M10N5M"), (1, 10, "5M10N5M"), (2 ** 20, 10, "5M10N5M"),          # equal but for the ref
             (0, 10, "5M11N5M"), (2 ** 20, 10, "5M11N5M"),                              # equal but for the end
             (1, top - 30, "10M20N1M"), (2 ** 20, top - 30, "10M20N1M"),                # a gap ending at 2^31 - 1
             (1, top - 30, "10M21N1M"),                                                 # ... and one beyond it: none
             (0, top - 30, "9M1N20M"), (0, top - 31, "10M1N20M"), (2, top - 40, "5M2N5M3N5M40N5M"),
             (2 ** 20, 0, "1M1N1M"), (0, 0, "1M" + "268435455N" * 8 + "6N1M")]  # (a word holds 28 bits)
    m = one_bucket(reads, n_entries=3, entry=[i % 3 for i in range(len(reads))])
    exp = both(ctx, m, 1)
    table = list(zip(*(a.tolist() for a in exp[0])))
    assert (1, top - 20, top) in table and (0, 1, top) in table and (2 ** 20, 1, 2) in table
    assert not any(e > top for _, _, e in table) and len(table) == 12
    assert table == sorted(table)


def test_a_junction_of_every_molecule_and_a_molecule_of_2000_reads(ctx):
    n = 300
    reads = [(0, 100, "10M50N10M")] * n + [(0, 100, "10M50N10M7N3M")] * 2000 + [(0, 100, "10M")] * 5
    m = one_bucket(reads, n_entries=n, entry=list(range(n)) + [7] * 2000 + [3] * 5)
    m["off"], m["col"] = np.array([0, 100, 100, 250, n], np.uint64), np.array([2, 9, 0, 2], np.uint32)  # (two buckets share a column)
    exp = both(ctx, m, 3)
    jn, (ojn, ocol, mol, rd), counts = exp
    assert ojn.tolist() == [0, 0, 1] and ocol.tolist() == [0, 2, 2]
    assert mol.tolist() == [150, 150, 1] and rd.tolist() == [150, 150 + 2000, 2000]
    assert [int(x) for x in counts] == [n + 2000, n + 4000, 2, 3]


def test_removed_entries_kept_zero_roots_and_unstaged_reads(ctx):
    # entries 0..5: 1 and 2 hang on 0 (kept), 4 hangs on 3 (a root the filter removed), 5 a molecule of its own
    reads = [(0, 10, "5M10N5M"), (0, 10, "5M10N5M"), (0, 10, "5M10N5M"), (0, 10, "5M20N5M"), (0, 10, "5M20N5M"), (0, 10, "5M30N5M"),
             (0, 10, "5M40N5M"), (0, 10, "5M30N5M")]
    m = one_bucket(reads, n_entries=6, kept=[1, 0, 0, 0, 0, 1], root=[0, 0, 0, 3, 3, 5], entry=[0, 1, 2, 3, 4, 5, jm.UNSTAGED, jm.UNSTAGED])
    exp = both(ctx, m, 1)
    assert list(zip(*(a.tolist() for a in exp[0]))) == [(0, 15, 25), (0, 15, 45)]
    assert exp[1][2].tolist() == [1, 1] and exp[1][3].tolist() == [3, 1]
    # what is not counted is not looked at: garbage in the ref and the words of such reads
    bad = dict(m, read_ref=m["read_ref"].copy(), cigar=m["cigar"].copy())
    for i in (3, 4, 6, 7):
        bad["read_ref"][i] = -1
        bad["cigar"][int(m["cigar_off"][i])] = (5 << 4) | 12
    both(ctx, bad, 1, exp)
    big = jm.make_inputs(77, [40] * 30 + [3] * 100, 6, removed=0.5, filtered=0.5, unstaged=0.5)
    assert int((~jm.counted_reads(big)).sum()) > 1000
    both(ctx, big, 6)


@pytest.mark.parametrize("n_cols", [1, 1 << 20])
def test_columns(ctx, n_cols):
    m = jm.make_inputs(9, [3, 0, 33, 1, 0, 0, 8] * 30, n_cols)
    if n_cols > 1:
        m["col"][:5] = n_cols - 1
        m["col"][5:40] = m["col"][40:75]  # several buckets sharing a column
    both(ctx, m, n_cols)


def test_grid_cus_1_and_3(ctx):
    m = jm.make_inputs(21, [3, 40, 1, 33, 7] * 80, 11)
    exp = both(ctx, m, 11)
    assert len(m["read_ref"]) > 3 * 16 * 256  # (more reads than a grid of three CUs has lanes: later trips)
    try:
        for cus in (1, 3):
            ctx.set_option("grid_cus", cus)
            both(ctx, m, 11, exp)
    finally:
        ctx.set_option("grid_cus", 0)


def test_capacity_one_too_small(ctx):
    import umi_collapse_rs_amd as umi
    m = jm.make_inputs(4, [3, 40, 1, 33, 7] * 20, 5)
    exp = jm.model_of(m)
    t = int(exp[2][1])
    assert t > 500
    for cap in (t - 1, 1, 0):
        with pytest.raises(umi.UmiHipError) as e:
            device_call(ctx, m, 5, capacity=cap, untouched=True)
        assert e.value.code == umi._lib.UMI_ERR_ARG and "capacity" in str(e.value)
        assert [int(x) for x in ctx.junction_counts] == [0, t, 0, 0]
        with pytest.raises(umi.UmiHipError) as e:
            host_call(ctx, m, 5, capacity=cap)
        assert e.value.code == umi._lib.UMI_ERR_ARG and [int(x) for x in ctx.junction_counts] == [0, t, 0, 0]
    same(device_call(ctx, m, 5, capacity=t), exp)


def test_empty_calls(ctx):
    e32, e8, i32 = np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.int32)
    for off in ([0], [0, 0, 0]):
        nb = len(off) - 1
        got = ctx.junction_matrix(i32, i32, e32, [0], e32, e8, e32, off, np.zeros(nb, np.uint32), 0)
        assert all(len(a) == 0 for a in got[0] + got[1]) and not got[2].any()
    assert not ctx.junction_matrix_device(0, 0, 0, 0, 0, 0, 0, 0, [0], 0, 3, 0, 0, 0, 0, 0, 0, 0, 0).any()  # (no bucket: no pointer is looked at)
    assert not ctx.junction_matrix_device(0, 0, 0, 0, 0, 5, 0, 0, [0, 0], 0, 3, 0, 0, 0, 0, 0, 0, 0, 0).any()
    m = jm.make_inputs(2, [3, 4], 2)
    none = dict(m, read_ref=i32, read_pos=i32, cigar=e32, cigar_off=np.zeros(1, np.uint64), read_entry=e32)
    got = host_call(ctx, none, 2)
    assert not got[2].any()
    assert not ctx.junction_matrix_device(0, 0, 0, 0, 0, 0, 0, 0, m["off"], 0, 2, 0, 0, 0, 0, 0, 0, 0, 0).any()  # (no read)
    unstaged = dict(m, read_entry=np.full(len(m["read_entry"]), jm.UNSTAGED, np.uint32))
    got = both(ctx, unstaged, 2)
    assert not got[2].any()


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    m = jm.make_inputs(6, [3, 40, 1, 33, 7] * 20, 5, filtered=0, removed=0, unstaged=0)
    n, nr = len(m["kept"]), len(m["read_ref"])
    a, b, c = nr // 3, nr // 2, nr - 5

    def raises(word, code=umi._lib.UMI_ERR_ARG, **changed):
        x = dict(m, **changed)
        for call in ("host", "device"):
            with pytest.raises(umi.UmiHipError) as e:
                if call == "host":
                    host_call(ctx, x, 5)
                else:
                    device_call(ctx, x, 5, untouched=True)
            assert e.value.code == code and word in str(e.value), str(e.value)

    def changed(name, at, values):
        v = m[name].copy()
        v[at] = values
        return {name: v}
    raises("read %d: read_ref < 0" % a, **changed("read_ref", [a, c], -1))
    word_of = lambda i: int(m["cigar_off"][i])
    for op in (9, 15):
        raises("read %d: a CIGAR op code above 8" % b, **changed("cigar", [word_of(b), word_of(c)], (4 << 4) | op))
    for value in (n, n + 7, 0xFFFFFFFE):
        raises("read %d: its read_entry" % a, **changed("read_entry", [a, c], value))
    first = int(np.flatnonzero(m["read_entry"] == m["read_entry"][a])[0])
    raises("read %d: the root" % first, **changed("root", int(m["read_entry"][a]), n))
    off = m["cigar_off"].copy()
    off[b] = off[b + 1] + 1
    raises("read %d: cigar_off falls" % b, code=umi._lib.UMI_ERR_ORDER, cigar_off=off)
    # the smallest read of any kind is told
    x = changed("read_ref", c, -1)
    x.update(changed("read_entry", a, n))
    raises("read %d: its read_entry" % a, **x)
    x = changed("read_ref", a, -1)
    x.update(changed("read_entry", c, n))
    raises("read %d: read_ref" % a, **x)
    # the buckets
    full = np.flatnonzero(np.diff(m["off"].astype(np.int64)))
    raises("3 non-empty buckets", **changed("col", full[:3], 5))
    boff = m["off"].copy()
    boff[5] = boff[6] + 1
    raises("monotone", off=boff)
    boff = m["off"].copy()
    boff[0] = 1
    raises("bucket_off[0]", off=boff)
    with pytest.raises(umi.UmiHipError) as e:
        host_call(ctx, m, 0)
    assert e.value.code == umi._lib.UMI_ERR_ARG
    # a null pointer, through the C interface: nothing is touched
    lib, p = umi.load(), umi._lib.ptr
    cap = n_words_N(m)
    outs = [np.full(cap, 7, np.int32) for _ in range(3)] + [np.full(cap, 7, np.uint32) for _ in range(3)] + [np.full(cap, 7, np.uint64)]
    kinds = [C.c_int32] * 3 + [C.c_uint32] * 3 + [C.c_uint64]
    args = [p(m["read_ref"], C.c_int32), p(m["read_pos"], C.c_int32), p(m["cigar"], C.c_uint32), p(m["cigar_off"], C.c_uint64),
            p(m["read_entry"], C.c_uint32), nr, p(m["kept"], C.c_uint8), p(m["root"], C.c_uint32), p(m["off"], C.c_uint64),
            len(m["off"]) - 1, p(m["col"], C.c_uint32), 5, cap] + [p(o, k) for o, k in zip(outs, kinds)]
    counts = np.full(4, 99, np.uint64)
    for i in (0, 1, 2, 3, 4, 6, 7, 8, 10, 13, 14, 15, 16, 17, 18, 19):
        x = list(args)
        x[i] = None
        assert lib.umi_junction_matrix(ctx._h, *x, p(counts, C.c_uint64)) == umi._lib.UMI_ERR_ARG, i
    assert lib.umi_junction_matrix(ctx._h, *args, None) == umi._lib.UMI_ERR_ARG
    assert lib.umi_junction_matrix(None, *args, p(counts, C.c_uint64)) == umi._lib.UMI_ERR_ARG
    x = list(args)
    x[5] = 1 << 32
    assert lib.umi_junction_matrix(ctx._h, *x, p(counts, C.c_uint64)) == umi._lib.UMI_ERR_ARG
    x = list(args)
    x[9] = 1 << 30
    assert lib.umi_junction_matrix(ctx._h, *x, p(counts, C.c_uint64)) == umi._lib.UMI_ERR_ARG
    assert all((o == 7).all() for o in outs) and (counts == 99).all()
    # the context is as good as before
    both(ctx, m, 5)


def test_device_form_on_a_stream_and_a_multi_device_context(ctx):
    import torch
    import umi_collapse_rs_amd as umi
    m = jm.make_inputs(8, [3, 40, 1, 33, 7] * 20, 5)
    exp = jm.model_of(m)
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, m, 5, stream=s.cuda_stream), exp)
    c = umi.Context([0, 0])
    try:
        same(host_call(c, m, 5), exp)
        same(device_call(c, m, 5), exp)
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
    t_keys, t_freq = dev(keys), dev(freq)
    t_kept = torch.zeros(len(keys), dtype=torch.uint8, device="cuda:0")
    t_root = torch.zeros(len(keys), dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_freq.data_ptr(), off, 12, t_kept.data_ptr(), t_root.data_ptr(),
                                 k=1, stream=s.cuda_stream)
    both(ctx, jm.make_inputs(8, [3, 40, 1, 33, 7] * 20, 5), 5)
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all() and stats["n_kept"] == int(okept.sum())
    # ... and the junctions over that call's own result: a read per entry
    n, nb = len(keys), len(off) - 1
    rng = np.random.default_rng(3)
    take = rng.permutation(n)[:3000]
    ref, rpos, words, woff = jm.make_reads(rng, jm.make_pool(rng), rng.choice([0, 1, 2], len(take)))
    m = dict(read_ref=ref, read_pos=rpos, cigar=words, cigar_off=woff, read_entry=take.astype(np.uint32), kept=okept,
             root=oroot.astype(np.uint32), off=off, col=(np.arange(nb) % 13).astype(np.uint32))
    both(ctx, m, 13)
