"""umi_correct_barcodes / umi_correct_barcodes_device on the GPU against tests/barcode_model.py: match, status
and counts by exact equality, and match against umi_correct_umis (the all-against-all call) as a second
oracle.  The inputs are barcode_model.gpu_inputs(); tests/test_barcode_model_cpu.py checks what they hold."""
import numpy as np
import pytest

import barcode_model as bm

pytestmark = pytest.mark.gpu
FIELDS = ("match", "status", "counts")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def same(got, exp, fields=FIELDS):
    for f in fields:
        a, b = np.asarray(got[f]), np.asarray(exp[f])
        assert a.shape == b.shape, (f, a.shape, b.shape)
        bad = np.flatnonzero(a != b)
        assert not len(bad), (f, bad[:10], a[bad[:10]], b[bad[:10]])


@pytest.mark.parametrize("mm", [0, 1])
@pytest.mark.parametrize("name", sorted(bm.gpu_inputs()))
def test_against_the_model(ctx, name, mm):
    _, L, wl, reads = bm.gpu_inputs()[name]
    same(ctx.correct_barcodes(reads, L, wl, mm), bm.expected(name, mm))


@pytest.mark.parametrize("mm", [0, 1])
@pytest.mark.parametrize("n", bm.N_READS)
def test_read_counts(ctx, n, mm):
    _, L, wl, reads = bm.gpu_inputs()["reads10000"]
    exp = bm.expected("reads10000", mm)
    got = ctx.correct_barcodes(reads[:n * L], L, wl, mm)
    assert len(got["match"]) == n and int(got["counts"].sum()) == n
    same(got, {"match": exp["match"][:n], "status": exp["status"][:n],
               "counts": np.bincount(exp["status"][:n], minlength=4).astype(np.uint64)})


@pytest.mark.parametrize("mm", [0, 1])
@pytest.mark.parametrize("name", ["L15", "L16", "L17", "L32", "n_wl2", "n_wl64", "clustered_low", "full3"])
def test_match_is_what_the_all_against_all_call_gives(ctx, name, mm):
    _, L, wl, reads = bm.gpu_inputs()[name]
    got = ctx.correct_barcodes(reads, L, wl, mm)
    assert (got["match"] == ctx.correct_umis(reads, L, wl, max_mismatches=mm, min_distance=1)["match"]).all()


def run(ctx, wl, reads, mm=1):
    L = len(wl[0])
    raw = np.frombuffer("".join(reads).encode(), np.uint8)
    got = ctx.correct_barcodes(raw, L, wl, mm)
    same(got, bm.correct(raw, L, wl, mm))
    return list(map(int, got["status"])), list(map(int, got["match"]))


def test_all_a_and_all_t_of_32_bases(ctx):
    # the packed keys are 0 and all ones: neither may stand for an empty slot, and no shift reaches 64
    wl = ["A" * 32, "T" * 32]
    reads = ["A" * 32, "T" * 32, "A" * 31 + "T", "T" + "A" * 31, "T" * 31 + "G", "N" + "T" * 31, "A" * 31 + "N",
             "C" * 32, "A" * 16 + "T" * 16, "NN" + "A" * 30]
    assert run(ctx, wl, reads) == ([0, 0, 1, 1, 1, 1, 1, 2, 2, 2], [0, 1, 0, 0, 1, 1, 0, -1, -1, -1])
    assert run(ctx, ["T" * 32], ["A" * 32, "T" * 32])[0] == [2, 0]
    assert run(ctx, ["A" * 32], ["A" * 32, "T" * 32])[0] == [0, 2]
    assert run(ctx, ["A"], ["A", "C", "N", "T"]) == ([0, 1, 1, 1], [0, 0, 0, 0])


@pytest.mark.parametrize("L", [1, 2, 16, 17, 32])
def test_corrected_base_at_the_first_and_the_last_position(ctx, L):
    wl = ["ACGT" * 8, "TGCA" * 8, "GGCC" * 8]
    wl = [w[:L] for w in wl][:3 if L > 1 else 1]
    sub = {"A": "C", "C": "G", "G": "T", "T": "A"}
    w = wl[-1]
    first, last = sub[w[0]] + w[1:], w[:-1] + sub[w[-1]]
    st, m = run(ctx, wl, [w, first, last, "N" + w[1:], w[:-1] + "N"])
    if L > 2:  # (shorter ones are next to each other: the model has decided)
        assert st == [0, 1, 1, 1, 1] and m == [len(wl) - 1] * 5
    st0 = run(ctx, wl, [first, last], mm=0)[0]
    if L > 2:
        assert st0 == [2, 2]


def test_ambiguous_pairs_made_on_purpose(ctx):
    for wl, read in (bm.AMBIGUOUS_SAME_POSITION, bm.AMBIGUOUS_DIFFERENT_POSITIONS):
        assert run(ctx, wl, [read] * 70) == ([3] * 70, [-1] * 70)
        assert run(ctx, wl, [read] * 3, mm=0) == ([2] * 3, [-1] * 3)


def test_two_runs_give_identical_bytes(ctx):
    _, L, wl, reads = bm.gpu_inputs()["clustered_high"]
    a, b = ctx.correct_barcodes(reads, L, wl), ctx.correct_barcodes(reads, L, wl)
    for f in FIELDS:
        assert a[f].tobytes() == b[f].tobytes()


# ---- the device form ------------------------------------------------------------------------------------

def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_call(ctx, reads, L, wl, mm=1, shift=0, want_status=True, stream=0):
    """the device form on buffers with a guard band filled beforehand; checks that nothing outside the outputs'
    own extent (and no output that was not asked for) was written, and that the input is as it was"""
    import torch
    n, G, fill = len(reads) // L, 64, 0x5A
    raw = torch.full((len(reads) + shift + G,), fill, dtype=torch.uint8, device="cuda:0")
    raw[shift:shift + len(reads)] = dev(reads)
    match = torch.full((n + G,), -0x5A5A5A5B, dtype=torch.int32, device="cuda:0")
    status = torch.full((n + G,), fill, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    counts = ctx.correct_barcodes_device(raw.data_ptr() + shift, n, L, wl, mm, match.data_ptr(),
                                         status.data_ptr() if want_status else 0, stream=stream)
    torch.cuda.synchronize()
    raw_h, match_h, status_h = (t.cpu().numpy() for t in (raw, match, status))
    assert (match_h[n:] == -0x5A5A5A5B).all() and (status_h[n if want_status else 0:] == fill).all()
    assert (raw_h[:shift] == fill).all() and (raw_h[shift + len(reads):] == fill).all()
    assert (raw_h[shift:shift + len(reads)] == reads).all()
    res = {"match": match_h[:n], "counts": counts}
    if want_status:
        res["status"] = status_h[:n]
    return res


@pytest.mark.parametrize("kw", [dict(), dict(want_status=False), dict(shift=1), dict(shift=3, mm=0)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()) or "all")
def test_device_form_equals_host_form(ctx, kw):
    _, L, wl, reads = bm.gpu_inputs()["L17"]
    mm = kw.get("mm", 1)
    got = device_call(ctx, reads, L, wl, **kw)
    host = ctx.correct_barcodes(reads, L, wl, mm)
    same(got, host, [f for f in FIELDS if f in got])
    same(host, bm.expected("L17", mm))


def test_device_form_on_a_stream(ctx):
    import torch
    _, L, wl, reads = bm.gpu_inputs()["L16"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, reads, L, wl, stream=s.cuda_stream), bm.expected("L16", 1))


# ---- errors ---------------------------------------------------------------------------------------------

def test_bad_read_byte_names_the_smallest_read_and_writes_nothing(ctx):
    import torch
    import umi_collapse_rs_amd as umi
    _, L, wl, reads = bm.gpu_inputs()["L17"]
    n = len(reads) // L
    bad = reads.copy()
    for r, b, ch in ((1900, 3, ord("x")), (1234, 16, ord("a")), (1234, 5, 0), (1500, 0, ord("n"))):
        bad[r * L + b] = ch
    outs = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
            torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")]
    d_in = dev(bad)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes_device(d_in.data_ptr(), n, L, wl, 1, outs[0].data_ptr(), outs[1].data_ptr())
    assert e.value.code == umi._lib.UMI_ERR_CHAR
    assert "Unknown character in cell barcode: 0 (read 1234)" in str(e.value)
    torch.cuda.synchronize()
    assert (outs[0].cpu().numpy() == 0x5A5A5A5A).all() and (outs[1].cpu().numpy() == 0x5A).all()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes(bad, L, wl)
    assert e.value.code == umi._lib.UMI_ERR_CHAR and "(read 1234)" in str(e.value)
    same(ctx.correct_barcodes(reads, L, wl), bm.expected("L17", 1))  # the context is as good as before


@pytest.mark.parametrize("name", ["L16", "L32"])
def test_duplicate_entry_names_the_smallest_and_writes_nothing(ctx, name):
    import torch
    import umi_collapse_rs_amd as umi
    _, L, wl, reads = bm.gpu_inputs()[name]
    n = len(reads) // L
    dup = wl.copy()
    # groups of equal entries: {7, 4000, 4500}, {100, 2000}, {3000, 3001}: 2000 is the smallest that equals an earlier one
    dup[4000] = dup[4500] = dup[7]
    dup[2000] = dup[100]
    dup[3001] = dup[3000]
    outs = [torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0"),
            torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")]
    d_in = dev(reads)
    for _ in range(2):  # (the message does not depend on scheduling)
        with pytest.raises(umi.UmiHipError) as e:
            ctx.correct_barcodes_device(d_in.data_ptr(), n, L, dup, 1, outs[0].data_ptr(), outs[1].data_ptr())
        assert e.value.code == umi._lib.UMI_ERR_ARG
        assert "duplicate entry in the barcode whitelist: entry 2000 equals an earlier one" in str(e.value)
    torch.cuda.synchronize()
    assert (outs[0].cpu().numpy() == 0x5A5A5A5A).all() and (outs[1].cpu().numpy() == 0x5A).all()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes(reads, L, ["A" * L, "A" * L])
    assert e.value.code == umi._lib.UMI_ERR_ARG and "entry 1 equals" in str(e.value)
    same(ctx.correct_barcodes(reads, L, wl), bm.expected(name, 1))


def test_bad_whitelist_byte(ctx):
    import umi_collapse_rs_amd as umi
    _, L, wl, reads = bm.gpu_inputs()["L17"]
    bad = wl.copy()
    bad[7, 4] = ord("N")
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes(reads, L, bad)
    assert e.value.code == umi._lib.UMI_ERR_CHAR and "Unknown character in whitelist: 78 (entry 7)" in str(e.value)


def test_argument_errors_with_a_context(ctx):
    import umi_collapse_rs_amd as umi
    _, L, wl, reads = bm.gpu_inputs()["L17"]
    for kw, word in ((dict(max_mismatches=-1), "max_mismatches"), (dict(max_mismatches=2), "max_mismatches")):
        with pytest.raises(umi.UmiHipError) as e:
            ctx.correct_barcodes(reads, L, wl, **kw)
        assert e.value.code == umi._lib.UMI_ERR_ARG and word in str(e.value)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes(reads, L, np.zeros(0, np.uint8))
    assert e.value.code == umi._lib.UMI_ERR_ARG and "empty" in str(e.value)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes(np.tile(np.frombuffer(b"A" * 33, np.uint8), 4), 33, ["C" * 33])
    assert e.value.code == umi._lib.UMI_ERR_ARG and "bc_len" in str(e.value)


# ---- other contexts -------------------------------------------------------------------------------------

def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the correction lets it end first, and its result is
    still handed out, and right, afterwards"""
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
    _, L, wl, reads = bm.gpu_inputs()["L17"]
    same(ctx.correct_barcodes(reads, L, wl), bm.expected("L17", 1))
    same(device_call(ctx, reads, L, wl), bm.expected("L17", 1))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    _, L, wl, reads = bm.gpu_inputs()["L16"]
    c = umi.Context([0, 0])
    try:
        same(c.correct_barcodes(reads, L, wl), bm.expected("L16", 1))
        same(device_call(c, reads, L, wl), bm.expected("L16", 1))
    finally:
        c.close()
