"""umi_correct_barcodes_multi / umi_correct_barcodes_multi_device on the GPU against tests/barcode_multi_model.py:
match, status, counts and exact_reads by exact equality.  The inputs are barcode_multi_model.gpu_inputs();
tests/test_barcode_multi_model_cpu.py checks what they hold."""
import numpy as np
import pytest

import barcode_model as bm
import barcode_multi_model as mm

pytestmark = pytest.mark.gpu
FIELDS = ("match", "status", "counts", "exact_reads")


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


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_call(ctx, reads, quals, L, wl, permille=975, pseudo=0, want_status=True, want_exact=True, shift=0, stream=0):
    """the device form on buffers with a guard band filled beforehand; checks that nothing outside the outputs' own
    extent (and no output that was not asked for) was written, and that the inputs are as they were"""
    import torch
    n, n_wl, G, fill = len(reads) // L, len(wl), 64, 0x5A
    raw = torch.full((len(reads) + shift + G,), fill, dtype=torch.uint8, device="cuda:0")
    raw[shift:shift + len(reads)] = dev(reads)
    qual = torch.full((len(reads) + shift + G,), fill, dtype=torch.uint8, device="cuda:0")
    qual[shift:shift + len(reads)] = dev(quals)
    match = torch.full((G + n + G,), -0x5A5A5A5B, dtype=torch.int32, device="cuda:0")
    status = torch.full((G + n + G,), fill, dtype=torch.uint8, device="cuda:0")
    exact = torch.full((G + n_wl + G,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    counts = ctx.correct_barcodes_multi_device(raw.data_ptr() + shift, qual.data_ptr() + shift, n, L, wl, permille, pseudo,
                                               match.data_ptr() + 4 * G, status.data_ptr() + G if want_status else 0,
                                               exact.data_ptr() + 4 * G if want_exact else 0, stream=stream)
    torch.cuda.synchronize()
    raw_h, qual_h, match_h, status_h, exact_h = (t.cpu().numpy() for t in (raw, qual, match, status, exact))
    assert (match_h[:G] == -0x5A5A5A5B).all() and (match_h[G + n:] == -0x5A5A5A5B).all()
    lo, hi = (G, G + n) if want_status else (0, 0)
    assert (status_h[:lo] == fill).all() and (status_h[hi:] == fill).all()
    lo, hi = (G, G + n_wl) if want_exact else (0, 0)
    assert (exact_h[:lo] == 0x5A5A5A5A).all() and (exact_h[hi:] == 0x5A5A5A5A).all()
    for h, src in ((raw_h, reads), (qual_h, quals)):
        assert (h[:shift] == fill).all() and (h[shift + len(reads):] == fill).all() and (h[shift:shift + len(reads)] == src).all()
    res = {"match": match_h[G:G + n], "counts": counts}
    if want_status:
        res["status"] = status_h[G:G + n]
    if want_exact:
        res["exact_reads"] = exact_h[G:G + n_wl].view(np.uint32)
    return res


@pytest.mark.parametrize("name", sorted(mm.gpu_inputs()))
def test_both_forms_against_the_model(ctx, name):
    _, L, wl, reads, quals = mm.gpu_inputs()[name]
    exp = mm.expected(name)
    same(ctx.correct_barcodes_multi(reads, quals, L, wl), exp)
    same(device_call(ctx, reads, quals, L, wl), exp)


@pytest.mark.parametrize("permille, pseudo", [(1000, 0), (0, 0), (500, 1), (975, 1), (975, 1000)])
@pytest.mark.parametrize("name", ["L17", "two_pass_L32", "full3_one_n", "no_exact", "hot"])
def test_other_parameters(ctx, name, permille, pseudo):
    _, L, wl, reads, quals = mm.gpu_inputs()[name]
    same(ctx.correct_barcodes_multi(reads, quals, L, wl, permille, pseudo), mm.expected(name, permille, pseudo))


@pytest.mark.parametrize("n", mm.N_READS)
def test_read_counts(ctx, n):
    _, L, wl, reads, quals = mm.gpu_inputs()["reads10000"]
    exp = mm.expected("reads10000") if n == 10000 else mm.correct_multi(reads[:n * L], quals[:n * L], L, wl)
    got = ctx.correct_barcodes_multi(reads[:n * L], quals[:n * L], L, wl)
    assert len(got["match"]) == n and int(got["counts"].sum()) == n and len(got["counts"]) == 5
    same(got, exp)
    if n:
        same(device_call(ctx, reads[:n * L], quals[:n * L], L, wl), exp)


def test_hand_made_cases(ctx):
    for name, (wl, reads, quals, permille, pseudo, status, match) in {**mm.hand_cases(), **mm.hand_quality_cases()}.items():
        L = len(wl[0])
        q = np.frombuffer(b"".join(quals) if quals is not None else bytes([33 + 30]) * (L * len(reads)), np.uint8)
        raw = np.frombuffer("".join(reads).encode(), np.uint8)
        got = ctx.correct_barcodes_multi(raw, q, L, wl, permille, pseudo)
        same(got, mm.correct_multi(raw, q, L, wl, permille, pseudo))
        assert (int(got["status"][-1]), int(got["match"][-1])) == (status, match), name


def test_first_three_statuses_are_the_plain_calls(ctx):
    _, L, wl, reads, quals = mm.gpu_inputs()["L16"]
    got, plain = ctx.correct_barcodes_multi(reads, quals, L, wl), ctx.correct_barcodes(reads, L, wl, 1)
    keep = plain["status"] != bm.AMBIGUOUS
    assert (got["status"][keep] == plain["status"][keep]).all() and (got["match"][keep] == plain["match"][keep]).all()
    assert (got["status"][~keep] >= 3).all()
    assert (got["counts"][:3] == plain["counts"][:3]).all() and int(got["counts"][3] + got["counts"][4]) == int(plain["counts"][3])


def test_two_runs_give_identical_bytes(ctx):
    for name in ("reads10000", "hot"):
        _, L, wl, reads, quals = mm.gpu_inputs()[name]
        a, b = ctx.correct_barcodes_multi(reads, quals, L, wl), ctx.correct_barcodes_multi(reads, quals, L, wl)
        for f in FIELDS:
            assert a[f].tobytes() == b[f].tobytes()


@pytest.mark.parametrize("kw", [dict(want_status=False), dict(want_exact=False), dict(want_status=False, want_exact=False),
                                dict(shift=1), dict(shift=3, permille=500, pseudo=1)],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_device_form_with_outputs_left_out_and_unaligned_inputs(ctx, kw):
    _, L, wl, reads, quals = mm.gpu_inputs()["L17"]
    got = device_call(ctx, reads, quals, L, wl, **kw)
    same(got, mm.expected("L17", kw.get("permille", 975), kw.get("pseudo", 0)), [f for f in FIELDS if f in got])


def test_device_form_on_a_stream(ctx):
    import torch
    _, L, wl, reads, quals = mm.gpu_inputs()["L16"]
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, reads, quals, L, wl, stream=s.cuda_stream), mm.expected("L16"))


# ---- refusals -------------------------------------------------------------------------------------------

class Outputs:
    """device outputs filled beforehand, to see that a refusal leaves them alone"""
    def __init__(self, n, n_wl):
        import torch
        self.match = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
        self.status = torch.full((n,), 0x5A, dtype=torch.uint8, device="cuda:0")
        self.exact = torch.full((n_wl,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")

    def untouched(self):
        import torch
        torch.cuda.synchronize()
        return all((t.cpu().numpy() == v).all() for t, v in ((self.match, 0x5A5A5A5A), (self.status, 0x5A), (self.exact, 0x5A5A5A5A)))


def refused(ctx, code, text, reads, quals, L, wl, permille=975, pseudo=0, no_qual=False):
    """both forms refuse with `code` and `text`; the device form's outputs stay as they were"""
    import umi_collapse_rs_amd as umi
    n = len(reads) // L
    out = Outputs(max(1, n), max(1, len(wl)))
    d_in, d_q = dev(reads), dev(quals)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.correct_barcodes_multi_device(d_in.data_ptr(), 0 if no_qual else d_q.data_ptr(), n, L, wl, permille, pseudo,
                                          out.match.data_ptr(), out.status.data_ptr(), out.exact.data_ptr())
    assert e.value.code == code and text in str(e.value), str(e.value)
    assert out.untouched()
    if not no_qual:
        with pytest.raises(umi.UmiHipError) as e:
            ctx.correct_barcodes_multi(reads, quals, L, wl, permille, pseudo)
        assert e.value.code == code and text in str(e.value), str(e.value)


def test_refusals_leave_the_outputs_alone(ctx):
    import umi_collapse_rs_amd as umi
    ARG, CHAR = umi._lib.UMI_ERR_ARG, umi._lib.UMI_ERR_CHAR
    _, L, wl, reads, quals = mm.gpu_inputs()["L17"]
    refused(ctx, ARG, "min_posterior_permille", reads, quals, L, wl, permille=1001)
    refused(ctx, ARG, "min_posterior_permille", reads, quals, L, wl, permille=-1)
    refused(ctx, ARG, "pseudocount", reads, quals, L, wl, pseudo=1001)
    refused(ctx, ARG, "pseudocount", reads, quals, L, wl, pseudo=-1)
    refused(ctx, ARG, "NULL", reads, quals, L, wl, no_qual=True)
    refused(ctx, ARG, "empty", reads, quals, L, np.zeros(0, np.uint8))
    refused(ctx, ARG, "bc_len", np.tile(np.frombuffer(b"A" * 33, np.uint8), 4), np.full(132, 70, np.uint8), 33, ["C" * 33])
    # a quality byte outside 33..126: the smallest read, its first bad byte
    bad = quals.copy()
    for r, b, ch in ((1900, 3, 32), (1234, 16, 127), (1234, 5, 10), (1500, 0, 255)):
        bad[r * L + b] = ch
    refused(ctx, CHAR, "Unknown character in cell barcode quality: 10 (read 1234)", reads, bad, L, wl)
    # a bad barcode byte of a smaller or the same read is reported in its place; of a later read, not
    for at, text in ((1233, "Unknown character in cell barcode: 120 (read 1233)"),
                     (1234, "Unknown character in cell barcode: 120 (read 1234)"),
                     (1235, "Unknown character in cell barcode quality: 10 (read 1234)")):
        bad_bc = reads.copy()
        bad_bc[at * L + 2] = ord("x")
        refused(ctx, CHAR, text, bad_bc, bad, L, wl)
    bad_bc = reads.copy()
    bad_bc[7 * L] = ord("n")
    refused(ctx, CHAR, "Unknown character in cell barcode: 110 (read 7)", bad_bc, quals, L, wl)
    # the list: a duplicate (the smallest entry that equals an earlier one), a byte outside ACGT
    dup = wl.copy()
    dup[4000] = dup[7]
    dup[2000] = dup[100]
    refused(ctx, ARG, "duplicate entry in the barcode whitelist: entry 2000 equals an earlier one", reads, bad, L, dup)
    odd = wl.copy()
    odd[7, 4] = ord("N")
    refused(ctx, CHAR, "Unknown character in whitelist: 78 (entry 7)", reads, quals, L, odd)
    # the context is as good as before, for both calls
    same(ctx.correct_barcodes_multi(reads, quals, L, wl), mm.expected("L17"))
    same(ctx.correct_barcodes(reads, L, wl), bm.correct(reads, L, wl, 1), ("match", "status", "counts"))


def test_no_reads(ctx):
    _, L, wl, _, _ = mm.gpu_inputs()["L16"]
    got = ctx.correct_barcodes_multi(np.zeros(0, np.uint8), np.zeros(0, np.uint8), L, wl)
    assert len(got["match"]) == 0 and (got["counts"] == 0).all() and len(got["counts"]) == 5
    counts = ctx.correct_barcodes_multi_device(0, 0, 0, L, wl, 975, 0, 0)
    assert (counts == 0).all()


# ---- other calls and contexts ---------------------------------------------------------------------------

def test_the_plain_call_answers_as_before_afterwards(ctx):
    for name in ("L16", "L32", "n_wl64"):
        _, L, wl, reads, quals = mm.gpu_inputs()[name]
        before = ctx.correct_barcodes(reads, L, wl, 1)
        same(ctx.correct_barcodes_multi(reads, quals, L, wl), mm.expected(name))
        after = ctx.correct_barcodes(reads, L, wl, 1)
        same(after, before, ("match", "status", "counts"))
        same(after, bm.correct(reads, L, wl, 1), ("match", "status", "counts"))
        assert len(after["counts"]) == 4
        same(ctx.correct_barcodes(reads, L, wl, 0), bm.correct(reads, L, wl, 0), ("match", "status", "counts"))


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the correction lets it end first, and its result is still
    handed out, and right, afterwards"""
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
    _, L, wl, reads, quals = mm.gpu_inputs()["L17"]
    same(ctx.correct_barcodes_multi(reads, quals, L, wl), mm.expected("L17"))
    same(device_call(ctx, reads, quals, L, wl), mm.expected("L17"))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    _, L, wl, reads, quals = mm.gpu_inputs()["L16"]
    c = umi.Context([0, 0])
    try:
        same(c.correct_barcodes_multi(reads, quals, L, wl), mm.expected("L16"))
        same(device_call(c, reads, quals, L, wl), mm.expected("L16"))
    finally:
        c.close()
