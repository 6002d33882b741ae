"""umi_assign_genes_transcripts / umi_assign_genes_transcripts_device on the GPU against tests/transcript_model.py:
gene, status and counts by exact equality, both forms, the device form between guard bytes and with its inputs looked
at afterwards.  The fuzz inputs are transcript_model.fuzz_annotation() / fuzz_reads() (tests/
test_transcript_model_cpu.py checks what they hold); the hand-written cases are tests/transcript_cases.py's, each
named after the way the kernel can go wrong."""
import numpy as np
import pytest

import annotation_model as am
import transcript_cases as tc
import transcript_model as tm

pytestmark = pytest.mark.gpu
FIELDS = ("gene", "status", "counts")
GUARD, FILL, FILL32 = 64, 0x5A, -0x5A5A5A5B
N_TR = tm.n_transcripts_of(tm.fuzz_annotation())


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


def device_call(ctx, exons, n_genes, n_tr, mode, arrays, stream=0):
    """the device form on outputs with guard bytes before and behind; checks that they are untouched and that the
    inputs are as they were"""
    import torch
    ref, pos, rev, cigar, off = arrays
    n = len(ref)
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene = torch.full((n + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
    status = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    counts = ctx.assign_genes_transcripts_device(exons, n_genes, n_tr, mode, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                                                 ins[3].data_ptr() if len(cigar) else 0, ins[4].data_ptr(), n,
                                                 gene.data_ptr() + 4 * GUARD, status.data_ptr() + GUARD, stream=stream)
    torch.cuda.synchronize()
    gene_h, status_h = gene.cpu().numpy(), status.cpu().numpy()
    for h, fill in ((gene_h, FILL32), (status_h, FILL)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
    for t, a in zip(ins, (ref, pos, rev, cigar.view(np.int32), off.view(np.int64))):
        assert (t.cpu().numpy() == a).all()
    return {"gene": gene_h[GUARD:GUARD + n], "status": status_h[GUARD:GUARD + n], "counts": counts}


def both(ctx, exons, reads, mode, n_genes=None, n_tr=None):
    """both forms against the model; returns [(status, gene)]"""
    exons, reads = list(exons), list(reads)
    n_genes = am.n_genes_of(tm.overlap_exons(exons)) if n_genes is None else n_genes
    n_tr = tm.n_transcripts_of(exons) if n_tr is None else n_tr
    exp = tm.assign_all(exons, reads, mode)
    arrays = am.pack_reads(reads)
    got = ctx.assign_genes_transcripts(exons, n_genes, n_tr, mode, *arrays)
    same(got, exp)
    same(device_call(ctx, exons, n_genes, n_tr, mode, arrays), exp)
    return [(int(s), int(g)) for s, g in zip(got["status"], got["gene"])]


def fuzz_call(c, mode=tm.FORWARD):
    return c.assign_genes_transcripts(list(tm.fuzz_annotation()), tm.N_GENES, N_TR, mode, *am.pack_reads(tm.fuzz_reads()))


# ---- the fuzz -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(tm.MODES))
def test_fuzz_against_the_model(ctx, mode):
    exons, arrays = list(tm.fuzz_annotation()), am.pack_reads(tm.fuzz_reads())
    exp = tm.fuzz_expected(tm.MODES[mode])
    same(ctx.assign_genes_transcripts(exons, tm.N_GENES, N_TR, tm.MODES[mode], *arrays), exp)
    same(device_call(ctx, exons, tm.N_GENES, N_TR, tm.MODES[mode], arrays), exp)


# ---- the hand-written cases -----------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(tc.CASES))
def test_case(ctx, name):
    exons, reads, want = tc.CASES[name]
    for mode in (tm.FORWARD, tm.REVERSE, tm.UNSTRANDED):
        got = both(ctx, exons, reads, mode)
        if want is not None and mode != tm.REVERSE:  # (the cases' reads lie on their transcripts' strand)
            assert got == want


def test_the_overlap_rule_says_otherwise_where_the_rules_differ(ctx):
    for name, theirs in (("fits A and grazes B", [tm.SEVERAL, tm.SEVERAL]), ("overlaps but fits nothing", [tm.ASSIGNED, tm.ASSIGNED])):
        exons, reads, want = tc.CASES[name]
        got = ctx.assign_genes(tm.overlap_exons(exons), am.n_genes_of(tm.overlap_exons(exons)), tm.FORWARD, *am.pack_reads(reads))
        assert list(map(int, got["status"])) == theirs and theirs != [s for s, _ in want]


def test_strands(ctx):
    j = tc.J
    ex = tc.tr(0, 0, [(500, 600), (300, 400), (100, 200)], "-") + tc.tr(1, 1, [(100, 200), (300, 400)], ".", ref=1)
    reads = [tc.R(190, *j), tc.R(190, *j, rev=True), tc.R(190, *j, ref=1), tc.R(190, *j, ref=1, rev=True)]
    assert [g for _, g in both(ctx, ex, reads, tm.FORWARD)] == [-1, 0, 1, 1]
    assert [g for _, g in both(ctx, ex, reads, tm.REVERSE)] == [0, -1, 1, 1]
    assert [g for _, g in both(ctx, ex, reads, tm.UNSTRANDED)] == [0, 0, 1, 1]


# ---- the table's size, the top, the grid ----------------------------------------------------------------

def test_a_comb_beyond_the_top_and_the_top_changes_nothing(ctx):
    exons, reads = tc.comb()
    assert len({(e[1], e[2]) for e in exons}) == 2 * am.GENE_TOP_CAP + 1
    exp, arrays = tm.assign_all(exons, reads, tm.FORWARD), am.pack_reads(reads)
    fuzz = tm.fuzz_expected(tm.FORWARD)
    try:
        for top in (0, 1):
            ctx.set_option("gene_top", top)
            same(ctx.assign_genes_transcripts(exons, 50, tm.n_transcripts_of(exons), tm.FORWARD, *arrays), exp)
            same(fuzz_call(ctx), fuzz)
        ctx.set_option("gene_top", 0)
        same(device_call(ctx, exons, 50, tm.n_transcripts_of(exons), tm.UNSTRANDED, arrays), tm.assign_all(exons, reads, tm.UNSTRANDED))
    finally:
        ctx.set_option("gene_top", 1)


@pytest.mark.parametrize("cus", [1, 3])
def test_grid_cus(ctx, cus):
    """5,000 reads are five trips of one CU's two blocks: the results are the model's and, byte for byte, the default grid's"""
    import umi_collapse_rs_amd as umi
    default = fuzz_call(ctx)
    c = umi.Context(0)
    try:
        c.set_option("grid_cus", cus)
        for top in (1, 0):
            c.set_option("gene_top", top)
            got = fuzz_call(c)
            same(got, tm.fuzz_expected(tm.FORWARD))
            assert all(got[f].tobytes() == default[f].tobytes() for f in FIELDS)
        same(device_call(c, list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.REVERSE, am.pack_reads(tm.fuzz_reads())),
             tm.fuzz_expected(tm.REVERSE))
    finally:
        c.close()


# ---- the contract ---------------------------------------------------------------------------------------

def test_no_reads_touch_nothing(ctx):
    import torch
    gene = torch.full((8,), FILL32, dtype=torch.int32, device="cuda:0")
    counts = ctx.assign_genes_transcripts_device(list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.FORWARD, 0, 0, 0, 0, 0, 0,
                                                 gene.data_ptr(), 0)
    torch.cuda.synchronize()
    assert list(counts) == [0, 0, 0] and (gene.cpu().numpy() == FILL32).all()
    got = ctx.assign_genes_transcripts(list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.FORWARD, *am.pack_reads([]))
    assert len(got["gene"]) == 0 and list(got["counts"]) == [0, 0, 0]


def test_no_exons_every_read_is_none(ctx):
    reads = list(tm.fuzz_reads()[:300])
    for mode in (tm.FORWARD, tm.UNSTRANDED):
        got = both(ctx, [], reads, mode, n_genes=0, n_tr=0)
        assert got == [(tm.NONE, -1)] * 300
    assert both(ctx, [], reads, tm.FORWARD, n_genes=5, n_tr=9) == [(tm.NONE, -1)] * 300


def test_more_transcripts_than_used(ctx):
    exons, arrays = list(tm.fuzz_annotation()), am.pack_reads(tm.fuzz_reads())
    for n_tr in (N_TR + 1, 10 ** 9):
        same(ctx.assign_genes_transcripts(exons, tm.N_GENES + 7, n_tr, tm.FORWARD, *arrays), tm.fuzz_expected(tm.FORWARD))
    # the transcripts' numbers need not be dense
    sparse = [e[:5] + (e[5] * 1000 + 5,) for e in exons]
    same(device_call(ctx, sparse, tm.N_GENES, 1000 * N_TR, tm.FORWARD, arrays), tm.fuzz_expected(tm.FORWARD))


def test_device_form_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.REVERSE, am.pack_reads(tm.fuzz_reads()), stream=s.cuda_stream),
         tm.fuzz_expected(tm.REVERSE))


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the assignment lets it end first, and its result is still
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
    same(fuzz_call(ctx), tm.fuzz_expected(tm.FORWARD))
    same(device_call(ctx, list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.FORWARD, am.pack_reads(tm.fuzz_reads())),
         tm.fuzz_expected(tm.FORWARD))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        same(fuzz_call(c, tm.UNSTRANDED), tm.fuzz_expected(tm.UNSTRANDED))
        same(device_call(c, list(tm.fuzz_annotation()), tm.N_GENES, N_TR, tm.UNSTRANDED, am.pack_reads(tm.fuzz_reads())),
             tm.fuzz_expected(tm.UNSTRANDED))
    finally:
        c.close()


# ---- errors: the outputs stay as they were --------------------------------------------------------------

def raw_call(ctx, exons, n_genes, n_tr, arrays, gene, status, counts):
    """the plain form through ctypes, on the caller's own output arrays; the return code and the message"""
    import ctypes as C
    import umi_collapse_rs_amd as umi
    lib, p = umi.load(), umi._lib.ptr
    ex = ctx._exon_arrays(exons) + [np.array([e[5] for e in exons], np.int32)]
    rc = lib.umi_assign_genes_transcripts(ctx._h, p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8),
                                          p(ex[4], C.c_int32), p(ex[5], C.c_int32), len(exons), n_genes, n_tr, tm.FORWARD,
                                          p(arrays[0], C.c_int32), p(arrays[1], C.c_int32), p(arrays[2], C.c_uint8),
                                          p(arrays[3], C.c_uint32), p(arrays[4], C.c_uint64), len(arrays[0]), p(gene, C.c_int32),
                                          p(status, C.c_uint8), p(counts, C.c_uint64))
    return rc, lib.umi_last_error().decode()


def test_errors_leave_the_outputs_as_they_were(ctx):
    import umi_collapse_rs_amd as umi
    ARG, ORDER = umi._lib.UMI_ERR_ARG, umi._lib.UMI_ERR_ORDER
    exons = list(tm.fuzz_annotation())
    reads = list(tm.fuzz_reads()[:3000])
    ref, pos, rev, cigar, off = am.pack_reads(reads)
    t0 = exons[0][5]
    other_ref, other_strand = (exons[0][0] + 1) % 3, "-" if exons[0][3] != "-" else "+"
    bad_ref, bad_cigar, bad_cigar2, bad_off, bad_off2 = ref.copy(), cigar.copy(), cigar.copy(), off.copy(), off.copy()
    bad_ref[[1234, 2500]] = -1, -7
    bad_cigar[[int(off[1500]), int(off[1709])]] = 5 << 4 | 9
    bad_cigar2[int(off[1501]) - 1] = 5 << 4 | 15  # the last word of read 1500
    bad_off[700] = bad_off[701] + 1  # read 699 runs into read 700's words (legal), read 700 runs backwards
    bad_off2[100] = bad_off2[-1] + 1000  # beyond the array: nothing is read there
    cases = [
        (exons + [(0, 1, 2, "+", 0, N_TR)], (ref, pos, rev, cigar, off), ARG, "transcript %d outside" % N_TR),
        (exons + [(0, 1, 2, "+", 0, -1)], (ref, pos, rev, cigar, off), ARG, "transcript -1 outside"),
        (exons + [(other_ref, 1, 2, exons[0][3], exons[0][4], t0)], (ref, pos, rev, cigar, off), ARG, "two references"),
        (exons + [(exons[0][0], 1, 2, other_strand, exons[0][4], t0)], (ref, pos, rev, cigar, off), ARG, "two strands"),
        (exons + [(exons[0][0], 1, 2, exons[0][3], exons[0][4] + 1, t0)], (ref, pos, rev, cigar, off), ARG, "two genes"),
        (exons, (bad_ref, pos, rev, cigar, off), ARG, "read 1234"),
        (exons, (ref, pos, rev, bad_cigar, off), ARG, "read 1500"),
        (exons, (ref, pos, rev, bad_cigar2, off), ARG, "read 1500"),
        (exons, (ref, pos, rev, cigar, bad_off), ORDER, "read 700"),
        (exons, (ref, pos, rev, cigar, bad_off2), ORDER, "read 99"),
    ]
    for ex, arrays, code, word in cases:
        gene, status = np.full(3000, FILL32, np.int32), np.full(3000, FILL, np.uint8)
        counts = np.full(3, 77, np.uint64)
        rc, msg = raw_call(ctx, ex, tm.N_GENES, N_TR, arrays, gene, status, counts)
        assert rc == code and word in msg, (word, rc, msg)
        assert (gene == FILL32).all() and (status == FILL).all(), word
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes_transcripts(ex, tm.N_GENES, N_TR, tm.FORWARD, *arrays)
        assert e.value.code == code and word in str(e.value)
    # op code 8 is legal; the device form tells the same; the context is as good as before
    ok = cigar.copy()
    ok[int(off[1500])] = 5 << 4 | 8
    ctx.assign_genes_transcripts(exons, tm.N_GENES, N_TR, tm.FORWARD, ref, pos, rev, ok, off)
    import torch
    bad = ref.copy()
    bad[77] = -1
    ins = [dev(bad), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene, status = torch.zeros(3000, dtype=torch.int32, device="cuda:0"), torch.zeros(3000, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_transcripts_device(exons, tm.N_GENES, N_TR, tm.FORWARD, *(t.data_ptr() for t in ins), 3000, gene.data_ptr(),
                                            status.data_ptr())
    assert e.value.code == ARG and "read 77" in str(e.value)
    # a transcript error is found before anything is launched: the device form's outputs are as they were
    gene.fill_(FILL32)
    torch.cuda.synchronize()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_transcripts_device(cases[2][0], tm.N_GENES, N_TR, tm.FORWARD, *(t.data_ptr() for t in ins), 3000,
                                            gene.data_ptr(), status.data_ptr())
    torch.cuda.synchronize()
    assert e.value.code == ARG and "two references" in str(e.value) and (gene.cpu().numpy() == FILL32).all()
    exp = tm.fuzz_expected(tm.FORWARD)
    same(ctx.assign_genes_transcripts(exons, tm.N_GENES, N_TR, tm.FORWARD, ref, pos, rev, cigar, off),
         {"gene": exp["gene"][:3000], "status": exp["status"][:3000],
          "counts": np.bincount(exp["status"][:3000], minlength=3).astype(np.uint64)})
