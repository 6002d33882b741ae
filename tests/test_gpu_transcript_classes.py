"""umi_assign_genes_transcripts_classes / umi_assign_genes_transcripts_classes_device on the GPU against
tests/transcript_intron_model.py: gene, status, tier, class and both sets of counts by exact equality, both forms, the
device form between guard bytes and with its inputs looked at afterwards.  The fuzz inputs are
transcript_intron_model.fuzz_annotation() / fuzz_reads() (tests/test_transcript_intron_model_cpu.py checks what they
hold)."""
import numpy as np
import pytest

import annotation_model as am
import intron_model as im
import transcript_intron_model as ti
import transcript_model as tm

pytestmark = pytest.mark.gpu
FIELDS = ("gene", "status", "tier", "cls", "counts", "class_counts")
PLAIN = ("gene", "status", "tier", "counts")
GUARD, FILL, FILL32 = 64, 0x5A, -0x5A5A5A5B
N_TR = tm.n_transcripts_of(tm.fuzz_annotation())
MODES = (tm.FORWARD, tm.REVERSE, tm.UNSTRANDED)


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


def device_call(ctx, exons, n_genes, n_tr, mode, introns, arrays, stream=0, classes=True):
    """the device form on outputs with guard bytes before and behind; checks that they are untouched, that the inputs
    are as they were and, without classes, that cls is as it was"""
    import torch
    ref, pos, rev, cigar, off = arrays
    n = len(ref)
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene = torch.full((n + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
    status, tier, cls = (torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    torch.cuda.synchronize()
    counts, class_counts = ctx.assign_genes_transcripts_classes_device(
        exons, n_genes, n_tr, mode, introns, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr() if len(cigar) else 0,
        ins[4].data_ptr(), n, gene.data_ptr() + 4 * GUARD, status.data_ptr() + GUARD, tier.data_ptr() + GUARD, cls.data_ptr() + GUARD,
        stream=stream, classes=classes)
    torch.cuda.synchronize()
    gene_h, status_h, tier_h, cls_h = gene.cpu().numpy(), status.cpu().numpy(), tier.cpu().numpy(), cls.cpu().numpy()
    for h, fill in ((gene_h, FILL32), (status_h, FILL), (tier_h, FILL), (cls_h, FILL)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
    for t, a in zip(ins, (ref, pos, rev, cigar.view(np.int32), off.view(np.int64))):
        assert (t.cpu().numpy() == a).all()
    out = {"gene": gene_h[GUARD:GUARD + n], "status": status_h[GUARD:GUARD + n], "tier": tier_h[GUARD:GUARD + n], "counts": counts}
    if classes:
        out["cls"], out["class_counts"] = cls_h[GUARD:GUARD + n], class_counts
    else:
        assert class_counts is None and (cls_h == FILL).all()  # (the poisoned cls is not touched)
    return out


def both(ctx, exons, reads, mode, introns, n_genes=None, n_tr=None, exp=None):
    """both forms against the model; returns the plain form's dict"""
    exons, reads = list(exons), list(reads)
    n_genes = am.n_genes_of(tm.overlap_exons(exons)) if n_genes is None else n_genes
    n_tr = tm.n_transcripts_of(exons) if n_tr is None else n_tr
    exp = ti.classify_all(exons, reads, mode, introns) if exp is None else exp
    arrays = am.pack_reads(reads)
    got = ctx.assign_genes_transcripts_classes(exons, n_genes, n_tr, mode, introns, *arrays)
    same(got, exp)
    same(device_call(ctx, exons, n_genes, n_tr, mode, introns, arrays), exp)
    return got


def fuzz_arrays():
    return am.pack_reads(ti.fuzz_reads())


def fuzz_call(c, mode=tm.FORWARD, introns=ti.EXON_FIRST, classes=True):
    return c.assign_genes_transcripts_classes(list(ti.fuzz_annotation()), ti.N_GENES, N_TR, mode, introns, *fuzz_arrays(), classes=classes)


# ---- the hand table -------------------------------------------------------------------------------------

@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_the_hand_table(ctx, introns):
    want = ti.hand_expected(ti.INTRONS[introns])
    got = both(ctx, ti.HAND_EXONS, ti.hand_reads(), tm.FORWARD, ti.INTRONS[introns], ti.HAND_N_GENES, ti.HAND_N_TRANSCRIPTS)
    assert [tuple(int(got[f][i]) for f in ("status", "gene", "tier", "cls")) for i in range(len(want))] == want
    for mode in (tm.REVERSE, tm.UNSTRANDED):
        both(ctx, ti.HAND_EXONS, ti.hand_reads(), mode, ti.INTRONS[introns], ti.HAND_N_GENES, ti.HAND_N_TRANSCRIPTS)


# ---- the fuzz -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("introns", sorted(ti.INTRONS))
@pytest.mark.parametrize("mode", sorted(tm.MODES))
def test_fuzz_against_the_model(ctx, mode, introns):
    m, n = tm.MODES[mode], ti.INTRONS[introns]
    exons, arrays = list(ti.fuzz_annotation()), fuzz_arrays()
    exp = ti.fuzz_expected(m, n)
    same(ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, m, n, *arrays), exp)
    same(device_call(ctx, exons, ti.N_GENES, N_TR, m, n, arrays), exp)


@pytest.mark.parametrize("mode", sorted(tm.MODES))
def test_against_the_existing_calls_on_the_same_arrays(ctx, mode):
    m = tm.MODES[mode]
    exons, arrays = list(ti.fuzz_annotation()), fuzz_arrays()
    off = ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, m, ti.OFF, *arrays)
    fit = ctx.assign_genes_transcripts(exons, ti.N_GENES, N_TR, m, *arrays)
    assert off["gene"].tobytes() == fit["gene"].tobytes() and off["status"].tobytes() == fit["status"].tobytes()
    assert not off["tier"].any() and list(off["counts"]) == [int(fit["counts"][0]), 0, int(fit["counts"][1]), int(fit["counts"][2])]
    full = ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, m, ti.ALL, *arrays)
    body = ctx.assign_genes_introns(tm.overlap_exons(exons), ti.N_GENES, m, im.ALL, *arrays)
    assert full["gene"].tobytes() == body["gene"].tobytes() and full["status"].tobytes() == body["status"].tobytes()
    assert list(full["counts"][2:]) == list(body["counts"][2:]) and int(full["counts"][:2].sum()) == int(body["counts"][:2].sum())


@pytest.mark.parametrize("introns", sorted(ti.INTRONS))
def test_without_classes(ctx, introns):
    n = ti.INTRONS[introns]
    exons, arrays = list(ti.fuzz_annotation()), fuzz_arrays()
    for mode in (tm.FORWARD, tm.UNSTRANDED):
        exp = ti.fuzz_expected(mode, n)
        got = fuzz_call(ctx, mode, n, classes=False)
        assert sorted(got) == sorted(PLAIN)
        same(got, exp, PLAIN)
        same(device_call(ctx, exons, ti.N_GENES, N_TR, mode, n, arrays, classes=False), exp, PLAIN)


# ---- the tables' sizes, the tops, the grid, the waves ---------------------------------------------------

def test_the_tops_change_nothing(ctx):
    exp = {n: ti.fuzz_expected(tm.FORWARD, n) for n in (ti.EXON_FIRST, ti.ALL)}
    try:
        for top, body_top in ((0, 0), (0, 1), (1, 0), (1, 1)):
            ctx.set_option("gene_top", top)
            ctx.set_option("gene_body_top", body_top)
            for n in exp:
                same(fuzz_call(ctx, tm.FORWARD, n), exp[n])
            same(fuzz_call(ctx, tm.FORWARD, ti.EXON_FIRST, classes=False), exp[ti.EXON_FIRST], PLAIN)
        ctx.set_option("gene_top", 0)
        same(device_call(ctx, list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.REVERSE, ti.ALL, fuzz_arrays()), ti.fuzz_expected(tm.REVERSE, ti.ALL))
    finally:
        ctx.set_option("gene_top", 1)
        ctx.set_option("gene_body_top", 1)


@pytest.mark.parametrize("n", [1, 63, 64, 65, 1023, 1024, 1025])
def test_read_counts_at_the_wave_and_block_edges(ctx, n):
    exons, reads = list(ti.fuzz_annotation()), ti.fuzz_reads()
    pick = list(reads[4990:4990 + n]) if n < 600 else list(reads[-n:])  # (both kinds of reads)
    for introns in (ti.EXON_FIRST, ti.ALL):
        full = ti.fuzz_expected(tm.FORWARD, introns)
        sl = slice(4990, 4990 + n) if n < 600 else slice(len(reads) - n, len(reads))
        exp = {f: full[f][sl] for f in ("gene", "status", "tier", "cls")}
        exp["counts"], exp["class_counts"] = ti.counts_of(exp["status"], exp["tier"]), np.bincount(exp["cls"], minlength=5).astype(np.uint64)
        both(ctx, exons, pick, tm.FORWARD, introns, ti.N_GENES, N_TR, exp=exp)


@pytest.mark.parametrize("cus", [1, 3])
def test_grid_cus(ctx, cus):
    """7,000 reads: with one CU's two blocks every lane makes three trips and more, in both kernels; the results are the
    model's and, byte for byte, the default grid's"""
    import umi_collapse_rs_amd as umi
    reads = list(ti.fuzz_reads()) + list(ti.fuzz_reads()[:1400])
    assert len(reads) == 7000
    exons, arrays = list(ti.fuzz_annotation()), am.pack_reads(reads)
    c = umi.Context(0)
    try:
        for introns in (ti.EXON_FIRST, ti.ALL):
            full = ti.fuzz_expected(tm.FORWARD, introns)
            exp = {f: np.concatenate([full[f], full[f][:1400]]) for f in ("gene", "status", "tier", "cls")}
            exp["counts"], exp["class_counts"] = ti.counts_of(exp["status"], exp["tier"]), np.bincount(exp["cls"], minlength=5).astype(np.uint64)
            default = ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, tm.FORWARD, introns, *arrays)
            same(default, exp)
            c.set_option("grid_cus", cus)
            for top in (1, 0):
                c.set_option("gene_top", top)
                got = c.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, tm.FORWARD, introns, *arrays)
                assert all(got[f].tobytes() == default[f].tobytes() for f in FIELDS)
            same(device_call(c, exons, ti.N_GENES, N_TR, tm.FORWARD, introns, arrays), exp)
    finally:
        c.close()


@pytest.mark.parametrize("n", [am.GENE_TOP_CAP - 1, am.GENE_TOP_CAP, am.GENE_TOP_CAP + 1, 2 * am.GENE_TOP_CAP + 1])
def test_a_transcript_comb_at_the_top_cap(ctx, n):
    exons, reads = tm.comb_annotation(n), tm.comb_reads(n)
    assert len({(e[1], e[2]) for e in exons}) == n
    both(ctx, exons, reads, tm.FORWARD, ti.EXON_FIRST, 50)
    exp = ti.classify_all(exons, reads, tm.UNSTRANDED, ti.ALL)
    same(ctx.assign_genes_transcripts_classes(list(exons), 50, tm.n_transcripts_of(exons), tm.UNSTRANDED, ti.ALL, *am.pack_reads(reads)), exp)


@pytest.mark.parametrize("n", [511, 512, 513, 1025])
def test_a_body_comb_at_the_body_top_cap(ctx, n):
    """one two-exon transcript per gene, reads in the introns and on their edges"""
    exons, reads = ti.body_comb(n), ti.body_comb_reads(n)
    got = both(ctx, exons, reads, tm.FORWARD, ti.EXON_FIRST, n, n)
    assert (got["class_counts"][[ti.EXONIC, ti.SPANNING, ti.INTRONIC]] > 100).all() and got["counts"][1] > 100  # (the input holds them)
    both(ctx, exons, reads, tm.FORWARD, ti.ALL, n, n)


# ---- the contract ---------------------------------------------------------------------------------------

def test_no_reads_touch_nothing(ctx):
    import torch
    gene = torch.full((8,), FILL32, dtype=torch.int32, device="cuda:0")
    tier, cls = (torch.full((8,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(2))
    counts, class_counts = ctx.assign_genes_transcripts_classes_device(list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.FORWARD, ti.ALL, 0, 0, 0,
                                                                       0, 0, 0, gene.data_ptr(), 0, tier.data_ptr(), cls.data_ptr())
    torch.cuda.synchronize()
    assert list(counts) == [0, 0, 0, 0] and list(class_counts) == [0] * 5
    assert (gene.cpu().numpy() == FILL32).all() and (tier.cpu().numpy() == FILL).all() and (cls.cpu().numpy() == FILL).all()
    got = ctx.assign_genes_transcripts_classes(list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.FORWARD, ti.EXON_FIRST, *am.pack_reads([]))
    assert len(got["gene"]) == 0 and len(got["cls"]) == 0 and list(got["counts"]) == [0] * 4 and list(got["class_counts"]) == [0] * 5


def test_no_lines_every_read_is_none(ctx):
    reads = list(ti.fuzz_reads()[:300])
    for introns in (ti.OFF, ti.EXON_FIRST, ti.ALL):
        for n_genes, n_tr in ((0, 0), (5, 9)):
            got = both(ctx, [], reads, tm.FORWARD, introns, n_genes, n_tr)
            assert (got["status"] == ti.NONE).all() and (got["gene"] == -1).all() and not got["cls"].any()
    same(device_call(ctx, [], 0, 0, tm.UNSTRANDED, ti.ALL, am.pack_reads(reads), classes=False),
         ti.classify_all([], reads, tm.UNSTRANDED, ti.ALL), PLAIN)


def test_device_form_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.REVERSE, ti.EXON_FIRST, fuzz_arrays(), stream=s.cuda_stream),
         ti.fuzz_expected(tm.REVERSE, ti.EXON_FIRST))


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
    same(fuzz_call(ctx), ti.fuzz_expected(tm.FORWARD, ti.EXON_FIRST))
    same(device_call(ctx, list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.FORWARD, ti.ALL, fuzz_arrays()), ti.fuzz_expected(tm.FORWARD, ti.ALL))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        same(fuzz_call(c, tm.UNSTRANDED, ti.ALL), ti.fuzz_expected(tm.UNSTRANDED, ti.ALL))
        same(device_call(c, list(ti.fuzz_annotation()), ti.N_GENES, N_TR, tm.UNSTRANDED, ti.EXON_FIRST, fuzz_arrays()),
             ti.fuzz_expected(tm.UNSTRANDED, ti.EXON_FIRST))
    finally:
        c.close()


# ---- errors: the outputs stay as they were --------------------------------------------------------------

def raw_call(ctx, exons, n_genes, n_tr, introns, arrays, gene, status, tier, cls, counts, class_counts, n_reads=None, device=False):
    """either form through ctypes, on the caller's own output arrays (None: NULL); the return code and the message"""
    import ctypes as C
    import umi_collapse_rs_amd as umi
    lib, p = umi.load(), umi._lib.ptr
    ex = ctx._exon_arrays(exons) + [np.array([e[5] for e in exons], np.int32)]
    q = lambda a, t: None if a is None else p(a, t)
    n = len(arrays[0]) if n_reads is None else n_reads
    if device:
        rc = lib.umi_assign_genes_transcripts_classes_device(
            ctx._h, p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32),
            p(ex[5], C.c_int32), len(exons), n_genes, n_tr, tm.FORWARD, introns, *arrays, n, gene, status, tier, cls, q(counts, C.c_uint64),
            q(class_counts, C.c_uint64), None)
    else:
        rc = lib.umi_assign_genes_transcripts_classes(
            ctx._h, p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32),
            p(ex[5], C.c_int32), len(exons), n_genes, n_tr, tm.FORWARD, introns, p(arrays[0], C.c_int32), p(arrays[1], C.c_int32),
            p(arrays[2], C.c_uint8), p(arrays[3], C.c_uint32), p(arrays[4], C.c_uint64), n, q(gene, C.c_int32), q(status, C.c_uint8),
            q(tier, C.c_uint8), q(cls, C.c_uint8), q(counts, C.c_uint64), q(class_counts, C.c_uint64))
    return rc, lib.umi_last_error().decode()


def test_errors_leave_the_outputs_as_they_were(ctx):
    import umi_collapse_rs_amd as umi
    ARG, ORDER = umi._lib.UMI_ERR_ARG, umi._lib.UMI_ERR_ORDER
    exons = list(ti.fuzz_annotation())
    reads = list(ti.fuzz_reads()[:3000])
    ref, pos, rev, cigar, off = am.pack_reads(reads)
    good = (ref, pos, rev, cigar, off)
    t0 = exons[0][5]
    other_ref, other_strand = (exons[0][0] + 1) % 3, "-" if exons[0][3] != "-" else "+"
    bad_ref, bad_cigar, bad_cigar2, bad_off, bad_off2 = ref.copy(), cigar.copy(), cigar.copy(), off.copy(), off.copy()
    bad_ref[[1234, 2500]] = -1, -7
    bad_cigar[[int(off[1500]), int(off[1709])]] = 5 << 4 | 9
    bad_cigar2[int(off[1501]) - 1] = 5 << 4 | 15  # the last word of read 1500
    bad_off[700] = bad_off[701] + 1  # read 699 runs into read 700's words (legal), read 700 runs backwards
    bad_off2[100] = bad_off2[-1] + 1000  # beyond the array: nothing is read there
    first = ti.EXON_FIRST
    cases = [
        (exons + [(0, 1, 2, "+", 0, N_TR)], good, first, ARG, "transcript %d outside" % N_TR),
        (exons + [(0, 1, 2, "+", 0, -1)], good, first, ARG, "transcript -1 outside"),
        (exons + [(other_ref, 1, 2, exons[0][3], exons[0][4], t0)], good, first, ARG, "two references"),
        (exons + [(exons[0][0], 1, 2, other_strand, exons[0][4], t0)], good, first, ARG, "two strands"),
        (exons + [(exons[0][0], 1, 2, exons[0][3], exons[0][4] + 1, t0)], good, first, ARG, "two genes"),
        (exons + [(0, 5, 5, "+", 0, 0)], good, first, ARG, "no interval"),
        (exons, good, 3, ARG, "unknown intron_mode 3"),
        (exons, good, -1, ARG, "unknown intron_mode -1"),
        (exons, (bad_ref, pos, rev, cigar, off), ti.ALL, ARG, "read 1234"),
        (exons, (ref, pos, rev, bad_cigar, off), first, ARG, "read 1500"),
        (exons, (ref, pos, rev, bad_cigar2, off), ti.ALL, ARG, "read 1500"),
        (exons, (ref, pos, rev, cigar, bad_off), first, ORDER, "read 700"),
        (exons, (ref, pos, rev, cigar, bad_off2), ti.OFF, ORDER, "read 99"),
    ]
    for ex, arrays, introns, code, word in cases:
        gene, status, tier, cls = np.full(3000, FILL32, np.int32), np.full(3000, FILL, np.uint8), np.full(3000, FILL, np.uint8), np.full(3000, FILL, np.uint8)
        counts, class_counts = np.full(4, 77, np.uint64), np.full(5, 77, np.uint64)
        rc, msg = raw_call(ctx, ex, ti.N_GENES, N_TR, introns, arrays, gene, status, tier, cls, counts, class_counts)
        assert rc == code and word in msg, (word, rc, msg)
        assert (gene == FILL32).all() and (status == FILL).all() and (tier == FILL).all() and (cls == FILL).all(), word
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes_transcripts_classes(ex, ti.N_GENES, N_TR, tm.FORWARD, introns, *arrays)
        assert e.value.code == code and word in str(e.value)
    # one of cls and class_counts without the other, a required pointer missing, the limit of 2^30: both forms
    outs = lambda: [np.zeros(3000, np.int32), np.zeros(3000, np.uint8), np.zeros(3000, np.uint8), np.zeros(3000, np.uint8),
                    np.zeros(4, np.uint64), np.zeros(5, np.uint64)]
    for hole, word in ((3, "together"), (5, "together"), (2, "required pointer"), (0, "required pointer"), (4, "counts is NULL")):
        o = outs()
        o[hole] = None
        rc, msg = raw_call(ctx, exons, ti.N_GENES, N_TR, first, good, *o)
        assert rc == ARG and word in msg, (hole, rc, msg)
    import torch
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    ptrs = [t.data_ptr() for t in ins]
    gene = torch.full((3000,), FILL32, dtype=torch.int32, device="cuda:0")
    status, tier, cls = (torch.full((3000,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    d_outs = [gene.data_ptr(), status.data_ptr(), tier.data_ptr(), cls.data_ptr()]
    for hole, word in ((3, "together"), (5, "together"), (2, "required pointer")):
        o = d_outs + [np.zeros(4, np.uint64), np.zeros(5, np.uint64)]
        o[hole] = None
        rc, msg = raw_call(ctx, exons, ti.N_GENES, N_TR, first, ptrs, *o, n_reads=3000, device=True)
        assert rc == ARG and word in msg, (hole, rc, msg)
    for device, arrays, o in ((False, good, outs()), (True, ptrs, d_outs + [np.zeros(4, np.uint64), np.zeros(5, np.uint64)])):
        rc, msg = raw_call(ctx, exons, ti.N_GENES, N_TR, first, arrays, *o, n_reads=1 << 30, device=device)
        assert rc == ARG and "30-bit" in msg, (rc, msg)
        rc, msg = raw_call(ctx, exons, ti.N_GENES, N_TR, 7, arrays, *o, n_reads=3000 if device else None, device=device)
        assert rc == ARG and "unknown intron_mode 7" in msg, (rc, msg)
    torch.cuda.synchronize()
    assert (gene.cpu().numpy() == FILL32).all() and (cls.cpu().numpy() == FILL).all()
    # the device form names the smallest bad read too; a transcript error is found before anything is launched
    bad = ref.copy()
    bad[[77, 2000]] = -1
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_transcripts_classes_device(exons, ti.N_GENES, N_TR, tm.FORWARD, ti.ALL, dev(bad).data_ptr(), *ptrs[1:], 3000, *d_outs)
    assert e.value.code == ARG and "read 77" in str(e.value)
    gene.fill_(FILL32)
    torch.cuda.synchronize()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_transcripts_classes_device(cases[2][0], ti.N_GENES, N_TR, tm.FORWARD, first, *ptrs, 3000, *d_outs)
    torch.cuda.synchronize()
    assert e.value.code == ARG and "two references" in str(e.value) and (gene.cpu().numpy() == FILL32).all()
    # op code 8 is legal, and the context is as good as before
    ok = cigar.copy()
    ok[int(off[1500])] = 5 << 4 | 8
    ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, tm.FORWARD, first, ref, pos, rev, ok, off)
    full = ti.fuzz_expected(tm.FORWARD, first)
    exp = {f: full[f][:3000] for f in ("gene", "status", "tier", "cls")}
    exp["counts"], exp["class_counts"] = ti.counts_of(exp["status"], exp["tier"]), np.bincount(exp["cls"], minlength=5).astype(np.uint64)
    same(ctx.assign_genes_transcripts_classes(exons, ti.N_GENES, N_TR, tm.FORWARD, first, ref, pos, rev, cigar, off), exp)
