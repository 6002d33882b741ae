"""umi_assign_genes_introns / umi_assign_genes_introns_device on the GPU against tests/intron_model.py: gene, status,
tier and the four counts by exact equality.  The fuzz inputs are annotation_model.fuzz_annotation() / fuzz_reads();
tests/test_intron_model_cpu.py checks what they and the combs hold."""
import numpy as np
import pytest

import annotation_model as am
import intron_model as im

pytestmark = pytest.mark.gpu
FIELDS = ("gene", "status", "tier", "counts")
GUARD, FILL, FILL32 = 64, 0x5A, -0x5A5A5A5B
STRANDS = sorted(am.MODES)
INTRONS = sorted(im.INTRONS)


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


def device_call(ctx, exons, n_genes, mode, introns, arrays, stream=0):
    """the device form on outputs with guard bytes before and behind; checks that they are untouched and that the
    inputs are as they were"""
    import torch
    ref, pos, rev, cigar, off = arrays
    n = len(ref)
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene = torch.full((n + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
    status = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    tier = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    counts = ctx.assign_genes_introns_device(exons, n_genes, mode, introns, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                                             ins[3].data_ptr() if len(cigar) else 0, ins[4].data_ptr(), n,
                                             gene.data_ptr() + 4 * GUARD, status.data_ptr() + GUARD, tier.data_ptr() + GUARD,
                                             stream=stream)
    torch.cuda.synchronize()
    gene_h, status_h, tier_h = gene.cpu().numpy(), status.cpu().numpy(), tier.cpu().numpy()
    for h, fill in ((gene_h, FILL32), (status_h, FILL), (tier_h, FILL)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
    for t, a in zip(ins, (ref, pos, rev, cigar.view(np.int32), off.view(np.int64))):
        assert (t.cpu().numpy() == a).all()
    return {"gene": gene_h[GUARD:GUARD + n], "status": status_h[GUARD:GUARD + n], "tier": tier_h[GUARD:GUARD + n], "counts": counts}


def both(ctx, exons, reads, mode, introns, n_genes=None, exp=None):
    """both forms against the model"""
    exons, reads = list(exons), list(reads)
    n_genes = am.n_genes_of(exons) if n_genes is None else n_genes
    exp = im.assign_all(exons, reads, mode, introns) if exp is None else exp
    arrays = am.pack_reads(reads)
    got = ctx.assign_genes_introns(exons, n_genes, mode, introns, *arrays)
    same(got, exp)
    same(device_call(ctx, exons, n_genes, mode, introns, arrays), exp)
    return got


# ---- the hand-written cases -----------------------------------------------------------------------------

@pytest.mark.parametrize("introns", INTRONS)
@pytest.mark.parametrize("mode", STRANDS)
def test_hand_cases(ctx, mode, introns):
    names, reads = zip(*im.hand_reads())
    got = both(ctx, im.HAND_EXONS, reads, am.MODES[mode], im.INTRONS[introns], n_genes=im.HAND_N_GENES)
    v = {w: (int(got["status"][i]), int(got["gene"][i]), int(got["tier"][i])) for i, w in enumerate(names)}
    # (tests/test_intron_model_cpu.py pins the model on these cases; a few of them again, on the device's answer)
    own = "+" if mode != "reverse" else "-"
    A, N, S, X, I = im.ASSIGNED, im.NONE, im.SEVERAL, im.TIER_EXON, im.TIER_INTRON
    assert v["exons of two genes, " + own] == (S, -1, 0)
    if introns == "off":
        assert v["inner exon, " + own] == (A, 1, X) and v["inner intron, " + own] == (N, -1, 0)
        assert not got["tier"].any() and got["counts"][1] == 0
        return
    assert v["inner exon, " + own] == ((A, 1, X) if introns == "exon-first" else (S, -1, 0))
    assert v["inner intron, " + own] == (S, -1, 0)
    assert v["outer intron clear of the inner body, " + own] == (A, 0, I)
    assert v["two exons of gene 0, N over gene 1's body, " + own] == (A, 0, X)
    assert v["gene 6's intron and gene 7's, " + own] == (S, -1, 0)
    assert v["exon end into the intron, " + own] == (A, 0, X)
    assert v["gene 9 on ., +"] == v["gene 9 on ., -"] == (A, 9, I)
    assert v["between gene 9's bodies, " + own] == (N, -1, 0) and v["gene 9 on the other reference, " + own] == (A, 9, I)
    assert v["coordinate 0, " + own] == (A, 10, X) and v["an intron near the top, " + own] == (A, 11, I)
    assert v["no block, " + own] == v["a reference without lines, " + own] == (N, -1, 0)
    inner = v["opposite: inner exon, +"]
    assert inner == {"forward": (A, 2, I), "reverse": (A, 3, X),
                     "unstranded": (A, 3, X) if introns == "exon-first" else (S, -1, 0)}[mode]


def test_no_lines_at_all(ctx):
    reads = [r for _, r in im.hand_reads()]
    for introns in im.INTRONS.values():
        got = both(ctx, [], reads, am.FORWARD, introns, n_genes=0)
        assert list(got["counts"]) == [0, 0, len(reads), 0]


# ---- the fuzz -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("introns", ["exon-first", "all"])
@pytest.mark.parametrize("mode", STRANDS)
def test_fuzz_against_the_model(ctx, mode, introns):
    exp = im.fuzz_expected(am.MODES[mode], im.INTRONS[introns])
    got = both(ctx, am.fuzz_annotation(), am.fuzz_reads(), am.MODES[mode], im.INTRONS[introns], n_genes=40, exp=exp)
    assert got["counts"][1] >= 50 and got["counts"][2] >= 50 and got["counts"][3] >= 50


@pytest.mark.parametrize("mode", STRANDS)
def test_off_is_umi_assign_genes(ctx, mode):
    exons, arrays = list(am.fuzz_annotation()), am.pack_reads(am.fuzz_reads())
    plain = ctx.assign_genes(exons, 40, am.MODES[mode], *arrays)
    got = both(ctx, exons, am.fuzz_reads(), am.MODES[mode], im.OFF, n_genes=40, exp=im.fuzz_expected(am.MODES[mode], im.OFF))
    same(got, plain, ("gene", "status"))
    assert not got["tier"].any()
    assert list(got["counts"]) == [plain["counts"][0], 0, plain["counts"][1], plain["counts"][2]]


def test_the_sampled_tops_change_nothing(ctx):
    exons, arrays = list(am.fuzz_annotation()), am.pack_reads(am.fuzz_reads())
    n = 2 * im.GENE_BODY_TOP_CAP + 1
    comb, comb_arrays = list(im.body_comb(n)), am.pack_reads(im.body_comb_reads(n))
    comb_exp = {i: im.assign_all(comb, im.body_comb_reads(n), am.FORWARD, i) for i in (im.EXON_FIRST, im.ALL)}
    try:
        for top, body_top in ((0, 1), (0, 0), (1, 0), (1, 1)):
            ctx.set_option("gene_top", top)
            ctx.set_option("gene_body_top", body_top)
            for introns in (im.EXON_FIRST, im.ALL):
                same(ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, *arrays), im.fuzz_expected(am.FORWARD, introns))
                same(ctx.assign_genes_introns(comb, n, am.FORWARD, introns, *comb_arrays), comb_exp[introns])
    finally:
        ctx.set_option("gene_top", 1)
        ctx.set_option("gene_body_top", 1)


# ---- sizes ----------------------------------------------------------------------------------------------

def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def read_counts():
    t = am.GENE_THREADS
    return [1, 63, 64, 65, t - 1, t, t + 1, cu_count() * am.GENE_BLOCKS_PER_CU * t + 1]


def test_read_counts(ctx):
    exons = list(am.fuzz_annotation())
    ref, pos, rev, cigar, off = am.pack_reads(am.fuzz_reads())
    words = np.diff(off.astype(np.int64))
    for introns in (im.EXON_FIRST, im.ALL):
        exp = im.fuzz_expected(am.FORWARD, introns)
        for n in read_counts():  # the fuzz reads over and over, cut at n
            reps = -(-n // len(ref))
            want = {f: np.tile(exp[f], reps)[:n] for f in ("gene", "status", "tier")}
            want["counts"] = im.counts_of(want["status"], want["tier"])
            n_off = np.concatenate([[0], np.cumsum(np.tile(words, reps)[:n])]).astype(np.uint64)
            arrays = (np.tile(ref, reps)[:n], np.tile(pos, reps)[:n], np.tile(rev, reps)[:n],
                      np.tile(cigar, reps)[:int(n_off[-1])], n_off)
            got = ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, *arrays)
            assert len(got["gene"]) == n and int(got["counts"].sum()) == n
            same(got, want)
            if n in (1, 65, am.GENE_THREADS + 1):
                same(device_call(ctx, exons, 40, am.FORWARD, introns, arrays), want)


def test_no_reads_touch_nothing(ctx):
    import torch
    gene = torch.full((8,), FILL32, dtype=torch.int32, device="cuda:0")
    tier = torch.full((8,), FILL, dtype=torch.uint8, device="cuda:0")
    counts = ctx.assign_genes_introns_device(list(am.fuzz_annotation()), 40, am.FORWARD, im.EXON_FIRST, 0, 0, 0, 0, 0, 0,
                                             gene.data_ptr(), 0, tier.data_ptr())
    torch.cuda.synchronize()
    assert list(counts) == [0, 0, 0, 0] and (gene.cpu().numpy() == FILL32).all() and (tier.cpu().numpy() == FILL).all()
    got = ctx.assign_genes_introns(list(am.fuzz_annotation()), 40, am.FORWARD, im.ALL, *am.pack_reads([]))
    assert len(got["gene"]) == len(got["tier"]) == 0 and list(got["counts"]) == [0, 0, 0, 0]


# the segments of a body table: on and beside the body top's capacity (stride 1 up to GENE_BODY_TOP_CAP segments, 2 up
# to twice that, then 4); the exon table of the same comb has twice as many
BODY_SIZES = [1, im.GENE_BODY_TOP_CAP - 1, im.GENE_BODY_TOP_CAP, im.GENE_BODY_TOP_CAP + 1, 2 * im.GENE_BODY_TOP_CAP + 1]


@pytest.mark.parametrize("n", BODY_SIZES)
def test_body_table_sizes(ctx, n):
    exons, reads = im.body_comb(n), im.body_comb_reads(n)
    for introns in (im.EXON_FIRST, im.ALL):
        got = both(ctx, exons, reads, am.FORWARD, introns, n_genes=n)
        if n > 1:
            assert min(got["counts"]) > 50
    if n == im.GENE_BODY_TOP_CAP + 1:
        both(ctx, exons, reads, am.UNSTRANDED, im.EXON_FIRST, n_genes=n)
        both(ctx, exons, reads, am.REVERSE, im.ALL, n_genes=n)


# ... and of an exon table, beside the exon top's capacity: annotation_model's comb of one-exon genes, whose fifty
# genes' bodies all lie over one another
@pytest.mark.parametrize("n", [am.GENE_TOP_CAP - 1, am.GENE_TOP_CAP, am.GENE_TOP_CAP + 1, 2 * am.GENE_TOP_CAP + 1])
def test_exon_table_sizes(ctx, n):
    exons, reads = am.comb_annotation(n), am.comb_reads(n)
    first = both(ctx, exons, reads, am.FORWARD, im.EXON_FIRST, n_genes=50)
    assert first["counts"][0] > 100 and first["counts"][3] > 100
    exp = im.assign_all(exons, reads, am.FORWARD, im.ALL)
    same(ctx.assign_genes_introns(list(exons), 50, am.FORWARD, im.ALL, *am.pack_reads(reads)), exp)


# ---- errors ---------------------------------------------------------------------------------------------

def test_argument_errors_before_any_launch(ctx):
    import umi_collapse_rs_amd as umi
    reads = am.pack_reads([im.M(150)])
    ok = (0, 100, 200, "+", 0)
    for ex, n_genes, mode, introns, word in (([(0, 100, 100, "+", 0)], 1, 0, 1, "interval"), ([(0, -1, 5, "+", 0)], 1, 0, 2, "interval"),
                                             ([ok, (0, 1, 2, "+", 1)], 1, 0, 1, "gene"), ([ok, (0, 1, 2, "*", 0)], 1, 0, 1, "strand"),
                                             ([ok], 1, 3, 1, "strand_mode"), ([(-1, 1, 2, "+", 0)], 1, 0, 0, "reference"),
                                             ([ok], 1, 0, 3, "intron_mode"), ([ok], 1, 0, -1, "intron_mode"), ([ok], 1, 3, 7, "intron_mode")):
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes_introns(ex, n_genes, mode, introns, *reads)
        assert e.value.code == umi._lib.UMI_ERR_ARG and word in str(e.value), (ex, str(e.value))
    import ctypes as C
    lib, p = umi.load(), umi._lib.ptr
    ex = ctx._exon_arrays([ok])
    counts = np.zeros(4, np.uint64)
    gene, status, tier = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.full(1, 9, np.uint8)
    ptrs = [p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32)]
    rd = [p(reads[0], C.c_int32), p(reads[1], C.c_int32), p(reads[2], C.c_uint8), p(reads[3], C.c_uint32), p(reads[4], C.c_uint64)]
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(tier, C.c_uint8), p(counts, C.c_uint64)]
    for i in range(5):  # a null exon array with one exon
        a = list(ptrs)
        a[i] = None
        assert lib.umi_assign_genes_introns(ctx._h, *a, 1, 1, 0, 1, *rd, 1, *outs) == umi._lib.UMI_ERR_ARG
    for i in range(5):  # a null read array with one read
        a = list(rd)
        a[i] = None
        assert lib.umi_assign_genes_introns(ctx._h, *ptrs, 1, 1, 0, 1, *a, 1, *outs) == umi._lib.UMI_ERR_ARG
    for i in range(4):
        a = list(outs)
        a[i] = None
        assert lib.umi_assign_genes_introns(ctx._h, *ptrs, 1, 1, 0, 1, *rd, 1, *a) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes_introns(None, *ptrs, 1, 1, 0, 1, *rd, 1, *outs) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes_introns(ctx._h, *ptrs, 1, 1, 0, 1, *rd, 1 << 30, *outs) == umi._lib.UMI_ERR_ARG
    assert tier[0] == 9
    assert lib.umi_assign_genes_introns(ctx._h, *ptrs, 1, 1, 0, 1, *rd, 1, *outs) == 0 and gene[0] == 0 and tier[0] == 0


def test_errors_found_on_the_device(ctx):
    import umi_collapse_rs_amd as umi
    exons = list(am.fuzz_annotation())
    reads = list(am.fuzz_reads()[:3000])
    ref, pos, rev, cigar, off = am.pack_reads(reads)
    first = im.fuzz_expected(am.FORWARD, im.EXON_FIRST)
    for introns in (im.EXON_FIRST, im.ALL):
        for r in (2000, 1234):
            bad = ref.copy()
            bad[r] = -1
            bad[2500] = -7
            with pytest.raises(umi.UmiHipError) as e:
                ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, bad, pos, rev, cigar, off)
            assert e.value.code == umi._lib.UMI_ERR_ARG and "read %d" % r in str(e.value)
        # a bad op code in a read that stops after phase 1 (assigned by an exon), and only in one that reaches phase 2
        # (its other words hit no exon): told alike, the smallest read first
        by_exon = [i for i in range(1000, 3000) if first["status"][i] == im.ASSIGNED and first["tier"][i] == 0 and off[i + 1] > off[i]]
        by_body = [i for i in range(1000, 3000) if first["tier"][i] == 1 and off[i + 1] - off[i] >= 2]
        for at, later in ((by_exon[0], by_body[-1]), (by_body[0], by_exon[-1]), (by_body[1], by_body[-1])):
            assert at < later
            for code in (9, 15):
                bad = cigar.copy()
                bad[int(off[at + 1]) - 1] = 5 << 4 | code  # (the last word: the walk has looked at the others by then)
                bad[int(off[later])] = 5 << 4 | code
                with pytest.raises(umi.UmiHipError) as e:
                    ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, ref, pos, rev, bad, off)
                assert e.value.code == umi._lib.UMI_ERR_ARG and "read %d:" % at in str(e.value)
        bad = off.copy()
        bad[700] = bad[701] + 1  # read 699 runs into read 700's words (legal), read 700 runs backwards
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, ref, pos, rev, cigar, bad)
        assert e.value.code == umi._lib.UMI_ERR_ORDER and "read 700" in str(e.value)
        bad = off.copy()
        bad[100] = bad[-1] + 1000  # beyond the array: nothing is read there
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes_introns(exons, 40, am.FORWARD, introns, ref, pos, rev, cigar, bad)
        assert e.value.code == umi._lib.UMI_ERR_ORDER and "read 99" in str(e.value)
    # the device form tells the same; the context is as good as before
    import torch
    bad = ref.copy()
    bad[77] = -1
    ins = [dev(bad), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    outs = [torch.zeros(3000, dtype=torch.int32, device="cuda:0"), torch.zeros(3000, dtype=torch.uint8, device="cuda:0"),
            torch.zeros(3000, dtype=torch.uint8, device="cuda:0")]
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_introns_device(exons, 40, am.FORWARD, im.EXON_FIRST, *(t.data_ptr() for t in ins), 3000,
                                        *(t.data_ptr() for t in outs))
    assert e.value.code == umi._lib.UMI_ERR_ARG and "read 77" in str(e.value)
    got = ctx.assign_genes_introns(exons, 40, am.FORWARD, im.EXON_FIRST, ref, pos, rev, cigar, off)
    want = {f: first[f][:3000] for f in ("gene", "status", "tier")}
    want["counts"] = im.counts_of(want["status"], want["tier"])
    same(got, want)


# ---- other contexts -------------------------------------------------------------------------------------

def test_device_form_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, list(am.fuzz_annotation()), 40, am.REVERSE, im.EXON_FIRST, am.pack_reads(am.fuzz_reads()), stream=s.cuda_stream),
         im.fuzz_expected(am.REVERSE, im.EXON_FIRST))


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
    exons, arrays = list(am.fuzz_annotation()), am.pack_reads(am.fuzz_reads())
    same(ctx.assign_genes_introns(exons, 40, am.FORWARD, im.EXON_FIRST, *arrays), im.fuzz_expected(am.FORWARD, im.EXON_FIRST))
    same(device_call(ctx, exons, 40, am.FORWARD, im.ALL, arrays), im.fuzz_expected(am.FORWARD, im.ALL))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        exons, arrays = list(am.fuzz_annotation()), am.pack_reads(am.fuzz_reads())
        exp = im.fuzz_expected(am.UNSTRANDED, im.EXON_FIRST)
        same(c.assign_genes_introns(exons, 40, am.UNSTRANDED, im.EXON_FIRST, *arrays), exp)
        same(device_call(c, exons, 40, am.UNSTRANDED, im.EXON_FIRST, arrays), exp)
    finally:
        c.close()
