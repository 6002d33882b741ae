"""umi_assign_genes / umi_assign_genes_device on the GPU against tests/annotation_model.py: gene, status and counts
by exact equality.  The fuzz inputs are annotation_model.fuzz_annotation() / fuzz_reads(); tests/
test_annotation_model_cpu.py checks what they hold."""
import numpy as np
import pytest

import annotation_model as am

pytestmark = pytest.mark.gpu
FIELDS = ("gene", "status", "counts")
GUARD, FILL, FILL32 = 64, 0x5A, -0x5A5A5A5B


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


def device_call(ctx, exons, n_genes, mode, arrays, stream=0):
    """the device form on outputs with guard bytes before and behind; checks that they are untouched and that the
    inputs are as they were"""
    import torch
    ref, pos, rev, cigar, off = arrays
    n = len(ref)
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene = torch.full((n + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
    status = torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0")
    torch.cuda.synchronize()
    counts = ctx.assign_genes_device(exons, n_genes, mode, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(),
                                     ins[3].data_ptr() if len(cigar) else 0, ins[4].data_ptr(), n,
                                     gene.data_ptr() + 4 * GUARD, status.data_ptr() + GUARD, stream=stream)
    torch.cuda.synchronize()
    gene_h, status_h = gene.cpu().numpy(), status.cpu().numpy()
    for h, fill in ((gene_h, FILL32), (status_h, FILL)):
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all()
    for t, a in zip(ins, (ref, pos, rev, cigar.view(np.int32), off.view(np.int64))):
        assert (t.cpu().numpy() == a).all()
    return {"gene": gene_h[GUARD:GUARD + n], "status": status_h[GUARD:GUARD + n], "counts": counts}


def both(ctx, exons, reads, mode, n_genes=None):
    """both forms against the model; returns the statuses and genes as lists"""
    exons, reads = list(exons), list(reads)
    n_genes = am.n_genes_of(exons) if n_genes is None else n_genes
    exp = am.assign_all(exons, reads, mode)
    arrays = am.pack_reads(reads)
    got = ctx.assign_genes(exons, n_genes, mode, *arrays)
    same(got, exp)
    same(device_call(ctx, exons, n_genes, mode, arrays), exp)
    return list(map(int, got["status"])), list(map(int, got["gene"]))


def M(pos, length=10, ref=0, rev=False):
    return (ref, pos, rev, (("M", length),))


# ---- the fuzz -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(am.MODES))
def test_fuzz_against_the_model(ctx, mode):
    exons, reads = am.fuzz_annotation(), am.fuzz_reads()
    exp = am.fuzz_expected(am.MODES[mode])
    arrays = am.pack_reads(reads)
    same(ctx.assign_genes(list(exons), 40, am.MODES[mode], *arrays), exp)
    same(device_call(ctx, list(exons), 40, am.MODES[mode], arrays), exp)


def test_the_modes_differ_as_the_model_says(ctx):
    exp = [am.fuzz_expected(m) for m in (am.FORWARD, am.REVERSE, am.UNSTRANDED)]
    assert (exp[0]["status"] != exp[1]["status"]).any() and (exp[0]["status"] != exp[2]["status"]).any()
    # a '.' exon is admissible under all three; a '+' exon to a forward read under forward and unstranded only
    ex = [(0, 100, 200, "+", 0), (0, 300, 400, "-", 1), (0, 500, 600, ".", 2)]
    reads = [M(150), M(150, rev=True), M(350), M(350, rev=True), M(550), M(550, rev=True)]
    assert both(ctx, ex, reads, am.FORWARD)[1] == [0, -1, -1, 1, 2, 2]
    assert both(ctx, ex, reads, am.REVERSE)[1] == [-1, 0, 1, -1, 2, 2]
    assert both(ctx, ex, reads, am.UNSTRANDED)[1] == [0, 0, 1, 1, 2, 2]


def test_the_sampled_top_changes_nothing(ctx):
    exons, reads = am.fuzz_annotation(), am.fuzz_reads()
    arrays = am.pack_reads(reads)
    try:
        ctx.set_option("gene_top", 0)
        same(ctx.assign_genes(list(exons), 40, am.FORWARD, *arrays), am.fuzz_expected(am.FORWARD))
        n = 2 * am.GENE_TOP_CAP + 1
        same(ctx.assign_genes(list(am.comb_annotation(n)), 50, am.FORWARD, *am.pack_reads(am.comb_reads(n))),
             am.assign_all(am.comb_annotation(n), am.comb_reads(n), am.FORWARD))
    finally:
        ctx.set_option("gene_top", 1)


# ---- off-by-one pairs, overlaps, spliced reads ----------------------------------------------------------

def test_off_by_one_at_both_ends_of_an_exon(ctx):
    ex = [(0, 100, 200, "+", 0)]
    reads = [M(90, 10), M(90, 11), M(200, 10), M(199, 10), M(0, 100), M(0, 101), M(100, 100), M(50, 300)]
    for mode in (am.FORWARD, am.UNSTRANDED):
        st, g = both(ctx, ex, reads, mode)
        assert st == [am.NONE, am.ASSIGNED, am.NONE, am.ASSIGNED, am.NONE, am.ASSIGNED, am.ASSIGNED, am.ASSIGNED]
        assert g == [-1, 0, -1, 0, -1, 0, 0, 0]


def test_overlap_cases(ctx):
    # gene 0: exons [100, 200) and [150, 260) (overlapping, one gene), then [600, 700) behind an intron;
    # gene 1 inside that intron at [350, 450); gene 2 inside gene 0's last exon at [620, 640)
    ex = [(0, 100, 200, "+", 0), (0, 150, 260, "+", 0), (0, 600, 700, "+", 0), (0, 350, 450, "+", 1), (0, 620, 640, "+", 2)]
    reads = [M(140, 30), M(190, 30), M(380, 20), M(625, 10), M(610, 20), M(600, 20), M(640, 20), M(300, 20)]
    st, g = both(ctx, ex, reads, am.FORWARD)
    assert st == [am.ASSIGNED, am.ASSIGNED, am.ASSIGNED, am.SEVERAL, am.SEVERAL, am.ASSIGNED, am.ASSIGNED, am.NONE]
    assert g == [0, 0, 1, -1, -1, 0, 0, -1]


def test_spliced_reads(ctx):
    ex = [(0, 100, 200, "+", 0), (0, 600, 700, "+", 0), (0, 350, 450, "+", 1), (0, 900, 950, "+", 2)]
    reads = [(0, 180, False, (("M", 20), ("N", 400), ("M", 30))),    # two exons of gene 0 across gene 1: gene 0
             (0, 180, False, (("M", 20), ("D", 400), ("M", 30))),    # the same with a deletion: one block over gene 1
             (0, 430, False, (("M", 20), ("N", 150), ("M", 30))),    # gene 1, then gene 0: several
             (0, 680, False, (("M", 20), ("N", 200), ("M", 30))),    # gene 0, then gene 2: several
             (0, 220, False, (("M", 20), ("N", 400), ("M", 30))),    # nothing, then gene 0
             (0, 220, False, (("M", 20), ("N", 30), ("M", 30))),     # nothing twice
             (0, 180, False, (("S", 5), ("M", 10), ("I", 3), ("M", 10), ("N", 400), ("=", 10), ("X", 2), ("P", 1), ("H", 4)))]
    st, g = both(ctx, ex, reads, am.FORWARD)
    assert st == [am.ASSIGNED, am.SEVERAL, am.SEVERAL, am.SEVERAL, am.ASSIGNED, am.NONE, am.ASSIGNED]
    assert g == [0, -1, -1, -1, 0, -1, 0]


def test_reads_without_blocks_and_long_cigars(ctx):
    ex = [(0, 100, 200, "+", 0), (0, 5000, 5100, "+", 1)]
    long_same = tuple(x for i in range(100) for x in (("M", 1), ("I", 1)))                  # 200 words, one block in gene 0
    long_two = tuple(x for i in range(100) for x in (("M", 30), ("N", 20)))                 # 200 words, 100 blocks up to 5100
    assert len(long_same) == len(long_two) == 200
    reads = [(0, 150, False, ()), (0, 150, False, (("S", 10), ("H", 3), ("I", 4), ("P", 1))), (0, 150, False, (("N", 10),)),
             (0, 150, False, (("M", 0),)), (0, 150, False, (("M", 1),)), (0, 150, False, long_same), (0, 150, False, long_two),
             (0, 95, False, (("N", 5), ("M", 1))), (0, 95, False, (("N", 4), ("M", 1)))]
    st, g = both(ctx, ex, reads, am.FORWARD)
    assert st == [am.NONE, am.NONE, am.NONE, am.NONE, am.ASSIGNED, am.ASSIGNED, am.SEVERAL, am.ASSIGNED, am.NONE]
    assert g[4:8] == [0, 0, -1, 0]


def test_coordinates_at_zero_and_at_the_top(ctx):
    top = 2 ** 31 - 1
    ex = [(0, 0, 1, "+", 0), (0, top - 2, top, "+", 1), (2 ** 31 - 1, top - 3, top, ".", 2)]
    reads = [M(0, 1), M(1, 1), M(top - 2, 1), M(top - 1, 5), M(top - 3, 1), M(top - 3, 5, ref=top), M(0, 5, ref=top),
             (0, 0, False, (("M", 1), ("D", 2 ** 28 - 1), ("D", 2 ** 28 - 1), ("N", 2 ** 28 - 1), ("N", 2 ** 28 - 1), ("M", 3)))]
    st, g = both(ctx, ex, reads, am.FORWARD)
    assert g == [0, -1, 1, 1, -1, 2, -1, 0]


# ---- sizes ----------------------------------------------------------------------------------------------

def cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def read_counts():
    t = am.GENE_THREADS
    return [0, 1, 63, 64, 65, t - 1, t, t + 1, cu_count() * am.GENE_BLOCKS_PER_CU * t + 1]


def test_read_counts(ctx):
    exons = list(am.fuzz_annotation())
    exp = am.fuzz_expected(am.FORWARD)
    ref, pos, rev, cigar, off = am.pack_reads(am.fuzz_reads())
    words = np.diff(off.astype(np.int64))
    for n in read_counts():  # the fuzz reads over and over, cut at n
        reps = -(-n // len(ref)) or 1
        e_gene, e_status = np.tile(exp["gene"], reps)[:n], np.tile(exp["status"], reps)[:n]
        want = {"gene": e_gene, "status": e_status, "counts": np.bincount(e_status, minlength=3).astype(np.uint64)}
        n_off = np.concatenate([[0], np.cumsum(np.tile(words, reps)[:n])]).astype(np.uint64)
        arrays = (np.tile(ref, reps)[:n], np.tile(pos, reps)[:n], np.tile(rev, reps)[:n],
                  np.tile(cigar, reps)[:int(n_off[-1])], n_off)
        got = ctx.assign_genes(exons, 40, am.FORWARD, *arrays)
        assert len(got["gene"]) == n and int(got["counts"].sum()) == n
        same(got, want)
        if n in (0, 1, 65, am.GENE_THREADS + 1):
            same(device_call(ctx, exons, 40, am.FORWARD, arrays), want)


def test_no_reads_touch_nothing(ctx):
    import torch
    gene = torch.full((8,), FILL32, dtype=torch.int32, device="cuda:0")
    counts = ctx.assign_genes_device(list(am.fuzz_annotation()), 40, am.FORWARD, 0, 0, 0, 0, 0, 0, gene.data_ptr(), 0)
    torch.cuda.synchronize()
    assert list(counts) == [0, 0, 0] and (gene.cpu().numpy() == FILL32).all()


# the segments of a table: none, one, and on and beside the sampled top's capacity (stride 1 up to GENE_TOP_CAP
# segments, 2 up to twice that, then 4)
ANNOTATION_SIZES = [0, 1, 2, am.GENE_TOP_CAP - 1, am.GENE_TOP_CAP, am.GENE_TOP_CAP + 1, 2 * am.GENE_TOP_CAP - 1,
                    2 * am.GENE_TOP_CAP, 2 * am.GENE_TOP_CAP + 1, 2 * am.GENE_TOP_CAP + 2]


@pytest.mark.parametrize("n", ANNOTATION_SIZES)
def test_annotation_sizes(ctx, n):
    exons, reads = am.comb_annotation(n), am.comb_reads(n)
    exp = am.assign_all(exons, reads, am.FORWARD)
    arrays = am.pack_reads(reads)
    same(ctx.assign_genes(list(exons), 50, am.FORWARD, *arrays), exp)
    if n:
        assert exp["counts"][am.ASSIGNED] > 100 and exp["counts"][am.NONE] > 100
    else:
        assert exp["counts"][am.NONE] == len(reads)
    if n in (0, am.GENE_TOP_CAP + 1):
        same(device_call(ctx, list(exons), 50, am.UNSTRANDED, arrays), am.assign_all(exons, reads, am.UNSTRANDED))


def test_absent_references(ctx):
    ex = [(0, 100, 200, "+", 0), (2, 100, 200, "+", 1), (5, 100, 200, "-", 2)]
    reads = [M(150, ref=r, rev=v) for r in (0, 1, 2, 3, 4, 5, 6, 1000, 2 ** 31 - 1) for v in (False, True)]
    st, g = both(ctx, ex, reads, am.FORWARD)
    assert g == [0, -1, -1, -1, 1, -1, -1, -1, -1, -1, -1, 2, -1, -1, -1, -1, -1, -1]
    both(ctx, ex, reads, am.UNSTRANDED)


# ---- errors ---------------------------------------------------------------------------------------------

def test_argument_errors_before_any_launch(ctx):
    import umi_collapse_rs_amd as umi
    reads = am.pack_reads([M(150)])
    ok = (0, 100, 200, "+", 0)
    for ex, n_genes, mode, word in (([(0, 100, 100, "+", 0)], 1, 0, "interval"), ([(0, 100, 99, "+", 0)], 1, 0, "interval"),
                                    ([(0, -1, 5, "+", 0)], 1, 0, "interval"), ([ok, (0, 1, 2, "+", 1)], 1, 0, "gene"),
                                    ([ok, (0, 1, 2, "+", -1)], 1, 0, "gene"), ([ok, (0, 1, 2, "*", 0)], 1, 0, "strand"),
                                    ([ok], 1, 3, "strand_mode"), ([ok], 1, -1, "strand_mode"), ([(-1, 1, 2, "+", 0)], 1, 0, "reference")):
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes(ex, n_genes, mode, *reads)
        assert e.value.code == umi._lib.UMI_ERR_ARG and word in str(e.value), (ex, str(e.value))
    import ctypes as C
    lib, p = umi.load(), umi._lib.ptr
    ex = ctx._exon_arrays([ok])
    counts = np.zeros(3, np.uint64)
    gene, status = np.zeros(1, np.int32), np.zeros(1, np.uint8)
    ptrs = [p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32)]
    rd = [p(reads[0], C.c_int32), p(reads[1], C.c_int32), p(reads[2], C.c_uint8), p(reads[3], C.c_uint32), p(reads[4], C.c_uint64)]
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(counts, C.c_uint64)]
    for i in range(5):  # a null exon array with one exon
        a = list(ptrs)
        a[i] = None
        assert lib.umi_assign_genes(ctx._h, *a, 1, 1, 0, *rd, 1, *outs) == umi._lib.UMI_ERR_ARG
    for i in range(5):  # a null read array with one read
        a = list(rd)
        a[i] = None
        assert lib.umi_assign_genes(ctx._h, *ptrs, 1, 1, 0, *a, 1, *outs) == umi._lib.UMI_ERR_ARG
    for i in range(3):
        a = list(outs)
        a[i] = None
        assert lib.umi_assign_genes(ctx._h, *ptrs, 1, 1, 0, *rd, 1, *a) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes(None, *ptrs, 1, 1, 0, *rd, 1, *outs) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes(ctx._h, *ptrs, 1, 1, 0, *rd, 1 << 30, *outs) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes(ctx._h, *ptrs, 1, 1, 0, *rd, 1, *outs) == 0 and gene[0] == 0


def test_errors_found_on_the_device(ctx):
    import umi_collapse_rs_amd as umi
    exons = list(am.fuzz_annotation())
    reads = list(am.fuzz_reads()[:3000])
    ref, pos, rev, cigar, off = am.pack_reads(reads)
    for r in (2000, 1234):
        bad = ref.copy()
        bad[r] = -1
        bad[2500] = -7
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes(exons, 40, am.FORWARD, bad, pos, rev, cigar, off)
        assert e.value.code == umi._lib.UMI_ERR_ARG and "read %d" % r in str(e.value)
    for code in (9, 15):
        bad = cigar.copy()
        bad[int(off[1500])] = 5 << 4 | code
        bad[int(off[1700 + code])] = 5 << 4 | code
        with pytest.raises(umi.UmiHipError) as e:
            ctx.assign_genes(exons, 40, am.FORWARD, ref, pos, rev, bad, off)
        assert e.value.code == umi._lib.UMI_ERR_ARG and "read 1500" in str(e.value)
    ok = cigar.copy()
    ok[int(off[1500])] = 5 << 4 | 8
    ctx.assign_genes(exons, 40, am.FORWARD, ref, pos, rev, ok, off)
    bad = off.copy()
    bad[700] = bad[701] + 1  # read 699 runs into read 700's words (legal), read 700 runs backwards
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes(exons, 40, am.FORWARD, ref, pos, rev, cigar, bad)
    assert e.value.code == umi._lib.UMI_ERR_ORDER and "read 700" in str(e.value)
    bad = off.copy()
    bad[100] = bad[-1] + 1000  # beyond the array: nothing is read there
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes(exons, 40, am.FORWARD, ref, pos, rev, cigar, bad)
    assert e.value.code == umi._lib.UMI_ERR_ORDER and "read 99" in str(e.value)
    # the device form tells the same; the context is as good as before
    import torch
    bad = ref.copy()
    bad[77] = -1
    ins = [dev(bad), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene, status = torch.zeros(3000, dtype=torch.int32, device="cuda:0"), torch.zeros(3000, dtype=torch.uint8, device="cuda:0")
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_device(exons, 40, am.FORWARD, *(t.data_ptr() for t in ins), 3000, gene.data_ptr(), status.data_ptr())
    assert e.value.code == umi._lib.UMI_ERR_ARG and "read 77" in str(e.value)
    exp = am.fuzz_expected(am.FORWARD)
    got = ctx.assign_genes(exons, 40, am.FORWARD, ref, pos, rev, cigar, off)
    same(got, {"gene": exp["gene"][:3000], "status": exp["status"][:3000],
               "counts": np.bincount(exp["status"][:3000], minlength=3).astype(np.uint64)})


# ---- other contexts -------------------------------------------------------------------------------------

def test_device_form_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, list(am.fuzz_annotation()), 40, am.REVERSE, am.pack_reads(am.fuzz_reads()), stream=s.cuda_stream),
         am.fuzz_expected(am.REVERSE))


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
    same(ctx.assign_genes(exons, 40, am.FORWARD, *arrays), am.fuzz_expected(am.FORWARD))
    same(device_call(ctx, exons, 40, am.FORWARD, arrays), am.fuzz_expected(am.FORWARD))
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
        same(c.assign_genes(exons, 40, am.UNSTRANDED, *arrays), am.fuzz_expected(am.UNSTRANDED))
        same(device_call(c, exons, 40, am.UNSTRANDED, arrays), am.fuzz_expected(am.UNSTRANDED))
    finally:
        c.close()
