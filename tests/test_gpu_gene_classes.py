"""umi_assign_genes_classes / umi_assign_genes_classes_device on the GPU against tests/velocity_model.py: gene, status,
tier, class and both sets of counts by exact equality, and against umi_assign_genes_introns on the same arrays.  The
fuzz inputs are velocity_model.fuzz_annotation() / fuzz_reads(); tests/test_velocity_model_cpu.py checks what they hold."""
import numpy as np
import pytest

import annotation_model as am
import intron_model as im
import velocity_model as vm

pytestmark = pytest.mark.gpu
FIELDS = ("gene", "status", "tier", "cls", "counts", "class_counts")
GUARD, FILL, FILL32 = 64, 0x5A, -0x5A5A5A5B
STRANDS = sorted(am.MODES)
N_GENES = vm.FUZZ_GENES


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
    """the device form on outputs with guard bytes before and behind; checks that they are untouched"""
    import torch
    ref, pos, rev, cigar, off = arrays
    n = len(ref)
    ins = [dev(ref), dev(pos), dev(rev), dev(cigar.view(np.int32)), dev(off.view(np.int64))]
    gene = torch.full((n + 2 * GUARD,), FILL32, dtype=torch.int32, device="cuda:0")
    status, tier, cls = (torch.full((n + 2 * GUARD,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(3))
    torch.cuda.synchronize()
    counts, class_counts = ctx.assign_genes_classes_device(
        exons, n_genes, mode, introns, ins[0].data_ptr(), ins[1].data_ptr(), ins[2].data_ptr(), ins[3].data_ptr() if len(cigar) else 0,
        ins[4].data_ptr(), n, gene.data_ptr() + 4 * GUARD, status.data_ptr() + GUARD, tier.data_ptr() + GUARD, cls.data_ptr() + GUARD,
        stream=stream)
    torch.cuda.synchronize()
    out = {"counts": counts, "class_counts": class_counts}
    for name, t, fill in (("gene", gene, FILL32), ("status", status, FILL), ("tier", tier, FILL), ("cls", cls, FILL)):
        h = t.cpu().numpy()
        assert (h[:GUARD] == fill).all() and (h[GUARD + n:] == fill).all(), name
        out[name] = h[GUARD:GUARD + n]
    return out


def both(ctx, exons, reads, mode, introns, n_genes=None, exp=None):
    """both forms against the model, and the four shared outputs against umi_assign_genes_introns"""
    exons, reads = list(exons), list(reads)
    n_genes = am.n_genes_of(exons) if n_genes is None else n_genes
    exp = vm.classify_all(exons, reads, mode, introns) if exp is None else exp
    arrays = am.pack_reads(reads)
    got = ctx.assign_genes_classes(exons, n_genes, mode, introns, *arrays)
    same(got, exp)
    same(device_call(ctx, exons, n_genes, mode, introns, arrays), exp)
    same(got, ctx.assign_genes_introns(exons, n_genes, mode, introns, *arrays), ("gene", "status", "tier", "counts"))
    return got


def test_hand_cases(ctx):
    reads = [(0, pos, False, cigar) for pos, cigar, _ in vm.HAND_READS]
    want = [c for _, _, c in vm.HAND_READS]
    for introns in (im.EXON_FIRST, im.ALL):
        got = both(ctx, vm.HAND_EXONS, reads, am.FORWARD, introns, n_genes=2)
        assert list(got["cls"]) == want
        assert list(got["class_counts"]) == [1, 3, 1, 3, 1]
    # a nested gene's exon that fills the intron exactly: the gap is still not gene 0's
    filled = vm.HAND_EXONS + ((0, 200, 300, "+", 2),)
    got = both(ctx, filled, reads, am.FORWARD, im.EXON_FIRST, n_genes=3)
    assert got["cls"][2] == vm.JUNCTION and got["status"][1] == im.SEVERAL
    # the introns model's own hand cases, on every strand mode
    names, hand = zip(*im.hand_reads())
    for mode in am.MODES.values():
        for introns in im.INTRONS.values():
            both(ctx, im.HAND_EXONS, hand, mode, introns, n_genes=im.HAND_N_GENES)


@pytest.mark.parametrize("introns", ["exon-first", "all"])
@pytest.mark.parametrize("mode", STRANDS)
def test_fuzz_against_the_model(ctx, mode, introns):
    exp = vm.fuzz_expected(am.MODES[mode], im.INTRONS[introns])
    got = both(ctx, vm.fuzz_annotation(), vm.fuzz_reads(), am.MODES[mode], im.INTRONS[introns], n_genes=N_GENES, exp=exp)
    assert min(got["class_counts"]) >= 50 and got["counts"][3] >= 20


def test_the_sampled_tops_change_nothing(ctx):
    exons, arrays = list(vm.fuzz_annotation()), am.pack_reads(vm.fuzz_reads())
    n = 2 * im.GENE_BODY_TOP_CAP + 1  # (its exon table has 2 n segments: a top of stride 1; am.GENE_TOP_CAP + 1 genes: stride 2)
    combs = {k: (list(im.body_comb(k)), im.body_comb_reads(k)) for k in (n, am.GENE_TOP_CAP + 1)}
    comb_exp = {(k, i): vm.classify_all(c, r, am.FORWARD, i) for k, (c, r) in combs.items() for i in (im.EXON_FIRST, im.ALL)}
    try:
        for top, body_top in ((0, 1), (0, 0), (1, 0), (1, 1)):
            ctx.set_option("gene_top", top)
            ctx.set_option("gene_body_top", body_top)
            for introns in (im.EXON_FIRST, im.ALL):
                same(ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, introns, *arrays), vm.fuzz_expected(am.FORWARD, introns))
                for k, (c, r) in combs.items():
                    same(ctx.assign_genes_classes(c, k, am.FORWARD, introns, *am.pack_reads(r)), comb_exp[(k, introns)])
    finally:
        ctx.set_option("gene_top", 1)
        ctx.set_option("gene_body_top", 1)


def test_read_counts(ctx):
    exons = list(vm.fuzz_annotation())
    ref, pos, rev, cigar, off = am.pack_reads(vm.fuzz_reads())
    words = np.diff(off.astype(np.int64))
    t = am.GENE_THREADS
    for introns in (im.EXON_FIRST, im.ALL):
        exp = vm.fuzz_expected(am.FORWARD, introns)
        for n in (1, 63, 64, 65, t - 1, t, t + 1, 2 * t + 1):
            want = {f: exp[f][:n] for f in ("gene", "status", "tier", "cls")}
            want["counts"], want["class_counts"] = im.counts_of(want["status"], want["tier"]), vm.class_counts_of(want["cls"])
            n_off = np.concatenate([[0], np.cumsum(words[:n])]).astype(np.uint64)
            arrays = (ref[:n], pos[:n], rev[:n], cigar[:int(n_off[-1])], n_off)
            got = ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, introns, *arrays)
            assert len(got["cls"]) == n and int(got["class_counts"].sum()) == n
            same(got, want)
            if n in (1, 65, t + 1):
                same(device_call(ctx, exons, N_GENES, am.FORWARD, introns, arrays), want)


def test_more_reads_than_the_grid_has_lanes(ctx):
    """a grid stride: the fuzz reads over and over, one read beyond what the resident blocks take at once"""
    import torch
    t = am.GENE_THREADS
    n = torch.cuda.get_device_properties(0).multi_processor_count * am.GENE_BLOCKS_PER_CU * t + 1
    exons = list(vm.fuzz_annotation())
    ref, pos, rev, cigar, off = am.pack_reads(vm.fuzz_reads())
    reps = -(-n // len(ref))
    exp = vm.fuzz_expected(am.FORWARD, im.EXON_FIRST)
    want = {f: np.tile(exp[f], reps)[:n] for f in ("gene", "status", "tier", "cls")}
    want["counts"], want["class_counts"] = im.counts_of(want["status"], want["tier"]), vm.class_counts_of(want["cls"])
    n_off = np.concatenate([[0], np.cumsum(np.tile(np.diff(off.astype(np.int64)), reps)[:n])]).astype(np.uint64)
    arrays = (np.tile(ref, reps)[:n], np.tile(pos, reps)[:n], np.tile(rev, reps)[:n], np.tile(cigar, reps)[:int(n_off[-1])], n_off)
    same(ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, im.EXON_FIRST, *arrays), want)


def test_no_reads_and_no_lines(ctx):
    import torch
    cls = torch.full((8,), FILL, dtype=torch.uint8, device="cuda:0")
    counts, class_counts = ctx.assign_genes_classes_device(list(vm.fuzz_annotation()), N_GENES, am.FORWARD, im.EXON_FIRST, 0, 0, 0, 0, 0, 0,
                                                           0, 0, 0, cls.data_ptr())
    torch.cuda.synchronize()
    assert list(counts) == [0, 0, 0, 0] and list(class_counts) == [0] * 5 and (cls.cpu().numpy() == FILL).all()
    got = ctx.assign_genes_classes(list(vm.fuzz_annotation()), N_GENES, am.FORWARD, im.ALL, *am.pack_reads([]))
    assert len(got["cls"]) == 0 and list(got["class_counts"]) == [0] * 5
    reads = list(vm.fuzz_reads()[:500])
    for introns in im.INTRONS.values():
        got = both(ctx, [], reads, am.FORWARD, introns, n_genes=0)
        assert list(got["counts"]) == [0, 0, 500, 0] and list(got["class_counts"]) == [500, 0, 0, 0, 0]


def test_off_classes_are_relative_to_the_lines(ctx):
    """intron mode off: no read is intronic; whole genes passed as exons: no read is intronic either, and a read inside
    its gene is exonic (one that runs over the gene's end is still spanning)"""
    exons, reads = vm.fuzz_annotation(), vm.fuzz_reads()
    got = both(ctx, exons, reads, am.FORWARD, im.OFF, n_genes=N_GENES)
    assert got["class_counts"][vm.INTRONIC] == 0 and got["class_counts"][vm.JUNCTION] > 50
    whole = im.bodies(exons)
    got = both(ctx, whole, reads, am.UNSTRANDED, im.EXON_FIRST, n_genes=N_GENES)
    assert got["class_counts"][vm.EXONIC] > 500 and got["counts"][1] == 0 and got["class_counts"][vm.INTRONIC] == 0


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    exons = list(vm.fuzz_annotation())
    reads = list(vm.fuzz_reads()[:3000])
    ref, pos, rev, cigar, off = am.pack_reads(reads)

    def raises(code, word, *arrays, call=ctx.assign_genes_classes, introns=im.EXON_FIRST):
        for fn in (call, ctx.assign_genes_introns):  # the introns call's errors, word for word
            with pytest.raises(umi.UmiHipError) as e:
                fn(exons, N_GENES, am.FORWARD, introns, *arrays)
            assert e.value.code == code and word in str(e.value), str(e.value)

    for introns in (im.EXON_FIRST, im.ALL):
        bad = cigar.copy()
        bad[int(off[1235]) - 1] = 5 << 4 | 9   # the last word of read 1234
        bad[int(off[2500])] = 5 << 4 | 15
        raises(umi._lib.UMI_ERR_ARG, "read 1234:", ref, pos, rev, bad, off, introns=introns)
        bad = off.copy()
        bad[700] = bad[701] + 1  # read 700 runs backwards
        raises(umi._lib.UMI_ERR_ORDER, "read 700", ref, pos, rev, cigar, bad, introns=introns)
        bad = ref.copy()
        bad[2000] = -1
        raises(umi._lib.UMI_ERR_ARG, "read 2000", bad, pos, rev, cigar, off, introns=introns)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, 3, ref, pos, rev, cigar, off)
    assert e.value.code == umi._lib.UMI_ERR_ARG and "intron_mode" in str(e.value)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.assign_genes_classes([(0, 5, 5, "+", 0)], 1, am.FORWARD, 1, ref, pos, rev, cigar, off)
    assert e.value.code == umi._lib.UMI_ERR_ARG and "interval" in str(e.value)
    # a null among the two new pointers, through the C interface
    import ctypes as C
    lib, p = umi.load(), umi._lib.ptr
    ex = ctx._exon_arrays(exons)
    one = am.pack_reads([reads[0]])
    ptrs = [p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32)]
    rd = [p(one[0], C.c_int32), p(one[1], C.c_int32), p(one[2], C.c_uint8), p(one[3], C.c_uint32), p(one[4], C.c_uint64)]
    gene, status, tier, cls = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.full(1, 9, np.uint8)
    counts, class_counts = np.zeros(4, np.uint64), np.zeros(5, np.uint64)
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(tier, C.c_uint8), p(cls, C.c_uint8), p(counts, C.c_uint64), p(class_counts, C.c_uint64)]
    for i in range(6):
        a = list(outs)
        a[i] = None
        assert lib.umi_assign_genes_classes(ctx._h, *ptrs, len(ex[0]), N_GENES, 0, 1, *rd, 1, *a) == umi._lib.UMI_ERR_ARG
    assert lib.umi_assign_genes_classes(None, *ptrs, len(ex[0]), N_GENES, 0, 1, *rd, 1, *outs) == umi._lib.UMI_ERR_ARG
    assert cls[0] == 9
    assert lib.umi_assign_genes_classes(ctx._h, *ptrs, len(ex[0]), N_GENES, 0, 1, *rd, 1, *outs) == 0
    assert cls[0] == vm.fuzz_expected(am.FORWARD, im.EXON_FIRST)["cls"][0]
    # the context is as good as before
    want = vm.fuzz_expected(am.FORWARD, im.EXON_FIRST)
    got = ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, im.EXON_FIRST, ref, pos, rev, cigar, off)
    assert (got["cls"] == want["cls"][:3000]).all()


def test_device_form_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    same(device_call(ctx, list(vm.fuzz_annotation()), N_GENES, am.REVERSE, im.EXON_FIRST, am.pack_reads(vm.fuzz_reads()), stream=s.cuda_stream),
         vm.fuzz_expected(am.REVERSE, im.EXON_FIRST))


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the assignment lets it end first, and its result is still handed
    out, and right, afterwards"""
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
    exons, arrays = list(vm.fuzz_annotation()), am.pack_reads(vm.fuzz_reads())
    same(ctx.assign_genes_classes(exons, N_GENES, am.FORWARD, im.EXON_FIRST, *arrays), vm.fuzz_expected(am.FORWARD, im.EXON_FIRST))
    same(device_call(ctx, exons, N_GENES, am.FORWARD, im.ALL, arrays), vm.fuzz_expected(am.FORWARD, im.ALL))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        exons, arrays = list(vm.fuzz_annotation()), am.pack_reads(vm.fuzz_reads())
        exp = vm.fuzz_expected(am.UNSTRANDED, im.EXON_FIRST)
        same(c.assign_genes_classes(exons, N_GENES, am.UNSTRANDED, im.EXON_FIRST, *arrays), exp)
        same(device_call(c, exons, N_GENES, am.UNSTRANDED, im.EXON_FIRST, arrays), exp)
    finally:
        c.close()
