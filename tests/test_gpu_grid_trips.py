"""Every analysis call under a grid of one CU and of three (option "grid_cus"), on the inputs of tests/grid_trip_inputs.py:
a few thousand items then send each grid-stride kernel round its loop three times, the last trip with a partial last
wave -- the code that on a whole device runs only beyond half a million items, which no test reaches.  Every output
equals the model's exactly (counts, statuses, refusals and the first bad read included) and, byte for byte, what a
context with the default grid returns; the host form of every call, and the _device form through the per-feature
file's own guard-band helper.  tests/test_grid_trip_inputs_cpu.py proves what each input holds.  The collapse itself
runs under the small grid at the end of the file.

Mutation check (on scratch copies of the library, never committed).  The mutant is "this capped loop makes one trip":
the stride is replaced by the loop's limit, so the body runs once.  Where later kernels take indices from what the
loop writes (val[] of count_reduce, velocity_reduce, mg_entry and cells_keys) the unwritten words would be whatever the
workspace held, so the mutant builds zero the single-shot workspace before every call; cells_call_kernel, whose flag[]
shares the sort's buffers, calls no cell in its later trips instead of writing nothing.  Nothing faulted.

Build A, every capped loop of the twelve analysis sources cut at once.  The per-feature files:
  all green (the gap)   test_gpu_stats, test_gpu_barcodes, test_gpu_barcodes_multi, test_gpu_whitelist, test_gpu_call_cells,
                        test_gpu_count_matrix, test_gpu_velocity_matrix, test_gpu_multigene
  one test red each     test_gpu_assign_genes::test_read_counts, test_gpu_assign_genes_introns::test_read_counts,
                        test_gpu_gene_classes::test_more_reads_than_the_grid_has_lanes (one read beyond the resident grid:
                        a second trip of one lane); test_gpu_consensus::test_sums_beyond_32_bits and
                        test_gpu_consensus_bam::test_sums_beyond_32_bits (2^26 reads in one cluster: the deep kernel's
                        chunk loop strides; one deep cluster, so nothing wraps and the deep call makes one trip)
  this file             every test of an analysis call red but test_consensus_seqs_lanes_and_tiles[700] and
                        test_consensus_bam_lanes_and_tiles[300] (one tile: no capped loop strides there; they are for the
                        lanes beyond lane 0); the collapse tests green (no collapse kernel was cut)
One kernel a source file at a time (seven builds; the tests of this file that turned red):
  stats_entry_kernel, stats_post_kernel        test_dedup_stats_* (all four)
  stats_lane_kernel, stats_wave_kernel         test_dedup_stats_lanes_and_waves_buckets[12], [43], _without_the_per_umi_table
  stats_deep_roots / _deep_count (together)    test_dedup_stats_deep_buckets
  barcode_build_kernel                         test_correct_barcodes[*], _multi[*], test_barcode_list_with_a_duplicate_...
  barcode_dup_kernel                           test_barcode_list_with_a_duplicate_beyond_its_first_trip[16], [17]
  barcode_check_kernel, _qual_check_kernel     test_barcode_bad_bytes_in_the_third_trip[16], [17]
  barcode_lookup_kernel                        test_correct_barcodes[*], test_correct_barcodes_multi[*]
  barcode_resolve_kernel                       test_correct_barcodes_multi[16], [17]
  correct_check_kernel                         test_correct_umis_bad_byte_in_the_third_trip[12], [20]
  correct_kernel                               test_correct_umis[*] (all six), test_option_range
  cells_keys_kernel, cells_call_kernel         test_call_cells[one_each], [runs]
  count_reduce_kernel                          test_count_matrix
  velocity_scatter_kernel, _reduce_kernel      test_velocity_matrix[0], [1]
  mg_entry_kernel, mg_write_kernel             test_filter_multigene[12], [22]
  gene_assign / _introns / _classes kernel     test_assign_genes[*] / test_assign_genes_introns[*] / test_assign_genes_classes[*]
  cons_vote_kernel (tile loop)                 test_consensus_seqs_lanes_and_tiles[4166]
  cons_deep_kernel (chunk loop)                test_consensus_seqs_deep_clusters
  cons_deep_call_kernel                        test_consensus_seqs_deep_clusters
  consb_vote_kernel (tile loop)                test_consensus_bam_lanes_and_tiles[1100]
  consb_deep_kernel, consb_deep_call_kernel    test_consensus_bam_deep_clusters
The first deep input left cons_deep_kernel's mutant green: half of 8,322 reads call the same bases with capped
qualities.  The deepest cluster now votes A over C at one base by a margin of 7 (grid_trip_inputs.CONS_CLOSE_MARGIN),
which any read left out moves.

Kernel names since: count_heads_kernel, velocity_heads_kernel, saturation_heads_kernel and mg_heads_key_kernel are one
kernel, pair_heads_kernel<256> (csrc/umihip_pair_table.h).  It loops grid-stride; of its callers only the saturation
curve launches it under the cap, the others in one trip as before, so none of the rows above is another kernel's now.
"""
import numpy as np
import pytest

import annotation_model as am
import barcode_model as bm
import barcode_multi_model as bmm
import cluster_model
import edit_model as em
import grid_trip_inputs as gi
import helpers as h
import intron_model as im
import oracle as orc
import seq_model as sm
import test_gpu_assign_genes as t_genes
import test_gpu_assign_genes_introns as t_introns
import test_gpu_barcodes as t_bc
import test_gpu_barcodes_multi as t_bcm
import test_gpu_call_cells as t_cells
import test_gpu_consensus as t_cons
import test_gpu_consensus_bam as t_consb
import test_gpu_count_matrix as t_count
import test_gpu_gene_classes as t_classes
import test_gpu_large_k as t_large_k
import test_gpu_multigene as t_mg
import test_gpu_stats as t_stats
import test_gpu_velocity_matrix as t_vel
import test_gpu_whitelist as t_wl

pytestmark = pytest.mark.gpu
DEFAULT = 0  # the key of the context that never sets the option
COUNTERS = ("n_umis", "n_buckets", "max_bucket", "n_kept", "n_pairs", "n_pairs_evaluated", "n_candidates", "n_edges")


@pytest.fixture(scope="module")
def ctxs():
    """{0: a context with the default grid, 1: "grid_cus" 1, 3: "grid_cus" 3}"""
    import umi_collapse_rs_amd as umi
    out = {DEFAULT: umi.Context(0)}
    for g in gi.GRIDS:
        out[g] = umi.Context(0)
        out[g].set_option("grid_cus", g)
    yield out
    for c in out.values():
        c.close()


class options:
    """an option on every context of the fixture for the length of a with block"""

    def __init__(self, ctxs, **values):
        self.ctxs, self.values = ctxs, values

    def __enter__(self):
        for c in self.ctxs.values():
            for name, (v, _) in self.values.items():
                c.set_option(name, v)

    def __exit__(self, *exc):
        for c in self.ctxs.values():
            for name, (_, back) in self.values.items():
                c.set_option(name, back)


def frozen(x):
    """a result as bytes and plain values, for ==: arrays by dtype, shape and content"""
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    if isinstance(x, dict):
        return tuple((k, frozen(v)) for k, v in sorted(x.items()))
    if isinstance(x, (list, tuple)):
        return tuple(frozen(v) for v in x)
    return x


def every_grid(ctxs, call, check):
    """call(context) under the default grid and under every small one: check(result) compares it with the model, and
    the small grids' results are the default grid's byte for byte"""
    ref = call(ctxs[DEFAULT])
    check(ref)
    for g in gi.GRIDS:
        got = call(ctxs[g])
        check(got)
        assert frozen(got) == frozen(ref), "grid_cus %d: not what the default grid returns" % g


def refused_alike(ctxs, call, code, *words):
    """call(context) is refused under every grid, with one and the same message"""
    import umi_collapse_rs_amd as umi
    texts = []
    for g in (DEFAULT,) + gi.GRIDS:
        with pytest.raises(umi.UmiHipError) as e:
            call(ctxs[g])
        assert e.value.code == code, (g, str(e.value))
        assert all(w in str(e.value) for w in words), (g, str(e.value))
        texts.append(str(e.value))
    assert len(set(texts)) == 1, texts


# ---- the option -----------------------------------------------------------------------------------------------------

def test_option_range():
    import torch
    import umi_collapse_rs_amd as umi
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    keys, nm, fr, off = h.one_word_batch(12, 1, 0.01)
    wl, reads = gi.correct_case(12, "tile_and_one")
    fresh, c = umi.Context(0), umi.Context(0)
    try:
        for bad in (-1, cus + 1, 2 ** 31):
            with pytest.raises(umi.UmiHipError) as e:
                c.set_option("grid_cus", bad)
            assert e.value.code == umi._lib.UMI_ERR_ARG and "grid_cus" in str(e.value)
        want = fresh.dedup_batch(keys, nm, fr, off, 12, 1)
        want_umis = fresh.correct_umis(reads, 12, wl, 1, 1)
        for v in (cus, 1, 0):  # the device's own count is allowed; 0 after 1 puts the default back
            c.set_option("grid_cus", v)
            kept, root, st = c.dedup_batch(keys, nm, fr, off, 12, 1)
            assert kept.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
            # (umi_stats reports no grid size; its pair counters do not depend on the grid)
            assert {f: st[f] for f in COUNTERS} == {f: want[2][f] for f in COUNTERS}
            assert frozen(c.correct_umis(reads, 12, wl, 1, 1)) == frozen(want_umis)
        # a refused value leaves the option as it was
        c.set_option("grid_cus", 1)
        with pytest.raises(umi.UmiHipError):
            c.set_option("grid_cus", cus + 1)
        assert frozen(c.correct_umis(reads, 12, wl, 1, 1)) == frozen(want_umis)
    finally:
        fresh.close()
        c.close()
    multi = umi.Context([0, 0])  # a multi-device context hands the option to its devices, refusals included
    try:
        multi.set_option("grid_cus", 1)
        with pytest.raises(umi.UmiHipError):
            multi.set_option("grid_cus", cus + 1)
        kept, root, _ = multi.dedup_batch(keys, nm, fr, off, 12, 1)
        assert kept.tobytes() == want[0].tobytes() and root.tobytes() == want[1].tobytes()
        assert frozen(multi.correct_umis(reads, 12, wl, 1, 1)) == frozen(want_umis)
    finally:
        multi.close()


# ---- umi_correct_umis -----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(gi.CORR_LISTS))
@pytest.mark.parametrize("L", gi.CORR_LENGTHS)
def test_correct_umis(ctxs, L, name):
    (wl, reads), exp = gi.correct_case(L, name), gi.correct_expected(L, name)
    every_grid(ctxs, lambda c: c.correct_umis(reads, L, wl, 1, 1), lambda got: t_wl.same(got, exp))
    for kw in (dict(), dict(in_place=True), dict(want_out=False, want_second=False), dict(shift=1)):
        every_grid(ctxs, lambda c: t_wl.device_call(c, reads, L, wl, 1, 1, **kw),
                   lambda got: t_wl.same(got, exp, [f for f in t_wl.FIELDS if f in got]))


@pytest.mark.parametrize("L", gi.CORR_LENGTHS)
def test_correct_umis_bad_byte_in_the_third_trip(ctxs, L):
    import umi_collapse_rs_amd as umi
    wl, reads = gi.correct_case(L, "tile_and_one")
    bad = gi.correct_bad_reads(L, "tile_and_one")
    word = "Unknown character in UMI sequence: %d (read 8200)" % ord("n")
    refused_alike(ctxs, lambda c: c.correct_umis(bad, L, wl, 1, 1), umi._lib.UMI_ERR_CHAR, word)
    refused_alike(ctxs, lambda c: t_wl.device_call(c, bad, L, wl, 1, 1), umi._lib.UMI_ERR_CHAR, word)
    exp = gi.correct_expected(L, "tile_and_one")  # ... and the contexts are as good as before
    every_grid(ctxs, lambda c: c.correct_umis(reads, L, wl, 1, 1), lambda got: t_wl.same(got, exp))


# ---- umi_correct_barcodes / _multi ----------------------------------------------------------------------------------

@pytest.mark.parametrize("mm", [0, 1])
@pytest.mark.parametrize("L", gi.BC_LENGTHS)
def test_correct_barcodes(ctxs, L, mm):
    (wl, reads, _), exp = gi.barcode_case(L), gi.barcode_expected(L, mm)
    every_grid(ctxs, lambda c: c.correct_barcodes(reads, L, wl, mm), lambda got: t_bc.same(got, exp))
    for kw in (dict(), dict(shift=3, want_status=False)):
        every_grid(ctxs, lambda c: t_bc.device_call(c, reads, L, wl, mm, **kw),
                   lambda got: t_bc.same(got, exp, [f for f in t_bc.FIELDS if f in got]))


@pytest.mark.parametrize("L", gi.BC_LENGTHS)
def test_barcode_list_with_a_duplicate_beyond_its_first_trip(ctxs, L):
    import umi_collapse_rs_amd as umi
    wl, reads, quals = gi.barcode_case(L)
    dup = gi.barcode_dup_list(L)
    word = "duplicate entry in the barcode whitelist: entry %d equals an earlier one" % gi.BC_DUP[0]
    refused_alike(ctxs, lambda c: c.correct_barcodes(reads, L, dup, 1), umi._lib.UMI_ERR_ARG, word)
    refused_alike(ctxs, lambda c: c.correct_barcodes_multi(reads, quals, L, dup), umi._lib.UMI_ERR_ARG, word)
    exp = gi.barcode_expected(L, 1)
    every_grid(ctxs, lambda c: c.correct_barcodes(reads, L, wl, 1), lambda got: t_bc.same(got, exp))


@pytest.mark.parametrize("L", gi.BC_LENGTHS)
def test_barcode_bad_bytes_in_the_third_trip(ctxs, L):
    import umi_collapse_rs_amd as umi
    wl, reads, quals = gi.barcode_case(L)
    bad, bad_q = gi.barcode_bad_reads(L), gi.barcode_bad_quals(L)
    word = "Unknown character in cell barcode: %d (read %d)" % (ord("n"), gi.BC_BAD[1][0])
    refused_alike(ctxs, lambda c: c.correct_barcodes(bad, L, wl, 1), umi._lib.UMI_ERR_CHAR, word)
    refused_alike(ctxs, lambda c: c.correct_barcodes_multi(bad, quals, L, wl), umi._lib.UMI_ERR_CHAR, word)
    word_q = "Unknown character in cell barcode quality: %d (read %d)" % (gi.BC_BAD_QUAL[2], gi.BC_BAD_QUAL[0])
    refused_alike(ctxs, lambda c: c.correct_barcodes_multi(reads, bad_q, L, wl), umi._lib.UMI_ERR_CHAR, word_q)
    # the bad barcode byte lies in an earlier read than the bad quality byte: it is the one reported
    refused_alike(ctxs, lambda c: c.correct_barcodes_multi(bad, bad_q, L, wl), umi._lib.UMI_ERR_CHAR, word)


@pytest.mark.parametrize("L", gi.BC_LENGTHS)
def test_correct_barcodes_multi(ctxs, L):
    (wl, reads, quals), exp = gi.barcode_case(L), gi.barcode_multi_expected(L)
    every_grid(ctxs, lambda c: c.correct_barcodes_multi(reads, quals, L, wl), lambda got: t_bcm.same(got, exp))
    every_grid(ctxs, lambda c: t_bcm.device_call(c, reads, quals, L, wl), lambda got: t_bcm.same(got, exp))
    plain = gi.barcode_expected(L, 1)  # the first pass is the plain call's
    got = ctxs[1].correct_barcodes_multi(reads, quals, L, wl)
    first = got["status"] != bmm.RESOLVED
    assert (got["status"][first] == plain["status"][first]).all() and (plain["status"][~first] == bm.AMBIGUOUS).all()


# ---- umi_count_matrix and umi_velocity_matrix -----------------------------------------------------------------------

def test_count_matrix(ctxs):
    case, exp = gi.count_case(), gi.count_expected()
    every_grid(ctxs, lambda c: c.count_matrix(*case), lambda got: t_count.same(got, exp))
    every_grid(ctxs, lambda c: t_count.device_call(c, *case), lambda got: t_count.same(got, exp))


@pytest.mark.parametrize("skip", [0, 1])
def test_velocity_matrix(ctxs, skip):
    m, exp = gi.velocity_case(), gi.velocity_expected()
    with options(ctxs, velocity_skip=(skip, 0)):
        every_grid(ctxs, lambda c: c.velocity_matrix(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"],
                                                     m["col"], gi.MATRIX_ROWS, gi.MATRIX_COLS), lambda got: t_vel.same(got, exp))
        every_grid(ctxs, lambda c: t_vel.device_call(c, m, gi.MATRIX_ROWS, gi.MATRIX_COLS), lambda got: t_vel.same(got, exp))


# ---- umi_filter_multigene -------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", gi.MG_LENGTHS)
def test_filter_multigene(ctxs, L):
    case = gi.multigene_case(L)
    exp = case.expected()
    every_grid(ctxs, lambda c: t_mg.host_call(c, case), lambda got: t_mg.same(got, exp))
    every_grid(ctxs, lambda c: t_mg.device_call(c, case), lambda got: t_mg.same(got, exp))
    every_grid(ctxs, lambda c: t_mg.device_call(c, case, want_freq=False), lambda got: t_mg.same(got, exp, want_freq=False))


# ---- umi_call_cells -------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", ["one_each", "runs"])
def test_call_cells(ctxs, name):
    case = gi.cells_cases()[name]
    for k, rule in enumerate(gi.cells_rules(name)):
        exp = gi.cells_expected(name, k)
        every_grid(ctxs, lambda c: t_cells.host_call(c, case, **rule), lambda got: t_cells.same(got, exp))
        every_grid(ctxs, lambda c: t_cells.device_call(c, case, **rule), lambda got: t_cells.same(got, exp))


# ---- umi_assign_genes, _introns, _classes ---------------------------------------------------------------------------

@pytest.mark.parametrize("top", [1, 0])
def test_assign_genes(ctxs, top):
    exons, arrays = list(am.fuzz_annotation()), am.pack_reads(gi.gene_reads())
    with options(ctxs, gene_top=(top, 1)):
        for mode in (am.FORWARD, am.UNSTRANDED):
            exp = gi.genes_expected(mode)
            every_grid(ctxs, lambda c: c.assign_genes(exons, gi.N_GENES, mode, *arrays), lambda got: t_genes.same(got, exp))
            every_grid(ctxs, lambda c: t_genes.device_call(c, exons, gi.N_GENES, mode, arrays), lambda got: t_genes.same(got, exp))


@pytest.mark.parametrize("tops", gi.GENE_TOPS, ids=lambda t: "top %d body %d" % t)
@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_assign_genes_introns(ctxs, introns, tops):
    exons, arrays, i = list(am.fuzz_annotation()), am.pack_reads(gi.gene_reads()), im.INTRONS[introns]
    exp = gi.introns_expected(am.FORWARD, i)
    with options(ctxs, gene_top=(tops[0], 1), gene_body_top=(tops[1], 1)):
        every_grid(ctxs, lambda c: c.assign_genes_introns(exons, gi.N_GENES, am.FORWARD, i, *arrays), lambda got: t_introns.same(got, exp))
        every_grid(ctxs, lambda c: t_introns.device_call(c, exons, gi.N_GENES, am.FORWARD, i, arrays),
                   lambda got: t_introns.same(got, exp))


@pytest.mark.parametrize("tops", gi.GENE_TOPS, ids=lambda t: "top %d body %d" % t)
@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_assign_genes_classes(ctxs, introns, tops):
    import velocity_model as vm
    exons, arrays, i = list(vm.fuzz_annotation()), am.pack_reads(gi.class_reads()), im.INTRONS[introns]
    exp = gi.classes_expected(am.FORWARD, i)
    with options(ctxs, gene_top=(tops[0], 1), gene_body_top=(tops[1], 1)):
        every_grid(ctxs, lambda c: c.assign_genes_classes(exons, gi.N_GENES_CLASSES, am.FORWARD, i, *arrays),
                   lambda got: t_classes.same(got, exp))
        every_grid(ctxs, lambda c: t_classes.device_call(c, exons, gi.N_GENES_CLASSES, am.FORWARD, i, arrays),
                   lambda got: t_classes.same(got, exp))


# ---- umi_dedup_stats ------------------------------------------------------------------------------------------------

def stats_calls(ctxs, case, exp, per_umi=True):
    keys, freq, kept, root, off, L = case
    every_grid(ctxs, lambda c: c.dedup_stats(keys, freq, kept, root, off, L, n_words=t_stats.sm.n_words_of(L), seed=5, hist_bins=65536,
                                             per_umi=per_umi), lambda got: t_stats.same(got, exp))
    every_grid(ctxs, lambda c: t_stats.device_call(c, case, 5, 65536, per_umi), lambda got: t_stats.same(got, exp))


@pytest.mark.parametrize("L", gi.STATS_LENGTHS)
def test_dedup_stats_lanes_and_waves_buckets(ctxs, L):
    stats_calls(ctxs, gi.stats_case_a(L), gi.stats_expected("a", L))


def test_dedup_stats_without_the_per_umi_table(ctxs):
    stats_calls(ctxs, gi.stats_case_a(12), gi.stats_expected("a", 12, per_umi=False), per_umi=False)


def test_dedup_stats_deep_buckets(ctxs):
    with options(ctxs, stats_split=(gi.STATS_B_SPLIT, 4096)):
        stats_calls(ctxs, gi.stats_case_b(), gi.stats_expected("b"))


# ---- umi_consensus_seqs ---------------------------------------------------------------------------------------------

def consensus_calls(ctxs, case, want):
    seqs, quals, staged, kept, root = case
    every_grid(ctxs, lambda c: c.consensus_seqs(seqs, quals, staged, kept, root), lambda got: t_cons.same(got, want))
    every_grid(ctxs, lambda c: t_cons.device_call(c, seqs, quals, staged, kept, root, odd=1)[0], lambda got: t_cons.same(got, want))


@pytest.mark.parametrize("n_entries", gi.CONS_ENTRIES)
def test_consensus_seqs_lanes_and_tiles(ctxs, n_entries):
    consensus_calls(ctxs, gi.cons_entries_case(n_entries), gi.cons_expected(n_entries))


def test_consensus_seqs_deep_clusters(ctxs):
    with options(ctxs, cons_split=(gi.CONS_SPLIT, 512)):
        consensus_calls(ctxs, gi.cons_deep_case(), gi.cons_expected("deep"))
    # the same clusters by one wave each: the split changes nothing
    consensus_calls(ctxs, gi.cons_deep_case(), gi.cons_expected("deep"))


# ---- umi_consensus_bam ----------------------------------------------------------------------------------------------

def consensus_bam_calls(ctxs, case, want):
    every_grid(ctxs, lambda c: t_consb.host_call(c, case), lambda got: t_consb.same(got, want))
    every_grid(ctxs, lambda c: t_consb.device_call(c, case, odd=3)[0], lambda got: t_consb.same(got, want))


@pytest.mark.parametrize("n_clusters", gi.CONSB_CLUSTERS)
def test_consensus_bam_lanes_and_tiles(ctxs, n_clusters):
    consensus_bam_calls(ctxs, gi.consb_clusters_case(n_clusters), gi.consb_expected(n_clusters))


def test_consensus_bam_deep_clusters(ctxs):
    with options(ctxs, cons_split=(gi.CONS_SPLIT, 512)):
        consensus_bam_calls(ctxs, gi.consb_deep_case(), gi.consb_expected("deep"))


# ---- the collapse under a small grid --------------------------------------------------------------------------------
# (its kernels size persistent grids from the same count: "fused_blocks" per CU, the segment index's pair, local and
# super-bin kernels, the whole-read pair kernel's 16 one-wave blocks)

MODES = ((0, 0), (1, 2))  # (algo, adj_max_freq)


def collapse_under_the_small_grid(ctxs, run, models):
    """run(ctx, algo, amf) -> (kept, root, stats) at "grid_cus" 1 against models[(algo, amf)] = (kept, root), and its
    counters against the default grid's"""
    for (algo, amf), (ekept, eroot) in models.items():
        ref = run(ctxs[DEFAULT], algo, amf)
        kept, root, st = run(ctxs[1], algo, amf)
        assert (np.asarray(kept) != 0).tolist() == (np.asarray(ekept) != 0).tolist(), (algo, amf)
        assert np.asarray(root).tolist() == np.asarray(eroot).tolist(), (algo, amf)
        assert kept.tobytes() == ref[0].tobytes() and root.tobytes() == ref[1].tobytes()
        assert {f: st[f] for f in COUNTERS} == {f: ref[2][f] for f in COUNTERS}, (algo, amf)


@pytest.mark.parametrize("k", [1, 3])
def test_collapse_one_word(ctxs, k):
    keys, nm, fr, off = h.one_word_batch(12, k, 0.01)
    models = {(a, f): orc.dedup_batch(keys, nm, fr, off, 12, k, 0.5, a, f)[:2] for a, f in MODES}
    models[(2, 0)] = cluster_model.batch_of_keys(keys, nm, off.astype(np.int64), k)
    collapse_under_the_small_grid(ctxs, lambda c, a, f: c.dedup_batch(keys, nm, fr, off, 12, k, 0.5, a, f), models)


def test_collapse_wide(ctxs):
    keys, nm, fr, off = h.wide_batch(43, 2)
    models = {(a, f): orc.dedup_batch_wide(keys, nm, fr, off, 43, 2, 0.5, a, f)[:2] for a, f in MODES}
    models[(2, 0)] = cluster_model.batch_of_keys(keys, nm, off.astype(np.int64), 2)
    collapse_under_the_small_grid(ctxs, lambda c, a, f: c.dedup_batch_wide(keys, nm, fr, off, 43, 2, 0.5, a, f), models)


def test_collapse_edit_distance(ctxs):
    buckets, mats, (keys, nm, fr, off) = em.batch(12, 0.0)
    models = {(a, f): em.model_batch(buckets, 2, 0.5, a, f, mats) for a, f in MODES}
    models[(2, 0)] = cluster_model.batch(mats, off.astype(np.int64), 2)
    collapse_under_the_small_grid(ctxs, lambda c, a, f: c.dedup_batch_edit(keys, nm, fr, off, 12, 2, 0.5, a, f), models)


def heavy_bin_bucket():
    """tests/test_gpu_seqs.py's heavy bin -- the second half of every read constant, so that part 1 of k = 1 is one
    bin -- cut to 2,000 entries: about 500 tile pairs for the pair kernel's 16 blocks"""
    from umi_collapse_rs_amd import synth
    seqs, _ = synth.fastq_reads(9, 12000, 3000, length=150, err=0.004, const_suffix=75, mean_copies=4.0)
    f = {}
    for s in seqs:
        f[s] = f.get(s, 0) + 1
    items = sorted(f.items(), key=lambda kv: -kv[1])[:2000]
    return [([s for s, _ in items], [v for _, v in items])]


@pytest.mark.parametrize("which", ["three buckets, k = 2", "heavy bin, k = 1"])
def test_collapse_whole_reads(ctxs, which):
    buckets, k = (h.seq_buckets(150, 2), 2) if which.startswith("three") else (heavy_bin_bucket(), 1)
    assert which.startswith("three") or len(buckets[0][0]) == 2000
    all_pairs = t_large_k.seq_pairs(buckets, k, join=True)
    for algo, amf in MODES:  # kept, root and the three counters against the model, as tests/test_gpu_large_k.py has it
        st = t_large_k.check_seqs(ctxs[1], buckets, all_pairs, k, algo, amf)
        ref = t_large_k.call_seqs(ctxs[DEFAULT], buckets, k, algo, amf)[2]
        assert {f: st[f] for f in COUNTERS} == {f: ref[f] for f in COUNTERS}
    seqs = [s for b in buckets for s in b[0]]
    off = np.cumsum([0] + [len(b[0]) for b in buckets])
    keys, nm = sm.encode(seqs, sm.words(150))
    ekept, eroot = cluster_model.batch_of_keys(keys, nm, off, k)
    kept, root, _ = t_large_k.call_seqs(ctxs[1], buckets, k, 2, 0)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
