"""tests/intron_model.py on hand-written cases and against a second, naive statement of the rule; what the generated
inputs of the GPU tests must hold; the library's refusals that need no device; and the program's refusals of
--gene-introns, each with status 101, its message, and no file left behind."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import annotation_model as am
import intron_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
A, N, S = im.ASSIGNED, im.NONE, im.SEVERAL
X, I = im.TIER_EXON, im.TIER_INTRON


# ---- the model ------------------------------------------------------------------------------------------

def test_bodies_of_lines():
    ex = [(0, 250, 300, "+", 0), (0, 180, 200, "+", 0), (0, 100, 150, "+", 0),   # the ends come from different lines
          (0, 500, 600, ".", 0), (1, 10, 20, "+", 0), (0, 120, 700, "-", 1), (0, 50, 60, "-", 1)]
    assert im.bodies(ex) == [(0, 100, 300, "+", 0), (0, 500, 600, ".", 0), (1, 10, 20, "+", 0), (0, 50, 700, "-", 1)]
    assert im.bodies([]) == []
    assert sorted(im.bodies(im.HAND_EXONS))[:4] == [(0, 100, 900, "+", 0), (0, 400, 550, "+", 1), (1, 100, 900, "+", 2), (1, 400, 550, "-", 3)]


def hand(what, mode, introns):
    reads = dict(im.hand_reads())
    return im.assign(list(im.HAND_EXONS), *reads[what], mode, introns)


def test_a_gene_nested_in_another_s_intron_on_the_same_strand():
    for mode, strand in ((am.FORWARD, "+"), (am.REVERSE, "-"), (am.UNSTRANDED, "+"), (am.UNSTRANDED, "-")):
        assert hand("inner exon, " + strand, mode, im.EXON_FIRST) == (A, 1, X)
        assert hand("inner exon, " + strand, mode, im.ALL) == (S, -1, 0)
        assert hand("inner exon, " + strand, mode, im.OFF) == (A, 1, X)
        for introns in (im.EXON_FIRST, im.ALL):
            assert hand("inner intron, " + strand, mode, introns) == (S, -1, 0)
            assert hand("outer intron clear of the inner body, " + strand, mode, introns) == (A, 0, I)
            assert hand("exon end into the intron, " + strand, mode, introns) == (A, 0, X)
            assert hand("intron into the exon start, " + strand, mode, introns) == (A, 0, X)
            assert hand("behind the inner body, " + strand, mode, introns) == (A, 0, I)
            assert hand("two exons of gene 0, N over gene 1's body, " + strand, mode, introns) == (A, 0, X)
            assert hand("the same with a deletion, " + strand, mode, introns) == (S, -1, 0)
        assert hand("inner intron, " + strand, mode, im.OFF) == (N, -1, 0)
    for introns in im.INTRONS.values():  # the other strand: nothing is admissible
        assert hand("inner exon, -", am.FORWARD, introns) == hand("inner exon, +", am.REVERSE, introns) == (N, -1, 0)


def test_the_same_nesting_on_opposite_strands():
    for introns in (im.EXON_FIRST, im.ALL):
        assert hand("opposite: inner exon, +", am.FORWARD, introns) == (A, 2, I)   # the outer gene's intron alone
        assert hand("opposite: inner exon, -", am.FORWARD, introns) == (A, 3, X)
        assert hand("opposite: inner exon, +", am.REVERSE, introns) == (A, 3, X)
        assert hand("opposite: inner intron, -", am.FORWARD, introns) == (A, 3, I)
        assert hand("opposite: inner intron, +", am.UNSTRANDED, introns) == (S, -1, 0)
        assert hand("opposite: outer intron, -", am.FORWARD, introns) == (N, -1, 0)
    assert hand("opposite: inner exon, +", am.UNSTRANDED, im.EXON_FIRST) == (A, 3, X)
    assert hand("opposite: inner exon, +", am.UNSTRANDED, im.ALL) == (S, -1, 0)


def test_two_genes_by_exons_or_by_introns_are_several():
    for introns in im.INTRONS.values():
        assert hand("exons of two genes, +", am.FORWARD, introns) == (S, -1, 0)
    for introns in (im.EXON_FIRST, im.ALL):
        assert hand("gene 6's intron and gene 7's, +", am.FORWARD, introns) == (S, -1, 0)
        assert hand("gene 6's intron and between the genes, +", am.FORWARD, introns) == (A, 6, I)
        assert hand("exon of one, body of both, +", am.FORWARD, introns) == (A, 4, X)  # gene 5's body starts at its first exon
        assert hand("intron of 5 alone, +", am.FORWARD, introns) == (A, 5, I)
    assert hand("gene 6's intron and gene 7's exon, +", am.FORWARD, im.EXON_FIRST) == (A, 7, X)
    assert hand("gene 6's intron and gene 7's exon, +", am.FORWARD, im.ALL) == (S, -1, 0)


def test_the_ends_of_a_body_and_bodies_per_group():
    for introns in (im.EXON_FIRST, im.ALL):
        got = [hand(w + ", -", am.FORWARD, introns) for w in ("before the body", "the body's first base", "the body's last base",
                                                              "behind the body", "in the body's first intron", "in its second")]
        assert got == [(N, -1, 0), (A, 8, X), (A, 8, X), (N, -1, 0), (A, 8, I), (A, 8, I)]
        for mode in am.MODES.values():  # a '.' body under every strand mode, on both strands
            assert hand("gene 9 on ., +", mode, introns) == hand("gene 9 on ., -", mode, introns) == (A, 9, I)
        assert hand("gene 9 on +, +", am.FORWARD, introns) == (A, 9, I) and hand("gene 9 on +, -", am.FORWARD, introns) == (N, -1, 0)
        assert hand("between gene 9's bodies, +", am.UNSTRANDED, introns) == (N, -1, 0)  # one body per group, not one per gene
        assert hand("across both of gene 9's bodies, +", am.FORWARD, introns) == (A, 9, X)
        assert hand("gene 9 on the other reference, +", am.FORWARD, introns) == (A, 9, I)
        assert hand("gene 9's coordinates of reference 4 on 5, +", am.FORWARD, introns) == (N, -1, 0)


def test_reads_without_blocks_the_ends_of_the_line_and_absent_references():
    for introns in (im.EXON_FIRST, im.ALL):
        for w in ("no words", "no block", "an N alone", "an empty M", "a reference without lines", "another", "a reference far away",
                  "behind gene 10", "at 2^31 - 1", "before gene 11", "beside it"):
            assert hand(w + ", +", am.FORWARD, introns) == (N, -1, 0), w
        assert [hand(w + ", +", am.FORWARD, introns) for w in ("coordinate 0", "an intron near 0", "gene 10's last base")] == \
            [(A, 10, X), (A, 10, I), (A, 10, X)]
        assert [hand(w + ", +", am.FORWARD, introns) for w in ("an intron near the top", "the top base", "beyond the top",
                                                              "gene 11's first base")] == [(A, 11, I), (A, 11, X), (A, 11, X), (A, 11, X)]
        assert hand("from 0 to the top, +", am.FORWARD, introns) == (S, -1, 0)
        assert hand("one exon, no intron, +", am.FORWARD, introns) == (A, 12, X)


def naive_sets(exons, ref, pos, reverse, cigar, mode):
    """the second statement: per base of every block, the genes whose exon covers it and the genes whose body does"""
    span = {}
    for r, s, e, strand, g in exons:
        if r == ref and am.admissible(strand, reverse, mode):
            span.setdefault((g, strand), []).append((s, e))
    E, B = set(), set()
    for s, e in am.blocks(pos, cigar):
        for base in range(s, e):
            for (g, _), lines in span.items():
                if any(xs <= base < xe for xs, xe in lines):
                    E.add(g)
                if min(l[0] for l in lines) <= base < max(l[1] for l in lines):
                    B.add(g)
    return E, B


def naive_verdict(E, B, introns):
    assert E <= B
    if introns == im.OFF or (introns == im.EXON_FIRST and E):
        B = E
    if len(B) != 1:
        return (N if not B else S), -1, 0
    return A, next(iter(B)), (X if E else I)


def test_the_model_against_the_naive_statement():
    exons, reads = list(am.fuzz_annotation()), am.fuzz_reads()[:200]
    hand_exons, hand_reads = list(im.HAND_EXONS), im.hand_reads()
    for mode in am.MODES.values():
        exp = {introns: im.assign_all(exons, reads, mode, introns) for introns in im.INTRONS.values()}
        for i, r in enumerate(reads):
            E, B = naive_sets(exons, *r, mode)
            for introns, e in exp.items():
                got = naive_verdict(E, B, introns)
                assert got == (e["status"][i], e["gene"][i], e["tier"][i]) == im.assign(exons, *r, mode, introns), (i, r)
        for what, r in hand_reads:
            E, B = naive_sets(hand_exons, *r, mode)
            for introns in im.INTRONS.values():
                assert naive_verdict(E, B, introns) == im.assign(hand_exons, *r, mode, introns), what


def test_off_is_the_exon_rule_and_counts_add_up():
    for mode in am.MODES.values():
        off, plain = im.fuzz_expected(mode, im.OFF), am.fuzz_expected(mode)
        assert (off["gene"] == plain["gene"]).all() and (off["status"] == plain["status"]).all() and not off["tier"].any()
        assert list(off["counts"]) == [plain["counts"][0], 0, plain["counts"][1], plain["counts"][2]]
        for introns in (im.EXON_FIRST, im.ALL):
            e = im.fuzz_expected(mode, introns)
            assert int(e["counts"].sum()) == len(e["gene"]) and not e["tier"][e["status"] != A].any()
            assert ((e["gene"] >= 0) == (e["status"] == A)).all()


# ---- what the generated inputs hold ---------------------------------------------------------------------

@pytest.mark.parametrize("mode", sorted(am.MODES))
def test_fuzz_input_has_fifty_reads_of_every_class(mode):
    classes = im.fuzz_classes(am.MODES[mode])
    assert sorted(classes) == ["intron", "none", "rescued", "several"]
    assert min(classes.values()) >= 50, classes


@pytest.mark.parametrize("n", [im.GENE_BODY_TOP_CAP - 1, im.GENE_BODY_TOP_CAP, im.GENE_BODY_TOP_CAP + 1, 2 * im.GENE_BODY_TOP_CAP + 1])
def test_body_combs_have_one_segment_a_gene_and_reads_in_the_gaps(n):
    exons = im.body_comb(n)
    b = im.bodies(exons)
    assert len(b) == n and len({x[4] for x in b}) == n
    assert all(b[i][2] < b[i + 1][1] for i in range(n - 1))  # apart: n segments in the body table, 2 n in the exons'
    exp = im.assign_all(exons, im.body_comb_reads(n), am.FORWARD, im.EXON_FIRST)
    assert min(exp["counts"]) > 50  # by exon, by intron, none, several (a spliced read over two genes)
    firsts = {i for i, t in zip(exp["gene"], exp["tier"]) if t == I}
    assert {0, n - 1} <= firsts


def test_the_sizes_the_gpu_tests_are_placed_by_are_the_library_s():
    import re
    text = open(os.path.join(ROOT, "umi_collapse_rs_amd", "csrc", "umihip_internal.h")).read()
    assert int(re.search(r"constexpr \w+ GENE_BODY_TOP_CAP = (\d+);", text).group(1)) == im.GENE_BODY_TOP_CAP


# ---- the library, before a device is looked at ----------------------------------------------------------

def test_library_refuses_bad_arguments_without_a_context():
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    lib = umi.load()
    for name in ("umi_assign_genes_introns", "umi_assign_genes_introns_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert (umi.UMI_INTRONS_OFF, umi.UMI_INTRONS_EXON_FIRST, umi.UMI_INTRONS_ALL) == (im.OFF, im.EXON_FIRST, im.ALL)
    assert (umi.UMI_GENE_TIER_EXON, umi.UMI_GENE_TIER_INTRON) == (X, I)
    p = _lib.ptr
    reads = am.pack_reads([(0, 150, False, (("M", 10),))])
    rd = [p(reads[0], C.c_int32), p(reads[1], C.c_int32), p(reads[2], C.c_uint8), p(reads[3], C.c_uint32), p(reads[4], C.c_uint64)]
    gene, status, tier, counts = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(1, np.uint8), np.full(4, 7, np.uint64)
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(tier, C.c_uint8), p(counts, C.c_uint64)]
    ex = [np.array([0], np.int32), np.array([100], np.int32), np.array([200], np.int32), np.frombuffer(b"+", np.uint8), np.array([0], np.int32)]
    xs = [p(ex[0], C.c_int32), p(ex[1], C.c_int32), p(ex[2], C.c_int32), p(ex[3], C.c_uint8), p(ex[4], C.c_int32)]
    for introns, strand_mode, word in ((3, 0, "intron_mode 3"), (-1, 0, "intron_mode -1"), (1, 3, "strand_mode"), (1, 0, "ctx is NULL")):
        assert lib.umi_assign_genes_introns(None, *xs, 1, 1, strand_mode, introns, *rd, 1, *outs) == _lib.UMI_ERR_ARG
        assert word in lib.umi_last_error().decode()
    assert lib.umi_assign_genes_introns(None, *xs, 1, 1, 0, 1, *rd, 1, outs[0], outs[1], None, outs[3]) == _lib.UMI_ERR_ARG
    assert "NULL" in lib.umi_last_error().decode()
    assert list(counts) == [7, 7, 7, 7]


# ---- the program's refusals -----------------------------------------------------------------------------

GOOD = "chr1\tsrc\texon\t101\t200\t.\t+\t.\tgene_id \"G1\"; gene_name \"One\";"


def refused(tmp_path, flags, gtf_lines=None):
    """the program's message for a run that must end with status 101 before anything is read or written"""
    argv = [CLI, "-i", "in.bam", "-o", "out.bam"] + flags
    if gtf_lines is not None:
        am.write_gtf(tmp_path / "a.gtf", gtf_lines)
        argv += ["--gene-annotation", "a.gtf"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert sorted(os.listdir(tmp_path)) == (["a.gtf"] if gtf_lines is not None else [])
    return r.stderr


@pytest.mark.parametrize("value", ["exon-first", "all", "off"])
def test_program_refuses_the_flag_without_a_gene_annotation(tmp_path, value):
    assert "--gene-introns goes with --gene-annotation only" in refused(tmp_path, ["--per-gene", "--gene-introns", value])


@pytest.mark.parametrize("value", ["exon_first", "ExonOverIntron", "", "on"])
def test_program_refuses_an_unknown_value(tmp_path, value):
    assert "--gene-introns wants off, exon-first or all: '%s'" % value in refused(tmp_path, ["--per-gene", "--gene-introns", value], [GOOD])


@pytest.mark.parametrize("a,b", [("exon-first", "all"), ("off", "exon-first"), ("all", "off")])
def test_program_refuses_the_flag_given_twice_with_different_values(tmp_path, a, b):
    msg = refused(tmp_path, ["--per-gene", "--gene-introns", a, "--gene-introns", b], [GOOD])
    assert "--gene-introns given twice with different values: '%s' and '%s'" % (a, b) in msg


def test_what_the_annotation_flag_refuses_stays_refused(tmp_path):
    assert "--gene-annotation goes with --per-gene only" in refused(tmp_path, ["--gene-introns", "exon-first"], [GOOD])
    assert "--gene-annotation does not go with --dump-staging" in refused(
        tmp_path, ["--per-gene", "--gene-introns", "all", "--dump-staging", "x"], [GOOD])


def test_help_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert "--gene-introns <M>" in r.stdout + r.stderr and "exon-first" in r.stdout + r.stderr
