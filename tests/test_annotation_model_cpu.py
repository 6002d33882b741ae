"""umi_assign_genes / --gene-annotation, the parts that need no GPU: the model of tests/annotation_model.py on
hand-written cases, what the inputs of the GPU tests hold, the library's refusals that come before a device is looked
at, and the program's refusals, each with status 101 and its message."""
import ctypes as C
import gzip
import os
import subprocess

import numpy as np
import pytest

import annotation_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


# ---- the model ------------------------------------------------------------------------------------------

def test_blocks_of_a_read():
    assert am.blocks(100, [("M", 50)]) == [(100, 150)]
    assert am.blocks(100, [("S", 5), ("M", 10), ("I", 3), ("M", 10), ("D", 2), ("=", 4), ("X", 1)]) == [(100, 127)]
    assert am.blocks(100, [("M", 10), ("N", 100), ("M", 5), ("N", 7), ("M", 1)]) == [(100, 110), (210, 215), (222, 223)]
    assert am.blocks(100, [("H", 3), ("S", 4), ("I", 2), ("P", 1)]) == []
    assert am.blocks(100, []) == [] and am.blocks(100, [("N", 10)]) == [] and am.blocks(100, [("M", 0)]) == []
    assert am.blocks(100, [("N", 10), ("M", 2)]) == [(110, 112)]


def test_hits_and_strands():
    ex = [(0, 100, 200, "+", 0), (0, 300, 400, "-", 1), (0, 500, 600, ".", 2), (1, 100, 200, "+", 3)]
    m = [("M", 10)]
    for mode, want in ((am.FORWARD, [0, -1, -1, 1, 2, 2]), (am.REVERSE, [-1, 0, 1, -1, 2, 2]), (am.UNSTRANDED, [0, 0, 1, 1, 2, 2])):
        got = [am.assign(ex, 0, p, rev, m, mode)[1] for p in (150, 350, 550) for rev in (False, True)]
        assert got == want, mode
    assert am.assign(ex, 1, 150, False, m, am.FORWARD) == (am.ASSIGNED, 3)
    assert am.assign(ex, 2, 150, False, m, am.FORWARD) == (am.NONE, -1)
    # half-open on both sides
    assert am.assign(ex, 0, 90, False, m, am.FORWARD) == (am.NONE, -1)
    assert am.assign(ex, 0, 91, False, m, am.FORWARD) == (am.ASSIGNED, 0)
    assert am.assign(ex, 0, 200, False, m, am.FORWARD) == (am.NONE, -1)
    assert am.assign(ex, 0, 199, False, m, am.FORWARD) == (am.ASSIGNED, 0)


def test_one_gene_twice_is_one_gene_and_two_genes_are_several():
    ex = [(0, 100, 200, "+", 0), (0, 150, 260, "+", 0), (0, 600, 700, "+", 0), (0, 350, 450, "+", 1), (0, 620, 640, "+", 2)]
    assert am.assign(ex, 0, 140, False, [("M", 30)], am.FORWARD) == (am.ASSIGNED, 0)
    assert am.assign(ex, 0, 380, False, [("M", 20)], am.FORWARD) == (am.ASSIGNED, 1)      # inside gene 0's intron
    assert am.assign(ex, 0, 625, False, [("M", 10)], am.FORWARD) == (am.SEVERAL, -1)      # inside gene 0's exon
    assert am.assign(ex, 0, 180, False, [("M", 20), ("N", 400), ("M", 15)], am.FORWARD) == (am.ASSIGNED, 0)
    assert am.assign(ex, 0, 180, False, [("M", 20), ("D", 400), ("M", 15)], am.FORWARD) == (am.SEVERAL, -1)
    assert am.assign(ex, 0, 430, False, [("M", 20), ("N", 150), ("M", 30)], am.FORWARD) == (am.SEVERAL, -1)


def test_the_two_forms_of_the_model_agree():
    ex, reads = am.fuzz_annotation(), am.fuzz_reads()[:400]
    for mode in (am.FORWARD, am.REVERSE, am.UNSTRANDED):
        got = am.assign_all(ex, reads, mode)
        for i, (ref, pos, rev, cigar) in enumerate(reads):
            assert am.assign(ex, ref, pos, rev, cigar, mode) == (got["status"][i], got["gene"][i])
        assert int(got["counts"].sum()) == len(reads)


# ---- what the GPU tests' inputs hold --------------------------------------------------------------------

def test_fuzz_inputs_hold_what_the_gpu_tests_need():
    ex, reads = am.fuzz_annotation(), am.fuzz_reads()
    assert len(reads) == 5000 and am.n_genes_of(ex) == 40 and 250 <= len(ex) <= 400
    assert {e[0] for e in ex} == {0, 1, 2} and {e[3] for e in ex} == {"+", "-", "."}
    assert sum(1 for e in ex if e[3] == ".") >= 10
    assert len(set(ex)) < len(ex)  # a repeated exon line
    assert {op for *_, c in reads for op, _ in c} == set(am.OPS)  # all nine operations
    assert sum(any(op == "N" for op, _ in c) for *_, c in reads) >= 0.10 * len(reads)
    assert 0.3 * len(reads) <= sum(1 for r in reads if r[2]) <= 0.5 * len(reads)
    for mode in (am.FORWARD, am.REVERSE, am.UNSTRANDED):
        counts = am.fuzz_expected(mode)["counts"]
        assert (counts >= 0.15 * len(reads)).all(), (mode, counts)
    # genes overlap on both strands: a read's verdict depends on the mode
    f, r, u = (am.fuzz_expected(m)["status"] for m in (am.FORWARD, am.REVERSE, am.UNSTRANDED))
    assert (f != r).mean() > 0.2 and (f != u).mean() > 0.2


@pytest.mark.parametrize("n", [1, am.GENE_TOP_CAP, am.GENE_TOP_CAP + 1, 2 * am.GENE_TOP_CAP + 1])
def test_comb_inputs_reach_both_ends_of_the_table(n):
    ex, reads = am.comb_annotation(n), am.comb_reads(n)
    assert len(ex) == n and len({(e[1], e[2]) for e in ex}) == n
    got = am.assign_all(ex, reads, am.FORWARD)
    hit = set(got["gene"][got["status"] == am.ASSIGNED].tolist())
    assert got["counts"][am.NONE] > 100 and len(hit) == min(n, 50)  # (a spliced read may reach two exons: several)
    firsts = {r[1] // 10 for r, s in zip(reads, got["status"]) if s == am.ASSIGNED and len(r[3]) == 1 and not r[2]}
    assert {0, n - 1} <= firsts


def test_the_sizes_the_gpu_tests_are_placed_by_are_the_library_s():
    import re
    text = open(os.path.join(ROOT, "umi_collapse_rs_amd", "csrc", "umihip_internal.h")).read()
    for name in ("GENE_THREADS", "GENE_BLOCKS_PER_CU", "GENE_TOP_CAP"):
        assert int(re.search(r"constexpr \w+ %s = (\d+);" % name, text).group(1)) == getattr(am, name), name


def test_gtf_lines_round_trip(tmp_path):
    ex = [(0, 0, 10, "+", 0), (1, 99, 200, "-", 1), (0, 5, 6, ".", 0)]
    lines = am.gtf_lines(ex, ["chrA", "chrB"], ["G0", "G1"], gene_names=["Alpha", None])
    assert lines[0].startswith("#") and lines[1] == ""
    assert lines[2].split("\t")[:8] == ["chrA", "synthetic", "exon", "1", "10", ".", "+", "."]
    assert 'gene_id "G0";' in lines[2] and 'gene_name "Alpha";' in lines[2] and "gene_name" not in lines[3]
    assert lines[3].split("\t")[3:5] == ["100", "200"]
    p = am.write_gtf(tmp_path / "a.gtf.gz", lines, gz=True)
    assert gzip.open(p, "rb").read().decode().splitlines() == lines


# ---- the library, before a device is looked at ----------------------------------------------------------

def test_library_refuses_bad_arguments_without_a_context():
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    lib = umi.load()
    for name in ("umi_assign_genes", "umi_assign_genes_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert (umi.UMI_GENE_ASSIGNED, umi.UMI_GENE_NONE, umi.UMI_GENE_SEVERAL) == (am.ASSIGNED, am.NONE, am.SEVERAL)
    assert (umi.UMI_STRAND_FORWARD, umi.UMI_STRAND_REVERSE, umi.UMI_STRAND_UNSTRANDED) == (am.FORWARD, am.REVERSE, am.UNSTRANDED)
    p = _lib.ptr
    reads = am.pack_reads([(0, 150, False, (("M", 10),))])
    rd = [p(reads[0], C.c_int32), p(reads[1], C.c_int32), p(reads[2], C.c_uint8), p(reads[3], C.c_uint32), p(reads[4], C.c_uint64)]
    gene, status, counts = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(3, np.uint64)
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(counts, C.c_uint64)]

    def call(ex, n_genes, mode):
        a = [np.array([e[0] for e in ex], np.int32), np.array([e[1] for e in ex], np.int32), np.array([e[2] for e in ex], np.int32),
             np.frombuffer("".join(e[3] for e in ex).encode(), np.uint8), np.array([e[4] for e in ex], np.int32)]
        rc = lib.umi_assign_genes(None, p(a[0], C.c_int32), p(a[1], C.c_int32), p(a[2], C.c_int32), p(a[3], C.c_uint8),
                                  p(a[4], C.c_int32), len(ex), n_genes, mode, *rd, 1, *outs)
        return rc, lib.umi_last_error().decode()

    ok = (0, 100, 200, "+", 0)
    for ex, n_genes, mode, word in (([(0, 5, 5, "+", 0)], 1, 0, "interval"), ([(0, 5, 4, "+", 0)], 1, 0, "interval"),
                                    ([(0, -1, 4, "+", 0)], 1, 0, "interval"), ([ok, (0, 1, 2, "-", 1)], 1, 0, "gene 1"),
                                    ([(0, 1, 2, "x", 0)], 1, 0, "strand"), ([ok], 1, 3, "strand_mode"), ([ok], 1, 0, "ctx is NULL")):
        rc, msg = call(ex, n_genes, mode)
        assert rc == _lib.UMI_ERR_ARG and word in msg, (ex, msg)


# ---- the program's refusals -----------------------------------------------------------------------------

GOOD = "chr1\tsrc\texon\t101\t200\t.\t+\t.\tgene_id \"G1\"; gene_name \"One\";"


def refused(tmp_path, flags, gtf_lines=None, gz=False):
    """the program's message for a run that must end with status 101 before anything is read or written"""
    argv = [CLI, "-i", "in.bam", "-o", "out.bam"] + flags
    if gtf_lines is not None:
        am.write_gtf(tmp_path / "a.gtf", gtf_lines, gz=gz)
        argv += ["--gene-annotation", "a.gtf"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert sorted(os.listdir(tmp_path)) == (["a.gtf"] if gtf_lines is not None else [])
    return r.stderr


def line(**kw):
    cols = GOOD.split("\t")
    for k, v in kw.items():
        cols[int(k[1:])] = v
    return "\t".join(cols)


def test_program_refuses_the_flag_without_per_gene_and_with_a_gene_tag(tmp_path):
    assert "--gene-annotation goes with --per-gene only" in refused(tmp_path, [], [GOOD])
    assert "--gene-annotation does not go with --gene-tag" in refused(tmp_path, ["--per-gene", "--gene-tag", "GX"], [GOOD])
    assert "--gene-annotation does not go with --dump-staging" in refused(tmp_path, ["--per-gene", "--dump-staging", "x"], [GOOD])


@pytest.mark.parametrize("flag,value", [("--annotation-feature", "gene"), ("--annotation-attribute", "gene_name"),
                                        ("--gene-strand", "reverse")])
def test_program_refuses_a_companion_flag_alone(tmp_path, flag, value):
    assert flag + " goes with --gene-annotation only" in refused(tmp_path, ["--per-gene", flag, value])


def test_program_refuses_an_unknown_strand_mode(tmp_path):
    assert "--gene-strand wants forward, reverse or unstranded: 'both'" in refused(tmp_path, ["--per-gene", "--gene-strand", "both"], [GOOD])


@pytest.mark.parametrize("flag,a,b", [("--gene-annotation", "a.gtf", "b.gtf"), ("--annotation-feature", "exon", "gene"),
                                      ("--annotation-attribute", "gene_id", "gene_name"), ("--gene-strand", "forward", "reverse")])
def test_program_refuses_a_flag_given_twice_with_different_values(tmp_path, flag, a, b):
    msg = refused(tmp_path, ["--per-gene", flag, a, flag, b])
    assert flag + " given twice with different values: '%s' and '%s'" % (a, b) in msg


@pytest.mark.parametrize("bad,word", [
    ("chr1\tsrc\texon\t101\t200\t.\t+\t.", "fewer than nine tab-separated columns"),
    ("chr1 src exon 101 200 . + . gene_id \"G1\";", "fewer than nine tab-separated columns"),
    (line(c3="x1"), "the start 'x1' is not a number"), (line(c3=""), "the start '' is not a number"),
    (line(c4="2e2"), "the end '2e2' is not a number"), (line(c3="-5"), "the start '-5' is not a number"),
    (line(c3="0"), "a start below 1"), (line(c3="201"), "the end 200 lies before the start 201"),
    (line(c4="2147483648"), "lies beyond 2^31 - 1"),
    (line(c6="*"), "the strand '*' is none of + - ."), (line(c6=""), "the strand '' is none of + - ."),
    (line(c8="transcript_id \"T1\";"), "no attribute gene_id"), (line(c8="gene_id \"\";"), "the attribute gene_id is empty"),
    (line(c8="gene_id \"a b\";"), "cannot: 32"), (line(c8="gene_id \"a;b\";"), "cannot: 59"),
    (line(c8="gene_id \"a,b\";"), "cannot: 44"), (line(c8="gene_id \"a\x7fb\";"), "cannot: 127"),
])
def test_program_refuses_a_bad_line(tmp_path, bad, word):
    msg = refused(tmp_path, ["--per-gene"], ["# header", GOOD, "", bad])
    assert word in msg and "a.gtf, line 4" in msg


def test_program_looks_at_taken_lines_only_and_wants_one(tmp_path):
    other = line(c2="CDS", c3="zz", c6="?", c8="")
    assert "holds no line of feature type exon" in refused(tmp_path, ["--per-gene"], ["# only a comment", "", other])
    assert "holds no line of feature type gene" in refused(tmp_path, ["--per-gene", "--annotation-feature", "gene"], [GOOD])
    assert "no attribute gene_biotype" in refused(tmp_path, ["--per-gene", "--annotation-attribute", "gene_biotype"], [GOOD])
    # a good file passes the flags' checks: what ends the run then is the input that is not there
    msg = refused(tmp_path, ["--per-gene"], [other, GOOD])
    assert "in.bam" in msg and "annotation" not in msg
    msg = refused(tmp_path, ["--per-gene"], [other, GOOD], gz=True)
    assert "in.bam" in msg and "annotation" not in msg


def test_program_refuses_a_file_that_cannot_be_read(tmp_path):
    r = subprocess.run([CLI, "-i", "in.bam", "-o", "out.bam", "--per-gene", "--gene-annotation", "none.gtf"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "cannot read the gene annotation none.gtf" in r.stderr and not os.listdir(tmp_path)
    (tmp_path / "bad.gz").write_bytes(b"\x1f\x8b\x08\x00garbage that is no deflate stream")
    r = subprocess.run([CLI, "-i", "in.bam", "-o", "out.bam", "--per-gene", "--gene-annotation", "bad.gz"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "cannot read the gene annotation bad.gz" in r.stderr


def test_what_per_gene_refuses_stays_refused(tmp_path):
    assert "--per-gene does not go with --paired" in refused(tmp_path, ["--per-gene", "--paired"], [GOOD])
    assert "--per-gene does not go with --two-pass" in refused(tmp_path, ["--per-gene", "--two-pass"], [GOOD])


def test_help_names_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--gene-annotation", "--annotation-feature", "--annotation-attribute", "--gene-strand"):
        assert flag in r.stdout
