"""umicollapse --gene-introns end to end, by the equivalence tests/test_gpu_gene_annotation_cli.py uses: a synthetic
BAM gets the model's verdicts under exon-first or all (tests/intron_model.py) written into GX and runs with --per-gene;
the same records without GX run with --gene-annotation, a GTF of exon lines alone, and the flag.  The two runs give the
same records and matrix files, and the same summary but for the lines the flags rename and add."""
import os
import struct
import subprocess

import pytest

import annotation_model as am
import bamio
import intron_model as im
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
REFS = ["chrA", "chrB", "chrC"]
GENE_IDS = ["ENSG%05d" % (7 * g + 3) for g in range(40)]
# the summary lines that only one of the two runs has: the tag run's, the annotation's, the new flag's
TAG_LINES = ("Number of reads without a gene tag",)
ANNOTATION_LINES = ("Number of reads outside every gene", "Gene annotation", "Gene strand", "Number of annotation lines on unknown references")
INTRON_LINES = ("Gene introns", "Number of reads assigned by an exon", "Number of reads assigned by an intron")
OWN_LINES = TAG_LINES + ANNOTATION_LINES + INTRON_LINES
CASES = [("forward", "exon-first"), ("forward", "all"), ("unstranded", "exon-first"), ("reverse", "all")]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("introns")
    exons = list(am.fuzz_annotation())
    header, recs, cells = am.annotation_bam(43, exons, REFS)
    out = dict(dir=d, exons=exons, recs=recs, header=header, plain=str(d / "plain.bam"), tiers={})
    tag_model.write_bam(out["plain"], header, recs)
    for mode, introns in CASES:
        tagged, tiers = im.with_gene_tags(recs, exons, GENE_IDS, am.MODES[mode], im.INTRONS[introns])
        out[(mode, introns)] = str(d / ("%s_%s.bam" % (mode, introns)))
        out["tiers"][(mode, introns)] = tiers
        tag_model.write_bam(out[(mode, introns)], header, tagged)
    lines = am.gtf_lines(exons, REFS, GENE_IDS)
    assert all(l.split("\t")[2] == "exon" for l in lines if "\t" in l)  # no gene line, no transcript line
    out["gtf"] = am.write_gtf(d / "genes.gtf", lines)
    return out


def run_cli(tmp_path, src, flags):
    tmp_path.mkdir(exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-gene", "--per-cell", "--count-matrix", mdir] + flags,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = {}
    for base, _, names in os.walk(mdir):
        for name in names:
            path = os.path.join(base, name)
            files[os.path.relpath(path, mdir)] = open(path, "rb").read()
    return bamio.bgzf_decompress(open(dst, "rb").read()), files, r.stderr


def summary(log, own=False):
    """the summary without its timings (own: the lines that only one of the two runs has, else all the others)"""
    lines = [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    return [l for l in lines if (l.split(":")[0] in OWN_LINES) == own]


def value(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def without_gx(data, stream):
    """a tag run's output with every record put back to what it was before GX was appended"""
    header, recs = bamio.split_records(stream)
    number = lambda rec: struct.unpack("<i", tag_model.parse_aux(rec)["xx"][1])[0]  # (annotation_bam numbers its records there)
    if "by_number" not in data:
        data["by_number"] = {number(rec): rec for rec in data["recs"]}
    plain = []
    for rec in recs:
        was = data["by_number"][number(rec)]
        assert rec[4:len(was)] == was[4:] and rec[len(was):len(was) + 3] == b"GXZ"
        plain.append(was)
    return header + b"".join(plain)


def check_pair(tmp_path, data, mode, introns, flags):
    """the tag run on the model's GX against the annotation run with the flag on the records without GX"""
    t_bam, t_files, t_log = run_cli(tmp_path / "tag", data[(mode, introns)], flags)
    a_flags = flags + ["--gene-annotation", data["gtf"], "--gene-strand", mode, "--gene-introns", introns]
    a_bam, a_files, a_log = run_cli(tmp_path / "annotation", data["plain"], a_flags)
    assert a_bam == without_gx(data, t_bam)
    assert sorted(a_files) == sorted(t_files) and len(t_files) >= 4
    for f in t_files:
        assert a_files[f] == t_files[f], f
    assert summary(a_log) == summary(t_log)
    assert [l.split(":")[0] for l in summary(t_log, own=True)] == list(TAG_LINES)
    assert [l.split(":")[0] for l in summary(a_log, own=True)] == list(ANNOTATION_LINES + INTRON_LINES)
    assert value(a_log, ANNOTATION_LINES[0]) == value(t_log, TAG_LINES[0])
    assert value(a_log, "Gene introns") == introns
    # the two counts: over every mapped record, as the model has them, and together the assigned ones
    tiers = [(st, tier) for st, tier, unmapped in data["tiers"][(mode, introns)] if not unmapped]
    by_exon = sum(1 for st, tier in tiers if st == im.ASSIGNED and tier == im.TIER_EXON)
    by_intron = sum(1 for st, tier in tiers if st == im.ASSIGNED and tier == im.TIER_INTRON)
    assert int(value(a_log, INTRON_LINES[1])) == by_exon and int(value(a_log, INTRON_LINES[2])) == by_intron
    assert by_exon + by_intron == sum(1 for st, _ in tiers if st == im.ASSIGNED) and by_exon > 50 and by_intron > 20
    assert len(bamio.split_records(a_bam)[1]) > 100
    return a_bam, a_files, a_log


@pytest.mark.parametrize("mode,introns", CASES)
def test_per_cell_count_matrix(tmp_path, data, mode, introns):
    check_pair(tmp_path, data, mode, introns, [])


def test_the_modes_differ_and_introns_add_reads(tmp_path, data):
    runs = {i: run_cli(tmp_path / i, data["plain"], ["--gene-annotation", data["gtf"], "--gene-introns", i]) for i in ("off", "exon-first", "all")}
    assert len({r[1]["matrix.mtx"] for r in runs.values()}) == 3
    outside = {i: int(value(r[2], ANNOTATION_LINES[0])) for i, r in runs.items()}
    assert outside["exon-first"] == outside["all"] < outside["off"]  # (none: no body under either rule)
    several = {i: int(value(r[2], "Number of reads assigned to several genes")) for i, r in runs.items()}
    assert several["all"] > several["exon-first"] > several["off"]


def test_with_cell_filter_and_multi_gene_filter(tmp_path, data):
    _, files, _ = check_pair(tmp_path, data, "forward", "exon-first",
                             ["--cell-filter", "min-molecules", "--cell-min-molecules", "20", "--umi-filtering", "multi-gene"])
    assert {"filtered/features.tsv", "filtered/barcodes.tsv", "filtered/matrix.mtx", "filtered/reads.mtx", "cells.tsv"} <= set(files)


def test_off_is_the_run_without_the_flag(tmp_path, data):
    flags = ["--gene-annotation", data["gtf"]]
    plain = run_cli(tmp_path / "plain", data["plain"], flags)
    off = run_cli(tmp_path / "off", data["plain"], flags + ["--gene-introns", "off"])
    assert off[0] == plain[0] and off[1] == plain[1]
    assert summary(off[2]) == summary(plain[2]) and summary(off[2], own=True) == summary(plain[2], own=True)
    assert not any(l.split(":")[0] in INTRON_LINES for l in off[2].splitlines())
    twice = run_cli(tmp_path / "twice", data["plain"], flags + ["--gene-introns", "all", "--gene-introns", "all"])
    assert value(twice[2], "Gene introns") == "all"
