"""umicollapse --gene-annotation end to end, as an equivalence: a synthetic BAM with spliced reads and reads on both
strands (annotation_model.annotation_bam) gets its model-assigned genes written into GX ('a;b' for several, no tag for
none) and runs with --per-gene; the same records without GX run with --gene-annotation and a GTF.  The two runs give
the same records, matrix files, filtered files and summary, but for the lines the flag renames and adds."""
import os
import struct
import subprocess

import pytest

import annotation_model as am
import bamio
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
REFS = ["chrA", "chrB", "chrC"]
GENE_IDS = ["ENSG%05d" % (7 * g + 3) for g in range(40)]
# the summary lines that only one of the two runs has
OWN_LINES = ("Number of reads without a gene tag", "Number of reads outside every gene", "Gene annotation", "Gene strand",
             "Number of annotation lines on unknown references")
UNKNOWN = ["chrZ\tsynthetic\texon\t10\t90\t.\t+\t.\tgene_id \"ENSG00003\";", "chrZ\tsynthetic\texon\t10\t90\t.\t-\t.\tgene_id \"ZZ9\";"]
OTHER = ["chrA\tsynthetic\ttranscript\tnot\tlooked\tat\t?\t.\t", "chrA\tsynthetic\tCDS\t1\t9000\t.\t+\t.\tgene_id \"CDS1\";"]


def gene_bodies(exons):
    """a `gene` feature per (gene, reference, strand): from its first exon's start to its last one's end"""
    span = {}
    for ref, s, e, strand, g in exons:
        if strand == ".":
            continue
        lo, hi = span.get((g, ref, strand), (s, e))
        span[(g, ref, strand)] = (min(lo, s), max(hi, e))
    return [(ref, lo, hi, strand, g) for (g, ref, strand), (lo, hi) in sorted(span.items())]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("annotation")
    exons = list(am.fuzz_annotation())
    header, recs, cells = am.annotation_bam(41, exons, REFS)
    out = dict(dir=d, exons=exons, recs=recs, header=header, plain=str(d / "plain.bam"), whitelist=str(d / "whitelist.txt"))
    tag_model.write_bam(out["plain"], header, recs)
    for mode_name, mode in am.MODES.items():
        out[mode_name] = str(d / (mode_name + ".bam"))
        tag_model.write_bam(out[mode_name], header, am.with_gene_tags(recs, exons, GENE_IDS, mode))
    bodies = gene_bodies(exons)
    out["bodies"] = bodies
    out["by_gene_feature"] = str(d / "bodies.bam")
    tag_model.write_bam(out["by_gene_feature"], header, am.with_gene_tags(recs, bodies, GENE_IDS, am.FORWARD))
    lines = am.gtf_lines(exons, REFS, GENE_IDS) + UNKNOWN + OTHER
    out["gtf"] = am.write_gtf(d / "genes.gtf", lines)
    out["gtf_gz"] = am.write_gtf(d / "genes.gtf.gz", lines, gz=True)
    names = [None if g % 3 == 0 else "Name%d" % g for g in range(40)]
    out["names"] = names
    out["gtf_names"] = am.write_gtf(d / "named.gtf", am.gtf_lines(exons, REFS, GENE_IDS, gene_names=names))
    out["gtf_bodies"] = am.write_gtf(d / "bodies.gtf", am.gtf_lines(exons, REFS, GENE_IDS) +
                                     am.gtf_lines(bodies, REFS, GENE_IDS, feature="gene")[2:])
    with open(out["whitelist"], "w") as f:
        f.write("".join(c + "\n" for c in sorted(cells)))
    return out


def run_cli(tmp_path, src, flags):
    tmp_path.mkdir(exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-gene", "--count-matrix", mdir] + flags,
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


def check_pair(tmp_path, data, flags, mode="forward", gtf="gtf", tagged=None, extra=()):
    """the tag run on the model's GX against the annotation run on the records without GX"""
    t_bam, t_files, t_log = run_cli(tmp_path / "tag", data[tagged or mode], flags)
    a_flags = flags + ["--gene-annotation", data[gtf]] + ([] if mode == "forward" else ["--gene-strand", mode]) + list(extra)
    a_bam, a_files, a_log = run_cli(tmp_path / "annotation", data["plain"], a_flags)
    assert a_bam == without_gx(data, t_bam)
    assert sorted(a_files) == sorted(t_files) and len(t_files) >= 4
    for f in t_files:
        assert a_files[f] == t_files[f], f
    assert summary(a_log) == summary(t_log)
    assert [l.split(":")[0] for l in summary(t_log, own=True)] == [OWN_LINES[0]]
    assert [l.split(":")[0] for l in summary(a_log, own=True)] == list(OWN_LINES[1:])
    assert value(a_log, OWN_LINES[1]) == value(t_log, OWN_LINES[0])
    assert value(a_log, "Gene strand") == mode
    assert int(value(a_log, "Number of reads assigned to several genes")) > 20 and int(value(a_log, "Number of genes")) > 10
    return a_bam, a_files, a_log, t_bam


def test_plain_run_and_a_gene_tag_that_is_not_looked_at(tmp_path, data):
    a_bam, a_files, a_log, t_bam = check_pair(tmp_path, data, [])
    assert value(a_log, "Gene annotation") == "40 genes, %d features" % len(data["exons"])
    assert value(a_log, "Number of annotation lines on unknown references") == "2"
    assert len(bamio.split_records(a_bam)[1]) > 100
    # the records with GX in them, and with another mode's GX: the tag plays no part
    for src in ("forward", "reverse"):
        g_bam, g_files, g_log = run_cli(tmp_path / ("gx_" + src), data[src], ["--gene-annotation", data["gtf"]])
        assert g_files == a_files and summary(g_log) == summary(a_log)
        assert len(bamio.split_records(g_bam)[1]) == len(bamio.split_records(a_bam)[1])
        if src == "forward":
            assert g_bam == t_bam  # byte for byte the tag run's file


@pytest.mark.parametrize("mode", ["reverse", "unstranded"])
def test_strand_modes(tmp_path, data, mode):
    a_bam, a_files, _, _ = check_pair(tmp_path, data, [], mode=mode)
    f_bam, f_files, _ = run_cli(tmp_path / "forward", data["plain"], ["--gene-annotation", data["gtf"]])
    assert a_files["matrix.mtx"] != f_files["matrix.mtx"] and a_bam != f_bam  # (the model's tags differ as much)


def test_per_cell_with_a_cell_whitelist(tmp_path, data):
    _, files, log, _ = check_pair(tmp_path, data, ["--per-cell", "--cell-tag", "CR", "--cell-whitelist", data["whitelist"]])
    assert len(files["barcodes.tsv"].splitlines()) == 6 and int(value(log, "Number of reads with a corrected cell barcode")) > 0


def test_multi_gene_filter(tmp_path, data):
    check_pair(tmp_path, data, ["--per-cell", "--umi-filtering", "multi-gene"])


def test_cell_filter(tmp_path, data):
    _, files, _, _ = check_pair(tmp_path, data, ["--per-cell", "--cell-filter", "min-molecules", "--cell-min-molecules", "20"])
    assert {"filtered/features.tsv", "filtered/barcodes.tsv", "filtered/matrix.mtx", "filtered/reads.mtx", "cells.tsv"} <= set(files)


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_both_stagings(tmp_path, data, stage):
    check_pair(tmp_path, data, ["--per-cell", "--stage", stage])


def test_two_devices(tmp_path, data):
    check_pair(tmp_path, data, ["--per-cell", "--devices", "0,0"])  # (the assignment runs on the first)


def test_other_options_of_per_gene(tmp_path, data):
    check_pair(tmp_path, data, ["--per-cell", "-k", "2", "--distance", "edit", "--algo", "cluster", "--num-threads", "3"])


def test_gzip_annotation_gives_the_plain_one_s_output(tmp_path, data):
    p = run_cli(tmp_path / "plain", data["plain"], ["--per-cell", "--gene-annotation", data["gtf"]])
    z = run_cli(tmp_path / "gz", data["plain"], ["--per-cell", "--gene-annotation", data["gtf_gz"]])
    assert z[0] == p[0] and z[1] == p[1] and summary(z[2]) == summary(p[2]) and summary(z[2], own=True) == summary(p[2], own=True)


def test_gene_name_lands_in_the_second_column(tmp_path, data):
    flags = ["--per-cell", "--cell-filter", "min-molecules", "--cell-min-molecules", "20"]
    p = run_cli(tmp_path / "ids", data["plain"], flags + ["--gene-annotation", data["gtf"]])
    n = run_cli(tmp_path / "names", data["plain"], flags + ["--gene-annotation", data["gtf_names"]])
    name_of = dict(zip(GENE_IDS, data["names"]))
    seen = set()
    for f in ("features.tsv", "filtered/features.tsv"):
        rows = [l.split("\t") for l in n[1][f].decode().splitlines()]
        assert [r[0] for r in rows] == [l.split("\t")[0] for l in p[1][f].decode().splitlines()]
        for gid, name, kind in rows:
            assert name == (name_of[gid] or gid) and kind == "Gene Expression"
            seen.add(name_of[gid] is None)
        assert [l.split("\t")[1] for l in p[1][f].decode().splitlines()] == [r[0] for r in rows]
    assert seen == {True, False}
    assert n[0] == p[0] and all(n[1][f] == p[1][f] for f in p[1] if not f.endswith("features.tsv"))


def test_feature_gene_assigns_intronic_reads_that_exon_drops(tmp_path, data):
    recs = [bamio.parse_record(r) for r in data["recs"]]
    by_exon = [am.assign(data["exons"], r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], am.FORWARD)[0] for r in recs]
    by_body = [am.assign(data["bodies"], r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], am.FORWARD)[0] for r in recs]
    assert sum(1 for e, b in zip(by_exon, by_body) if e == am.NONE and b == am.ASSIGNED) > 30  # intronic reads
    _, _, g_log, _ = check_pair(tmp_path, data, [], gtf="gtf_bodies", tagged="by_gene_feature", extra=["--annotation-feature", "gene"])
    _, _, e_log = run_cli(tmp_path / "exon", data["plain"], ["--gene-annotation", data["gtf_bodies"]])
    assert int(value(g_log, OWN_LINES[1])) < int(value(e_log, OWN_LINES[1]))
    assert value(g_log, "Gene annotation") == "40 genes, %d features" % len(data["bodies"])
