"""umicollapse --gene-rule transcript --transcript-introns end to end.  As an equivalence: a BAM of a few hundred of the
fuzz reads (transcript_intron_model.cli_bam) gets the genes that tests/transcript_intron_model.py assigns written into GX
('a;b' for several, no tag for none) and runs with plain --per-gene; the same records without GX run with
--gene-annotation GTF --gene-rule transcript --transcript-introns M.  The two runs give the same records, matrix files and
molecule counts.  --velocity: DIR/velocity's five files and the summary's class and molecule lines against the model,
and a layer that the gene-level --gene-introns exon-first --velocity fills otherwise.  --transcript-introns off is the
run without the flag, byte for byte."""
import os
import struct
import subprocess

import pytest

import annotation_model as am
import bamio
import intron_model as im
import tag_model
import transcript_intron_model as ti
import transcript_model as tm
import velocity_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
LAYERS = ("spliced.mtx", "unspliced.mtx", "ambiguous.mtx")
FIVE = ("features.tsv", "barcodes.tsv") + LAYERS
READ_LINES = ("Number of exonic reads", "Number of junction reads", "Number of exon-intron reads", "Number of intronic reads")
MOLECULE_LINES = ("Number of spliced molecules", "Number of unspliced molecules", "Number of ambiguous molecules")
TIER_LINES = ("Transcript introns", "Number of reads assigned by a transcript", "Number of reads assigned by a gene body")
# the summary lines that only one of a pair's two runs has
OWN_LINES = ("Number of reads without a gene tag", "Number of reads outside every gene", "Gene annotation", "Gene strand",
             "Number of annotation lines on unknown references", "Gene rule", "Number of transcripts") + TIER_LINES


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("transcript_introns")
    header, recs, cells = ti.cli_bam()
    exons = list(ti.fuzz_annotation())
    out = dict(dir=d, recs=recs, exons=exons, plain=str(d / "plain.bam"), by_number={})
    tag_model.write_bam(out["plain"], header, recs)
    out["gtf"] = am.write_gtf(d / "genes.gtf", tm.gtf_lines(exons, ti.REF_NAMES, ti.GENE_IDS))
    for name in ("exon-first", "all"):
        out[name] = ti.expected_cli(recs, am.FORWARD, ti.INTRONS[name])
        out[name + ".bam"] = str(d / (name + ".bam"))
        tag_model.write_bam(out[name + ".bam"], header, out[name]["tagged"])
    number = lambda rec: struct.unpack("<i", tag_model.parse_aux(rec)["xx"][1])[0]
    out["number"], out["by_number"] = number, {number(rec): rec for rec in recs}
    return out


def run_cli(tmp_path, src, flags):
    tmp_path.mkdir(parents=True, exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-gene", "--per-cell", "--count-matrix", mdir] + flags,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = {}
    for base, _, names in os.walk(mdir):
        for name in names:
            path = os.path.join(base, name)
            files[os.path.relpath(path, mdir)] = open(path, "rb").read()
    return open(dst, "rb").read(), files, r.stderr


def rule_flags(data, introns):
    return ["--gene-annotation", data["gtf"], "--gene-rule", "transcript", "--transcript-introns", introns]


def summary(log, own=False, own_lines=OWN_LINES):
    lines = [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    return [l for l in lines if (l.split(":")[0] in own_lines) == own]


def value(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def without_gx(data, stream):
    """a tag run's output with every record put back to what it was before GX was appended"""
    header, recs = bamio.split_records(stream)
    plain = []
    for rec in recs:
        was = data["by_number"][data["number"](rec)]
        assert rec[4:len(was)] == was[4:] and rec[len(was):len(was) + 3] == b"GXZ"
        plain.append(was)
    return header + b"".join(plain)


def check_pair(tmp_path, data, introns, flags):
    """the tag run on the model's GX against the rule's run on the records without GX"""
    t_bam, t_files, t_log = run_cli(tmp_path / "tag", data[introns + ".bam"], flags)
    a_bam, a_files, a_log = run_cli(tmp_path / "rule", data["plain"], flags + rule_flags(data, introns))
    assert bamio.bgzf_decompress(a_bam) == without_gx(data, bamio.bgzf_decompress(t_bam))
    assert sorted(a_files) == sorted(t_files) and len(t_files) >= 4
    for f in t_files:
        assert a_files[f] == t_files[f], f
    assert summary(a_log) == summary(t_log)
    assert value(a_log, "Number of reads after deduplicating") == value(t_log, "Number of reads after deduplicating")
    assert [l.split(":")[0] for l in summary(t_log, own=True)] == [OWN_LINES[0]]
    assert [l.split(":")[0] for l in summary(a_log, own=True)] == list(OWN_LINES[1:])
    assert value(a_log, OWN_LINES[1]) == value(t_log, OWN_LINES[0])
    e = data[introns]
    assert value(a_log, "Transcript introns") == introns
    assert [int(value(a_log, l)) for l in TIER_LINES[1:]] == [int(c) for c in e["counts"][:2]] and min(e["counts"][:2]) > (50 if introns == "exon-first" else 0)
    assert int(value(a_log, "Number of reads after deduplicating")) == e["molecules"] or "--umi-filtering" in flags
    assert "Gene introns" not in a_log and "assigned by an exon" not in a_log
    return a_bam, a_files, a_log


@pytest.mark.parametrize("stage", ["gpu", "host"])
@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_against_the_model_s_tags(tmp_path, data, introns, stage):
    _, _, log = check_pair(tmp_path, data, introns, ["--stage", stage])
    assert "staging (%s)" % stage in log


def test_the_two_modes_differ(data):
    first, full = data["exon-first"], data["all"]
    assert sum(a[:2] != b[:2] for a, b in zip(first["verdicts"], full["verdicts"])) > 10  # (a fit the bodies overrule)
    assert first["files"]["spliced.mtx"] != full["files"]["spliced.mtx"]


def test_cell_filter_and_multi_gene_filter(tmp_path, data):
    _, files, log = check_pair(tmp_path, data, "exon-first", ["--cell-filter", "min-molecules", "--cell-min-molecules", "20",
                                                              "--umi-filtering", "multi-gene"])
    assert {"filtered/features.tsv", "filtered/barcodes.tsv", "filtered/matrix.mtx", "filtered/reads.mtx", "cells.tsv"} <= set(files)
    e = ti.expected_cli(data["recs"], am.FORWARD, ti.EXON_FIRST, multigene=True)
    assert int(value(log, "Number of reads after deduplicating")) == e["molecules"]
    assert int(value(log, "Number of molecules removed as multi-gene UMIs")) == data["exon-first"]["molecules"] - e["molecules"] > 10


def layer_pairs(files, prefix="velocity/"):
    total = {}
    for f in LAYERS:
        for l in files[prefix + f].decode().splitlines()[2:]:
            r, c, v = l.split()
            total[(r, c)] = total.get((r, c), 0) + int(v)
    return total


@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_velocity_against_the_model(tmp_path, data, introns):
    bam, files, log = run_cli(tmp_path / "with", data["plain"], rule_flags(data, introns) + ["--velocity"])
    plain_bam, plain_files, plain_log = run_cli(tmp_path / "without", data["plain"], rule_flags(data, introns) + ["--stage", "host"])
    e = data[introns]
    for f in ("features.tsv", "barcodes.tsv"):
        assert files["velocity/" + f] == files[f], f
    assert files["velocity/barcodes.tsv"] == e["files"]["barcodes.tsv"]
    assert [l.split(b"\t")[0] for l in files["features.tsv"].splitlines()] == [l.split(b"\t")[0] for l in e["files"]["features.tsv"].splitlines()]
    for f in LAYERS:
        assert files["velocity/" + f] == e["files"][f], f
    own = ("Velocity",) + READ_LINES + MOLECULE_LINES
    assert [l.split(":")[0] for l in summary(log, True, own)] == list(own) and value(log, "Velocity") == "on"
    assert [int(value(log, l)) for l in READ_LINES] == [int(c) for c in e["class_counts"][1:]]
    assert [int(value(log, l)) for l in MOLECULE_LINES] == e["layers"]
    assert sum(e["layers"]) == e["molecules"] == int(value(log, "Number of reads after deduplicating"))
    assert min(e["class_counts"]) > (20 if introns == "exon-first" else 5) and min(e["layers"]) > (20 if introns == "exon-first" else 0)
    # the three layers add up to matrix.mtx, pair by pair
    assert layer_pairs(files) == {tuple(l.split()[:2]): int(l.split()[2]) for l in files["matrix.mtx"].decode().splitlines()[2:]}
    # everything else is the run without --velocity
    assert "staging (host)" in log and bam == plain_bam
    rest = {f: b for f, b in files.items() if not f.startswith("velocity")}
    assert rest == plain_files
    assert summary(log, False, own) == summary(plain_log, False, own) and summary(plain_log, True, own) == []
    assert sorted(f for f in files if f.startswith("velocity/")) == sorted("velocity/" + f for f in FIVE)


def test_the_gene_level_velocity_fills_a_layer_otherwise(tmp_path, data):
    """the hand table's read 3 in the fuzz: a record that fits a spliced isoform over an intron another isoform retains is
    a junction read here and exonic under --gene-introns exon-first --velocity, with the same gene"""
    lines = tm.overlap_exons(data["exons"])
    some = []
    for rec, v in zip(data["recs"], data["exon-first"]["verdicts"]):
        r = bamio.parse_record(rec)
        if v[4] and v[0] == ti.ASSIGNED and v[3] == ti.JUNCTION:
            theirs = vm.classify(lines, r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], am.FORWARD, im.EXON_FIRST)
            some.append(theirs[:2] == (im.ASSIGNED, v[1]) and theirs[3] == vm.EXONIC)
    assert sum(some) >= 1  # (a condition on the input)
    _, files, _ = run_cli(tmp_path / "transcript", data["plain"], rule_flags(data, "exon-first") + ["--velocity"])
    _, theirs, _ = run_cli(tmp_path / "gene", data["plain"], ["--gene-annotation", data["gtf"], "--gene-introns", "exon-first", "--velocity"])
    # (the two runs' matrices name other genes: a pair is a gene's id and a cell's barcode)
    def named(fs, f):
        genes = [l.split(b"\t")[0] for l in fs["features.tsv"].splitlines()]
        cells = fs["barcodes.tsv"].splitlines()
        return {(genes[int(l.split()[0]) - 1], cells[int(l.split()[1]) - 1]): int(l.split()[2]) for l in fs[f].decode().splitlines()[2:]}
    pairs = set(named(files, "matrix.mtx")) & set(named(theirs, "matrix.mtx"))
    assert len(pairs) > 20
    assert any(named(files, "velocity/" + f).get(p, 0) != named(theirs, "velocity/" + f).get(p, 0) for f in LAYERS for p in pairs)


def test_off_and_no_flag_give_identical_bytes(tmp_path, data):
    flags = ["--gene-annotation", data["gtf"], "--gene-rule", "transcript"]
    none = run_cli(tmp_path / "none", data["plain"], flags)
    off = run_cli(tmp_path / "off", data["plain"], flags + ["--transcript-introns", "off"])
    assert off[0] == none[0] and off[1] == none[1]  # the BAM file's bytes and every matrix file's
    timing = lambda log: [l for l in log.splitlines() if "seconds" in l or l.startswith("phases:")]
    rest = lambda log: [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    assert rest(off[2]) == rest(none[2]) and len(timing(off[2])) == len(timing(none[2]))
    assert "Transcript introns" not in none[2] and "assigned by a" not in none[2]
