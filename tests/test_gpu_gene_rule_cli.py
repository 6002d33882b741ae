"""umicollapse --gene-rule end to end, as an equivalence: a synthetic BAM (annotation_model.annotation_bam, a third of its
reads laid along a transcript of the annotation so that spliced reads fit) gets the genes that tests/
transcript_model.py assigns written into GX ('a;b' for several, no tag for none) and runs with plain --per-gene; the
same records without GX run with --gene-annotation GTF --gene-rule transcript.  The two runs give the same records,
matrix files, filtered files and summary, but for the lines the flags rename and add.  --gene-rule overlap is the run
without the flag, byte for byte."""
import os
import struct
import subprocess

import numpy as np
import pytest

import annotation_model as am
import bamio
import tag_model
import transcript_model as tm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
REFS = ["chrA", "chrB", "chrC"]
GENE_IDS = ["ENSG%05d" % (7 * g + 3) for g in range(tm.N_GENES)]
# the summary lines that only one of the two runs has
OWN_LINES = ("Number of reads without a gene tag", "Number of reads outside every gene", "Gene annotation", "Gene strand",
             "Number of annotation lines on unknown references", "Gene rule", "Number of transcripts")
UNKNOWN = ['chrZ\tsynthetic\texon\t10\t90\t.\t+\t.\tgene_id "ENSG00003"; transcript_id "TZ";']
OTHER = ["chrA\tsynthetic\ttranscript\tnot\tlooked\tat\t?\t.\t", 'chrA\tsynthetic\tCDS\t1\t9000\t.\t+\t.\tgene_id "CDS1";']


def aux_of(rec):
    """the record's aux bytes"""
    l_rn, n_cig, l_seq = rec[4 + 8], struct.unpack_from("<H", rec, 4 + 12)[0], struct.unpack_from("<i", rec, 4 + 16)[0]
    return rec[4 + 32 + l_rn + 4 * n_cig + (l_seq + 1) // 2 + l_seq:]


def along_transcripts(recs, exons, seed=3):
    """every third mapped record laid along a transcript (transcript_model.read_from_transcript), mostly on its strand;
    its name, tags and number stay; the records in coordinate order again"""
    rng = np.random.default_rng(seed)
    trs = tm.transcripts_of(exons)
    ids = sorted(trs)
    out = []
    for i, rec in enumerate(recs):
        r = bamio.parse_record(rec)
        if i % 3 == 0 and not r["flag"] & 0x4:
            ref, strand, _, xs = trs[ids[int(rng.integers(0, len(ids)))]]
            total = sum(e - s for s, e in xs)
            length = min(total, int(rng.integers(25, 300 if rng.random() < 0.4 else 100)))
            pos, cigar = tm.read_from_transcript(rng, xs, int(rng.integers(0, total - length + 1)), length)
            rev = (strand == "-") != (rng.random() < 0.2)
            seq_len = sum(n for op, n in cigar if op in "MIS=X")
            quals = rng.integers(20, 41, seq_len).astype(np.uint8).tobytes()
            rec = bamio.make_record(r["qname"] if isinstance(r["qname"], str) else r["qname"].decode(), (r["flag"] & ~0x10) | (0x10 if rev else 0),
                                    ref, pos, r["mapq"], cigar, seq_len, quals, tags=aux_of(rec))
            r = bamio.parse_record(rec)
        out.append((r["tid"] if r["tid"] >= 0 else 1 << 30, r["pos"], i, rec))
    out.sort(key=lambda t: t[:3])
    return [t[3] for t in out]


def reads_of(recs):
    """(ref, pos, reverse, cigar) of the mapped records, as the program's one call sees them"""
    rs = [bamio.parse_record(r) for r in recs]
    return [(r["tid"], r["pos"], bool(r["flag"] & 0x10), tuple(r["cigar"])) for r in rs if not r["flag"] & 0x4 and r["tid"] >= 0]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("gene_rule")
    exons = list(tm.fuzz_annotation())
    header, recs, cells = am.annotation_bam(41, exons, REFS, n_reads=3000)
    recs = along_transcripts(recs, exons)
    out = dict(dir=d, exons=exons, recs=recs, header=header, plain=str(d / "plain.bam"))
    tag_model.write_bam(out["plain"], header, recs)
    for mode_name in ("forward", "unstranded"):
        out[mode_name] = str(d / (mode_name + ".bam"))
        tag_model.write_bam(out[mode_name], header, tm.with_gene_tags(recs, exons, GENE_IDS, tm.MODES[mode_name]))
    out["gtf"] = am.write_gtf(d / "genes.gtf", tm.gtf_lines(exons, REFS, GENE_IDS) + UNKNOWN + OTHER)
    out["gtf_tx"] = am.write_gtf(d / "tx.gtf", tm.gtf_lines(exons, REFS, GENE_IDS, attribute="tx"))
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
    return open(dst, "rb").read(), files, r.stderr


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


def check_pair(tmp_path, data, flags, mode="forward", gtf="gtf", extra=()):
    """the tag run on the model's GX against the transcript-rule run on the records without GX"""
    t_bam, t_files, t_log = run_cli(tmp_path / "tag", data[mode], flags)
    a_flags = flags + ["--gene-annotation", data[gtf], "--gene-rule", "transcript"] + ([] if mode == "forward" else ["--gene-strand", mode]) + list(extra)
    a_bam, a_files, a_log = run_cli(tmp_path / "rule", data["plain"], a_flags)
    assert bamio.bgzf_decompress(a_bam) == without_gx(data, bamio.bgzf_decompress(t_bam))
    assert sorted(a_files) == sorted(t_files) and len(t_files) >= 4
    for f in t_files:
        assert a_files[f] == t_files[f], f
    assert summary(a_log) == summary(t_log)
    assert [l.split(":")[0] for l in summary(t_log, own=True)] == [OWN_LINES[0]]
    assert [l.split(":")[0] for l in summary(a_log, own=True)] == list(OWN_LINES[1:])
    assert value(a_log, OWN_LINES[1]) == value(t_log, OWN_LINES[0])
    assert value(a_log, "Gene strand") == mode and value(a_log, "Gene rule") == "transcript"
    return a_bam, a_files, a_log


def test_transcript_rule_against_the_model_s_tags(tmp_path, data):
    a_bam, a_files, a_log = check_pair(tmp_path, data, [])
    exons = data["exons"]
    assert value(a_log, "Gene annotation") == "%d genes, %d features" % (tm.N_GENES, len(exons))
    assert value(a_log, "Number of annotation lines on unknown references") == "1"
    assert value(a_log, "Number of transcripts") == str(len(tm.transcripts_of(exons)))
    # the model's numbers: the reads of each verdict, and spliced reads among the assigned
    reads = reads_of(data["recs"])
    exp = tm.assign_all(exons, reads, tm.FORWARD)
    # (the summary counts the reads that carry their UMI and cell tags; the tag run's equal line has been compared)
    assert 100 < int(value(a_log, "Number of reads assigned to several genes")) <= int(exp["counts"][tm.SEVERAL])
    assert int(exp["counts"][tm.ASSIGNED]) > 400
    assert sum(1 for r, s in zip(reads, exp["status"]) if s == tm.ASSIGNED and any(op == "N" for op, _ in r[3])) > 100
    over = am.assign_all(tm.overlap_exons(exons), reads, tm.FORWARD)
    assert ((exp["status"] == tm.ASSIGNED) & (over["status"] == tm.SEVERAL)).sum() > 20
    assert ((exp["status"] == tm.NONE) & (over["status"] == tm.ASSIGNED)).sum() > 20
    assert len(bamio.split_records(bamio.bgzf_decompress(a_bam))[1]) > 100
    # and the overlap rule gives another matrix on the same input
    _, o_files, _ = run_cli(tmp_path / "overlap", data["plain"], ["--gene-annotation", data["gtf"]])
    assert o_files["matrix.mtx"] != a_files["matrix.mtx"]


def test_unstranded(tmp_path, data):
    check_pair(tmp_path, data, ["--per-cell"], mode="unstranded")


def test_cell_filter_and_multi_gene_filter(tmp_path, data):
    _, files, _ = check_pair(tmp_path, data, ["--per-cell", "--cell-filter", "min-molecules", "--cell-min-molecules", "20",
                                              "--umi-filtering", "multi-gene"])
    assert {"filtered/features.tsv", "filtered/barcodes.tsv", "filtered/matrix.mtx", "filtered/reads.mtx", "cells.tsv"} <= set(files)


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_both_stagings(tmp_path, data, stage):
    check_pair(tmp_path, data, ["--per-cell", "--stage", stage])


def test_overlap_and_no_flag_give_identical_bytes(tmp_path, data):
    flags = ["--per-cell", "--gene-annotation", data["gtf"]]
    none = run_cli(tmp_path / "none", data["plain"], flags)
    over = run_cli(tmp_path / "overlap", data["plain"], flags + ["--gene-rule", "overlap"])
    assert over[0] == none[0] and over[1] == none[1]  # the BAM file's bytes and every matrix file's
    timing = lambda log: [l for l in log.splitlines() if "seconds" in l or l.startswith("phases:")]
    rest = lambda log: [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    assert rest(over[2]) == rest(none[2]) and len(timing(over[2])) == len(timing(none[2]))
    assert "Gene rule" not in none[2] and "Number of transcripts" not in none[2]


def test_a_transcript_id_on_two_references_is_two_transcripts(tmp_path, data):
    exons = data["exons"]
    ids = tm.transcript_ids(exons, GENE_IDS)
    # one more line: the first transcript's id and gene on another reference (a PAR gene's second copy)
    ref, s, e, strand, g, t = exons[0]
    par = "\t".join([REFS[(ref + 1) % 3], "synthetic", "exon", str(s + 1), str(e), ".", strand, ".",
                     'gene_id "%s"; transcript_id "%s";' % (GENE_IDS[g], ids[t])])
    # and one on the same reference, on the other strand
    flipped = "\t".join([REFS[ref], "synthetic", "exon", str(s + 1), str(e), ".", "-" if strand != "-" else "+", ".",
                         'gene_id "%s"; transcript_id "%s";' % (GENE_IDS[g], ids[t])])
    gtf = am.write_gtf(tmp_path / "par.gtf", tm.gtf_lines(exons, REFS, GENE_IDS) + [par, flipped])
    _, _, log = run_cli(tmp_path / "par", data["plain"], ["--gene-annotation", gtf, "--gene-rule", "transcript"])
    assert value(log, "Number of transcripts") == str(len(tm.transcripts_of(exons)) + 2)
    assert value(log, "Gene annotation") == "%d genes, %d features" % (tm.N_GENES, len(exons) + 2)


def test_another_transcript_attribute(tmp_path, data):
    a = run_cli(tmp_path / "a", data["plain"], ["--per-cell", "--gene-annotation", data["gtf"], "--gene-rule", "transcript"])
    b = run_cli(tmp_path / "b", data["plain"], ["--per-cell", "--gene-annotation", data["gtf_tx"], "--gene-rule", "transcript",
                                                "--annotation-transcript-attribute", "tx"])
    assert bamio.bgzf_decompress(a[0]) == bamio.bgzf_decompress(b[0]) and a[1] == b[1]
    assert value(b[2], "Number of transcripts") == value(a[2], "Number of transcripts")
    assert value(b[2], "Number of annotation lines on unknown references") == "0"
    r = subprocess.run([CLI, "-i", data["plain"], "-o", str(tmp_path / "c.bam"), "--umi-tag", "UB", "--per-gene", "--gene-annotation",
                        data["gtf_tx"], "--gene-rule", "transcript"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 101 and "no attribute transcript_id" in r.stderr
