"""umicollapse --junction-matrix end to end against tests/junction_model.py (expected_cli): DIR/junctions' files byte for
byte and the five summary lines, with GX tags and with --gene-annotation, with the multi-gene filter, the cell filter and
without --per-cell; everything else -- the BAM, DIR's other files, the other summary lines -- against the same run without
the flag under --stage host; and a BAM without a spliced read."""
import os
import subprocess

import numpy as np
import pytest

import annotation_model as am
import bamio
import junction_model as jm
import tag_model
import velocity_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
OWN_LINES = ("Junction matrix", "Number of spliced reads counted", "Number of junction occurrences", "Number of distinct junctions",
             "Number of (cell, junction) pairs")
ANNOTATED = ["--gene-introns", "exon-first"]


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("junctions")
    header, recs, _ = vm.velocity_bam()
    tagged = jm.tagged_records(recs)
    plain, with_gx = str(d / "in.bam"), str(d / "gx.bam")
    tag_model.write_bam(plain, header, recs)
    tag_model.write_bam(with_gx, header, tagged)
    gtf = am.write_gtf(d / "genes.gtf", am.gtf_lines(vm.fuzz_annotation(), vm.REF_NAMES, vm.GENE_IDS))
    return dict(plain=plain, gx=with_gx, header=header, tagged=tagged, gtf=gtf, expected={})


def expected(data, **model):
    key = tuple(sorted(model.items()))
    if key not in data["expected"]:
        data["expected"][key] = jm.expected_cli(data["tagged"], vm.REF_NAMES, **model)
    return data["expected"][key]


def run_cli(tmp_path, src, flags, per_cell=True, junctions=True):
    tmp_path.mkdir(parents=True, exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    cmd = [CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-gene", "--count-matrix", mdir] + (["--per-cell"] if per_cell else []) + \
        flags + (["--junction-matrix"] if junctions else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = {}
    for base, _, names in os.walk(mdir):
        for name in names:
            path = os.path.join(base, name)
            files[os.path.relpath(path, mdir)] = open(path, "rb").read()
    return open(dst, "rb").read(), files, r.stderr


def summary(log, own):
    lines = [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    return [l for l in lines if (l.split(":")[0] in OWN_LINES) == own]


def value(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def check(tmp_path, src, flags, e, per_cell=True):
    """a run with the flag against the model and against the run without it under --stage host"""
    bam, files, log = run_cli(tmp_path / "with", src, flags, per_cell)
    plain_bam, plain_files, plain_log = run_cli(tmp_path / "without", src, flags + ["--stage", "host"], per_cell, junctions=False)
    own = {f: v for f, v in files.items() if f.startswith("junctions" + os.sep)}
    want = {"junctions/" + f: v for f, v in e["files"].items()}
    want["junctions/barcodes.tsv"] = files["barcodes.tsv"]
    if e["filtered"] is not None:
        want.update({"junctions/filtered/" + f: v for f, v in e["filtered"].items()})
        want["junctions/filtered/barcodes.tsv"] = files["filtered/barcodes.tsv"]
    assert sorted(own) == sorted(want)
    for f in want:
        assert own[f] == want[f], (f, own[f][:300], want[f][:300])
    # the summary's five lines, behind every other
    assert [l.split(":")[0] for l in summary(log, True)] == list(OWN_LINES)
    lines = [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    assert [l.split(":")[0] for l in lines[-5:]] == list(OWN_LINES)
    assert value(log, "Junction matrix") == "on"
    assert [int(value(log, what)) for what in OWN_LINES[1:]] == [int(c) for c in e["counts"]]
    # everything else is the run without the flag
    assert "staging (host)" in log
    assert bam == plain_bam
    rest = {f: v for f, v in files.items() if f not in own}
    assert sorted(rest) == sorted(plain_files)
    for f in rest:
        assert rest[f] == plain_files[f], f
    assert summary(log, False) == summary(plain_log, False) and summary(plain_log, True) == []
    return files, log


def test_with_gx_tags(tmp_path, data):
    e = expected(data)
    files, _ = check(tmp_path, data["gx"], [], e)
    c = [int(x) for x in e["counts"]]
    assert c[0] > 100 and c[1] > c[0] and c[2] > 100 and c[3] >= c[2]
    assert len(files["junctions/features.tsv"].splitlines()) == c[2]
    first = files["junctions/features.tsv"].splitlines()[0].split(b"\t")
    assert first[0] == vm.REF_NAMES[0].encode() and int(first[1]) <= int(first[2])


def test_with_the_annotation(tmp_path, data):
    check(tmp_path, data["plain"], ["--gene-annotation", data["gtf"]] + ANNOTATED, expected(data))


def test_with_the_multi_gene_filter(tmp_path, data):
    e = expected(data, multigene=True)
    check(tmp_path, data["gx"], ["--umi-filtering", "multi-gene"], e)
    assert int(e["counts"][1]) < int(expected(data)["counts"][1])  # (reads under a removed UMI count nowhere)


def test_with_the_cell_filter(tmp_path, data):
    # the threshold: the second smallest of the cells' totals, so that some cells are called and not all
    plain = expected(data)
    st = plain["st"]
    totals = np.bincount(np.repeat(st["bucket_cell"].astype(np.int64), np.diff(st["bucket_off"].astype(np.int64))),
                         weights=np.asarray(plain["mask"]) != 0).astype(np.int64)
    assert len(totals) >= 3 and len(set(totals.tolist())) == len(totals)
    t = int(np.sort(totals)[1])
    e = expected(data, cell_min_molecules=t)
    files, _ = check(tmp_path, data["plain"], ["--gene-annotation", data["gtf"]] + ANNOTATED +
                     ["--cell-filter", "min-molecules", "--cell-min-molecules", str(t)], e)
    assert 0 < len(e["called"]) < len(totals)
    raw, called = files["junctions/features.tsv"].splitlines(), files["junctions/filtered/features.tsv"].splitlines()
    assert 0 < len(called) < len(raw) and [l for l in raw if l in set(called)] == called  # (dropped, and the rest in table order)
    assert files["junctions/matrix.mtx"] == expected(data)["files"]["matrix.mtx"]  # (the raw directory does not know the filter)


def test_without_per_cell(tmp_path, data):
    e = expected(data, per_cell=False)
    files, _ = check(tmp_path, data["gx"], [], e, per_cell=False)
    assert files["junctions/barcodes.tsv"] == b"all\n"
    assert int(e["counts"][3]) == int(e["counts"][2])  # (one column: a pair per junction)


def test_no_spliced_read(tmp_path, data):
    """the records whose CIGARs hold no N: empty matrices with their headers"""
    recs = [rec for rec in data["tagged"] if not any(op == "N" for op, _ in bamio.parse_record(rec)["cigar"])]
    assert len(recs) > 100
    src = str(tmp_path / "unspliced.bam")
    tag_model.write_bam(src, data["header"], recs)
    e = jm.expected_cli(recs, vm.REF_NAMES)
    assert not e["counts"].any()
    files, log = check(tmp_path, src, [], e)
    n_cells = len(files["barcodes.tsv"].splitlines())
    head = (jm.MTX_HEADER + "0 %d 0\n" % n_cells).encode()
    assert files["junctions/features.tsv"] == b"" and files["junctions/matrix.mtx"] == head == files["junctions/reads.mtx"]
    assert int(value(log, "Number of reads after deduplicating")) > 50
