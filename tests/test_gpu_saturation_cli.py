"""umicollapse --saturation-curve end to end against tests/saturation_model.py (expected_cli): FILE byte for byte and the
two summary lines, with the cell filter, the multi-gene filter, without --per-cell and with other points and another seed;
everything else -- the BAM, DIR's files, the other summary lines -- against the same run without the flag under
--stage host; and two runs against each other."""
import os
import subprocess

import numpy as np
import pytest

import annotation_model as am
import saturation_model as sm
import tag_model
import velocity_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
OWN_LINES = ("Saturation curve", "Sequencing saturation")


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("saturation")
    header, recs, cells = vm.velocity_bam()
    src = str(d / "in.bam")
    tag_model.write_bam(src, header, recs)
    gtf = am.write_gtf(d / "genes.gtf", am.gtf_lines(vm.fuzz_annotation(), vm.REF_NAMES, vm.GENE_IDS))
    return dict(src=src, recs=recs, gtf=gtf)


def run_cli(tmp_path, data, flags, per_cell=True, curve=True):
    tmp_path.mkdir(parents=True, exist_ok=True)
    dst, mdir, out = str(tmp_path / "out.bam"), str(tmp_path / "matrix"), str(tmp_path / "curve.tsv")
    cmd = [CLI, "-i", data["src"], "-o", dst, "--umi-tag", "UB", "--per-gene", "--count-matrix", mdir, "--gene-annotation", data["gtf"],
           "--gene-introns", "exon-first"] + (["--per-cell"] if per_cell else []) + flags + (["--saturation-curve", out] if curve else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = {}
    for base, _, names in os.walk(mdir):
        for name in names:
            path = os.path.join(base, name)
            files[os.path.relpath(path, mdir)] = open(path, "rb").read()
    assert sorted(os.listdir(tmp_path)) == sorted(["out.bam", "matrix"] + (["curve.tsv"] if curve else []))
    return open(dst, "rb").read(), files, r.stderr, open(out, "rb").read() if curve else None


def summary(log, own):
    lines = [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]
    return [l for l in lines if (l.split(":")[0] in OWN_LINES) == own]


def value(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def check(tmp_path, data, flags, own_flags=(), per_cell=True, **model):
    """a run with the flag against the model, against the run without it under --stage host, and against a second run"""
    bam, files, log, curve = run_cli(tmp_path / "with", data, flags + list(own_flags), per_cell)
    plain_bam, plain_files, plain_log, _ = run_cli(tmp_path / "without", data, flags + ["--stage", "host"], per_cell, curve=False)
    e = sm.expected_cli(data["recs"], per_cell=per_cell, **model)
    assert curve == e["file"], (curve.decode(), e["file"].decode())
    lines = [l.split("\t") for l in curve.decode().splitlines()]
    L = len(e["curve"])
    assert len(lines) == L + 1 and lines[0] == sm.HEADER.split() and [l[0] for l in lines[1:]] == ["%d/%d" % (j + 1, L) for j in range(L)]
    # the last line: the run's molecules, and the staged reads under kept roots
    assert int(lines[-1][2]) == e["molecules"] == int(value(log, "Number of reads after deduplicating")) > 100
    assert int(lines[-1][1]) == e["reads"] > e["molecules"]
    assert int(lines[1][2]) < e["molecules"] or L == 1
    # the summary's two lines
    assert [l.split(":")[0] for l in summary(log, True)] == list(OWN_LINES)
    assert value(log, "Saturation curve") == "%d points, seed %d" % (L, model.get("seed", 0))
    assert value(log, "Sequencing saturation") == lines[-1][3] == sm.saturation_text(e["reads"], e["molecules"])
    # everything else is the run without the flag
    assert "staging (host)" in log
    assert bam == plain_bam
    assert sorted(files) == sorted(plain_files)
    for f in files:
        assert files[f] == plain_files[f], f
    assert summary(log, False) == summary(plain_log, False) and summary(plain_log, True) == []
    # two runs give the same file
    assert run_cli(tmp_path / "again", data, flags + list(own_flags), per_cell)[3] == curve
    return files, log, e


def test_against_the_model(tmp_path, data):
    files, _, e = check(tmp_path, data, [])
    assert e["cell_mask"] is None and e["curve"][-1, 3] == len(files["barcodes.tsv"].splitlines()) >= 3
    assert e["curve"][-1, 6] > 10 and e["curve"][-1, 7] > 3 and (e["curve"][-1, :3] > e["curve"][0, :3]).all()


def test_with_the_cell_filter(tmp_path, data):
    # the threshold: the second smallest of the cells' totals, so that some cells are called and not all
    plain = sm.expected_cli(data["recs"])
    st = plain["st"]
    totals = np.bincount(np.repeat(st["bucket_cell"].astype(np.int64), np.diff(st["bucket_off"].astype(np.int64))),
                         weights=np.asarray(plain["mask"]) != 0).astype(np.int64)
    assert len(totals) >= 3 and len(set(totals.tolist())) == len(totals)
    t = int(np.sort(totals)[1])
    files, _, e = check(tmp_path, data, ["--cell-filter", "min-molecules", "--cell-min-molecules", str(t)], cell_min_molecules=t)
    called = files["filtered/barcodes.tsv"].splitlines()
    assert 0 < len(called) == int(e["cell_mask"].sum()) == int(e["curve"][-1, 3]) < len(files["barcodes.tsv"].splitlines())
    assert e["curve"][-1, 4] < e["curve"][-1, 1] and (e["curve"][:, :3] == plain["curve"][:, :3]).all()


def test_with_the_multi_gene_filter(tmp_path, data):
    _, log, e = check(tmp_path, data, ["--umi-filtering", "multi-gene"], multigene=True)
    plain = sm.expected_cli(data["recs"])
    assert int(value(log, "Number of molecules removed as multi-gene UMIs")) == plain["molecules"] - e["molecules"] > 10
    assert e["reads"] < plain["reads"]  # (reads under a removed UMI count nowhere)


def test_without_per_cell(tmp_path, data):
    files, _, e = check(tmp_path, data, [], per_cell=False)
    assert files["barcodes.tsv"] == b"all\n" and (e["curve"][:, 3] == 1).all()
    assert (e["curve"][:, 6] == e["curve"][:, 1]).all() and (e["curve"][:, 7] == e["curve"][:, 2]).all()


def test_other_points_and_another_seed(tmp_path, data):
    _, _, e = check(tmp_path, data, [], ["--saturation-points", "4", "--saturation-seed", "9"], n_levels=4, seed=9)
    assert len(e["curve"]) == 4 and (e["curve"][-1] == sm.expected_cli(data["recs"])["curve"][-1]).all()
