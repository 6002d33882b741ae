"""umicollapse --algo cr end to end against tests/cr_model.py: a small tagged BAM whose (cell, gene) buckets hold
one-mismatch neighbours, chains and ties through --per-cell --per-gene --count-matrix -- the matrix files byte for
byte, the records written, both stagings, name UMIs against --umi-tag -- and the difference from --algo dir and
--algo cluster at -k 1 that the rule is there for."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import cr_model as cm
import gene_model as gm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    header, recs = cm.cr_bam()
    src = str(tmp_path_factory.mktemp("cr_cli") / "in.bam")
    tag_model.write_bam(src, header, recs)
    exp, st, kept = gm.expected_output(recs, per_cell=True, dedup=cm.dedup_staged)
    return dict(src=src, recs=recs, exp=exp, st=st, kept=kept, files=gm.expected_matrix(st, kept))


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def run_cli(tmp_path, src, flags):
    tmp_path.mkdir(exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--per-cell", "--per-gene", "--count-matrix", mdir] + flags,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = bamio.split_records(bamio.bgzf_decompress(open(dst, "rb").read()))[1]
    return recs, {f: open(os.path.join(mdir, f), "rb").read() for f in FILES}, r.stderr


def test_the_matrix_and_the_records_are_the_models(tmp_path, bam):
    assert 150 <= len(bam["recs"]) <= 400
    assert sum(cm.chains(u, f) for u, f in cm.staged_buckets(bam["st"])) > 0
    runs = {}
    for name, flags in (("gpu", ["--umi-tag", "UB", "--stage", "gpu"]), ("host", ["--umi-tag", "UB", "--stage", "host"]),
                        ("name", ["--stage", "host"])):
        got, files, log = run_cli(tmp_path / name, bam["src"], flags + ["--algo", "cr"])
        assert line(log, "UMI correction") == "cr"
        for f in FILES:
            assert files[f] == bam["files"][f], (name, f)
        # the written records are the kept entries' representatives
        assert got == bam["exp"], name
        assert int(line(log, "Number of reads after deduplicating")) == len(got) == int(bam["kept"].sum())
        mol, reads = gm.parse_matrix(files)
        assert mol == gm.histogram(got) and sum(reads.values()) == int(bam["st"]["freq"].sum())
        runs[name] = (got, files)
    assert runs["gpu"] == runs["host"] == runs["name"]   # both stagings; name UMIs and --umi-tag


def test_the_result_is_neither_dir_nor_cluster_at_k1(tmp_path, bam):
    _, cr, _ = run_cli(tmp_path / "cr", bam["src"], ["--umi-tag", "UB", "--algo", "cr"])
    _, dr, log = run_cli(tmp_path / "dir", bam["src"], ["--umi-tag", "UB", "--algo", "dir", "-k", "1"])
    _, cl, _ = run_cli(tmp_path / "cluster", bam["src"], ["--umi-tag", "UB", "--algo", "cluster", "-k", "1"])
    assert "UMI correction" not in log
    assert cr["matrix.mtx"] != dr["matrix.mtx"]
    assert cr["matrix.mtx"] != cl["matrix.mtx"]
    assert cr["features.tsv"] == dr["features.tsv"] and cr["barcodes.tsv"] == cl["barcodes.tsv"]
    # -p plays no part
    _, cr2, _ = run_cli(tmp_path / "cr_p", bam["src"], ["--umi-tag", "UB", "--algo", "cr", "-p", "0.05"])
    assert cr2 == cr


def test_the_later_calls_accept_the_contract(tmp_path, bam):
    """--umi-filtering multi-gene and --output-stats check kept[] and root[] (kept[i] implies root[i] == i, kept[root[i]])"""
    prefix = str(tmp_path / "stats")
    got, files, log = run_cli(tmp_path / "run", bam["src"], ["--umi-tag", "UB", "--algo", "cr", "--umi-filtering", "multi-gene",
                                                            "--output-stats", prefix])
    mol, _ = gm.parse_matrix(files)
    assert sum(mol.values()) == int(line(log, "Number of reads after deduplicating")) == len(got)
    removed = int(line(log, "Number of molecules removed as multi-gene UMIs"))
    assert len(got) == int(bam["kept"].sum()) - removed
    for f in ("_per_umi_per_position.tsv", "_edit_distance.tsv", "_per_umi.tsv"):
        assert os.path.getsize(prefix + f) > 0
    assert open(prefix + "_edit_distance.tsv").readline().split("\t")[3] == "cr"
