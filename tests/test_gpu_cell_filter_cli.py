"""umicollapse --cell-filter end to end on the skewed-depth BAM of tests/cells_model.py: the four raw files, the BAM and
the summary's earlier lines byte for byte what a run without the flag gives; filtered/*, cells.tsv and the new summary
lines what cells_model.files_model makes of the raw matrix.mtx and reads.mtx of the same run."""
import os
import subprocess

import pytest

import cells_model as cm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
RAW = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx")
ADDED = ("filtered/features.tsv", "filtered/barcodes.tsv", "filtered/matrix.mtx", "filtered/reads.mtx", "cells.tsv")
SEED = 33  # (tests/test_cells_model_cpu.py checks what this BAM gives under each rule)
NEW_LINES = ("Cell filter", "Number of candidate cells", "Number of cells called", "Molecule threshold",
             "Number of molecules in called cells", "Number of reads in called cells", "Median molecules per called cell",
             "Median genes per called cell")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    header, recs, cells = cm.cells_bam(SEED)
    d = tmp_path_factory.mktemp("cells")
    src, wl = str(d / "in.bam"), str(d / "whitelist.txt")
    tag_model.write_bam(src, header, recs)
    with open(wl, "w") as f:
        f.write("".join(c + "\n" for c in sorted(cells)))
    return dict(src=src, whitelist=wl)


def run_cli(tmp_path, src, flags):
    tmp_path.mkdir(exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-cell", "--per-gene", "--count-matrix", mdir] + flags,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    files = {}
    for base, _, names in os.walk(mdir):
        for name in names:
            path = os.path.join(base, name)
            files[os.path.relpath(path, mdir)] = open(path, "rb").read()
    return open(dst, "rb").read(), files, r.stderr


def summary(log):
    """the summary without its timings"""
    return [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]


def value(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def check_rule(tmp_path, bam, name, flags):
    rule_flags, rule = cm.CLI_RULES[name]
    p_bam, p_files, p_log = run_cli(tmp_path / "plain", bam["src"], flags)
    f_bam, f_files, f_log = run_cli(tmp_path / "filter", bam["src"], flags + rule_flags)
    # what was there stays: the BAM, the four raw files, every earlier summary line
    assert sorted(p_files) == sorted(RAW) and sorted(f_files) == sorted(RAW + ADDED)
    assert f_bam == p_bam
    for f in RAW:
        assert f_files[f] == p_files[f], f
    new = [l for l in summary(f_log) if l.split(":")[0] in NEW_LINES]
    assert [l.split(":")[0] for l in new] == list(NEW_LINES)
    assert [l for l in summary(f_log) if l not in new] == summary(p_log)
    # what is added is the model's, from the raw files of the same run
    exp, counts = cm.files_model({f: f_files[f] for f in RAW}, **rule)
    for f in ADDED:
        assert f_files[f] == exp[f], (f, f_files[f][:300], exp[f][:300])
    assert value(f_log, "Cell filter") == name
    got = [int(value(f_log, what)) for what in NEW_LINES[1:]]
    assert got == [counts[k] for k in ("candidates", "called", "threshold", "molecules_in_cells", "reads_in_cells", "median_molecules",
                                        "median_genes")]
    assert counts["called"] >= 1 and counts["candidates"] > counts["called"]
    return counts


@pytest.mark.parametrize("name", sorted(cm.CLI_RULES))
def test_each_rule(tmp_path, bam, name):
    counts = check_rule(tmp_path, bam, name, [])
    assert counts["called"] >= 2 and counts["candidates"] - counts["called"] >= 2 and counts["candidates"] == len(cm.DEPTHS)


def test_with_the_multi_gene_filter(tmp_path, bam):
    """the call sees what matrix.mtx holds: the doubled UMI's molecule is gone from the deepest cell"""
    counts = check_rule(tmp_path, bam, "min-molecules", ["--umi-filtering", "multi-gene"])
    assert counts["molecules"] == sum(cm.DEPTHS)


def test_with_a_cell_whitelist(tmp_path, bam):
    check_rule(tmp_path, bam, "top-cells", ["--cell-tag", "CR", "--cell-whitelist", bam["whitelist"]])


def test_with_algo_cluster(tmp_path, bam):
    check_rule(tmp_path, bam, "cr2.2", ["--algo", "cluster"])
