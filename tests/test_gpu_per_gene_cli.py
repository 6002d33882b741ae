"""umicollapse --per-gene --count-matrix end to end against tests/gene_model.py: the records written, record for
record, the four matrix files byte for byte, the summary lines -- and, whatever the model says, the matrix against
the (cell, gene) histogram of the records the program actually wrote."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import gene_model as gm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    header, recs, cells = gm.gene_bam(21)
    d = tmp_path_factory.mktemp("gene")
    src = str(d / "in.bam")
    tag_model.write_bam(src, header, recs)
    lst = str(d / "cells.txt")
    with open(lst, "w") as f:
        f.write("# the kit's cell barcodes\n" + "\n".join(sorted(cells)) + "\n")
    return dict(src=src, recs=recs, cells=cells, list=lst)


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def run_cli(tmp_path, src, flags, matrix=True):
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    r = subprocess.run([CLI, "-i", src, "-o", dst] + flags + (["--count-matrix", mdir] if matrix else []),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = bamio.split_records(bamio.bgzf_decompress(open(dst, "rb").read()))[1]
    files = {f: open(os.path.join(mdir, f), "rb").read() for f in FILES} if matrix else None
    return recs, files, r.stderr


def check_run(tmp_path, bam, flags, per_cell=True, cell_key=lambda cb: cb, **model):
    """one run against the model, and against itself"""
    got, files, log = run_cli(tmp_path, bam["src"], ["--umi-tag", "UB", "--per-gene"] + flags)
    exp, st, kept = gm.expected_output(bam["recs"], per_cell=per_cell, **model)
    assert len(got) == len(exp) > 0
    assert got == exp
    exp_files = gm.expected_matrix(st, kept)
    for f in FILES:
        assert files[f] == exp_files[f], f
    c = st["counters"]
    assert int(line(log, "Number of reads without a gene tag")) == c["no_gene"] > 0
    assert int(line(log, "Number of reads assigned to several genes")) == c["several"] > 0
    assert int(line(log, "Number of reads without a UMI tag")) == c["no_umi"]
    assert int(line(log, "Number of genes")) == c["genes"] == len(st["genes"])
    assert int(line(log, "Number of (cell, gene) groups" if per_cell else "Number of gene groups")) == c["groups"]
    assert "alignment positions:" not in log.replace("per alignment position", "").replace("over all alignment positions", "")
    # the matrix is the histogram of what was written, and adds up to the summary's count
    mol, reads = gm.parse_matrix(files)
    hist = {}
    for (cb, gx), v in gm.histogram(got, per_cell=per_cell).items():
        hist[(cell_key(cb), gx)] = hist.get((cell_key(cb), gx), 0) + v
    assert {k: v for k, v in mol.items() if v} == hist
    assert sum(mol.values()) == int(line(log, "Number of reads after deduplicating")) == len(got)
    assert sum(reads.values()) == int(st["freq"].sum())
    return got, files, log


def test_both_stagings_give_the_models_output_and_matrix(tmp_path, bam):
    (tmp_path / "gpu").mkdir()
    (tmp_path / "host").mkdir()
    g_recs, g_files, g_log = check_run(tmp_path / "gpu", bam, ["--per-cell", "--stage", "gpu"])
    h_recs, h_files, h_log = check_run(tmp_path / "host", bam, ["--per-cell", "--stage", "host"])
    assert "staging (gpu)" in g_log and "staging (host)" in h_log
    assert g_recs == h_recs and g_files == h_files
    assert g_files["barcodes.tsv"].splitlines()[0].endswith(b"-1") and len(g_files["barcodes.tsv"].splitlines()) == 7


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_without_per_cell(tmp_path, bam, stage):
    _, files, _ = check_run(tmp_path, bam, ["--stage", stage], per_cell=False)
    assert files["barcodes.tsv"] == b"all\n"
    assert files["matrix.mtx"].splitlines()[1].split()[1] == b"1"


def test_adjacency_k2_avgqual(tmp_path, bam):
    check_run(tmp_path, bam, ["--per-cell", "-k", "2", "--algo", "adj", "--merge", "avgqual"], k=2, algo="adj", merge="avgqual")


def test_edit_distance(tmp_path, bam):
    import edit_model as em

    def dedup(st, k, p, algo):
        umis = em.decode(st["keys"], st["umi_len"])
        off = st["bucket_off"].astype(np.int64)
        buckets = [(umis[off[b]:off[b + 1]], [int(f) for f in st["freq"][off[b]:off[b + 1]]]) for b in range(len(off) - 1)]
        return em.model_batch(buckets, k, p, 0 if algo == "dir" else 1, 0)[0]
    _, _, log = check_run(tmp_path, bam, ["--per-cell", "--distance", "edit", "-k", "2"], k=2, dedup=dedup)
    assert "UMI distance: edit" in log


def test_two_devices(tmp_path, bam):
    check_run(tmp_path, bam, ["--per-cell", "--devices", "0,0"])


def test_four_threads(tmp_path, bam):
    check_run(tmp_path, bam, ["--per-cell", "--num-threads", "4"])


def test_cell_whitelist(tmp_path, bam):
    """raw barcodes (CR) corrected to the kit's list: barcodes.tsv holds the listed barcodes, in id order"""
    _, files, log = check_run(tmp_path, bam, ["--per-cell", "--cell-tag", "CR", "--cell-whitelist", bam["list"]],
                              cell_tag="CR", cell_list=bam["cells"], cell_key=lambda cb: cb[:-2])
    names = files["barcodes.tsv"].splitlines()
    assert sorted(names) == sorted(c.encode() for c in bam["cells"])
    assert int(line(log, "Number of reads with a corrected cell barcode")) > 0


def test_per_gene_writes_fewer_records_than_per_position(tmp_path, bam):
    """the same reads -- those with one gene -- grouped by (cell, gene) and by (position, cell): a molecule
    fragmented at two places is kept once only with --per-gene"""
    one = [r for r in bam["recs"] if gm.gene_class(tag_model.parse_aux(r).get("GX", (None, None))[1]) == "one"]
    src = str(tmp_path / "one.bam")
    tag_model.write_bam(src, bamio.make_header([("chr1", 10_000_000), ("chr2", 5_000_000)]), one)
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    with_flag, _, log = run_cli(tmp_path / "a", src, ["--umi-tag", "UB", "--per-cell", "--per-gene"], matrix=False)
    without, _, log0 = run_cli(tmp_path / "b", src, ["--umi-tag", "UB", "--per-cell"], matrix=False)
    assert 0 < len(with_flag) < len(without)
    assert int(line(log, "Number of reads without a gene tag")) == 0
    assert "gene" not in log0 and "Number of unique alignment positions" in log0
    assert not os.path.exists(str(tmp_path / "a" / "matrix"))
