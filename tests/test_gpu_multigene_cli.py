"""umicollapse --per-gene --umi-filtering multi-gene end to end against tests/multigene_model.py: the records written,
record for record, the four matrix files byte for byte, the summary's lines -- and, whatever the model says, the
matrix against the (cell, gene) histogram of the records the program actually wrote."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import cluster_model as clm
import gene_model as gm
import multigene_model as mm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx")
STATS = ("_per_umi_per_position.tsv", "_edit_distance.tsv", "_per_umi.tsv")
SEED = 21  # (tests/test_multigene_model_cpu.py finds every planted case in it)


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    header, recs = mm.multigene_bam(SEED)
    src = str(tmp_path_factory.mktemp("multigene") / "in.bam")
    tag_model.write_bam(src, header, recs)
    return dict(src=src, recs=recs)


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def run_cli(tmp_path, src, flags, stats=False):
    tmp_path.mkdir(exist_ok=True)
    dst, mdir, prefix = str(tmp_path / "out.bam"), str(tmp_path / "matrix"), str(tmp_path / "stats")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-tag", "UB", "--per-gene", "--count-matrix", mdir] + flags +
                       (["--output-stats", prefix] if stats else []), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    recs = bamio.split_records(bamio.bgzf_decompress(open(dst, "rb").read()))[1]
    files = {f: open(os.path.join(mdir, f), "rb").read() for f in FILES}
    if stats:
        files.update({f: open(prefix + f, "rb").read() for f in STATS})
    return recs, files, r.stderr


def summary(log):
    """the summary without its timings"""
    return [l for l in log.splitlines() if "seconds" not in l and not l.startswith("phases:")]


def check_run(tmp_path, bam, flags, per_cell=True, **model):
    """one filtered run against the model, and against itself"""
    got, files, log = run_cli(tmp_path, bam["src"], flags + ["--umi-filtering", "multi-gene"])
    e = mm.expected(bam["recs"], per_cell=per_cell, **model)
    assert len(got) == len(e["records"]) > 0
    assert got == e["records"]
    for f in FILES:
        assert files[f] == e["files"][f], f
    c = e["counts"]
    assert line(log, "UMI filtering") == "multi-gene"
    assert int(line(log, "Number of UMIs seen in several genes of a cell")) == c["runs"] > 0
    assert int(line(log, "Number of molecules removed as multi-gene UMIs")) == c["removed"] > 0
    assert int(line(log, "Number of reads in removed molecules")) == c["removed_reads"] > 0
    assert int(line(log, "Number of reads after deduplicating")) == len(got) == int(np.count_nonzero(e["kept"])) - c["removed"]
    # the matrix: no zero lines, NNZ the lines, the histogram of what was written, the reads of the survivors
    mol, reads = gm.parse_matrix(files)
    assert all(v > 0 for v in mol.values())
    assert mol == gm.histogram(got, per_cell=per_cell)
    assert sum(mol.values()) == len(got)
    assert sum(reads.values()) == int(e["st"]["freq"].sum()) - c["removed_reads"]
    return got, files, log, e


def test_both_stagings_give_the_models_output_and_matrix(tmp_path, bam):
    g_recs, g_files, g_log, e = check_run(tmp_path / "gpu", bam, ["--per-cell", "--stage", "gpu"])
    h_recs, h_files, h_log, _ = check_run(tmp_path / "host", bam, ["--per-cell", "--stage", "host"])
    assert "staging (gpu)" in g_log and "staging (host)" in h_log
    assert g_recs == h_recs and g_files == h_files
    assert mm.classes(e) == set(mm.CLASSES)
    # fewer lines than the unfiltered matrix has: a pair lost all its molecules
    plain = gm.expected_matrix(e["st"], e["kept"])
    assert len(g_files["matrix.mtx"].splitlines()) < len(plain["matrix.mtx"].splitlines())


def test_without_per_cell(tmp_path, bam):
    _, files, _, e = check_run(tmp_path, bam, [], per_cell=False)
    assert files["barcodes.tsv"] == b"all\n"
    assert mm.CLASSES[6] not in mm.classes(e)  # (the two cells' UMI is one cell's now)


def test_two_devices(tmp_path, bam):
    check_run(tmp_path, bam, ["--per-cell", "--devices", "0,0"])


def test_algo_cluster(tmp_path, bam):
    check_run(tmp_path, bam, ["--per-cell", "--algo", "cluster"],
              dedup=lambda st, k, p, algo: clm.batch_of_keys(st["keys"], st["nmask"], st["bucket_off"], k))


def test_edit_distance(tmp_path, bam):
    import edit_model as em

    def dedup(st, k, p, algo):
        umis = em.decode(st["keys"], st["umi_len"])
        off = st["bucket_off"].astype(np.int64)
        buckets = [(umis[off[b]:off[b + 1]], [int(f) for f in st["freq"][off[b]:off[b + 1]]]) for b in range(len(off) - 1)]
        return em.model_batch(buckets, k, p, 0, 0)
    _, _, log, _ = check_run(tmp_path, bam, ["--per-cell", "--distance", "edit", "-k", "2"], k=2, dedup=dedup)
    assert "UMI distance: edit" in log


def test_none_changes_nothing_and_output_stats_describe_the_collapse(tmp_path, bam):
    """--umi-filtering none: every file and the summary as without the flag; --output-stats: its three files the same
    with none and with multi-gene, while everything else differs"""
    flags = ["--per-cell"]
    p_recs, p_files, p_log = run_cli(tmp_path / "plain", bam["src"], flags, stats=True)
    n_recs, n_files, n_log = run_cli(tmp_path / "none", bam["src"], flags + ["--umi-filtering", "none"], stats=True)
    m_recs, m_files, m_log = run_cli(tmp_path / "multi", bam["src"], flags + ["--umi-filtering", "multi-gene"], stats=True)
    assert p_recs == n_recs and p_files == n_files and summary(p_log) == summary(n_log)
    assert "UMI filtering" not in n_log and "multi-gene" not in n_log
    exp, st, kept = gm.expected_output(bam["recs"], per_cell=True)
    assert p_recs == exp and all(p_files[f] == gm.expected_matrix(st, kept)[f] for f in FILES)
    for f in STATS:
        assert m_files[f] == n_files[f] and len(m_files[f]) > 20, f
    assert len(m_recs) < len(n_recs) and m_files["matrix.mtx"] != n_files["matrix.mtx"] and m_files["reads.mtx"] != n_files["reads.mtx"]
    assert m_files["features.tsv"] == n_files["features.tsv"] and m_files["barcodes.tsv"] == n_files["barcodes.tsv"]
