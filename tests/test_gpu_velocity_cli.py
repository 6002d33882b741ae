"""umicollapse --velocity end to end against tests/velocity_model.py (expected_cli): DIR/velocity's five files byte for
byte and the eight summary lines, under both intron modes, with the multi-gene filter, the cell filter, --algo cluster
and -k 0; everything else -- the BAM, the raw files, filtered/, cells.tsv, the other summary lines -- against the same
run without the flag under --stage host; and the refusals."""
import os
import subprocess

import numpy as np
import pytest

import annotation_model as am
import bamio
import cluster_model as clm
import intron_model as im
import tag_model
import velocity_model as vm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
LAYERS = ("spliced.mtx", "unspliced.mtx", "ambiguous.mtx")
FIVE = ("features.tsv", "barcodes.tsv") + LAYERS
READ_LINES = ("Number of exonic reads", "Number of junction reads", "Number of exon-intron reads", "Number of intronic reads")
MOLECULE_LINES = ("Number of spliced molecules", "Number of unspliced molecules", "Number of ambiguous molecules")
OWN_LINES = ("Velocity",) + READ_LINES + MOLECULE_LINES


@pytest.fixture(scope="module")
def data(tmp_path_factory):
    d = tmp_path_factory.mktemp("velocity")
    header, recs, cells = vm.velocity_bam()
    src = str(d / "in.bam")
    tag_model.write_bam(src, header, recs)
    gtf = am.write_gtf(d / "genes.gtf", am.gtf_lines(vm.fuzz_annotation(), vm.REF_NAMES, vm.GENE_IDS))
    return dict(src=src, recs=recs, gtf=gtf)


def run_cli(tmp_path, data, flags, introns="exon-first", velocity=True, ok=True):
    tmp_path.mkdir(parents=True, exist_ok=True)
    dst, mdir = str(tmp_path / "out.bam"), str(tmp_path / "matrix")
    cmd = [CLI, "-i", data["src"], "-o", dst, "--umi-tag", "UB", "--per-gene", "--per-cell", "--count-matrix", mdir,
           "--gene-annotation", data["gtf"], "--gene-introns", introns] + flags + (["--velocity"] if velocity else [])
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


def check(tmp_path, data, flags, introns="exon-first", **model):
    """a run with the flag against the model, and against the run without it under --stage host"""
    bam, files, log = run_cli(tmp_path / "with", data, flags, introns)
    plain_bam, plain_files, plain_log = run_cli(tmp_path / "without", data, flags + ["--stage", "host"], introns, velocity=False)
    e = vm.expected_cli(data["recs"], am.FORWARD, im.INTRONS[introns], **model)
    # the five files: the raw names' bytes, the model's layers
    for f in ("features.tsv", "barcodes.tsv"):
        assert files["velocity/" + f] == files[f], f
    assert files["velocity/barcodes.tsv"] == e["files"]["barcodes.tsv"]
    assert [l.split(b"\t")[0] for l in files["features.tsv"].splitlines()] == [l.split(b"\t")[0] for l in e["files"]["features.tsv"].splitlines()]
    for f in LAYERS:
        assert files["velocity/" + f] == e["files"][f], f
        lines = files["velocity/" + f].decode().splitlines()
        assert int(lines[1].split()[2]) == len(lines) - 2 and all(int(l.split()[2]) > 0 for l in lines[2:])
    # the summary's eight lines
    assert [l.split(":")[0] for l in summary(log, True)] == list(OWN_LINES) and value(log, "Velocity") == "on"
    assert [int(value(log, l)) for l in READ_LINES] == [int(c) for c in e["class_counts"][1:]]
    assert [int(value(log, l)) for l in MOLECULE_LINES] == e["layers"]
    assert sum(e["layers"]) == e["molecules"] == int(value(log, "Number of reads after deduplicating"))
    assert int(value(log, READ_LINES[3])) == int(value(log, "Number of reads assigned by an intron"))
    assert min(e["class_counts"]) > 20 and min(e["layers"]) > 10
    # the layers add up to matrix.mtx, pair by pair
    total = {}
    for f in LAYERS:
        for l in files["velocity/" + f].decode().splitlines()[2:]:
            r, c, v = l.split()
            total[(r, c)] = total.get((r, c), 0) + int(v)
    assert total == {tuple(l.split()[:2]): int(l.split()[2]) for l in files["matrix.mtx"].decode().splitlines()[2:]}
    # everything else is the run without the flag
    assert "staging (host)" in log
    assert bam == plain_bam
    rest = {f: b for f, b in files.items() if not f.startswith("velocity")}
    assert sorted(rest) == sorted(plain_files) and not any(f.startswith("velocity") for f in plain_files)
    for f in rest:
        assert rest[f] == plain_files[f], f
    assert summary(log, False) == summary(plain_log, False) and summary(plain_log, True) == []
    assert sorted(f for f in files if f.startswith("velocity/") and "filtered" not in f) == sorted("velocity/" + f for f in FIVE)
    return files, log, e


@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_against_the_model(tmp_path, data, introns):
    files, _, _ = check(tmp_path, data, [], introns)
    assert not any("filtered" in f for f in files)


def test_with_the_multi_gene_filter(tmp_path, data):
    _, log, e = check(tmp_path, data, ["--umi-filtering", "multi-gene"], multigene=True)
    plain = vm.expected_cli(data["recs"], am.FORWARD, im.EXON_FIRST)
    assert int(value(log, "Number of molecules removed as multi-gene UMIs")) == plain["molecules"] - e["molecules"] > 10


def test_with_the_cell_filter(tmp_path, data):
    # the threshold: the second smallest of the cells' totals, so that some cells are called and not all
    plain = vm.expected_cli(data["recs"], am.FORWARD, im.EXON_FIRST)
    totals = np.bincount(plain["triplets"][1], weights=sum(v.astype(np.int64) for v in plain["triplets"][2:])).astype(np.int64)
    assert len(totals) >= 3 and len(set(totals.tolist())) == len(totals)
    files, _, e = check(tmp_path, data, ["--cell-filter", "min-molecules", "--cell-min-molecules", str(int(np.sort(totals)[1]))])
    cells = files["barcodes.tsv"].splitlines()
    called = files["filtered/barcodes.tsv"].splitlines()
    assert 0 < len(called) < len(cells)
    assert files["velocity/filtered/barcodes.tsv"] == files["filtered/barcodes.tsv"]
    assert files["velocity/filtered/features.tsv"] == files["filtered/features.tsv"]
    new_col = {cells.index(c): i for i, c in enumerate(called)}
    row, col = e["triplets"][0], e["triplets"][1]
    take = np.array([int(c) in new_col for c in col])
    renumbered = np.array([new_col[int(c)] for c in col[take]], np.uint32)
    want = vm.layer_files(e["st"]["genes"], called, len(e["st"]["genes"]), len(called),
                          (row[take], renumbered) + tuple(v[take] for v in e["triplets"][2:]))
    total = {}
    for f in LAYERS:
        assert files["velocity/filtered/" + f] == want[f], f
        for l in files["velocity/filtered/" + f].decode().splitlines()[2:]:
            r, c, v = l.split()
            total[(r, c)] = total.get((r, c), 0) + int(v)
    assert total == {tuple(l.split()[:2]): int(l.split()[2]) for l in files["filtered/matrix.mtx"].decode().splitlines()[2:]}
    assert sorted(f for f in files if f.startswith("velocity/filtered/")) == sorted("velocity/filtered/" + f for f in FIVE)


def test_algo_cluster_and_k_0(tmp_path, data):
    check(tmp_path / "cluster", data, ["--algo", "cluster"], algo="cluster",
          dedup=lambda st, k, p, algo: clm.batch_of_keys(st["keys"], st["nmask"], st["bucket_off"], k))
    _, _, e = check(tmp_path / "k0", data, ["-k", "0"], k=0)
    assert e["molecules"] == len(e["mask"])  # (every entry is its own molecule)


def test_refusals(tmp_path, data):
    base = [CLI, "-i", data["src"], "-o", str(tmp_path / "out.bam"), "--umi-tag", "UB", "--per-gene", "--per-cell", "--velocity"]
    m, g = ["--count-matrix", str(tmp_path / "m")], ["--gene-annotation", data["gtf"]]
    for flags, word in ((g + ["--gene-introns", "all"], "--velocity goes with --count-matrix"),
                        (m + ["--gene-introns", "all"], "--gene-introns goes with --gene-annotation only"),
                        (m, "--velocity goes with --gene-annotation"),
                        (m + g, "--velocity goes with --gene-introns exon-first or all"),
                        (m + g + ["--gene-introns", "off"], "--velocity goes with --gene-introns exon-first or all"),
                        (m + g + ["--gene-introns", "all", "--stage", "gpu"], "--stage gpu does not go with --paired, --tag, --call-consensus, --velocity"),
                        (m + g + ["--gene-introns", "all", "--tag"], "--per-gene does not go with --tag"),
                        (m + g + ["--gene-introns", "all", "--gene-tag", "XG"], "--gene-annotation does not go with --gene-tag")):
        r = subprocess.run(base + flags, capture_output=True, text=True, timeout=120)
        assert r.returncode == 101 and word in r.stderr, (flags, r.returncode, r.stderr)
        assert not os.path.exists(str(tmp_path / "out.bam")) and not os.path.exists(str(tmp_path / "m"))  # (nothing was begun)
