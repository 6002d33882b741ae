"""umicollapse --output-stats end to end: the three files byte for byte against the writers of tests/stats_model.py,
fed the staging the Python models compute and the oracle's collapse; the output BAM and stderr (its times aside)
identical to the same run without the flag.  Four small BAMs: UMIs of 12 bases in the name and in tags with cell
barcodes and N (every flag set), UMIs of 24 bases -- two key words -- in the name with N (the sets that need no tag
and take two words), a single-cell BAM with genes (--per-gene --count-matrix), and a paired one (--paired)."""
import os
import re
import subprocess

import numpy as np
import pytest

import bamio
import cluster_model
import gene_model as gm
import oracle as orc
import stats_model as sm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
NAMES = ("_per_umi_per_position.tsv", "_edit_distance.tsv", "_per_umi.tsv")
ALGO = {"dir": 0, "adj": 1, "cluster": 2}


@pytest.fixture(scope="module")
def bams(tmp_path_factory):
    d = tmp_path_factory.mktemp("stats")
    out = {}
    for name, (header, recs) in (("tags", tag_model.tagged_bam(5, 60, 14)),
                                 ("long", bamio.synthetic_bam(6, 50, 14, umi_len=24)),
                                 ("genes", gm.gene_bam(21)[:2]),
                                 ("paired", tag_model.tagged_bam(7, 40, 10, paired=True))):
        src = str(d / (name + ".bam"))
        tag_model.write_bam(src, header, recs)
        out[name] = dict(src=src, recs=recs)
    return out


def run(src, dst, flags):
    r = subprocess.run([CLI, "-i", src, "-o", dst] + flags, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    return bamio.bgzf_decompress(open(dst, "rb").read()), re.sub(r"\d+\.\d+", "#", r.stderr)


def collapse(st, k=1, algo="dir"):
    keys = np.ascontiguousarray(st["keys"], np.uint64)
    if algo == "cluster":  # (the oracle restates the reference, which has no such mode: tests/cluster_model.py defines it)
        return cluster_model.batch_of_keys(keys, st["nmask"], st["bucket_off"].astype(np.int64), k)
    call = orc.dedup_batch_wide if keys.ndim == 2 else orc.dedup_batch
    kept, root, _ = call(keys, st["nmask"], st["freq"], st["bucket_off"], max(st["umi_len"], 1), k, 0.5, ALGO[algo])
    return kept, root


def check_run(tmp_path, bam, flags, st, algo="dir", seed=None, kept_root=None):
    """one run with the flag against the model's files, and against the same run without it"""
    (tmp_path / "with").mkdir()
    (tmp_path / "without").mkdir()
    prefix = str(tmp_path / "with" / "qc")
    extra = ["--output-stats", prefix] + (["--output-stats-seed", str(seed)] if seed is not None else [])
    got_bam, got_log = run(bam["src"], str(tmp_path / "with" / "o.bam"), flags + extra)
    exp_bam, exp_log = run(bam["src"], str(tmp_path / "without" / "o.bam"), flags)
    assert got_bam == exp_bam and len(got_bam) > 0
    assert got_log == exp_log
    kept, root = kept_root if kept_root is not None else collapse(st, algo=algo)
    keys = np.ascontiguousarray(st["keys"], np.uint64).reshape(-1)
    exp = sm.stats_files(keys, st["freq"], kept, root, st["bucket_off"], st["umi_len"], algo, seed=seed or 0)
    files = [open(prefix + n, "rb").read().decode() for n in NAMES]
    for name, a, b in zip(NAMES, files, exp):
        assert a == b, name
    assert len(files[2].splitlines()) > 10 and len(files[0].splitlines()) > 2
    return files, got_log


@pytest.mark.parametrize("which", ["tags", "long"])
@pytest.mark.parametrize("flags,algo", [([], "dir"), (["--algo", "adj"], "adj"), (["--algo", "cluster"], "cluster"),
                                        (["--tag"], "dir"), (["--stage", "gpu"], "dir"), (["--stage", "host"], "dir")],
                         ids=["plain", "adj", "cluster", "tag", "stage gpu", "stage host"])
def test_umis_in_the_name(tmp_path, bams, which, flags, algo):
    st, _ = tag_model.stage(bams[which]["recs"])
    assert st["umi_len"] == (12 if which == "tags" else 24)
    files, log = check_run(tmp_path, bams[which], flags, st, algo=algo)
    assert "N" in "".join(l.split("\t")[0] for l in files[2].splitlines()[1:])  # reads with N are counted as they are
    if flags in ([], ["--stage", "gpu"]):
        assert "staging (gpu)" in log  # (asking for root[] alone does not move the staging to the host)
    if flags in (["--tag"], ["--stage", "host"]):
        assert "staging (host)" in log


@pytest.mark.parametrize("which", ["tags", "long"])
def test_two_seeds(tmp_path, bams, which):
    st, _ = tag_model.stage(bams[which]["recs"])
    (tmp_path / "a").mkdir()
    (tmp_path / "b").mkdir()
    a, _ = check_run(tmp_path / "a", bams[which], [], st, seed=1)
    b, _ = check_run(tmp_path / "b", bams[which], [], st, seed=2 ** 64 - 1)
    assert a[0] == b[0] and a[2] == b[2] and a[1] != b[1]
    col = lambda text, j: [l.split("\t")[j] for l in text.splitlines()[1:]]
    assert col(a[1], 1) == col(b[1], 1) and col(a[1], 3) == col(b[1], 3) and col(a[1], 2) != col(b[1], 2)


def test_umi_tag_per_cell(tmp_path, bams):
    st, _ = tag_model.stage(bams["tags"]["recs"], umi_tag="UB", per_cell=True)
    check_run(tmp_path, bams["tags"], ["--umi-tag", "UB", "--per-cell"], st)


def test_per_gene_count_matrix(tmp_path, bams):
    st = gm.stage(bams["genes"]["recs"], per_cell=True)
    check_run(tmp_path, bams["genes"], ["--umi-tag", "UB", "--per-cell", "--per-gene", "--count-matrix", str(tmp_path / "m")], st)


def test_umi_whitelist(tmp_path, bams):
    """half of the file's UMIs are listed, none may be corrected: the reads with a listed UMI are what is counted"""
    recs = bams["tags"]["recs"]
    umis = sorted({tag_model.parse_aux(r)["UB"][1] for r in recs if "UB" in tag_model.parse_aux(r)})
    listed = {u for j, u in enumerate(u for u in umis if b"N" not in u) if j % 2 == 0}
    lst = str(tmp_path / "kit.txt")
    with open(lst, "w") as f:
        f.write("\n".join(u.decode() for u in sorted(listed)) + "\n")
    st, _ = tag_model.stage([r for r in recs if tag_model.parse_aux(r).get("UB", (None, None))[1] in listed], umi_tag="UB")
    files, log = check_run(tmp_path, bams["tags"], ["--umi-tag", "UB", "--umi-whitelist", lst, "--whitelist-max-mismatches", "0"], st)
    assert "uncorrectable UMI" in log
    assert {l.split("\t")[0].encode() for l in files[2].splitlines()[1:]} <= listed


def test_distance_edit_k2(tmp_path, bams):
    import edit_model as em
    st, _ = tag_model.stage(bams["tags"]["recs"])
    umis = em.decode(st["keys"], st["umi_len"])
    off = st["bucket_off"].astype(np.int64)
    buckets = [(umis[off[b]:off[b + 1]], [int(f) for f in st["freq"][off[b]:off[b + 1]]]) for b in range(len(off) - 1)]
    check_run(tmp_path, bams["tags"], ["--distance", "edit", "-k", "2"], st, kept_root=em.model_batch(buckets, 2, 0.5, 0, 0))


def test_paired(tmp_path, bams):
    st, _ = tag_model.stage(bams["paired"]["recs"], paired=True)
    _, log = check_run(tmp_path, bams["paired"], ["--paired"], st)
    assert "staging (host)" in log
