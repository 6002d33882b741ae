"""umicollapse --algo cluster end to end, in every mode that takes --algo.  Expected records: the models of the
flags' own tests with their collapse at percentage = inf, algo "dir" -- the oracle's directional mode, which
equals the connected components while freq < 2^31 - 1 (tests/test_cluster_model_cpu.py) -- or with the collapse
replaced by tests/cluster_model.py where the model takes one."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import bam_consensus_model as bm
import bamio
import cluster_model as clm
import consensus_model as cons
import edit_model as em
import gene_model as gm
import seq_model as sm
import tag_model
from umi_collapse_rs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
INF = float("inf")
FILES = ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx")


def run_cli(tmp_path, header, recs, extra, name="out.bam"):
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / name)
    if not os.path.exists(src):
        tag_model.write_bam(src, header, recs)
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--algo", "cluster"] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stream = bamio.bgzf_decompress(open(dst, "rb").read())
    return stream, bamio.split_records(stream)[1], r.stderr


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def model_kept(st, k=1):
    """the cluster model's mask over a staged dict (one-word keys)"""
    return clm.batch_of_keys(st["keys"], st["nmask"], st["bucket_off"], k)


@pytest.fixture(scope="module")
def tagged():
    return tag_model.tagged_bam(31, 150, 20, n_cells=5, err=0.04)


def test_plain_and_percentage_plays_no_part(tmp_path, tagged):
    """--algo cluster by itself, on the GPU's staging and the host's; -p beside it changes no byte.  The file is one
    on which the components differ from the directional result at the default -p."""
    header, recs = tagged
    exp, st, n_kept = tag_model.expected_output(recs, p=INF)
    kept, _ = model_kept(st)
    assert int(kept.sum()) == n_kept
    exp_dir, _, n_dir = tag_model.expected_output(recs)
    assert n_dir > n_kept  # (a run that took the flag for `dir` would not pass)
    one, got, log = run_cli(tmp_path, header, recs, [])
    assert got == exp
    assert int(line(log, "Number of reads after deduplicating")) == n_kept
    for extra in (["-p", "0.1"], ["-p", "0"], ["--stage", "host"], ["--stage", "gpu", "--num-threads", "3"]):
        other, _, _ = run_cli(tmp_path, header, recs, extra, "other.bam")
        assert other == one, extra


def test_two_pass_equals_one_pass(tmp_path, tagged):
    header, recs = tagged
    one, _, log1 = run_cli(tmp_path, header, recs, [], "one.bam")
    two, _, log2 = run_cli(tmp_path, header, recs, ["--two-pass", "--two-pass-window", "64"], "two.bam")
    assert one == two
    assert int(line(log2, "two-pass").split()[0]) > 1
    assert line(log1, "Number of reads after deduplicating") == line(log2, "Number of reads after deduplicating")


def test_tag(tmp_path, tagged):
    """--tag: MI / cs per component."""
    header, recs = tagged
    exp, _, groups = tag_model.expected_tagged_output(recs, p=INF)
    _, got, log = run_cli(tmp_path, header, recs, ["--tag"])
    assert got == exp
    assert int(line(log, "Number of groups of reads")) == groups
    assert tag_model.expected_tagged_output(recs)[2] > groups


def test_paired(tmp_path):
    header, recs = tag_model.tagged_bam(33, 60, 12, n_cells=5, paired=True, err=0.04)
    exp, _, _ = tag_model.expected_output(recs, p=INF, umi_tag="RX", per_cell=True, paired=True)
    _, got, _ = run_cli(tmp_path, header, recs, ["--paired", "--umi-tag", "RX", "--per-cell"])
    assert got == exp
    assert any(bamio.parse_record(r)["flag"] & 0x80 for r in got)


@pytest.mark.parametrize("extra", [[], ["--devices", "0,0"], ["--stage", "host"]])
def test_umi_tag_per_cell(tmp_path, tagged, extra):
    header, recs = tagged
    exp, st, n_kept = tag_model.expected_output(recs, p=INF, umi_tag="UB", per_cell=True)
    assert int(model_kept(st)[0].sum()) == n_kept
    _, got, log = run_cli(tmp_path, header, recs, ["--umi-tag", "UB", "--per-cell"] + extra)
    assert got == exp
    assert int(line(log, "Number of reads after deduplicating")) == n_kept


def test_count_matrix(tmp_path):
    """--per-cell --per-gene --count-matrix: the four files of gene_model with its collapse replaced by the
    cluster model."""
    header, recs, cells = gm.gene_bam(35, err=0.05)
    src, mdir = str(tmp_path / "in.bam"), str(tmp_path / "matrix")
    tag_model.write_bam(src, header, recs)
    exp, st, kept = gm.expected_output(recs, per_cell=True, dedup=lambda st, k, p, algo: model_kept(st, k)[0])
    assert 0 < kept.sum() < len(kept)
    r = subprocess.run([CLI, "-i", src, "-o", str(tmp_path / "out.bam"), "--algo", "cluster", "--umi-tag", "UB", "--per-cell",
                        "--per-gene", "--count-matrix", mdir], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    got = bamio.split_records(bamio.bgzf_decompress(open(str(tmp_path / "out.bam"), "rb").read()))[1]
    assert got == exp
    want = gm.expected_matrix(st, kept)
    for f in FILES:
        assert open(os.path.join(mdir, f), "rb").read() == want[f], f


def test_distance_edit(tmp_path):
    """--distance edit -k 2: the components of the edit graph (tests/edit_model.py's matrix)."""
    rng = np.random.default_rng(2036)
    recs, i = [], 0
    for p in range(40):
        for umi in em.shifted_reads(rng, 8, 12, mean_copies=4.0, n_frac=0.003):
            recs.append(bamio.make_record("r%d_%s" % (i, umi), 0, 0, 1000 + 10 * p, int(rng.integers(0, 61)),
                                          [("M", 50)], 50, rng.integers(20, 41, 50).astype(np.uint8).tobytes()))
            i += 1
    header = bamio.make_header([("chr1", 10_000_000)])
    st, pre = bamio.stage_like_reference(recs, merge="mapqual")
    umis = em.decode(st["keys"], 12)
    off = st["bucket_off"].astype(np.int64)
    mats = [em.edit_matrix(umis[off[b]:off[b + 1]]) for b in range(len(off) - 1)]
    kept, _ = clm.batch(mats, off, 2)
    hkept, _ = clm.batch([em.hamming_matrix(umis[off[b]:off[b + 1]]) for b in range(len(off) - 1)], off, 2)
    assert hkept.sum() > kept.sum()  # (shifts that only the edit distance joins)
    exp = [recs[j] for j in pre] + [recs[int(st["rep"][j])] for j in np.nonzero(kept)[0]]
    _, got, log = run_cli(tmp_path, header, recs, ["--distance", "edit", "-k", "2"])
    assert got == exp and "UMI distance: edit" in log


def test_call_consensus(tmp_path):
    """--call-consensus: the voters are the component's reads that line up."""
    header, recs = bm.synthetic_bam(37, err=0.03)
    exp, counts = bm.expected_output(recs, p=INF)
    _, counts_dir = bm.expected_output(recs)
    assert counts_dir["kept"] > counts["kept"] and counts["changed"] >= 20
    _, got, log = run_cli(tmp_path, header, recs, ["--call-consensus"])
    assert len(got) == len(exp)
    for j, (g, e) in enumerate(zip(got, exp)):
        assert g == e, j
    assert int(line(log, "Number of reads after deduplicating")) == counts["kept"]


def fastq_workload():
    seqs, quals = synth.fastq_reads(43, 3000, 700, lengths=[18, 60, 100, 150], err=0.015, n_frac=0.002)
    names = [b"r%d extra words" % i for i in range(len(seqs))]
    return seqs, quals, names


def fastq_model(seqs, quals, k):
    """staging, and the cluster model's (kept, root) over the per-word distance of seq_model's keys"""
    ent, off, blen = sm.stage(seqs, quals, 1)
    kept, root = np.zeros(len(ent), bool), np.arange(len(ent))
    for b, L in enumerate(blen):
        lo, hi = off[b], off[b + 1]
        keys, nm = sm.encode([e[0] for e in ent[lo:hi]], max(1, sm.words(L)))
        r = clm.components(clm.word_distance(keys, nm), k)
        root[lo:hi] = r.astype(np.int64) + lo
        kept[lo:hi] = clm.kept_of(r).astype(bool)
    return ent, off, blen, kept, root


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_fastq(tmp_path, stage):
    """-m fastq --algo cluster, plain, with --tag and with --consensus, against seq_model / consensus_model with the
    cluster model's roots."""
    seqs, quals, names = fastq_workload()
    src = tmp_path / "in.fq.gz"
    src.write_bytes(gzip.compress(synth.fastq_text(seqs, quals, names)))
    ent, off, blen, kept, root = fastq_model(seqs, quals, 2)
    dkept, _ = sm.dedup(ent, off, blen, 2, 0)
    assert dkept.sum() > kept.sum()
    base = [CLI, "-m", "fastq", "-i", str(src), "-k", "2", "--algo", "cluster", "--stage", stage]
    for flags, want in (([], sm.output(seqs, quals, names, ent, off, kept, root)),
                        (["--tag"], sm.output(seqs, quals, names, ent, off, kept, root, tag=True)),
                        (["--consensus"], cons.output(seqs, quals, names, ent, kept, root)[0])):
        dst = tmp_path / ("out%s.fq" % "".join(flags))
        r = subprocess.run(base + ["-o", str(dst)] + flags, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        assert dst.read_bytes() == want, flags
