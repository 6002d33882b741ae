"""umicollapse --distance edit end to end: a synthetic BAM whose UMIs carry shifts, the decompressed output
against the reference's staging (tests/bamio.py) followed by the Levenshtein model (tests/edit_model.py)."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bamio
import edit_model as em

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
L = 12


@pytest.fixture(scope="module")
def bam():
    """About 40 positions x 30 reads, coordinate-sorted; every position's UMIs from the shifted molecule model."""
    rng = np.random.default_rng(2026)
    recs, i = [], 0
    for p in range(40):
        for umi in em.shifted_reads(rng, 8, L, mean_copies=4.0, n_frac=0.003):
            recs.append(bamio.make_record("r%d_%s" % (i, umi), 0, 0, 1000 + 10 * p, int(rng.integers(0, 61)),
                                          [("M", 50)], 50, rng.integers(20, 41, 50).astype(np.uint8).tobytes()))
            i += 1
    return bamio.make_header([("chr1", 10_000_000)]), recs


def staged_buckets(st):
    umis = em.decode(st["keys"], L)
    off = st["bucket_off"].astype(np.int64)
    return [(umis[off[b]:off[b + 1]], [int(f) for f in st["freq"][off[b]:off[b + 1]]]) for b in range(len(off) - 1)]


def expected(recs, k, algo, **kw):
    st, pre = bamio.stage_like_reference(recs, **kw)
    buckets = staged_buckets(st)
    kept, root = em.model_batch(buckets, k, 0.5, 0 if algo == "dir" else 1, 0)
    return [recs[i] for i in pre] + [recs[int(st["rep"][i])] for i in np.nonzero(kept)[0]], st, kept, root, buckets


def run_cli(tmp_path, header, recs, extra):
    tmp_path.mkdir(exist_ok=True)
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / "out.bam")
    with open(src, "wb") as f:
        f.write(bamio.bgzf_compress(header + b"".join(recs)))
    r = subprocess.run([CLI, "-i", src, "-o", dst] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    out_header, out_recs = bamio.split_records(bamio.bgzf_decompress(open(dst, "rb").read()))
    return out_header, out_recs, r.stderr


def test_the_file_holds_shifts(bam):
    _, recs = bam
    _, _, _, _, buckets = expected(recs, 2, "dir", merge="mapqual")
    assert 800 <= len(recs) <= 2000 and len(buckets) == 40
    assert sum(em.shift_only_pairs(u, 2) for u, _ in buckets) > 0


@pytest.mark.parametrize("stage", ["gpu", "host"])
@pytest.mark.parametrize("algo", ["dir", "adj"])
def test_edit_distance_end_to_end(tmp_path, bam, algo, stage):
    header, recs = bam
    exp, st, kept, _, _ = expected(recs, 2, algo, merge="mapqual")
    oh, orecs, log = run_cli(tmp_path, header, recs, ["--distance", "edit", "-k", "2", "--algo", algo, "--stage", stage])
    assert oh == header and orecs == exp
    assert "UMI distance: edit" in log and "staging (%s)" % stage in log
    assert "Number of reads after deduplicating: %d" % int(kept.sum()) in log


def test_two_pass_writes_the_same_stream(tmp_path, bam):
    header, recs = bam
    exp, _, _, _, _ = expected(recs, 2, "dir", merge="mapqual")
    _, one, _ = run_cli(tmp_path / "one", header, recs, ["--distance", "edit", "-k", "2"])
    _, two, log = run_cli(tmp_path / "two", header, recs, ["--distance", "edit", "-k", "2", "--two-pass", "--two-pass-window", "300"])
    assert one == exp and two == exp
    assert "UMI distance: edit" in log and "two-pass:" in log


def test_tag_follows_the_models_roots(tmp_path, bam):
    header, recs = bam
    _, st, kept, root, _ = expected(recs, 2, "dir", merge="mapqual")
    cluster_id = np.cumsum(kept) - 1
    cluster_reads = np.zeros(len(kept), np.int64)
    np.add.at(cluster_reads, root.astype(np.int64), st["freq"])
    index = {}
    off = st["bucket_off"].astype(np.int64)
    for b in range(len(off) - 1):
        for e in range(off[b], off[b + 1]):
            index[(b, int(st["keys"][e]))] = e
    exp = []
    for ri, b, umi in st["reads"]:
        key, _ = em.encode([umi.decode()])
        e = index[(b, int(key[0]))]
        r = int(root[e])
        tags = b"".join(t + b"i" + struct.pack("<i", int(v)) for t, v in
                        ((b"MI", cluster_id[r]), (b"cs", cluster_reads[r]), (b"su", st["freq"][e])))
        body = recs[ri][4:] + tags
        exp.append(struct.pack("<i", len(body)) + body)
    oh, orecs, log = run_cli(tmp_path, header, recs, ["--distance", "edit", "-k", "2", "--tag"])
    assert orecs == exp
    assert "Number of groups of reads: %d" % int(kept.sum()) in log and "UMI distance: edit" in log


def test_hamming_is_the_default_and_differs(tmp_path, bam):
    header, recs = bam
    _, plain, log0 = run_cli(tmp_path / "plain", header, recs, ["-k", "2"])
    _, ham, log1 = run_cli(tmp_path / "ham", header, recs, ["-k", "2", "--distance", "hamming"])
    _, edit, log2 = run_cli(tmp_path / "edit", header, recs, ["-k", "2", "--distance", "edit"])
    exp, _ = bamio.expected_output(recs, k=2, merge="mapqual")
    assert plain == exp and ham == exp
    assert edit != plain and len(edit) < len(plain)
    assert "UMI distance" not in log0 and "UMI distance" not in log1 and "UMI distance: edit" in log2


def test_k1_is_the_hamming_result(tmp_path, bam):
    header, recs = bam
    _, plain, _ = run_cli(tmp_path / "plain", header, recs, ["-k", "1"])
    _, edit, _ = run_cli(tmp_path / "edit", header, recs, ["-k", "1", "--distance", "edit"])
    assert edit == plain


def test_a_long_umi_in_the_file_is_refused(tmp_path):
    recs = [bamio.make_record("r0_" + "ACGT" * 6, 0, 0, 1000, 60, [("M", 50)], 50, bytes([30] * 50))]
    src = str(tmp_path / "in.bam")
    with open(src, "wb") as f:
        f.write(bamio.bgzf_compress(bamio.make_header([("chr1", 10_000)]) + b"".join(recs)))
    for extra in ([], ["--two-pass"]):
        r = subprocess.run([CLI, "-i", src, "-o", str(tmp_path / "out.bam"), "--distance", "edit"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 101 and "at most 21 bases" in r.stderr, r.stderr
