"""Whole-read staging (umi_stage_seqs, umicollapse -m fastq --stage gpu), the parts that need no GPU:
the identity that lets the device compute the average quality with an integer division, and the
CLI's refusals, which come before any GPU is needed."""
import os
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def test_avg_qual_integer_division_is_the_f32_quotient():
    """(int)((float)s / (float)len) == s / len (C division, truncation toward zero) for every len in
    1..256 and every sum of len quality bytes, s in [-33 len, 222 len]."""
    for L in range(1, 257):
        s = np.arange(-33 * L, 222 * L + 1, dtype=np.int64)
        f32 = (s.astype(np.float32) / np.float32(L)).astype(np.int64)  # astype truncates toward zero
        c = np.sign(s) * (np.abs(s) // L)
        bad = np.flatnonzero(f32 != c)
        assert bad.size == 0, (L, s[bad[:5]])


@pytest.fixture(scope="module")
def cli():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])
    return CLI


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300,
                          env=dict(os.environ, HIP_VISIBLE_DEVICES="-1"))


@pytest.mark.parametrize("flags", [["--stage", "gpu", "--dump-staging", "d.bin"],
                                   ["--stage", "gpu", "--devices", "0,1"],
                                   ["--stage", "gpu", "--two-pass"],
                                   ["--stage", "gpu", "--paired"],
                                   ["--stage", "gpu", "--algo", "cc"],
                                   ["--stage", "device"]])
def test_refused_before_the_gpu(cli, tmp_path, flags):
    src = tmp_path / "a.fq"
    src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    flags = [str(tmp_path / f) if f.endswith(".bin") else f for f in flags]
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq")] + flags)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert r.stderr.strip() and "hip" not in r.stderr.lower()
    assert not (tmp_path / "o.fq").exists()
    if "--dump-staging" in flags:
        assert "--dump-staging" in r.stderr
