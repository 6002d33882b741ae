"""umicollapse --two-pass, the parts that need no GPU: what it refuses before any device work."""
import os
import subprocess

import pytest

import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


@pytest.fixture
def bam(tmp_path):
    header, recs = bamio.synthetic_bam(3, 20, 10)
    path = tmp_path / "in.bam"
    with open(str(path), "wb") as f:
        f.write(bamio.bgzf_compress(header + b"".join(recs)))
    return str(path)


def test_input_must_be_a_regular_file(tmp_path):
    fifo = str(tmp_path / "in.fifo")
    os.mkfifo(fifo)
    r = run(["-i", fifo, "-o", str(tmp_path / "o.bam"), "--two-pass"])  # (must not block on the FIFO)
    assert r.returncode != 0
    assert "regular file" in r.stderr
    r = run(["-i", str(tmp_path), "-o", str(tmp_path / "o.bam"), "--two-pass"])
    assert r.returncode != 0 and "regular file" in r.stderr


@pytest.mark.parametrize("value", ["0", "-5", "x", "12k"])
def test_window_below_one_is_refused(tmp_path, bam, value):
    r = run(["-i", bam, "-o", str(tmp_path / "o.bam"), "--two-pass", "--two-pass-window", value])
    assert r.returncode != 0
    assert "--two-pass-window" in r.stderr
    assert not os.path.exists(str(tmp_path / "o.bam"))


def test_tag_with_two_pass_is_refused(tmp_path, bam):
    r = run(["-i", bam, "-o", str(tmp_path / "o.bam"), "--tag", "--two-pass", "--two-pass-window", "64"])
    assert r.returncode != 0
    assert "Cannot track clusters with the two pass algorithm!" in r.stderr


def test_fastq_mode_still_refuses_two_pass(tmp_path):
    src = tmp_path / "in.fq"
    src.write_text("@r1\nACGT\n+\nIIII\n")
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--two-pass", "--two-pass-window", "64"])
    assert r.returncode != 0
    assert "--two-pass" in r.stderr


def test_two_pass_with_dump_staging_keeps_the_one_pass_staging(tmp_path, bam):
    """--dump-staging stops before the GPU, so this runs here: with --two-pass it writes the one-pass arrays"""
    outs = []
    for extra in ([], ["--two-pass", "--two-pass-window", "16"]):
        dump = str(tmp_path / ("d%d.bin" % len(outs)))
        r = run(["-i", bam, "-o", str(tmp_path / "o.bam"), "--dump-staging", dump] + extra)
        assert r.returncode == 0, r.stderr
        assert "two-pass:" not in r.stderr
        outs.append(open(dump, "rb").read())
    assert outs[0] == outs[1]


def test_two_pass_with_passthrough_keeps_the_one_pass_round_trip(tmp_path, bam):
    dst = str(tmp_path / "o.bam")
    r = run(["-i", bam, "-o", dst, "--passthrough", "--two-pass", "--two-pass-window", "16"])
    assert r.returncode == 0, r.stderr
    header, recs = bamio.synthetic_bam(3, 20, 10)
    assert bamio.bgzf_decompress(open(dst, "rb").read()) == header + b"".join(recs)


def test_help_describes_two_pass():
    r = run(["--help"])
    assert r.returncode == 0
    assert "--two-pass-window" in r.stdout
    assert "accepted and rejected" not in r.stdout
