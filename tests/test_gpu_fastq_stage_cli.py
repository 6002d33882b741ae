"""umicollapse -m fastq --stage gpu against --stage host on the MI355X: the same decompressed output
(and the model's), the same summary lines but the phases line, and the same status and message for
malformed input, whichever record comes first."""
import gzip
import os
import subprocess

import pytest

import seq_model as sm
from umi_collapse_rs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")

CASES = [  # algo, merge, -u, --tag, input .gz, output .gz (the matrix of test_gpu_fastq_cli.py)
    ("dir", "avgqual", 0, False, False, False),
    ("dir", "any", 5, False, True, True),
    ("adj", "avgqual", 0, False, True, False),
    ("adj", "any", 3, True, False, True),
    ("dir", "avgqual", 2, True, True, False),
]


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600)


def summary(stderr):
    """the summary lines without those that carry times"""
    return [l for l in stderr.splitlines() if "seconds" not in l and not l.startswith("phases:")]


@pytest.fixture(scope="module")
def reads():
    seqs, quals = synth.fastq_reads(43, 4000, 900, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    names = [b"r%d extra words" % i for i in range(len(seqs))]
    return seqs, quals, names


@pytest.mark.parametrize("k", [0, 1, 2])
@pytest.mark.parametrize("algo,merge,trim,tag,gz_in,gz_out", CASES)
def test_gpu_stage_matches_host_stage(tmp_path, reads, k, algo, merge, trim, tag, gz_in, gz_out):
    seqs, quals, names = reads
    text = synth.fastq_text(seqs, quals, names)
    src = tmp_path / ("in.fq.gz" if gz_in else "in.fq")
    src.write_bytes(gzip.compress(text) if gz_in else text)
    outs, sums = {}, {}
    for stage in ("gpu", "host"):
        dst = tmp_path / (stage + (".fq.gz" if gz_out else ".fq"))
        args = ["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", str(k), "--algo", algo, "--merge", merge,
                "-u", str(trim), "--stage", stage] + (["--tag"] if tag else [])
        r = run(args)
        assert r.returncode == 0, r.stderr
        assert "staging (%s)" % stage in r.stderr
        got = dst.read_bytes()
        outs[stage] = gzip.decompress(got) if gz_out else got
        sums[stage] = summary(r.stderr)
    assert outs["gpu"] == outs["host"]
    assert sums["gpu"] == sums["host"]
    ent, off, blen = sm.stage(seqs, quals, 1 if merge == "avgqual" else 0)
    kept, root = sm.dedup(ent, off, blen, k, 0 if algo == "dir" else 1)
    assert outs["gpu"] == sm.output(seqs, quals, names, ent, off, kept, root, trim=trim, tag=tag)


def test_auto_stages_on_the_gpu(tmp_path, reads):
    seqs, quals, names = reads
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq")])
    assert r.returncode == 0 and "staging (gpu)" in r.stderr, r.stderr
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--dump-staging", str(tmp_path / "d.bin")])
    assert r.returncode == 0, r.stderr  # (auto with --dump-staging: the host staging, no GPU)


def rec(name, seq, qual=None):
    return b"@" + name + b"\n" + seq + b"\n+\n" + (qual if qual is not None else b"I" * len(seq)) + b"\n"


GOOD = b"".join(rec(b"g%d" % i, b"ACGTACGTAC"[: 4 + i % 6]) for i in range(40))
MALFORMED = {
    "char": GOOD + rec(b"x", b"ACGXT") + GOOD,
    "char_first": rec(b"x", b"NNNNa") + GOOD,
    "too_long": GOOD + rec(b"x", b"A" * 257) + GOOD,
    "shorter_than_u": GOOD + rec(b"x", b"AC") + GOOD,
    "char_then_long": GOOD + rec(b"x", b"ACG.") + GOOD + rec(b"y", b"C" * 300) + GOOD,
    "long_then_char": GOOD + rec(b"y", b"C" * 300) + GOOD + rec(b"x", b"ACG.") + GOOD,
    "short_then_char": GOOD + rec(b"y", b"A") + rec(b"x", b"ACG.") + GOOD,
    "char_then_short": GOOD + rec(b"x", b"ACGTTTT-") + rec(b"y", b"A") + GOOD,
}


@pytest.mark.parametrize("case", sorted(MALFORMED))
def test_malformed_same_message(tmp_path, case):
    src = tmp_path / "bad.fq"
    src.write_bytes(MALFORMED[case])
    res = {}
    for stage in ("gpu", "host"):
        r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / (stage + ".fq")), "-u", "3", "--stage", stage])
        res[stage] = (r.returncode, r.stderr)
    assert res["gpu"] == res["host"]
    assert res["gpu"][0] == 101 and "FASTQ record" in res["gpu"][1]


def test_empty_input(tmp_path):
    src = tmp_path / "empty.fq"
    src.write_bytes(b"")
    outs = {}
    for stage in ("gpu", "host"):
        dst = tmp_path / (stage + ".fq")
        r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "--stage", stage])
        assert r.returncode == 0, r.stderr
        outs[stage] = (dst.read_bytes(), summary(r.stderr))
    assert outs["gpu"] == outs["host"] and outs["gpu"][0] == b""
