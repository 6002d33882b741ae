"""umicollapse -m fastq end to end on the MI355X: output records byte for byte (after decompression)
against the model of the fastq mode's definition."""
import gzip
import os
import subprocess

import numpy as np
import pytest

import seq_model as sm
from umi_collapse_rs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600)


def expected(seqs, quals, names, k, algo, merge, trim=0, tag=False):
    ent, off, blen = sm.stage(seqs, quals, merge)
    kept, root = sm.dedup(ent, off, blen, k, algo)
    return sm.output(seqs, quals, names, ent, off, kept, root, trim=trim, tag=tag)


CASES = [  # algo, merge, -u, --tag, input .gz, output .gz
    ("dir", "avgqual", 0, False, False, False),
    ("dir", "any", 5, False, True, True),
    ("adj", "avgqual", 0, False, True, False),
    ("adj", "any", 3, True, False, True),
    ("dir", "avgqual", 2, True, True, False),
]


@pytest.mark.parametrize("algo,merge,trim,tag,gz_in,gz_out", CASES)
def test_cli_fastq(tmp_path, algo, merge, trim, tag, gz_in, gz_out):
    seqs, quals = synth.fastq_reads(41, 4000, 900, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    names = [b"r%d extra words" % i for i in range(len(seqs))]
    text = synth.fastq_text(seqs, quals, names)
    src = tmp_path / ("in.fq.gz" if gz_in else "in.fq")
    src.write_bytes(gzip.compress(text) if gz_in else text)
    dst = tmp_path / ("out.fq.gz" if gz_out else "out.fq")
    args = ["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", "2", "--algo", algo, "--merge", merge,
            "-u", str(trim)]
    if tag:
        args.append("--tag")
    r = run(args)
    assert r.returncode == 0, r.stderr
    got = dst.read_bytes()
    if gz_out:
        got = gzip.decompress(got)
    want = expected(seqs, quals, names, 2, 0 if algo == "dir" else 1, 1 if merge == "avgqual" else 0, trim, tag)
    assert got == want


def test_cli_fastq_empty_reads_and_one_length(tmp_path):
    seqs = [b"", b"ACGTACGTAC", b"", b"ACGTACGTAA", b"ACGTACGTAC"]
    quals = [b"", b"IIIIIIIIII", b"", b"!!!!!!!!!!", b"##########"]
    names = [b"e%d" % i for i in range(len(seqs))]
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    dst = tmp_path / "out.fq"
    r = run(["-m", "fastq", "-i", str(src), "-o", str(dst)])
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == expected(seqs, quals, names, 1, 0, 1)
    assert dst.read_bytes().count(b"@e0\n\n+\n\n") == 1  # one length-0 read survives


@pytest.mark.parametrize("k", [8, 31])
def test_cli_fastq_large_k(tmp_path, k):
    """-k 8 and -k 31 (reads of 256 bases are cut into 9 and 32 parts) against the model's output."""
    seqs, quals = synth.fastq_reads(43 + k, 5000, 600, lengths=[60, 150, 256], err=0.03, n_frac=0.002)
    names = [b"r%d" % i for i in range(len(seqs))]
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    dst = tmp_path / "out.fq"
    r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", str(k)])
    assert r.returncode == 0, r.stderr
    want = expected(seqs, quals, names, k, 0, 1)
    assert 0 < want.count(b"\n") // 4 < len({s for s in seqs})  # something collapses, something stays
    assert dst.read_bytes() == want
