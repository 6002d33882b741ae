"""umicollapse -m fastq --consensus end to end on the MI355X: the output byte for byte (after
decompression) against the model (tests/consensus_model.py), with the reads staged on the device and on
the host, --consensus-min-reads, and the run without the flag unchanged."""
import gzip
import os
import subprocess

import pytest

import consensus_model as cm
import seq_model as sm
from umi_collapse_rs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=600)


def workload():
    seqs, quals = synth.fastq_reads(41, 4000, 900, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    names = [b"r%d extra words" % i for i in range(len(seqs))]
    return seqs, quals, names


CASES = [  # algo, merge, -u, input .gz, output .gz
    ("dir", "avgqual", 0, False, False),
    ("dir", "any", 5, True, True),
    ("adj", "avgqual", 0, True, False),
    ("adj", "any", 3, False, True),
    ("dir", "avgqual", 2, True, False),
]


@pytest.mark.parametrize("algo,merge,trim,gz_in,gz_out", CASES)
def test_cli_consensus(tmp_path, algo, merge, trim, gz_in, gz_out):
    seqs, quals, names = workload()
    text = synth.fastq_text(seqs, quals, names)
    src = tmp_path / ("in.fq.gz" if gz_in else "in.fq")
    src.write_bytes(gzip.compress(text) if gz_in else text)
    want, dropped = cm.expected_cli(seqs, quals, names, 2, 0 if algo == "dir" else 1, 1 if merge == "avgqual" else 0, trim)
    assert dropped == 0 and want
    if algo == "dir":  # the consensus is not the kept read with a longer header
        plain = sm.output(seqs, quals, names, *staged_and_collapsed(seqs, quals, algo, merge), trim=trim)
        assert want.replace(b" cluster_size=", b"\0").count(b"\n") == plain.count(b"\n")
        assert [l for l in want.split(b"\n")[1::4]] != [l for l in plain.split(b"\n")[1::4]]
    outs = {}
    for stage in ("gpu", "host", "auto"):
        dst = tmp_path / (stage + (".fq.gz" if gz_out else ".fq"))
        r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", "2", "--algo", algo, "--merge", merge, "-u", str(trim),
                 "--consensus", "--stage", stage])
        assert r.returncode == 0, r.stderr
        assert "Number of clusters below --consensus-min-reads: 0\n" in r.stderr
        got = dst.read_bytes()
        outs[stage] = gzip.decompress(got) if gz_out else got
    assert outs["gpu"] == want
    assert outs["host"] == want
    assert outs["auto"] == want


def staged_and_collapsed(seqs, quals, algo, merge):
    ent, off, blen = sm.stage(seqs, quals, 1 if merge == "avgqual" else 0)
    kept, root = sm.dedup(ent, off, blen, 2, 0 if algo == "dir" else 1)
    return ent, off, kept, root


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_min_reads(tmp_path, stage):
    seqs, quals, names = workload()
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    want, dropped = cm.expected_cli(seqs, quals, names, 2, 0, 1, 0, min_reads=3)
    assert dropped > 100 and want.count(b"\n") > 400
    dst = tmp_path / "out.fq"
    r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", "2", "--consensus", "--consensus-min-reads", "3",
             "--stage", stage])
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == want  # the records left, in the order of the file
    assert "Number of clusters below --consensus-min-reads: %d\n" % dropped in r.stderr


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_without_the_flag_nothing_changes(tmp_path, stage):
    seqs, quals, names = workload()
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    dst = tmp_path / "out.fq"
    r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "-k", "2", "--stage", stage])
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == sm.output(seqs, quals, names, *staged_and_collapsed(seqs, quals, "dir", "avgqual"))
    assert "consensus" not in r.stderr


def test_empty_reads_and_an_empty_file(tmp_path):
    seqs = [b"", b"ACGTACGTAC", b"", b"ACGTACGTAA", b"ACGTACGTAC"]
    quals = [b"", b"IIIIIIIIII", b"", b"!!!!!!!!!!", b"##########"]
    names = [b"e%d" % i for i in range(len(seqs))]
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals, names))
    want, _ = cm.expected_cli(seqs, quals, names, 1, 0, 1)
    assert want.count(b"@e0 cluster_size=2\n\n+\n\n") == 1  # the two empty reads: one empty consensus
    for stage in ("gpu", "host"):
        dst = tmp_path / (stage + ".fq")
        r = run(["-m", "fastq", "-i", str(src), "-o", str(dst), "--consensus", "--stage", stage])
        assert r.returncode == 0, r.stderr
        assert dst.read_bytes() == want
    empty = tmp_path / "empty.fq"
    empty.write_bytes(b"")
    dst = tmp_path / "none.fq"
    r = run(["-m", "fastq", "-i", str(empty), "-o", str(dst), "--consensus"])
    assert r.returncode == 0, r.stderr
    assert dst.read_bytes() == b""
