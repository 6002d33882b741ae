"""`umicollapse --algo cluster`, the parts that need no GPU: the flag is taken in bam and fastq mode (the staging
runs and the dump is written), near misses and the reference's `cc` stay refused, the help names it."""
import os
import subprocess

import pytest

import bamio
from umi_collapse_rs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cluster_cli")
    header, recs = bamio.synthetic_bam(3, 20, 10, extras=False)
    bam = str(d / "in.bam")
    with open(bam, "wb") as f:
        f.write(bamio.bgzf_compress(header + b"".join(recs)))
    seqs, quals = synth.fastq_reads(5, 200, 40, lengths=[30, 50], err=0.01)
    fq = str(d / "in.fastq")
    with open(fq, "wb") as f:
        f.write(synth.fastq_text(seqs, quals))
    return d, bam, fq


@pytest.mark.parametrize("mode", ["bam", "fastq"])
def test_algo_cluster_is_accepted(inputs, mode):
    d, bam, fq = inputs
    dump = str(d / ("stage_%s.bin" % mode))
    base = ["-i", bam] if mode == "bam" else ["-m", "fastq", "-i", fq]
    r = run(base + ["-o", str(d / "unused"), "--algo", "cluster", "--dump-staging", dump])
    assert r.returncode == 0, r.stderr
    assert os.path.getsize(dump) > 32
    # the staging does not depend on the algorithm
    dump_dir = str(d / ("stage_dir_%s.bin" % mode))
    assert run(base + ["-o", str(d / "unused"), "--algo", "dir", "--dump-staging", dump_dir]).returncode == 0
    assert open(dump, "rb").read() == open(dump_dir, "rb").read()
    # -p is accepted beside it
    assert run(base + ["-o", str(d / "unused"), "--algo", "cluster", "-p", "0.1", "--dump-staging", dump]).returncode == 0


@pytest.mark.parametrize("mode", ["bam", "fastq"])
@pytest.mark.parametrize("name", ["clusters", "cc", "Cluster", ""])
def test_other_spellings_are_refused(inputs, mode, name):
    d, bam, fq = inputs
    base = ["-i", bam] if mode == "bam" else ["-m", "fastq", "-i", fq]
    r = run(base + ["-o", str(d / "unused"), "--algo", name, "--dump-staging", str(d / "never.bin")])
    assert r.returncode != 0
    assert "Invalid algorithm combination" in r.stderr
    assert not os.path.exists(str(d / "never.bin"))


def test_help_names_cluster():
    r = run(["--help"])
    assert r.returncode == 0
    assert "adj, dir or cluster" in r.stdout and "-p plays no part" in r.stdout
