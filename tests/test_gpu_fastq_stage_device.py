"""umicollapse -m fastq --stage gpu on a GPU other than the first: the CLI's device buffers must be on the
context's device (tests/test_fastq_stage_device_cpu.py checks the order of the calls without a GPU)."""
import os
import subprocess

import pytest

from umi_collapse_rs_amd import synth

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def n_devices():
    import torch
    return torch.cuda.device_count()


@pytest.mark.parametrize("tag", [False, True])
def test_second_device_matches_host_staging(tmp_path, tag):
    if n_devices() < 2:
        pytest.skip("one GPU visible")
    seqs, quals = synth.fastq_reads(44, 3000, 700, lengths=[30, 100, 150], err=0.01, n_frac=0.002)
    src = tmp_path / "in.fq"
    src.write_bytes(synth.fastq_text(seqs, quals))
    outs = {}
    for stage in ("gpu", "host"):
        dst = tmp_path / (stage + ".fq")
        r = subprocess.run([CLI, "-m", "fastq", "-i", str(src), "-o", str(dst), "-k", "2", "--stage", stage,
                            "--device", "1"] + (["--tag"] if tag else []), capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        outs[stage] = dst.read_bytes()
    assert outs["gpu"] == outs["host"] and outs["gpu"]
