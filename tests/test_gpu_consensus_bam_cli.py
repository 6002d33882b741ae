"""umicollapse --call-consensus end to end on the MI355X: the output record for record (after
decompression) against the model (tests/bam_consensus_model.py) over a file whose clusters hold voters
and non-voters, under the options it works with, --call-consensus-min-reads, and the run without the
flag unchanged."""
import os
import subprocess

import pytest

import bam_consensus_model as bm
import bamio
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module")
def bam(tmp_path_factory):
    header, recs = bm.synthetic_bam(3)
    src = str(tmp_path_factory.mktemp("bamcons") / "in.bam")
    tag_model.write_bam(src, header, recs)
    return src, header, recs


def run(src, dst, extra):
    r = subprocess.run([CLI, "-i", src, "-o", str(dst)] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stream = bamio.bgzf_decompress(open(dst, "rb").read())
    return stream, bamio.split_records(stream)[1], r.stderr


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return int(l.split(":", 1)[1].strip())
    raise AssertionError("no line '%s' in\n%s" % (what, log))


@pytest.mark.parametrize("extra,kw", [
    ([], {}),
    (["--algo", "adj"], dict(algo="adj")),
    (["-k", "0"], dict(k=0)),
    (["--merge", "any", "--num-threads", "3"], dict(merge="any")),
    (["--keep-unmapped", "--merge", "avgqual"], dict(keep_unmapped=True, merge="avgqual")),
    (["--umi-tag", "RX", "--per-cell"], dict(stage=tag_model.stage, umi_tag="RX", per_cell=True)),
    (["--call-consensus-min-reads", "3"], dict(min_reads=3)),
    (["--devices", "0,0"], {}),
])
def test_output_is_the_models(bam, tmp_path, extra, kw):
    src, header, recs = bam
    exp, counts = bm.expected_output(recs, **kw)
    # an identity kernel -- the kept read's own bases -- would not pass: the model's records differ from them
    assert counts["changed"] >= (100 if "min_reads" not in kw else 20)
    stream, got, log = run(src, tmp_path / "o.bam", ["--call-consensus"] + extra)
    assert stream.startswith(header)
    assert len(got) == len(exp)
    for j, (g, e) in enumerate(zip(got, exp)):
        assert g == e, (j, g, e)
    assert line(log, "Number of reads after deduplicating") == counts["kept"]
    assert line(log, "Number of clusters below --call-consensus-min-reads") == counts["below"]
    assert line(log, "Number of clusters without a consensus") == counts["without"] >= 1
    if "min_reads" in kw:
        assert counts["below"] > 0 and len(got) == counts["kept"] - counts["below"]
    assert "staging (host)" in log


def test_model_differs_from_the_kept_reads(bam):
    _, _, recs = bam
    exp, counts = bm.expected_output(recs)
    assert counts["changed"] >= 100


def test_plain_run_is_unchanged(bam, tmp_path):
    src, header, recs = bam
    exp, _ = bamio.expected_output(recs)
    stream, got, log = run(src, tmp_path / "p.bam", [])
    assert stream == header + b"".join(exp)
    assert "consensus" not in log
