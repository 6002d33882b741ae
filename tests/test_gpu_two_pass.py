"""umicollapse --two-pass on the GPU: the same decompressed output stream and summary lines as the
one-pass run (and as the restatement in tests/bamio.py), over many windows, paired, unsorted input,
and the bound on what is held in memory."""
import os
import re
import subprocess

import numpy as np
import pytest

import bamio

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SUMMARY = ("Number of input reads", "Number of removed unmapped reads", "Number of unpaired reads",
           "Number of chimeric reads", "Number of unique alignment positions", "Number of UMIs",
           "Average number of UMIs per alignment position", "Max number of UMIs over all alignment positions",
           "Number of reads after deduplicating")


def write_bam(path, header, recs):
    with open(path, "wb") as f:
        f.write(bamio.bgzf_compress(header + b"".join(recs)))


def run(src, dst, extra):
    r = subprocess.run([CLI, "-i", str(src), "-o", str(dst)] + extra, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return bamio.bgzf_decompress(open(str(dst), "rb").read()), r.stderr


def summary(log):
    return [l for l in log.splitlines() if l.split(":")[0] in SUMMARY]


def two_pass_stats(log):
    m = re.search(r"two-pass: (\d+) windows, at most (\d+) reads held", log)
    assert m, log
    return int(m.group(1)), int(m.group(2))


def both(tmp_path, header, recs, extra):
    """one-pass and --two-pass on the same file: (one-pass stream, two-pass stream, logs, windows, held)"""
    src = tmp_path / "in.bam"
    write_bam(src, header, recs)
    one, log1 = run(src, tmp_path / "one.bam", extra)
    two, log2 = run(src, tmp_path / "two.bam", extra + ["--two-pass"])
    assert "two-pass:" not in log1
    windows, held = two_pass_stats(log2)
    return one, two, log1, log2, windows, held


@pytest.mark.parametrize("extra,kw", [
    (["--algo", "dir", "--merge", "mapqual"], dict(algo="dir", merge="mapqual")),
    (["--algo", "adj", "--merge", "avgqual"], dict(algo="adj", merge="avgqual")),
    (["--merge", "any", "-k", "2"], dict(merge="any", k=2)),
    (["--stage", "host", "--merge", "avgqual"], dict(merge="avgqual")),
    (["--stage", "gpu", "--merge", "any"], dict(merge="any")),
    (["--keep-unmapped", "-u", "10", "--stage", "gpu"], dict(merge="mapqual", keep_unmapped=True, umi_len=10)),
    (["--keep-unmapped", "--stage", "host", "--algo", "adj"], dict(algo="adj", merge="mapqual", keep_unmapped=True)),
    (["--num-threads", "4", "--devices", "0,0"], dict(merge="mapqual")),
])
def test_two_pass_equals_one_pass_over_many_windows(tmp_path, extra, kw):
    header, recs = bamio.synthetic_bam(7, 150, 60, umi_len=10, err=0.03)
    one, two, log1, log2, windows, held = both(tmp_path, header, recs, extra + ["--two-pass-window", "64"])
    assert two == one
    exp, _ = bamio.expected_output(recs, **kw)
    assert bamio.split_records(two) == (header, exp)
    assert summary(log2) == summary(log1) and len(summary(log1)) >= 4
    assert windows > 10
    assert held < len(recs) // 4


@pytest.mark.parametrize("stage", ["gpu", "host"])
def test_two_pass_wide_umis(tmp_path, stage):
    """24-base UMIs: keys of two words through the windows"""
    header, recs = bamio.synthetic_bam(9, 120, 50, umi_len=24, err=0.02)
    one, two, log1, log2, windows, _ = both(tmp_path, header, recs, ["--stage", stage, "--two-pass-window", "64"])
    assert two == one
    exp, _ = bamio.expected_output(recs, merge="mapqual")
    assert bamio.split_records(two)[1] == exp
    assert summary(log2) == summary(log1)
    assert windows > 10


@pytest.mark.parametrize("extra,kw", [
    ([], {}),
    (["--remove-unpaired", "--remove-chimeric", "--merge", "avgqual"],
     dict(remove_unpaired=True, remove_chimeric=True, merge="avgqual")),
    (["--remove-unpaired"], dict(remove_unpaired=True)),
    (["--algo", "adj", "--num-threads", "4"], dict(algo="adj")),
])
def test_two_pass_paired(tmp_path, extra, kw):
    header, recs = bamio.synthetic_paired_bam(21, 120, 50)
    kw.setdefault("merge", "mapqual")
    one, two, log1, log2, windows, _ = both(tmp_path, header, recs, ["--paired", "--two-pass-window", "64"] + extra)
    assert two == one
    exp, _ = bamio.expected_output(recs, paired=True, **kw)
    assert bamio.split_records(two)[1] == exp
    assert sum(1 for r in exp if bamio.parse_record(r)["flag"] & 0x80) > 100  # mates really travel
    assert summary(log2) == summary(log1)
    assert windows > 10


@pytest.mark.parametrize("paired", [False, True])
def test_two_pass_unsorted_input(tmp_path, paired):
    """shuffled records: still the one-pass output, only more is held"""
    if paired:
        header, recs = bamio.synthetic_paired_bam(23, 100, 40)
        extra, kw = ["--paired"], dict(paired=True, merge="mapqual")
    else:
        header, recs = bamio.synthetic_bam(13, 150, 40, umi_len=10, err=0.03)
        extra, kw = ["--keep-unmapped"], dict(keep_unmapped=True, merge="mapqual")
    order = np.random.default_rng(5).permutation(len(recs))
    mixed = [recs[i] for i in order]
    one, two, log1, log2, windows, _ = both(tmp_path, header, mixed, extra + ["--two-pass-window", "64"])
    assert two == one
    exp, _ = bamio.expected_output(mixed, **kw)
    assert bamio.split_records(two)[1] == exp
    assert summary(log2) == summary(log1)


def _child_peak_rss_kb(cmd):
    """peak RSS of `cmd` run in a fresh child of a fresh process (getrusage(RUSAGE_CHILDREN) only grows)"""
    code = ("import resource, subprocess, sys\n"
            "r = subprocess.run(sys.argv[1:], stdout=subprocess.DEVNULL, stderr=subprocess.PIPE, text=True)\n"
            "assert r.returncode == 0, r.stderr\n"
            "print(resource.getrusage(resource.RUSAGE_CHILDREN).ru_maxrss)\n")
    r = subprocess.run(["python3", "-c", code] + cmd, capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stderr
    return int(r.stdout.strip())


def test_two_pass_bounded_memory(tmp_path):
    """2 M sorted reads in 20,000 positions, window 65,536: at most 4 windows' worth of reads held, and
    peak RSS at least half the inflated BAM below the one-pass run's"""
    src, window = tmp_path / "big.bam", 65536
    subprocess.run(["python3", os.path.join(ROOT, "tools", "make_bam.py"), str(src), "--reads", "2000000",
                    "--positions", "20000"], check=True, capture_output=True, timeout=900)
    inflated = len(bamio.bgzf_decompress(open(str(src), "rb").read()))
    extra = ["--num-threads", "8"]
    one, log1 = run(src, tmp_path / "one.bam", extra)
    two, log2 = run(src, tmp_path / "two.bam", extra + ["--two-pass", "--two-pass-window", str(window)])
    assert two == one
    assert summary(log2) == summary(log1)
    windows, held = two_pass_stats(log2)
    assert "Number of input reads: 2000000" in log2
    assert windows >= 2_000_000 // (2 * window)
    assert held <= 4 * window
    rss_one = _child_peak_rss_kb([CLI, "-i", str(src), "-o", str(tmp_path / "r1.bam")] + extra)
    rss_two = _child_peak_rss_kb([CLI, "-i", str(src), "-o", str(tmp_path / "r2.bam"), "--two-pass",
                                  "--two-pass-window", str(window)] + extra)
    print("inflated %d MB, peak RSS one-pass %d MB, two-pass %d MB" % (inflated >> 20, rss_one >> 10, rss_two >> 10))
    assert (rss_one - rss_two) * 1024 >= inflated // 2
