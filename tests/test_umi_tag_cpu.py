"""umicollapse --umi-tag / --per-cell / --cell-tag without a GPU: the staging (--dump-staging) against
tests/tag_model.py, the refusals that end a run with status 101, and the summary counts."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bamio
import tag_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def dump(tmp_path, header, recs, flags):
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "stage.bin")
    tag_model.write_bam(src, header, recs)
    r = run(["-i", src, "-o", str(tmp_path / "unused.bam"), "--dump-staging", out] + flags)
    return r, out


def check_staging(got, exp):
    assert got["umi_len"] == exp["umi_len"]
    for f in ("keys", "nmask", "freq", "bucket_off"):
        assert got[f].shape == exp[f].shape and (got[f] == exp[f]).all(), f
    assert (got["rep"].astype(np.int64) == exp["rep"].astype(np.int64)).all()


@pytest.mark.parametrize("umi_len", [12, 24])
@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("mode", ["name+cell", "tag", "tag+cell"])
def test_staging_matches_the_model(tmp_path, umi_len, threads, mode):
    header, recs = tag_model.tagged_bam(11 + umi_len, 40, 12, umi_len=umi_len, n_cells=5)
    flags, kw = ["--merge", "avgqual", "--num-threads", str(threads)], dict(merge="avgqual")
    if "tag" in mode:
        flags += ["--umi-tag", "RX"]
        kw["umi_tag"] = "RX"
    if "cell" in mode:
        flags += ["--per-cell"]
        kw["per_cell"] = True
    r, out = dump(tmp_path, header, recs, flags)
    assert r.returncode == 0, r.stderr
    got = tag_model.read_staging(out, per_cell="cell" in mode)
    exp, _ = tag_model.stage(recs, **kw)
    check_staging(got, exp)
    assert exp["umi_len"] == umi_len and exp["nmask"].any()
    if "cell" in mode:
        assert (got["bucket_cell"] == exp["bucket_cell"]).all()
        c = exp["counters"]
        assert c["groups"] > c["positions"] and c["no_cell"] > 0  # cells really split positions
        assert "Number of (position, cell) groups: %d" % c["groups"] in r.stderr
    if "tag" in mode:
        assert exp["counters"]["no_umi"] > 0


def test_same_position_and_umi_in_two_cells_are_two_entries(tmp_path):
    """equal (position, UMI) in different cells: one entry per cell with --per-cell, one without"""
    header = bamio.make_header([("chr1", 100000)])
    q = bytes([30] * 50)
    recs = [bamio.make_record("a%d" % i, 0, 0, 500, 60, [("M", 50)], 50, q,
                              tags=tag_model.aux_z("UB", "ACGTACGTAC") + tag_model.aux_z("CB", c))
            for i, c in enumerate(["AAAC-1", "AAAG-1", "AAAC-1", "AAAC-1"])]
    r, out = dump(tmp_path, header, recs, ["--umi-tag", "UB", "--per-cell"])
    assert r.returncode == 0, r.stderr
    got = tag_model.read_staging(out, per_cell=True)
    assert list(got["bucket_off"]) == [0, 1, 2] and list(got["freq"]) == [3, 1]
    assert list(got["bucket_cell"]) == [0, 1]
    assert "Number of unique alignment positions: 1\n" in r.stderr
    assert "Number of (position, cell) groups: 2\n" in r.stderr
    r, out = dump(tmp_path, header, recs, ["--umi-tag", "UB"])
    assert r.returncode == 0, r.stderr
    got = tag_model.read_staging(out)
    assert list(got["bucket_off"]) == [0, 1] and list(got["freq"]) == [4]
    assert "(position, cell)" not in r.stderr


def test_summary_counts(tmp_path):
    header, recs = tag_model.tagged_bam(5, 30, 10, n_cells=4, miss_umi=0.1, miss_cell=0.1)
    exp, _ = tag_model.stage(recs, umi_tag="UB", per_cell=True)
    c = exp["counters"]
    # (--dump-staging adds the lines of the tags to what it prints; the GPU tests check a whole run's summary)
    r, out = dump(tmp_path, header, recs, ["--umi-tag", "UB", "--per-cell"])
    assert r.returncode == 0, r.stderr
    got = tag_model.read_staging(out, per_cell=True)
    assert len(got["bucket_off"]) - 1 == c["groups"] and len(got["freq"]) == len(exp["freq"])
    assert "Number of reads without a UMI tag: %d\n" % c["no_umi"] in r.stderr
    assert "Number of reads without a cell barcode: %d\n" % c["no_cell"] in r.stderr
    assert "Number of unique alignment positions: %d\n" % c["positions"] in r.stderr
    assert "Number of (position, cell) groups: %d\n" % c["groups"] in r.stderr
    assert c["no_umi"] > 0 and c["no_cell"] > 0
    # without the flags none of the new lines appears
    r, out = dump(tmp_path, header, recs, [])
    assert r.returncode == 0, r.stderr
    assert "without a" not in r.stderr and "(position, cell)" not in r.stderr


def one_read_bam(tmp_path, tags, name="r1_ACGTACGTACGT"):
    header = bamio.make_header([("chr1", 100000)])
    good = bamio.make_record("r0_ACGTACGTACGT", 0, 0, 500, 60, [("M", 50)], 50, bytes([30] * 50),
                             tags=tag_model.aux_z("RX", "ACGTACGTACGT") + tag_model.aux_z("CB", "AAAC-1"))
    bad = bamio.make_record(name, 0, 0, 700, 60, [("M", 50)], 50, bytes([30] * 50), tags=tags)
    src = str(tmp_path / "in.bam")
    tag_model.write_bam(src, header, [good, bad])
    return src


def expect_101(tmp_path, src, flags, text):
    """one pass (up to the staging dump) and --two-pass (whose census ends the run before any GPU work)"""
    for extra in (["--dump-staging", str(tmp_path / "s.bin")], ["--two-pass"]):
        r = run(["-i", src, "-o", str(tmp_path / "o.bam")] + flags + extra)
        assert r.returncode == 101, (extra, r.returncode, r.stderr)
        assert text in r.stderr, (extra, r.stderr)


@pytest.mark.parametrize("name", ["R", "RXX", "1X", "R_", "", "X-"])
def test_bad_tag_names_are_refused(tmp_path, name):
    src = one_read_bam(tmp_path, tag_model.aux_z("RX", "ACGTACGTACGT"))
    for flag in ("--umi-tag", "--cell-tag"):
        r = run(["-i", src, "-o", str(tmp_path / "o.bam"), flag, name])
        assert r.returncode == 101 and "two characters" in r.stderr, r.stderr
    assert run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "r9", "--dump-staging",
                str(tmp_path / "s.bin")]).returncode == 0


def test_wrong_type_is_refused(tmp_path):
    src = one_read_bam(tmp_path, b"RXi" + struct.pack("<i", 5) + tag_model.aux_z("CB", "AAAC-1"))
    expect_101(tmp_path, src, ["--umi-tag", "RX"], "tag RX of read r1_ACGTACGTACGT is of type i, not Z")
    src = one_read_bam(tmp_path, tag_model.aux_z("RX", "ACGTACGTACGT") + b"CBA" + b"x")
    expect_101(tmp_path, src, ["--umi-tag", "RX", "--per-cell"], "tag CB of read r1_ACGTACGTACGT is of type A, not Z")
    expect_101(tmp_path, src, ["--per-cell"], "is of type A, not Z")  # (name UMIs, the barcode's type)


def test_wrong_length_is_refused(tmp_path):
    src = one_read_bam(tmp_path, tag_model.aux_z("RX", "ACGTACGTAC"))
    expect_101(tmp_path, src, ["--umi-tag", "RX"], "UMI tag RX of read r1_ACGTACGTACGT holds 10 bases, not 12")
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "RX", "-u", "10", "--dump-staging",
             str(tmp_path / "s.bin")])
    assert r.returncode == 101 and "read r0_ACGTACGTACGT holds 12 bases, not 10" in r.stderr


@pytest.mark.parametrize("value", ["ACGT-TGCAACGT", "ACGTACGTACGt"])
def test_unknown_character_in_a_tag(tmp_path, value):
    src = one_read_bam(tmp_path, tag_model.aux_z("RX", value)[:-1 - len(value)] + value.encode()[:12] + b"\0")
    expect_101(tmp_path, src, ["--umi-tag", "RX"], "Unknown character")


@pytest.mark.parametrize("aux", [
    b"RXZACGT",                              # Z without its NUL
    b"XBBi" + struct.pack("<I", 1000) + b"\0" * 8,  # B array longer than the record
    b"XBBA" + struct.pack("<I", 1) + b"x",   # no such B subtype
    b"XQq" + b"\0" * 4,                      # no such type
    b"XIi" + b"\0\0",                        # i cut short
    b"RX",                                   # a tag without its type
])
def test_malformed_aux_block_is_a_clean_failure(tmp_path, aux):
    src = one_read_bam(tmp_path, aux)
    expect_101(tmp_path, src, ["--umi-tag", "RX"], "malformed aux block in read r1_ACGTACGTACGT")


def test_fastq_mode_refuses_the_flags(tmp_path):
    src = tmp_path / "in.fq"
    src.write_text("@r1\nACGT\n+\nIIII\n")
    for flags in (["--umi-tag", "RX"], ["--cell-tag", "CB"], ["--per-cell"]):
        r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq")] + flags)
        assert r.returncode == 101, (flags, r.stderr)
        assert "do not go with fastq mode" in r.stderr


def test_umi_sep_is_ignored_with_umi_tag(tmp_path):
    header, recs = tag_model.tagged_bam(3, 10, 8, umi_in_name=False)
    r1, out = dump(tmp_path, header, recs, ["--umi-tag", "RX", "--umi_sep", "58"])
    assert r1.returncode == 0, r1.stderr
    got = tag_model.read_staging(out)
    exp, _ = tag_model.stage(recs, umi_tag="RX")
    check_staging(got, exp)
    # name mode cannot read these files
    assert run(["-i", str(tmp_path / "in.bam"), "-o", str(tmp_path / "o.bam"), "--dump-staging",
                str(tmp_path / "s.bin")]).returncode == 101
