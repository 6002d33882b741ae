"""The consensus of BAM mode's clusters (--call-consensus), the parts that need no GPU: the model
(bam_consensus_model.py) against columns worked by hand, what the GPU CLI suite's file is chosen for,
the CLI's refusals and its help text."""
import os
import subprocess

import pytest

import bam_consensus_model as bm
import bamio

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)


def col(votes):
    """one column: votes = [(base letter, quality)] -> (called nibble, quality, disagree)"""
    s, q, depth, dis = bm.vote([(bm.pack(b), bytes([w])) for b, w in votes], 1)
    assert depth == len(votes) and s[0] & 15 == 0
    return s[0] >> 4, q[0], dis


def test_columns_by_hand():
    assert col([("A", 30), ("A", 20), ("C", 40)]) == (1, 10, 1)       # S_A = 50 against 40
    assert col([("A", 20), ("C", 10), ("C", 10)]) == (2, 0, 1)        # a tie on S: two reads beat one
    assert col([("G", 10), ("C", 10)]) == (2, 0, 1)                   # a tie on both: the first of ACGT
    assert col([("T", 10), ("G", 10), ("C", 9), ("C", 1)]) == (2, 0, 2)  # S 10, 10, 10; n 2 for C
    assert col([("N", 40), ("=", 40), ("M", 40)]) == (15, 0, 0)       # nobody voted
    assert col([("N", 40), ("T", 0)]) == (8, 0, 0)                    # a vote of weight 0 is a vote
    assert col([("A", 200), ("A", 93)]) == (1, 93, 0)                 # S = 186: the call is capped at 93
    assert col([("A", 255), ("C", 93), ("C", 1)]) == (2, 1, 1)        # 255 weighs 93: 93 against 94
    assert col([("A", 93), ("A", 255)]) == col([("A", 255), ("A", 93)])


def test_odd_length_padding_and_order():
    # three bases in two bytes; the voters' own padding nibbles are not zero and must not show
    a = (bytes([0x12, 0x4F]), bytes([30, 30, 30]))   # A C G
    b = (bytes([0x12, 0x81]), bytes([10, 10, 40]))   # A C T
    c = (bytes([0xF2, 0x88]), bytes([10, 10, 5]))    # N C T
    s, q, depth, dis = bm.vote([a, b, c], 3)
    assert s == bytes([0x12, 0x80]) and q == bytes([40, 50, 15]) and depth == 3 and dis == 1
    assert bm.vote([c, a, b], 3) == (s, q, depth, dis)
    assert bm.vote([], 3) == (bytes([0xFF, 0xF0]), bytes(3), 0, 0)
    assert bm.pack("ACGTN") == bytes([0x12, 0x48, 0xF0]) and bm.nibbles(bm.pack("ACGTN"), 5) == [1, 2, 4, 8, 15]


def test_record_builder_matches_bamio():
    quals = bytes(range(20, 27))
    mine = bm.make_record("q_ACGT", 16, 1, 77, 9, [("S", 2), ("M", 5)], "AAAAAAA", quals, tags=b"NMc\x01")
    theirs = bamio.make_record("q_ACGT", 16, 1, 77, 9, [("S", 2), ("M", 5)], 7, quals, tags=b"NMc\x01")
    o, l_seq, cigar = bm.fields(mine)
    assert l_seq == 7 and len(cigar) == 8 and len(mine) == len(theirs)
    assert mine[:o] == theirs[:o] and mine[o + 4:] == theirs[o + 4:] and mine[o:o + 4] == bytes([0x11, 0x11, 0x11, 0x10])
    assert bamio.parse_record(mine)["qual"] == quals


def test_the_cli_suites_file_has_what_it_is_chosen_for():
    header, recs = bm.synthetic_bam(3)
    parsed = [bamio.parse_record(r) for r in recs]
    cigars = {"".join("%d%s" % (l, op) for op, l in p["cigar"]) for p in parsed}
    assert cigars == {"50M", "5S45M", "20M2D30M", "20M1I29M", "49M"}
    assert {p["flag"] & 0x10 for p in parsed} == {0, 0x10} and {p["tid"] for p in parsed} == {0, 1}
    assert sum(p["qual"][0] == 0xFF for p in parsed) >= 10
    exp, counts = bm.expected_output(recs)
    plain, _ = bamio.expected_output(recs)
    assert len(exp) == len(plain) == counts["kept"]
    assert counts["changed"] >= 100 and counts["without"] >= 1 and counts["below"] == 0
    # the same records in the same order: everything in front of the sequence but block_size is the kept read's
    for e, p in zip(exp, plain):
        o, l_seq, _ = bm.fields(p)
        assert e[4:o] == p[4:o] and (e == p or len(e) == len(p) + 21)
    _, c3 = bm.expected_output(recs, min_reads=3)
    assert 0 < c3["below"] < counts["kept"] and c3["without"] == counts["without"]
    # clusters hold non-voters: some cluster's depth is below its reads
    import struct
    assert any(struct.unpack_from("<i", e, len(e) - 18)[0] < struct.unpack_from("<i", e, len(e) - 11)[0]
               for e, p in zip(exp, plain) if e != p)


REFUSED = [
    (["-m", "fastq", "--call-consensus"], "--call-consensus"),
    (["--call-consensus", "--tag"], "--call-consensus"),
    (["--call-consensus", "--two-pass"], "--call-consensus"),
    (["--call-consensus", "--paired"], "--call-consensus"),
    (["--call-consensus", "--dump-staging", "DUMP"], "--call-consensus"),
    (["--call-consensus", "--passthrough"], "--call-consensus"),
    (["--call-consensus-min-reads", "2"], "--call-consensus-min-reads"),
    (["-m", "fastq", "--call-consensus-min-reads", "2"], "--call-consensus-min-reads"),
    (["--call-consensus", "--call-consensus-min-reads", "0"], "--call-consensus-min-reads"),
    (["--call-consensus", "--call-consensus-min-reads", "-2"], "--call-consensus-min-reads"),
    (["--call-consensus", "--call-consensus-min-reads", "3x"], "--call-consensus-min-reads"),
    (["--call-consensus", "--call-consensus-min-reads", ""], "--call-consensus-min-reads"),
    (["-m", "bam", "--consensus"], "--consensus"),  # (as in test_consensus_cpu.py: the boundary between the two flags)
    (["-m", "bam", "--consensus-min-reads", "2"], "--consensus-min-reads"),
]


@pytest.mark.parametrize("flags,word", REFUSED)
def test_refused(tmp_path, flags, word):
    header, recs = bm.synthetic_bam(1, n_positions=2, reads_per_position=3, tags=False)
    src = tmp_path / "a.bam"
    src.write_bytes(bamio.bgzf_compress(header + b"".join(recs)))
    out = tmp_path / "o.bam"
    flags = [str(tmp_path / "d.bin") if f == "DUMP" else f for f in flags]
    r = run(["-i", str(src), "-o", str(out)] + flags)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert word in r.stderr
    assert not out.exists() and not (tmp_path / "d.bin").exists()


def test_help_names_the_flags():
    r = run(["--help"])
    assert r.returncode == 0
    assert "--call-consensus " in r.stdout and "--call-consensus-min-reads" in r.stdout
    assert "--consensus " in r.stdout and "--consensus-min-reads" in r.stdout
