"""The consensus of fastq mode's clusters, the parts that need no GPU: the model (consensus_model.py)
against columns worked by hand, the numbers the GPU suite's main workload is chosen for, the CLI's
refusals and its help text."""
import os
import subprocess

import numpy as np
import pytest

import consensus_model as cm
import seq_model as sm
from umi_collapse_rs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)


def col(votes):
    b, q = cm.column([(ord(x), ord(y)) for x, y in votes])
    return chr(b), q - 33


# quality characters: '!' 0, '+' 10, '5' 20, '?' 30, 'I' 40, '~' 93
def test_clear_winner():
    # A: 40 + 30 = 70 (2 votes), C: 20: A, 70 - 20 = 50
    assert col([("A", "I"), ("A", "?"), ("C", "5")]) == ("A", 50)


def test_tie_on_s_decided_by_n():
    # G: 20 + 20 = 40 from two votes, A: 40 from one: G wins on n, quality 40 - 40 = 0
    assert col([("A", "I"), ("G", "5"), ("G", "5")]) == ("G", 0)


def test_tie_on_both_decided_by_acgt_order():
    assert col([("T", "?"), ("C", "?")]) == ("C", 0)
    assert col([("T", "?"), ("G", "?"), ("C", "?")]) == ("C", 0)
    assert col([("G", "5"), ("T", "5")]) == ("G", 0)
    assert col([("C", "5"), ("A", "5")]) == ("A", 0)


def test_all_n():
    assert col([("N", "I"), ("N", "~")]) == ("N", 0)
    # an N beside a vote changes nothing
    assert col([("N", "~"), ("T", "+")]) == ("T", 10)


def test_all_quality_zero():
    # every S is 0: two C against one A, C wins on n; quality 0
    assert col([("A", "!"), ("C", "!"), ("C", "!")]) == ("C", 0)
    # and a tie on n as well goes to the first of ACGT
    assert col([("T", "!"), ("G", "!")]) == ("G", 0)


def test_q_capped_at_93():
    assert col([("A", "I"), ("A", "I"), ("A", "I")]) == ("A", 93)  # 120
    assert col([("A", "~")]) == ("A", 93)
    assert col([("A", "~"), ("A", "~"), ("C", "~")]) == ("A", 93)  # 186 - 93


def test_q_floored_at_0():
    # A 40 wins over C 30 and G 30, 40 - 60 < 0
    assert col([("A", "I"), ("C", "?"), ("G", "?")]) == ("A", 0)


def test_quality_bytes_below_33_count_zero():
    assert cm.column([(ord("A"), 10), (ord("C"), 34)]) == (ord("C"), 34)


def test_one_member_and_length_zero():
    assert cm.consensus([(b"ACGTN", b"!+5?I")]) == (b"ACGTN", b"!+5?!")
    assert cm.consensus([(b"", b""), (b"", b"")]) == (b"", b"")


def test_consensus_is_order_independent_and_column_wise():
    members = [(b"ACGT", b"I5+!"), (b"ACCT", b"5I?!"), (b"TCGN", b"+++~"), (b"ACGA", b"!!!!")]
    want = cm.consensus(members)
    assert want == (b"ACCT", bytes(33 + q for q in (50, 70, 10, 0)))
    assert cm.consensus(members[::-1]) == want


def test_main_workload_numbers():
    """What the GPU suite's main case is chosen for: clusters whose consensus is not the kept read, and
    tied columns."""
    seqs, quals = synth.fastq_reads(41, 4000, 900, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    ent, off, blen = sm.stage(seqs, quals, 1)
    kept, root = sm.dedup(ent, off, blen, 2, 0, join=True)
    cl = cm.clusters(seqs, quals, cm.entry_of_reads(seqs, ent), kept, root)
    assert len(cl) == int(kept.sum()) and sum(m for *_, m in cl) == len(seqs)
    assert max(m for *_, m in cl) >= 8
    differ = sum(1 for r, s, q, m in cl if s != seqs[ent[r][2]])
    assert differ >= 100
    text, dropped = cm.output(seqs, quals, [b"r%d" % i for i in range(len(seqs))], ent, kept, root, trim=3, min_reads=3)
    assert dropped == sum(1 for *_, m in cl if m < 3) and text.count(b"\n") == 4 * (len(cl) - dropped)


REFUSED = [
    (["-m", "bam", "--consensus"], "--consensus"),
    (["-m", "fastq", "--consensus", "--tag"], "--tag"),
    (["-m", "fastq", "--consensus", "--dump-staging", "DUMP"], "--dump-staging"),
    (["-m", "fastq", "--consensus", "--consensus-min-reads", "0"], "--consensus-min-reads"),
    (["-m", "fastq", "--consensus", "--consensus-min-reads", "-2"], "--consensus-min-reads"),
    (["-m", "fastq", "--consensus", "--consensus-min-reads", "3x"], "--consensus-min-reads"),
    (["-m", "fastq", "--consensus", "--consensus-min-reads", ""], "--consensus-min-reads"),
    (["-m", "fastq", "--consensus-min-reads", "2"], "--consensus-min-reads"),
    (["-m", "bam", "--consensus-min-reads", "2"], "--consensus-min-reads"),
]


@pytest.mark.parametrize("flags,word", REFUSED)
def test_refused(tmp_path, flags, word):
    src = tmp_path / "a.fq"
    src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    out = tmp_path / "o.fq"
    flags = [str(tmp_path / "d.bin") if f == "DUMP" else f for f in flags]
    r = run(["-i", str(src), "-o", str(out)] + flags)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert word in r.stderr
    assert not out.exists()


def test_help_names_the_flags():
    r = run(["--help"])
    assert r.returncode == 0
    assert "--consensus " in r.stdout and "--consensus-min-reads" in r.stdout
