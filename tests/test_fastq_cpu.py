"""umicollapse -m fastq, the parts that need no GPU: reading plain / gzip / multi-member gzip input,
the staging (--dump-staging) against a plain-Python model of the fastq mode's definition, the
refusals, and umi_encode_seqs against to_bitset."""
import gzip
import os
import struct
import subprocess

import numpy as np
import pytest

import seq_model as sm
from umi_collapse_rs_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300)


def read_dump(path):
    b = open(path, "rb").read()
    n, nb, _, w = struct.unpack_from("<4Q", b, 0)
    o = 32
    keys = np.frombuffer(b, np.uint64, n * w, o).reshape(n, w); o += 8 * n * w
    nm = np.frombuffer(b, np.uint64, n * w, o).reshape(n, w); o += 8 * n * w
    freq = np.frombuffer(b, np.int32, n, o); o += 4 * n
    rep = np.frombuffer(b, np.uint32, n, o); o += 4 * n
    off = np.frombuffer(b, np.uint64, nb + 1, o); o += 8 * (nb + 1)
    blen = np.frombuffer(b, np.int32, nb, o); o += 4 * nb
    assert o == len(b)
    return keys, nm, freq, rep, off, blen


def mixed_reads():
    seqs, quals = synth.fastq_reads(5, 3000, 600, lengths=[1, 21, 22, 43, 85, 86, 100, 150], err=0.01, n_frac=0.002)
    # length 0 twice, a read of 256 bases, repeated sequences with different qualities (avgqual ties)
    seqs += [b"", b"ACGT" * 64, b"", seqs[3], seqs[3]]
    quals += [b"", b"I" * 256, b"", b"!" * len(seqs[3]), b"I" * len(seqs[3])]
    return seqs, quals


@pytest.mark.parametrize("merge", ["any", "avgqual"])
def test_staging_plain_gzip_members(tmp_path, merge):
    seqs, quals = mixed_reads()
    text = synth.fastq_text(seqs, quals)
    half = text.index(b"@read1500\n")
    files = {"plain": text, "gz": gzip.compress(text),
             "members": gzip.compress(text[:half]) + gzip.compress(text[half:]) + gzip.compress(b"")}
    ent, off, blen = sm.stage(seqs, quals, 1 if merge == "avgqual" else 0)
    w = max(sm.words(L) for L in blen)
    keys, nm = sm.encode([e[0] for e in ent], w)
    dumps = []
    for name, data in files.items():
        src = tmp_path / ("in_" + name + ".fq")
        src.write_bytes(data)
        dump = tmp_path / (name + ".bin")
        r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--merge", merge,
                 "--dump-staging", str(dump)])
        assert r.returncode == 0, r.stderr
        dumps.append(read_dump(dump))
    for d in dumps[1:]:
        for a, b in zip(dumps[0], d):
            assert np.array_equal(a, b)
    k2, n2, freq, rep, o2, bl2 = dumps[0]
    assert list(bl2) == blen and list(o2) == off
    assert list(freq) == [e[1] for e in ent] and list(rep) == [e[2] for e in ent]
    assert np.array_equal(k2, keys) and np.array_equal(n2, nm)
    assert 0 in blen and blen.index(0) > 0  # length 0: a bucket of its own, in first-appearance order


def test_bgzf_input(tmp_path):
    seqs, quals = mixed_reads()
    text = synth.fastq_text(seqs, quals)
    src_plain, src_bgzf = tmp_path / "a.fq", tmp_path / "b.fq.gz"
    src_plain.write_bytes(text)
    import bamio
    src_bgzf.write_bytes(bamio.bgzf_compress(text))
    for src, dump in ((src_plain, "p.bin"), (src_bgzf, "g.bin")):
        r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--dump-staging", str(tmp_path / dump)])
        assert r.returncode == 0, r.stderr
    assert open(tmp_path / "p.bin", "rb").read() == open(tmp_path / "g.bin", "rb").read()


BAD = {
    "truncated": b"@a\nACGT\n+\nIIII\n@b\nACGT\n+\n",
    "no_at": b"@a\nACGT\n+\nIIII\nb\nACGT\n+\nIIII\n",
    "no_plus": b"@a\nACGT\n-\nIIII\n",
    "qual_len": b"@a\nACGT\n+\nIII\n",
    "char": b"@a\nACGX\n+\nIIII\n",
    "too_long": b"@a\n" + b"A" * 257 + b"\n+\n" + b"I" * 257 + b"\n",
}


@pytest.mark.parametrize("case", sorted(BAD))
def test_malformed(tmp_path, case):
    src = tmp_path / "bad.fq"
    src.write_bytes(BAD[case])
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--dump-staging", str(tmp_path / "d.bin")])
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert r.stderr.strip()
    if case == "char":
        assert "Unknown character" in r.stderr


def test_trim_longer_than_read(tmp_path):
    src = tmp_path / "a.fq"
    src.write_bytes(b"@a\nACGT\n+\nIIII\n@b\nAC\n+\nII\n")
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "-u", "3", "--dump-staging",
             str(tmp_path / "d.bin")])
    assert r.returncode == 101 and r.stderr.strip()


@pytest.mark.parametrize("flags", [["--paired"], ["--remove-unpaired"], ["--remove-chimeric"], ["--keep-unmapped"],
                                   ["--two-pass"], ["--stage", "gpu"], ["--devices", "0,1"],
                                   ["--merge", "mapqual"], ["--algo", "cc"]])
def test_refused(tmp_path, flags):
    src = tmp_path / "a.fq"
    src.write_bytes(b"@a\nACGT\n+\nIIII\n")
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--dump-staging",
             str(tmp_path / "d.bin")] + flags)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert r.stderr.strip()
    if flags[0] == "--merge":
        assert "Invalid algorithm combination" in r.stderr


@pytest.mark.parametrize("L", [1, 21, 22, 42, 43, 85, 86, 150, 256])
def test_encode_seqs(L):
    from umi_collapse_rs_amd import to_bitset_seq
    rng = np.random.default_rng(L)
    seqs = [rng.choice(np.frombuffer(b"ACGTN", np.uint8), L).tobytes() for _ in range(40)]
    seqs[0] = b"N" * L
    keys, nm = to_bitset_seq(seqs, 12)
    k2, n2 = sm.encode(seqs, 12)
    assert np.array_equal(keys, k2) and np.array_equal(nm, n2)
    assert not keys[:, sm.words(L):].any()


def test_encode_seqs_refusals():
    from umi_collapse_rs_amd import UmiHipError, to_bitset_seq
    with pytest.raises(UmiHipError):
        to_bitset_seq([b"ACGX"])
    with pytest.raises(UmiHipError):
        to_bitset_seq([b"A" * 257], 12)
    with pytest.raises(UmiHipError):
        to_bitset_seq([b"A" * 30], 1)  # 30 bases need two words
