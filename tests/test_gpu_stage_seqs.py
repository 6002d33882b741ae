"""umi_stage_seqs (whole reads staged on the MI355X) field by field against the fastq mode's staging
model (tests/seq_model.py): lengths across the word edges, N bases, duplicates and quality ties, a deep
bucket that takes the order's sort route, a full F1-shaped call, the errors, and the device form
feeding umi_dedup_seqs_device."""
import ctypes as C

import numpy as np
import pytest

import seq_model as sm
from umi_collapse_rs_amd import Context, UmiHipError, synth
from umi_collapse_rs_amd._lib import Stats, load, ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
    yield c
    c.close()


def fast_stage(seqs, quals, merge):
    """sm.stage with the average quality as an integer quotient (the identity test_stage_seqs_cpu.py
    proves): the same result, fast enough for a million reads"""
    buckets = {}
    for i, (s, q) in enumerate(zip(seqs, quals)):
        d = buckets.setdefault(len(s), {})
        sc = 0
        if merge and s:
            t = sum(q) - 33 * len(s)
            sc = t // len(s) if t >= 0 else -((-t) // len(s))
        e = d.get(s)
        if e is None:
            d[s] = [1, i, sc]
        else:
            e[0] += 1
            if merge and not (e[2] >= sc):
                e[1], e[2] = i, sc
    ent, off, blen = [], [0], []
    for L, d in buckets.items():
        items = sorted(d.items(), key=lambda kv: -kv[1][0])
        ent += [(s, e[0], e[1]) for s, e in items]
        off.append(len(ent))
        blen.append(L)
    return ent, off, blen


def check(ctx, seqs, quals, merge, fast=False):
    got = ctx.stage_seqs(seqs, quals, merge=merge)
    ent, off, blen = (fast_stage if fast else sm.stage)(seqs, quals, merge)
    w = max([1] + [sm.words(len(s)) for s in seqs])
    keys, nm = sm.encode([e[0] for e in ent], w)
    assert list(got["bucket_len"]) == blen
    assert list(got["bucket_off"]) == off
    assert np.array_equal(got["freq"], np.array([e[1] for e in ent], np.int32))
    assert np.array_equal(got["rep"], np.array([e[2] for e in ent], np.uint64))
    assert got["keys"].shape == (len(ent), w)
    assert np.array_equal(got["keys"], keys)
    assert np.array_equal(got["nmask"], nm)
    assert got["any_n"] == any(b"N" in s for s in seqs)
    entry = {e[0]: j for j, e in enumerate(ent)}
    assert np.array_equal(got["entry_of_read"], np.array([entry[s] for s in seqs], np.uint32))
    return got


MERGES = [0, 1]


@pytest.mark.parametrize("merge", MERGES)
def test_one_length(ctx, merge):
    seqs, quals = synth.fastq_reads(1, 20000, 6000, length=150, err=0.005)
    check(ctx, seqs, quals, merge)


@pytest.mark.parametrize("merge", MERGES)
def test_mixed_lengths_and_word_edges(ctx, merge):
    lengths = [1, 2, 3, 20, 21, 22, 42, 43, 64, 85, 86, 100, 127, 128, 129, 150, 170, 171, 200, 255, 256]
    seqs, quals = synth.fastq_reads(2, 6000, 1500, lengths=lengths, err=0.01)
    seqs += [b"", b"A" * 256, b"", b"T" * 256]
    quals += [b"", b"I" * 256, b"", b"#" * 256]
    check(ctx, seqs, quals, merge)


@pytest.mark.parametrize("merge", MERGES)
@pytest.mark.parametrize("with_n", [False, True])
def test_n_bases(ctx, merge, with_n):
    seqs, quals = synth.fastq_reads(3, 5000, 1500, lengths=[21, 22, 43, 86, 150, 256], err=0.01,
                                    n_frac=0.01 if with_n else 0.0)
    if with_n:  # N at bases that straddle two words
        for p in (21, 42, 85, 106, 149, 170, 213, 234):
            s = bytearray(b"ACGT" * 64)
            s[p] = ord("N")
            seqs.append(bytes(s))
            quals.append(b"5" * 256)
    got = check(ctx, seqs, quals, merge)
    assert got["any_n"] == with_n


@pytest.mark.parametrize("merge", MERGES)
def test_all_identical(ctx, merge):
    rng = np.random.default_rng(4)
    seqs = [b"ACGTTGCAAC" * 15] * 3000
    quals = [bytes(rng.integers(33, 75, 150, dtype=np.uint8)) for _ in seqs]
    got = check(ctx, seqs, quals, merge)
    assert len(got["freq"]) == 1 and got["freq"][0] == 3000


@pytest.mark.parametrize("merge", MERGES)
def test_all_distinct(ctx, merge):
    rng = np.random.default_rng(5)
    seqs = list({bytes(rng.choice(np.frombuffer(b"ACGT", np.uint8), 60)) for _ in range(4000)})
    quals = [bytes(rng.integers(33, 75, 60, dtype=np.uint8)) for _ in seqs]
    check(ctx, seqs, quals, merge)


@pytest.mark.parametrize("merge", MERGES)
def test_quality_ties(ctx, merge):
    base = [b"ACGTACGTAC", b"GGGGGCCCCC", b"ACGTACGTAA"]
    seqs, quals = [], []
    for i in range(300):
        s = base[i % 3]
        seqs.append(s)
        # equal averages from different bytes, a few higher ones later in the file
        quals.append(b"I" * 10 if i % 7 else (b"H" * 5 + b"J" * 5 if i % 2 else b"K" * 10))
    check(ctx, seqs, quals, merge)


@pytest.mark.parametrize("merge", MERGES)
@pytest.mark.parametrize("n", [0, 1])
def test_zero_and_one_read(ctx, merge, n):
    seqs, quals = [b"ACGTN"][:n], [b"IIII#"][:n]
    got = check(ctx, seqs, quals, merge)
    assert len(got["bucket_off"]) == n + 1


@pytest.mark.parametrize("merge", MERGES)
def test_deep_bucket(ctx, merge):
    """a bucket of 200,000+ entries: the order goes through the sort, not one wave per bucket"""
    rng = np.random.default_rng(6)
    seqs = [r.tobytes() for r in rng.choice(np.frombuffer(b"ACGT", np.uint8), (230_000, 90))]
    seqs += seqs[:40_000:3] + [b"ACGT" * 5] * 10
    quals = [r.tobytes() for r in rng.integers(33, 75, (len(seqs) - 10, 90), dtype=np.uint8)] + [b"I" * 20] * 10
    got = check(ctx, seqs, quals, merge, fast=True)
    assert int(np.diff(got["bucket_off"]).max()) >= 200_000


def test_full_size_f1(ctx):
    seqs, quals = synth.fastq_reads(7, 1_000_000, 300_000, length=150, err=0.005)
    check(ctx, seqs, quals, 1, fast=True)


def test_bad_character_names_the_first_read(ctx):
    seqs = [b"ACGT"] * 10
    quals = [b"IIII"] * 10
    last = list(seqs)
    last[9] = b"ACGa"
    with pytest.raises(UmiHipError, match=r"Unknown character in sequence: 97 \(read 9\)"):
        ctx.stage_seqs(last, quals, merge=1)
    both = list(seqs)
    both[0] = b"AXGT"
    both[9] = b"ACGa"
    with pytest.raises(UmiHipError, match=r"Unknown character in sequence: 88 \(read 0\)"):
        ctx.stage_seqs(both, quals, merge=0)
    mid = [b"A" * 200] * 100
    mid[70] = b"A" * 150 + b"." + b"A" * 49
    mid[31] = b"A" * 190 + b"-" + b"A" * 9
    with pytest.raises(UmiHipError, match=r"Unknown character in sequence: 45 \(read 31\)"):
        ctx.stage_seqs(mid, [b"I" * 200] * 100, merge=1)


def test_refusals(ctx):
    with pytest.raises(UmiHipError):
        ctx.stage_seqs([b"A" * 257], [b"I" * 257])
    with pytest.raises(UmiHipError):
        ctx.stage_seqs([b"A" * 30, b"C" * 10], [b"I" * 30, b"I" * 10], n_words=1)
    with pytest.raises(ValueError):
        ctx.stage_seqs([b"ACGT"], None, merge=1)
    got = ctx.stage_seqs([b"A" * 30], None, merge=0, n_words=12)  # wider than needed: zero words behind
    assert got["keys"].shape == (1, 12) and not got["keys"][:, 2:].any()


def test_device_form_feeds_dedup_seqs_device(ctx):
    import torch
    seqs, quals = synth.fastq_reads(8, 30000, 8000, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    n = len(seqs)
    host = ctx.stage_seqs(seqs, quals, merge=1)
    kept_h, root_h, _ = ctx.dedup_seqs(host["keys"], host["nmask"], host["freq"], host["bucket_off"],
                                       host["bucket_len"], k=2)
    text = b"".join(seqs) + b"".join(quals)
    lens = np.array([len(s) for s in seqs], np.uint32)
    pos = np.zeros(n, np.uint64)
    pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    pos = np.concatenate([pos, pos + np.uint64(sum(map(len, seqs)))])
    w = host["keys"].shape[1]
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(text, np.uint8).copy()).to(dev)
    d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_keys = torch.zeros(n * w, dtype=torch.int64, device=dev)
    d_nm = torch.zeros(n * w, dtype=torch.int64, device=dev)
    d_freq = torch.zeros(n, dtype=torch.int32, device=dev)
    d_rep = torch.zeros(n, dtype=torch.int64, device=dev)
    d_eor = torch.zeros(n, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    boff, blen, e, any_n = ctx.stage_seqs_device(d_text.data_ptr(), d_pos.data_ptr(), d_pos.data_ptr() + 8 * n,
                                                 d_len.data_ptr(), n, w, d_keys.data_ptr(), d_nm.data_ptr(),
                                                 d_freq.data_ptr(), d_rep.data_ptr(), d_eor.data_ptr(), merge=1)
    assert e == len(host["freq"]) and any_n == host["any_n"]
    assert np.array_equal(boff, host["bucket_off"]) and np.array_equal(blen, host["bucket_len"])
    assert np.array_equal(d_eor.cpu().numpy().view(np.uint32), host["entry_of_read"])
    assert np.array_equal(d_rep.cpu().numpy()[:e].view(np.uint64), host["rep"])
    d_kept = torch.zeros(e, dtype=torch.uint8, device=dev)
    d_root = torch.zeros(e, dtype=torch.int32, device=dev)
    st = Stats()
    rc = load().umi_dedup_seqs_device(ctx._h, d_keys.data_ptr(), d_nm.data_ptr() if any_n else None, w,
                                      d_freq.data_ptr(), ptr(boff, C.c_uint64), ptr(blen, C.c_int32), len(blen), 2,
                                      0.5, 0, 0, d_kept.data_ptr(), d_root.data_ptr(), None, C.byref(st))
    assert rc == 0
    torch.cuda.synchronize()
    assert np.array_equal(d_kept.cpu().numpy(), kept_h)
    assert np.array_equal(d_root.cpu().numpy().view(np.uint32), root_h)
