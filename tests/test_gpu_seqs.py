"""umi_dedup_seqs (whole reads as keys, up to 256 bases) on the MI355X: kept and root bit-identical to
an independent numpy model with the reference's per-word arithmetic, several lengths in one call, the
partition of deep buckets, heavy bins, and a cross-check with the wide batched call."""
import numpy as np
import pytest

import seq_model as sm
from umi_collapse_rs_amd import UMI_ALGO_ADJACENCY, UMI_ALGO_DIRECTIONAL, Context, synth, to_bitset_seq

pytestmark = pytest.mark.gpu
UMI_KERNEL_SEQ_PAIRS = 3


@pytest.fixture(scope="module")
def ctx():
    c = Context(0, profile=True)
    yield c
    c.close()


def bucket(seed, L, n_mol, err, n_frac=0.0, n_pos=()):
    """distinct sequences of one length in rank order, with their freq"""
    seqs, _ = synth.fastq_reads(seed, 4 * n_mol, n_mol, length=L, err=err, n_frac=n_frac, mean_copies=3.0)
    if n_pos and L:
        extra = []
        for s in seqs[:50]:  # N at the straddling bases
            a = bytearray(s)
            for p in n_pos:
                if p < L:
                    a[p] = ord("N")
            extra.append(bytes(a))
        seqs = seqs + extra
    freq = {}
    for s in seqs:
        freq[s] = freq.get(s, 0) + 1
    items = sorted(freq.items(), key=lambda kv: -kv[1])  # stable: first appearance on ties
    return [s for s, _ in items], [f for _, f in items]


def call(ctx, buckets, k, algo=UMI_ALGO_DIRECTIONAL, p=0.5, adj=0, nmask=True):
    seqs = [s for b in buckets for s in b[0]]
    freq = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    blen = [len(b[0][0]) if b[0] else 0 for b in buckets]
    w = max(1, max(sm.words(L) for L in blen))
    keys, nm = to_bitset_seq(seqs, w)
    kept, root, st = ctx.dedup_seqs(keys, nm if nmask else None, freq, off, blen, k=k, percentage=p, algo=algo,
                                    adj_max_freq=adj)
    return kept, root, st, (seqs, freq, off, blen, keys, nm)


def model(buckets, k, algo=0, p=0.5, adj=0, join=False):
    ent = [(s, f, 0) for b in buckets for s, f in zip(*b)]
    off = list(np.cumsum([0] + [len(b[0]) for b in buckets]))
    blen = [len(b[0][0]) if b[0] else 0 for b in buckets]
    return sm.dedup(ent, off, blen, k, algo, p, adj, join=join)


LENGTHS = [1, 21, 22, 43, 85, 86, 100, 151, 250, 256]
STRADDLE = (21, 42, 85, 106, 149, 170, 213, 234)


@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_lengths_in_one_call(ctx, k):
    buckets = [bucket(10 + L, L, 300 if L > 4 else 30, 0.02 if L > 30 else 0.06, n_frac=0.003, n_pos=STRADDLE)
               for L in LENGTHS]
    kept, root, st, _ = call(ctx, buckets, k)
    mk, mr = model(buckets, k)
    assert np.array_equal(kept.astype(bool), mk)
    assert np.array_equal(root, mr)
    assert st["n_buckets"] == len(LENGTHS)


@pytest.mark.parametrize("p", [0.5, 1.0, float("nan"), float("inf"), float("-inf"), -0.5])
def test_thresholds(ctx, p):
    buckets = [bucket(3, 100, 400, 0.01), bucket(4, 151, 400, 0.01, n_frac=0.002)]
    kept, root, _, _ = call(ctx, buckets, 2, p=p)
    mk, mr = model(buckets, 2, p=p)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)


@pytest.mark.parametrize("adj", [0, 1, 3])
def test_adjacency(ctx, adj):
    buckets = [bucket(5, 86, 400, 0.02), bucket(6, 150, 800, 0.01, n_pos=STRADDLE)]
    kept, root, _, _ = call(ctx, buckets, 2, algo=UMI_ALGO_ADJACENCY, adj=adj)
    mk, mr = model(buckets, 2, algo=1, adj=adj)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)


def test_without_nmask(ctx):
    buckets = [bucket(7, 150, 600, 0.01)]
    kept, root, _, _ = call(ctx, buckets, 1, nmask=False)
    mk, mr = model(buckets, 1)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)


def test_deep_bucket_partition(ctx):
    b = bucket(8, 150, 9000, 0.01, n_frac=0.001, n_pos=STRADDLE)
    assert len(b[0]) >= 20000
    kept, root, st, _ = call(ctx, [b], 2)
    mk, mr = model([b], 2, join=True)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)
    assert st["kernel_id"] == UMI_KERNEL_SEQ_PAIRS
    assert st["n_pairs_evaluated"] < st["n_pairs"] // 100


def test_heavy_bin(ctx):
    # the second half constant: part 1 of k = 1 is one bin of the whole bucket
    seqs, _ = synth.fastq_reads(9, 12000, 3000, length=150, err=0.004, const_suffix=75, mean_copies=4.0)
    f = {}
    for s in seqs:
        f[s] = f.get(s, 0) + 1
    items = sorted(f.items(), key=lambda kv: -kv[1])
    b = ([s for s, _ in items], [v for _, v in items])
    assert len(b[0]) >= 2000
    kept, root, st, _ = call(ctx, [b], 1)
    mk, mr = model([b], 1, join=True)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)
    n = len(b[0])
    assert st["n_pairs_evaluated"] > n * (n - 1) // 8  # a large share of the bucket is one bin of part 1


def test_cross_check_wide(ctx):
    for L in (21, 22, 43, 85):
        for k in (1, 2):
            b = bucket(20 + L, L, 2000, 0.03, n_frac=0.002, n_pos=STRADDLE)
            kept, root, _, (seqs, freq, off, blen, keys, nm) = call(ctx, [b], k)
            w = sm.words(L)
            k2, r2, _ = ctx.dedup_batch_wide(keys[:, :w], nm[:, :w], freq, off, L, k=k)
            assert np.array_equal(kept, k2) and np.array_equal(root, r2), (L, k)


def test_large_bucket_200k(ctx):
    seqs, _ = synth.fastq_reads(11, 400000, 140000, length=150, err=0.004, mean_copies=3.0)
    f = {}
    for s in seqs:
        f[s] = f.get(s, 0) + 1
    items = sorted(f.items(), key=lambda kv: -kv[1])
    b = ([s for s, _ in items], [v for _, v in items])
    assert len(b[0]) >= 200000
    kept, root, st, _ = call(ctx, [b], 1)
    mk, mr = model([b], 1, join=True)
    assert np.array_equal(kept.astype(bool), mk) and np.array_equal(root, mr)
    assert st["kernel_id"] == UMI_KERNEL_SEQ_PAIRS and st["n_pairs_evaluated"] < st["n_pairs"]


def test_refusals(ctx):
    from umi_collapse_rs_amd import UmiHipError
    keys, nm = to_bitset_seq([b"ACGT" * 10, b"ACGT" * 10], 1 + 1)
    with pytest.raises(UmiHipError):  # 40 bases need 2 words: n_words 1 is too few
        ctx.dedup_seqs(keys[:, :1], nm[:, :1], [1, 1], [0, 2], [40])
    with pytest.raises(UmiHipError):
        ctx.dedup_seqs(keys, nm, [1, 1], [0, 2], [257])
