"""The inputs of tests/test_gpu_large_k.py, checked on the CPU for every parametrised case: each holds,
in every bucket size class, a pair at distance exactly k and one at exactly k + 1, pairs at exactly k
of all three directional kinds, and a removal that goes through a distance-k edge -- so an off-by-one
in a kernel's limit cannot hide behind an input that has no pair at the limit."""
import numpy as np
import pytest

import helpers as h
import oracle as orc
import seq_model as sm


@pytest.mark.parametrize("n_frac", [0.0, 0.01])
@pytest.mark.parametrize("L,k", h.ONE_WORD_BOUNDARY + h.ONE_WORD_HUGE)
def test_one_word_inputs_have_pairs_at_the_limit(L, k, n_frac):
    keys, nm, fr, off = h.one_word_batch(L, k, n_frac)
    kk = min(k, L)
    assert np.diff(off.astype(np.int64)).max() <= (2000 if k >= L else 3000)
    kept = orc.dedup_batch(keys, nm, fr, off, L, k)[0]
    assert np.array_equal(kept, orc.dedup_batch(keys, nm, fr, off, L, kk)[0])
    h.assert_k_decides(h.limit_census(keys, nm, fr, off, kk), L, k, kept,
                       orc.dedup_batch(keys, nm, fr, off, L, kk - 1)[0])
    assert bool(nm.any()) == bool(n_frac)


@pytest.mark.parametrize("L,k", h.WIDE_CASES)
def test_wide_inputs_have_pairs_at_the_limit(L, k):
    keys, nm, fr, off = h.wide_batch(L, k)
    kk = min(k, L)
    assert np.diff(off.astype(np.int64)).max() >= 2000 and (k < L or np.diff(off.astype(np.int64)).max() == 2000)
    kept = orc.dedup_batch_wide(keys, nm, fr, off, L, k)[0]
    h.assert_k_decides(h.limit_census(keys, nm, fr, off, kk), L, k, kept,
                       orc.dedup_batch_wide(keys, nm, fr, off, L, kk - 1)[0])
    assert nm[:, 1].any()  # an N at or behind the straddling base


@pytest.mark.parametrize("L,k", h.SEQ_CASES)
def test_whole_read_inputs_have_pairs_at_the_limit(L, k):
    buckets = h.seq_buckets(L, k)
    kk = min(k, L)
    seqs = [s for b in buckets for s in b[0]]
    fr = [f for b in buckets for f in b[1]]
    off = np.cumsum([0] + [len(b[0]) for b in buckets])
    assert len(buckets[0][0]) == 2 and len(buckets[1][0]) < 512 <= len(buckets[2][0])
    keys, nm = sm.encode(seqs, sm.words(L))
    ent = [(s, f, 0) for s, f in zip(seqs, fr)]
    kept = sm.dedup(ent, list(off), [L] * 3, kk)[0]
    census = h.limit_census(keys[2:], nm[2:], fr[2:], off[1:] - 2, kk)  # (the pair's class has one pair only)
    # (both buckets are of one size class here: the split that matters is below / from 512 entries)
    h.assert_k_decides(census, L, k, kept, sm.dedup(ent, list(off), [L] * 3, kk - 1)[0])
    for b in (1, 2):
        c = h.limit_census(keys[off[b]:off[b + 1]], nm[off[b]:off[b + 1]], fr[off[b]:off[b + 1]],
                           [0, off[b + 1] - off[b]], kk)
        assert all(v["at_k"] and (kk == L or v["at_k1"]) for v in c.values())
    if h.seq_partitioned(L, k):  # the bucket of 512 entries or more is cut into k + 1 parts
        big = buckets[2][0]
        bk, bn = sm.encode(big, sm.words(L))
        h.assert_tight_pigeonhole(big, sm.pairs_brute(bk, bn, k), k + 1)
