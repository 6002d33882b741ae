"""The inputs of tests/test_gpu_seg_probe.py (tests/seg_probe_inputs.py), checked without a GPU: every input
goes through the oracle, has the sizes and the sub-bucket geometry its test is about, and holds both
symmetric and one-way pairs."""
import collections

import numpy as np
import pytest

import chain_inputs as ci
import seg_probe_inputs as sp


def census(batch, bucket, p):
    umis, freq = batch.buckets[bucket]
    adj = ci.permitted_pairs(umis, freq, 1, p)
    return int(np.triu(adj & adj.T, 1).sum()), int((adj & ~adj.T).sum())


def rests(batch, bucket=0):
    return [r for _, _, r in sp.geometry(batch.sizes()[bucket], batch.L)]


def check_reference(batch, p=0.5):
    okept, oroot = batch.reference(p)
    idx = np.arange(len(okept))
    assert ((okept == 1) == (oroot == idx)).all() and 0 < okept.sum() < len(okept)


def test_first_eligible_and_its_variants():
    b = sp.first_eligible()
    assert sp.SEG_MIN <= b.sizes()[0] < 1024 and sp.geometry(b.sizes()[0], 8) == [(0, 2, 6), (4, 2, 6)]
    for p in (0.5, 1.0):
        check_reference(b, p)
        sym, one = census(b, 0, p)
        assert sym > 0 and one > 0
    n = sp.with_n()
    assert n.nmask is not None and n.nm.any() and n.sizes()[0] >= sp.SEG_MIN
    check_reference(n)
    d = sp.duplicated()
    count = collections.Counter(d.umis)
    assert sorted(count.values())[-2:] == [2, 3] and len(d.umis) == b.sizes()[0] + 3
    assert (np.diff(d.fr) <= 0).all() and d.fr.min() >= 1  # rank order
    check_reference(d)


def test_dense():
    b = sp.dense()
    assert 1900 <= b.sizes()[0] <= 2100 and max(rests(b)) <= sp.PROBE_MAX_REST
    for p in (0.5, 1.0):
        check_reference(b, p)
    sym, one = census(b, 0, 0.5)
    # ~9 partners per entry: ~4.4 pairs per entry counted once, most of them permitted in some direction;
    # more one-way pairs than a block's private slot of 512 holds
    assert sym > 512 and one > 512 and (sym + one) / b.sizes()[0] > 3
    # one giant component of neighbours
    assert b.reference(1.0)[0].sum() < b.sizes()[0] // 8


@pytest.mark.parametrize("n_raw,want", [(3300, [(0, 3, 4), (3, 3, 4)]), (6000, [(0, 3, 4), (3, 4, 3)])])
def test_uneven(n_raw, want):
    b = sp.uneven(n_raw)
    assert sp.geometry(b.sizes()[0], 7) == want
    assert want[1][1] < 4 or n_raw == 6000  # part 1 (four bases) indexed by three of them
    check_reference(b)
    check_reference(b, 1.0)


def test_mixed():
    b = sp.mixed()
    big = [(i, n) for i, n in enumerate(b.sizes()) if n >= sp.SEG_MIN]
    assert len(big) == 4 and len(b.sizes()) == 7 and all(n <= 128 for n in b.sizes() if n < sp.SEG_MIN)
    r = [rests(b, i) for i, _ in big]
    assert r[0] == [7, 7] and r[2] == [7, 7] and r[1] == [5, 5] and r[3] == [5, 4]
    check_reference(b)
    check_reference(b, 1.0)


def test_deep():
    b12, b13 = sp.deep(12), sp.deep(13)
    assert rests(b12) == [6, 6] and rests(b13) == [7, 7]
    assert b12.sizes()[0] >= 65536 and b13.sizes()[0] >= 65536
