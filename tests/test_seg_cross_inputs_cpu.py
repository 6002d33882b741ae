"""The inputs of tests/test_gpu_seg_cross.py hold what their names say, and the model of the cross pairs
(tests/seg_cross_inputs.py) agrees with a count that knows nothing of super-bins: cross pairs + pairs inside the
super-bins = all pairs at distance 1; on a small bucket also with the distances taken pair by pair, and with the
oracle's result (a bucket whose every pair at distance 1 is permitted both ways collapses to its components)."""
import numpy as np
import pytest

import oracle as orc
import seg_cross_inputs as sci
from helpers import dist_blocks


def sizes(batch, shape):
    sb, _ = sci.codes_of(batch[0], shape["L"], shape["nb0"], shape["g"])
    return np.bincount(sb, minlength=4 ** (shape["nb0"] - shape["g"]))


def check_model(batch, shape):
    keys = batch[0]
    L, nb0, g = shape["L"], shape["nb0"], shape["g"]
    assert sci.shape_of(len(keys), L)[0] == nb0
    cross, inside = sci.cross_pairs(keys, L, nb0, g), sci.inside_pairs(keys, L, nb0, g)
    assert len(cross) + len(inside) == sci.neighbours(keys, L)
    sb, rest = sci.codes_of(keys, L, nb0, g)
    z = sb[cross[:, 0]] ^ sb[cross[:, 1]]
    assert (rest[cross[:, 0]] == rest[cross[:, 1]]).all() and (np.bitwise_count((z | (z >> 1)) & 0x5555) == 1).all()
    return cross


def test_model_against_pairwise_distances_and_the_oracle():
    rng = np.random.default_rng(1)
    umis = sci.random_umis(rng, 2500, 6)
    batch = sci.batch_of(umis, [1] * len(umis))
    keys, nm, fr, off = batch
    cross = check_model(batch, dict(L=6, nb0=3, g=1)) if sci.shape_of(len(keys), 6)[0] == 3 else None
    n1 = sum(int(((d == 1) & (np.arange(len(keys))[None, :] > (r0 + np.arange(len(d)))[:, None])).sum())
             for r0, d in dist_blocks(keys, nm))
    assert n1 == sci.neighbours(keys, 6)
    assert len(sci.cross_pairs(keys, 6, 3, 1)) + len(sci.inside_pairs(keys, 6, 3, 1)) == n1
    assert cross is None or len(cross) > 0
    # all freq 1: every pair at distance 1 is permitted both ways, the survivors are the components' first entries
    parent = np.arange(len(keys))

    def find(i):
        while parent[i] != i:
            parent[i] = parent[parent[i]]
            i = parent[i]
        return i
    for i, j in np.concatenate([sci.cross_pairs(keys, 6, 3, 1), sci.inside_pairs(keys, 6, 3, 1)]):
        a, b = find(i), find(j)
        parent[max(a, b)] = min(a, b)
    roots = np.array([find(i) for i in range(len(keys))])
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, 6, 1, 0.5, 0, 0)
    assert (okept.astype(bool) == (roots == np.arange(len(keys)))).all()
    assert (oroot == roots).all()


def test_shape_and_rule_restated():
    assert sci.shape_of(970714, 12) == (6, 2)
    assert sci.shape_of(39261, 10) == (5, 3) and sci.shape_of(39261, 10, g=2, smin=64) == (5, 2)
    assert sci.shape_of(39990, 12) == (5, 0) and sci.shape_of(39990, 12, smin=64) == (5, 1)
    assert sci.shape_of(5000, 8, cap=8192) == (4, 4)
    assert sci.cross_planned(12, 2) and sci.cross_planned(13, 2) and not sci.cross_planned(14, 2)
    assert sci.cross_planned(14, 2, map_mb=32) and not sci.cross_planned(12, 0) and not sci.cross_planned(12, 2, seg_cross=0)


@pytest.mark.parametrize("partners", [None, [4, 13]])
def test_lone_entry(partners):
    batch, shape, n_partners = sci.lone_entry_with_all_partners(partners=partners)
    assert sci.shape_of(len(batch[0]), 10) == (5, 3)
    cross = check_model(batch, shape)
    sz = sizes(batch, shape)
    assert n_partners == (6 if partners is None else 2) and sz[5] == 1
    assert (sz == 1).sum() == 1 + n_partners and (sz == 0).sum() == 6 - n_partners and sz.max() <= 5632
    sb, rest = sci.codes_of(batch[0], 10, 5, 3)
    lone = int(np.nonzero(sb == 5)[0][0])
    mine = cross[(cross[:, 0] == lone) | (cross[:, 1] == lone)]
    other = np.where(mine[:, 0] == lone, mine[:, 1], mine[:, 0])
    assert len(mine) == n_partners and (sz[sb[other]] == 1).all()  # found once each, above and below its code
    assert (sb[other] < 5).any() and (sb[other] > 5).any()


def test_map_edges():
    batch, shape = sci.map_edges()
    cross = check_model(batch, shape)
    sb, rest = sci.codes_of(batch[0], 10, 5, 3)
    for r in (0, 31, 4 ** 8 - 32, 4 ** 8 - 1):
        got = {tuple(sorted((int(sb[i]), int(sb[j])))) for i, j in cross if rest[i] == r}
        assert {(0, 1), (0, 4)} <= got, (r, got)
    sz = sizes(batch, shape)
    assert sz.min() >= 2 and sz.max() <= 5632 * 3 // 4


@pytest.mark.parametrize("m", [0, 1, 63, 64, 65, 128, 200])
def test_queue_fill(m):
    batch, shape = sci.queue_fill(m)
    assert sci.shape_of(len(batch[0]), 10) == (5, 3)
    cross = check_model(batch, shape)
    sb, rest = sci.codes_of(batch[0], 10, 5, 3)
    sz = sizes(batch, shape)
    assert sz[2] == m and sz[3] == m
    between = cross[(np.minimum(sb[cross[:, 0]], sb[cross[:, 1]]) == 2) & (np.maximum(sb[cross[:, 0]], sb[cross[:, 1]]) == 3)]
    assert len(between) == m
    # nothing else of super-bin 2's hits falls into the first chunk of its map
    from2 = cross[(sb[cross[:, 0]] == 2) | (sb[cross[:, 1]] == 2)]
    assert len(from2) == m


def test_dense_one_way():
    batch, shape = sci.dense_one_way()
    assert sci.shape_of(len(batch[0]), 8, cap=2048) == (4, 2) and sci.shape_of(len(batch[0]), 8) == (4, 2)
    cross = check_model(batch, shape)
    fr = batch[2].astype(np.int64)
    thr = (np.float32(0.5) * (fr + 1).astype(np.float32)).astype(np.int64)
    i, j = np.minimum(cross[:, 0], cross[:, 1]), np.maximum(cross[:, 0], cross[:, 1])
    one_way = (fr[j] <= thr[i]) != (fr[i] <= thr[j])
    sb, _ = sci.codes_of(batch[0], 8, 4, 2)
    lower = np.minimum(sb[cross[:, 0]], sb[cross[:, 1]])
    assert np.bincount(lower[one_way], minlength=16).max() > 512  # one block per super-bin at grid_cus = 1


def test_fallback_inputs():
    batch, shape = sci.crowded_super_bin()
    sz = sizes(batch, shape)
    assert (sz > 2048).sum() == 1 and len(batch[0]) // 16 <= 2048 // 4 * 3
    both, _ = sci.crowded_super_bin(freq=sci.three_classes)
    both = sci.with_key_twice(both, seed=1)
    assert len(np.unique(both[0])) == len(both[0]) - 20 and (sizes(both, shape) > 2048).sum() == 1
    assert sci.neighbours(np.unique(both[0]), 10) // 2 > 1024  # (two of three pairs one-way: the list of 1,024 runs over)
    twice = sci.with_key_twice(sci.uniform(20000, 10, seed=6))
    assert len(np.unique(twice[0])) == len(twice[0]) - 20 and sci.shape_of(len(twice[0]), 10) == (5, 3)
