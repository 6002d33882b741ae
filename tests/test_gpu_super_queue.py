"""seg_super_kernel's hit queue: a wave queues the hits of its bit tests (and of the walk, where a key stands twice) in
LDS and decides them 64 at a time; what is left is decided before the super-bin's sets are written out.

Every case is checked as test_gpu_super_rounds.three_ways does: kept and root against the oracle bit for bit, against
seg_super=0 with the counted statistics equal, with root and without it.

Queue edges: which wave holds a record follows from its place in the sub-bucket arrays, so a super-bin of at most 64
entries sits wholly in wave 0 and that wave's hits are the super-bin's pairs.  An L = 8 bucket of ~190 entries (seg_min
lowered to take it, part 0 indexed by 2 bases, seg_super_bases = 1: four super-bins by base 1) holds in super-bin 0 a set
of 64 entries found by a seeded search to have exactly 0, 1, 63, 64, 65, 127, 128, 129 pairs (around the drain threshold
of 64 and the queue's 128 words) or all 288 of the 4^3 subcube.  The other cases: every code of a 4^5 subcube (7,680
pairs, 15 partners each: many drains per wave, one giant component; three classes of freq: more one-way pairs than the
waves' private slots hold, through the queue; one entry twice: the walk through the queue), a hub with all its 24
neighbours in one lane's mask, and a 1,024-thread block at the default cap."""
import numpy as np
import pytest

from test_gpu_seg_local import deep_bucket
from test_gpu_seg_super import CLUSTER, MODES, super_sizes, three_classes
from test_gpu_super_rounds import SMALL, batch_of, count_pairs, neighbours, rows_of, three_ways

pytestmark = pytest.mark.gpu

L8 = 8
SYMMETRIC = [(0.5, 0), (0.5, CLUSTER)]  # all freq 1: p = 1.0 permits the same pairs as p = 0.5


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def all_modes(c, name, batch, L, modes=MODES, **opts):
    return [three_ways(c, "queue/" + name, batch, L, p=p, algo=algo, **opts) for p, algo in modes]


# ---- queue edges: one wave, an exact number of hits ----------------------------------------------------------------

EDGE_PAIRS = (0, 1, 63, 64, 65, 127, 128, 129, 288)


def set_with_pairs(target, n=64, seed=0):
    """n codes of 7 bases with exactly `target` pairs within one substitution: a seeded walk over n-subsets of a pool
    (all codes for few pairs, a 4^4 subcube for dozens, the 4^3 subcube for the densest) that swaps one member for
    one outsider whenever the count comes no further from the target"""
    rng = np.random.default_rng(9200 + 7 * target + seed)
    free = 7 if target <= 1 else 4 if target < 288 else 3
    pool = [int(c) for c in rng.permutation(4 ** free)]
    inside, outside = pool[:n], pool[n:]
    have = set(inside)
    pairs = count_pairs(inside, 7)
    for _ in range(200000):
        if pairs == target:
            break
        i, o = int(rng.integers(0, n)), int(rng.integers(0, len(outside)))
        old, new = inside[i], outside[o]
        have.discard(old)
        after = pairs - sum(w in have for w in neighbours(old, 7)) + sum(w in have for w in neighbours(new, 7))
        if abs(after - target) <= abs(pairs - target):
            inside[i], outside[o], pairs = new, old, after
            have.add(new)
        else:
            have.add(old)
    assert pairs == target == count_pairs(inside, 7), "no set of %d codes with %d pairs" % (n, target)
    return inside


def edge_rows(target):
    """super-bin 0 (base 1 = A): the set with `target` pairs; super-bins 1..3: 40 random codes of a 4^4 subcube each.
    A 7-base code is bases 0, 2, 3, ..., 7 of the row -- the kernel's rest-code for g = 1 of 2 index bases."""
    rng = np.random.default_rng(9300 + target)
    rows = []
    for j in range(4):
        codes = set_with_pairs(target) if j == 0 else [int(c) for c in rng.choice(4 ** 4, 40, replace=False)]
        r7 = rows_of(codes, 7)
        r = np.zeros((len(codes), L8), np.int64)
        r[:, 0], r[:, 1], r[:, 2:] = r7[:, 0], j, r7[:, 1:]
        rows.append(r)
    return np.concatenate(rows)


@pytest.mark.parametrize("target", EDGE_PAIRS)
def test_queue_edges(ctx, target):
    rows = edge_rows(target)
    rng = np.random.default_rng(9400 + target)
    fr = np.minimum(rng.geometric(0.7, len(rows)), 40)
    try:
        ctx.set_option("seg_min", 128)
        for name, freq, modes in (("sym", np.ones(len(rows), np.int64), SYMMETRIC), ("freq", fr, MODES)):
            batch = batch_of(rows, freq, rng)
            sizes = super_sizes(batch[0], 2, 1)
            assert sizes.tolist() == [64, 40, 40, 40]  # (each within one wave)
            opts = dict(seg_super_bases=1, seg_super_min=2)
            all_modes(ctx, "edge/%d/%s" % (target, name), batch, L8, modes, seg_super_cap=2048, **opts)
            all_modes(ctx, "edge/%d/%s" % (target, name), batch, L8, modes[:1], **opts)  # (1,024 threads)
    finally:
        ctx.set_option("seg_min", 512)


# ---- many drains per wave ------------------------------------------------------------------------------------------

def isolated(rng, n, taken, L=L8):
    """n codes none of which is within one substitution of a code in `taken` or of another"""
    near = set()
    for c in taken:
        near.add(c)
        near.update(neighbours(c, L))
    out = []
    while len(out) < n:
        c = int(rng.integers(0, 4 ** L))
        if c not in near:
            out.append(c)
            near.update([c] + neighbours(c, L))
    return out


@pytest.fixture(scope="module")
def subcube():
    """every code over bases 0, 2, 3, 5, 6 with bases 1, 4, 7 = C, G, T (1,024 codes, 7,680 pairs) and 200 entries
    without a neighbour: one super-bin of a 256-thread block, five records to a thread"""
    rng = np.random.default_rng(9500)
    free = [0, 2, 3, 5, 6]
    rows = np.zeros((1024, L8), np.int64)
    rows[:, 1], rows[:, 4], rows[:, 7] = 1, 2, 3
    rows[:, free] = rows_of(range(1024), 5)
    codes = [sum(int(b) << (2 * i) for i, b in enumerate(r)) for r in rows]
    assert count_pairs(codes, L8) == 7680
    pad = isolated(rng, 200, codes)
    assert count_pairs(codes + pad, L8) == 7680
    return np.concatenate([rows, rows_of(pad, L8)])


def one_super_bin(batch, cap=2048):
    sizes = super_sizes(batch[0], 3, 3)
    assert len(sizes) == 1 and 64 <= sizes[0] <= cap // 4 * 3  # (the planner: 3 index bases, g = 3)


def test_subcube_one_giant_component(ctx, subcube):
    batch = batch_of(subcube, np.ones(len(subcube), np.int64), np.random.default_rng(9501))
    one_super_bin(batch)
    sts = all_modes(ctx, "subcube/sym", batch, L8, SYMMETRIC, **SMALL)
    assert sts[0]["n_edges"] == 7680  # (every pair is permitted)
    for st in sts:
        assert st["n_candidates"] == 7680 and st["n_kept"] == 1 + 200


def test_subcube_one_way_pairs_beyond_the_slots(ctx, subcube):
    """three classes of freq at p = 0.5: two of three pairs one-way, over 4 waves with 512 private places each"""
    rng = np.random.default_rng(9502)
    batch = batch_of(subcube, rng.permutation(three_classes(len(subcube))), rng)
    one_super_bin(batch)
    st = all_modes(ctx, "subcube/one-way", batch, L8, **SMALL)[0]
    assert st["n_candidates"] == 7680 and st["n_edges"] * 7 // 10 > 4 * 512


def test_subcube_with_a_key_twice(ctx, subcube):
    """one entry twice: the walk finds 7,680 + 1 + 15 pairs and queues them as two positions"""
    rows = np.concatenate([subcube, subcube[333:334]])
    batch = batch_of(rows, np.ones(len(rows), np.int64), np.random.default_rng(9503))
    assert len(np.unique(batch[0])) == len(batch[0]) - 1
    one_super_bin(batch)
    for st in all_modes(ctx, "subcube/twice", batch, L8, SYMMETRIC, **SMALL):
        assert st["n_candidates"] == 7680 + 16 and st["n_kept"] == 1 + 200
    rng = np.random.default_rng(9504)
    fr = np.minimum(rng.geometric(0.5, len(subcube)), 40)
    fr[333] = 1
    batch = batch_of(rows, np.concatenate([fr, [1]]), rng)
    all_modes(ctx, "subcube/twice/freq", batch, L8, **SMALL)


# ---- the fullest lane ----------------------------------------------------------------------------------------------

@pytest.mark.parametrize("hub", [0, 4 ** L8 - 1])
def test_hub_and_its_24_neighbours(ctx, hub):
    """hub AAAAAAAA: all 24 partners have larger codes, one lane pushes 24 times; hub TTTTTTTT: it holds none itself"""
    rng = np.random.default_rng(9600 + (hub & 1))
    star = [hub] + neighbours(hub, L8)
    rows = rows_of(star + isolated(rng, 700, star), L8)
    # (the neighbours that differ from the hub in the same base are within one of each other: 24 + 8 * 3 pairs)
    assert count_pairs([sum(int(b) << (2 * i) for i, b in enumerate(r)) for r in rows], L8) == 48
    fr = np.ones(len(rows), np.int64)
    batch = batch_of(rows, fr, rng)
    one_super_bin(batch)
    for st in all_modes(ctx, "hub/%d/sym" % hub, batch, L8, SYMMETRIC, **SMALL):
        assert st["n_candidates"] == 48 and st["n_kept"] == 1 + 700
    fr[0] = 9
    for st in all_modes(ctx, "hub/%d/top" % hub, batch_of(rows, fr, rng), L8, **SMALL):
        assert st["n_candidates"] == 48


# ---- 1,024 threads at the default cap --------------------------------------------------------------------------------

def test_default_cap_block_of_1024_threads(ctx):
    batch = deep_bucket(np.random.default_rng(9700), 3200, L8)
    assert 2049 <= len(batch[0]) <= 4000
    one_super_bin(batch, 5632)
    codes = [sum(((int(k) >> (3 * b)) & 3) << (2 * b) for b in range(L8)) for k in batch[0]]
    n_pairs = count_pairs(codes, L8)
    assert n_pairs > 16 * 64  # (every wave drains more than once)
    for st in all_modes(ctx, "deep", batch, L8, seg_super_min=64):
        assert st["n_candidates"] == n_pairs
