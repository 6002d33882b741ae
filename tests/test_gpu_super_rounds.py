"""seg_super_kernel's components and the pair kernel's tiles around it: the tiles leave out part-1 hits inside a super-bin
where the scan has found every super-bin of the segment taken, and the drain drops them where it has not.  (The cases
were written for a seg_super_kernel that finds its components by rounds of min-label hooking -- a long path is what
such rounds converge slowest on; that kernel was slower and is not in the tree, DESIGN.md 5a, the cases hold for the
union-find one as well.)

Every case is checked three ways: against the oracle, kept and root bit for bit; against the same context with
seg_super=0, where n_edges, n_candidates, n_pairs_evaluated and n_kept are equal as well; with root and without it.

Shapes: L = 8 buckets of 600..4,000 entries are one super-bin (the planner indexes part 0 by 2..4 bases and takes g =
all of them: the rest-code is the whole UMI), L = 10 buckets of ~20,000 are sixteen (g = 3: bases 3 and 4 shared);
seg_super_min = 64 and seg_super_cap = 2,048 (256-thread blocks) unless a case says otherwise.

The path: an induced path in the Hamming graph over 8 bases -- consecutive codes differ in one base, no other two are
within one -- grown by a seeded walk, so its codes (the positions in the super-bin are their ranks) go up and down.
With one-way links: at p = 0.5 a pair is symmetric only between two entries of freq 1, so symmetric and one-way links
cannot alternate strictly there; freqs 1, 1, 3 along the path give sets of two chained by two one-way pairs, and the
strict alternation is run at p = 1.0 (freqs F, F, F - 2, F - 2, ...: tests/chain_inputs.py's comb)."""
import numpy as np
import pytest

import oracle as orc
from helpers import canonical
from test_gpu_seg_local import deep_bucket
from test_gpu_seg_super import CLUSTER, COUNTED, call, oracle_of, super_sizes

pytestmark = pytest.mark.gpu

SMALL = dict(seg_super_min=64, seg_super_cap=2048)
L8 = 8


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def three_ways(c, name, batch, L, p=0.5, algo=0, **opts):
    """the oracle, seg_super=0 and a call without root; returns the statistics of the call with the path on"""
    okept, oroot = oracle_of("rounds/" + name, batch, L, 1, p, algo)
    kept, root, st = call(c, batch, L, 1, p, algo, **dict(opts, seg_super=1))
    what = "%s p=%g algo=%d %s" % (name, p, algo, opts)
    assert (kept == okept).all(), "%s: kept differs at %s" % (what, np.nonzero(kept != okept)[0][:10])
    assert (root == oroot).all(), "%s: root differs at %s" % (what, np.nonzero(root != oroot)[0][:10])
    assert st["n_kept"] == int(okept.sum()), what
    kept0, root0, st0 = call(c, batch, L, 1, p, algo, **dict(opts, seg_super=0))
    assert (kept0 == okept).all() and (root0 == oroot).all(), what + " (seg_super=0)"
    kept1, none, st1 = call(c, batch, L, 1, p, algo, want_root=False, **dict(opts, seg_super=1))
    assert none is None and (kept1 == okept).all(), what + " (no root)"
    for f in COUNTED:
        assert st[f] == st0[f] == st1[f], (what, f, st[f], st0[f], st1[f])
    return st


def batch_of(rows, freq, rng=None):
    """one bucket of the given rows (bases 0..3) with their freqs, in rank order; rng: equal freqs in shuffled order"""
    order = np.arange(len(rows)) if rng is None else rng.permutation(len(rows))
    umis = ["".join("ACGT"[b] for b in rows[i]) for i in order]
    fr = [int(freq[i]) for i in order]
    umis, fr, _ = canonical(umis, fr)
    keys, nm = orc.encode_keys(umis)
    return keys, nm, np.array(fr, np.int32), np.array([0, len(umis)], np.uint64)


def code_of(row):
    return sum(int(b) << (2 * i) for i, b in enumerate(row))


def neighbours(code, L):
    return [code ^ (d << (2 * b)) for b in range(L) for d in (1, 2, 3)]


def rows_of(codes, L):
    return np.array([[(c >> (2 * b)) & 3 for b in range(L)] for c in codes], np.int64)


_paths = {}


def induced_path(n, L=L8, seed=0):
    """codes of n nodes: consecutive ones differ in one base, no two others are within one (a seeded greedy walk)"""
    if (n, L, seed) not in _paths:
        for attempt in range(50):
            rng = np.random.default_rng(9100 + 97 * seed + attempt)
            near = np.zeros(4 ** L, np.int32)  # visited nodes within one of a code
            seen = np.zeros(4 ** L, bool)
            cur = int(rng.integers(0, 4 ** L))
            path = []
            while True:
                path.append(cur)
                seen[cur] = True
                nb = neighbours(cur, L)
                near[nb] += 1
                if len(path) == n:
                    break
                free = [w for w in nb if not seen[w] and near[w] == 1]
                if not free:
                    break
                cur = free[int(rng.integers(0, len(free)))]
            if len(path) == n:
                break
        assert len(path) == n, "no induced path of %d nodes" % n
        _paths[(n, L, seed)] = path
    return _paths[(n, L, seed)]


def count_pairs(codes, L):
    """pairs of the codes within one substitution"""
    have = set(codes)
    return sum(1 for c in codes for w in neighbours(c, L) if w > c and w in have)


PATH_N = 1000


@pytest.fixture(scope="module")
def path_rows():
    codes = induced_path(PATH_N)
    assert count_pairs(codes, L8) == PATH_N - 1  # a path, nothing else
    ranks = np.argsort(np.argsort(codes))
    turns = np.sum(np.diff(np.sign(np.diff(ranks))) != 0)
    assert turns > PATH_N // 10, "positions along the path must go up and down"
    return rows_of(codes, L8)


@pytest.mark.parametrize("order", ["along", "shuffled"])
def test_one_long_path(ctx, path_rows, order):
    """all freq 1: 999 symmetric pairs, one component whose diameter is the whole super-bin -- many rounds"""
    rng = None if order == "along" else np.random.default_rng(9001)
    batch = batch_of(path_rows, np.ones(PATH_N, np.int64), rng)
    st = three_ways(ctx, "path/" + order, batch, L8, **SMALL)
    assert st["n_kept"] == 1 and st["n_edges"] == st["n_candidates"] == PATH_N - 1  # (every pair is permitted)


def test_path_with_one_way_links(ctx, path_rows):
    """freqs 1, 1, 3 along the path at p = 0.5: one symmetric link, then two one-way ones; F, F, F - 2, F - 2 at
    p = 1.0: symmetric and one-way links alternate.  The pieces must stay apart in the forest and the one-way pairs
    must reach the tail"""
    batch = batch_of(path_rows, np.array([1, 1, 3] * PATH_N)[:PATH_N], np.random.default_rng(9002))
    st = three_ways(ctx, "path/1-1-3", batch, L8, **SMALL)
    assert st["n_edges"] == st["n_candidates"] == PATH_N - 1  # (666 of them one-way)
    top = 2 * ((PATH_N + 1) // 2)
    comb = batch_of(path_rows, np.array([top - 2 * (i // 2) for i in range(PATH_N)]))
    st = three_ways(ctx, "path/comb", comb, L8, p=1.0, **SMALL)
    assert st["n_edges"] == PATH_N - 1 and st["n_kept"] == 1  # (499 of them one-way)


def test_key_twice_on_the_path(ctx, path_rows):
    """a key twice in the input: the super-bin is walked pair by pair and united as before"""
    rows = np.concatenate([path_rows, path_rows[500:501]])
    batch = batch_of(rows, np.ones(len(rows), np.int64), np.random.default_rng(9003))
    assert len(np.unique(batch[0])) == len(batch[0]) - 1
    st = three_ways(ctx, "path/twice", batch, L8, **SMALL)
    assert st["n_kept"] == 1


def star_rows(rng, n_fill=700):
    centre = int(rng.integers(0, 4 ** L8))
    star = [centre] + neighbours(centre, L8)
    fill = [int(c) for c in rng.choice(4 ** L8, n_fill, replace=False) if int(c) not in set(star)]
    return rows_of(star + fill, L8), len(star)


def test_star(ctx):
    """one code with all 24 neighbours there, among 700 others: symmetric (all freq 1), and with the centre on top
    (freq 9: 24 one-way pairs out of it)"""
    rng = np.random.default_rng(9004)
    rows, n_star = star_rows(rng)
    three_ways(ctx, "star/sym", batch_of(rows, np.ones(len(rows), np.int64), rng), L8, **SMALL)
    fr = np.ones(len(rows), np.int64)
    fr[0] = 9
    st = three_ways(ctx, "star/centre", batch_of(rows, fr, rng), L8, **SMALL)
    assert st["n_edges"] >= n_star - 1


def crowd(rng, n, free_bases, L=L8):
    """n distinct codes that vary in free_bases bases only: mean degree 3 * free_bases * n / 4^free_bases"""
    codes = rng.choice(4 ** free_bases, n, replace=False)
    rows = np.zeros((n, L), np.int64)
    rows[:, :free_bases] = rows_of(codes, free_bases)
    return rows[:, rng.permutation(L)] if free_bases < L else rows


def test_more_entries_than_threads(ctx):
    """1,500 entries in a 256-thread block, six records per thread, 4,096 codes to choose from (mean degree 6.6:
    one giant component across every stride); then 4,000 in a 1,024-thread block at the default cap"""
    rng = np.random.default_rng(9005)
    rows = crowd(rng, 1500, 6)
    fr = np.minimum(rng.geometric(0.5, len(rows)), 40)
    three_ways(ctx, "crowd/1500", batch_of(rows, np.ones(len(rows), np.int64), rng), L8, **SMALL)
    three_ways(ctx, "crowd/1500/freq", batch_of(rows, fr, rng), L8, **SMALL)
    rows = crowd(rng, 4000, 7)
    three_ways(ctx, "crowd/4000", batch_of(rows, np.minimum(rng.geometric(0.7, 4000), 40), rng), L8)


def sized_super_bins(rng, sizes, loose=()):
    """an L = 10 bucket whose super-bin j (bases 3 and 4 = j) has sizes[j] entries with random other bases; the
    super-bins in `loose` hold no two entries within one substitution"""
    rows = []
    for j, n in enumerate(sizes):
        if j in loose:
            codes, near = [], set()
            while len(codes) < n:
                c = int(rng.integers(0, 4 ** 8))
                if c not in near:
                    codes.append(c)
                    near.update([c] + neighbours(c, 8))
        else:
            codes = rng.choice(4 ** 8, n, replace=False)
        r8 = rows_of(codes, 8)
        r = np.zeros((n, 10), np.int64)
        r[:, :3], r[:, 5:] = r8[:, :3], r8[:, 3:]
        r[:, 3], r[:, 4] = j & 3, j >> 2
        rows.append(r)
    return np.concatenate(rows)


@pytest.fixture(scope="module")
def extremes():
    """sixteen super-bins: one of 2 entries (a pair), one of exactly the cap, one of cap + 1 (the tiles'), one of 200
    without any pair, twelve of ~1,200; to a part-1 bin of the crowded super-bin and to one of a taken one, entries
    that differ from one of theirs in base 0 (inside the super-bin) and in base 3 (across)"""
    rng = np.random.default_rng(9006)
    sizes = [2, 2048, 1200, 200, 1200, 1200, 2049] + [1200] * 9
    rows = sized_super_bins(rng, sizes, loose=(3,))
    rows[1] = rows[0]
    rows[1, 7] = (rows[0, 7] + 1) & 3  # the two of super-bin 0: one substitution apart
    extra = []
    for j in (6, 9):  # (a change of base 3 leads to other super-bins of ~1,200)
        mine = rows[(rows[:, 3] == (j & 3)) & (rows[:, 4] == (j >> 2))][0]
        for base in (0, 3):
            for d in (1, 2):
                e = mine.copy()
                e[base] = (e[base] + d) & 3
                extra.append(e)
    rows = np.unique(np.concatenate([rows, np.array(extra)]), axis=0)
    fr = np.minimum(rng.geometric(0.5, len(rows)), 40)
    return batch_of(rows, fr, rng)


def test_extremes_and_a_mixed_segment(ctx, extremes):
    """super-bins of 2, of the cap, of cap + 1 and without a pair; the scan's word says "not all taken", the drain
    decides the part-1 hits inside and across super-bins as before"""
    sizes = super_sizes(extremes[0], 5, 3)
    assert (sizes > 2048).sum() == 1 and sizes.min() == 2 and (sizes == 2048).sum() == 1 and (sizes == 200).sum() == 1
    assert 64 <= len(extremes[0]) // 16 <= 1536
    three_ways(ctx, "extremes", extremes, 10, **SMALL)
    three_ways(ctx, "extremes", extremes, 10, algo=CLUSTER, **SMALL)
    # (cap 2,049: the crowded one is taken as well, at exactly its size, by 1,024-thread blocks)
    three_ways(ctx, "extremes", extremes, 10, seg_super_min=64, seg_super_cap=int(sizes.max()))


@pytest.fixture(scope="module")
def all_taken():
    return deep_bucket(np.random.default_rng(9007), 20000, 10)


def test_every_super_bin_taken(ctx, all_taken):
    """sixteen super-bins of ~1,240, all below the cap: the tiles of part 1 leave out the hits inside them"""
    sizes = super_sizes(all_taken[0], 5, 3)
    assert sizes.max() <= 2048 and sizes.min() >= 2
    for p, algo in ((0.5, 0), (1.0, 0), (0.5, CLUSTER)):
        three_ways(ctx, "all_taken", all_taken, 10, p=p, algo=algo, **SMALL)


def test_non_sliced_walk(ctx, all_taken, extremes):
    """seg_sliced=0: the tiles compare a column at a time and the drain drops the hits inside a taken super-bin"""
    try:
        three_ways(ctx, "all_taken", all_taken, 10, seg_sliced=0, **SMALL)
        three_ways(ctx, "extremes", extremes, 10, seg_sliced=0, **SMALL)
    finally:
        ctx.set_option("seg_sliced", 1)


def test_cluster_on_the_path_and_on_a_random_super_bin(ctx, path_rows):
    rng = np.random.default_rng(9008)
    fr = np.minimum(rng.geometric(0.5, PATH_N), 40)
    st = three_ways(ctx, "path/cluster", batch_of(path_rows, fr, rng), L8, algo=CLUSTER, **SMALL)
    assert st["n_kept"] == 1
    rows = crowd(rng, 1400, 7)
    three_ways(ctx, "crowd/cluster", batch_of(rows, np.minimum(rng.geometric(0.5, 1400), 40), rng), L8, algo=CLUSTER, **SMALL)


@pytest.mark.parametrize("seed", range(20))
def test_random_super_bins(ctx, seed):
    """even seeds: 1,400 entries over 4^7 codes in a 256-thread block (mean degree 1.8); odd seeds: 3,800 over 4^8
    in a 1,024-thread block at the default cap (1.4, the flagship's); freqs mostly 1, so that most pairs are symmetric"""
    rng = np.random.default_rng(9100 + seed)
    if seed % 2 == 0:
        rows, opts = crowd(rng, 1400, 7), SMALL
    else:
        rows, opts = crowd(rng, 3800, 8), {}
    fr = np.minimum(rng.geometric(0.8, len(rows)), 40)
    algo = CLUSTER if seed % 5 == 4 else 0
    st = three_ways(ctx, "fuzz/%d" % seed, batch_of(rows, fr, rng), L8, algo=algo, **opts)
    assert st["n_candidates"] == count_pairs([code_of(r) for r in rows], L8)
