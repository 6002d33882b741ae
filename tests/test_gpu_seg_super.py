"""Runs of adjacent part-0 sub-buckets decided as one unit in LDS (seg_super_kernel, options seg_super,
seg_super_bases, seg_super_cap, seg_super_min): the kept mask and the roots equal the oracle's with the option on
and off, n_kept is right, and the statistics that count pairs and edges do not move.  Every case runs directional
at p = 0.5 and p = 1.0 and once as connected components.  Cases: L = 10 (super-bins of 64, 16 and 4 bins) and
L = 12 (4 bins, several super-bins per block), super-bins above and below the cap in one call and a call where
none is taken, a key twice in the input (the walk instead of the lookups), a clustered position, one-way pairs
beyond a wave's private slot, segments and calls the path is not planned for, a call without root, option bounds."""
import numpy as np
import pytest

import oracle as orc
from helpers import canonical
from test_gpu_seg_local import deep_bucket, join, mid_buckets

pytestmark = pytest.mark.gpu

CLUSTER = 2  # UMI_ALGO_CLUSTER
MODES = [(0.5, 0), (1.0, 0), (0.5, CLUSTER)]
DEFAULTS = dict(seg_super=1, seg_super_bases=0, seg_super_cap=5632, seg_super_min=1024)
COUNTED = ("n_edges", "n_candidates", "n_pairs_evaluated", "n_kept")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


_oracle = {}


def oracle_of(name, batch, L, k, p, algo):
    """the oracle's answer for a named input, computed once (connected components: its directional algorithm with
    every pair within k permitted both ways, p = inf, as tests/test_gpu_cluster.py takes it)"""
    key = (name, L, k, p, algo)
    if key not in _oracle:
        keys, nm, fr, off = batch
        okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, k, float("inf") if algo == CLUSTER else p, 0, 0)
        _oracle[key] = (okept, oroot)
    return _oracle[key]


def call(c, batch, L, k, p, algo, want_root=True, **opts):
    keys, nm, fr, off = batch
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        return c.dedup_batch(keys, nm if nm.any() else None, fr, off, L, k, p, algo, 0, want_root=want_root)
    finally:
        for name, v in DEFAULTS.items():
            c.set_option(name, v)


def on_and_off(c, name, batch, L, k=1, modes=MODES, **opts):
    """seg_super 1 (with opts) and 0 against the oracle, bit for bit; the counted statistics equal.  Returns the
    statistics of the runs with the path on."""
    out = []
    for p, algo in modes:
        okept, oroot = oracle_of(name, batch, L, k, p, algo)
        sts = []
        for on in (1, 0):
            kept, root, st = call(c, batch, L, k, p, algo, **dict(opts, seg_super=on))
            what = "%s p=%g algo=%d seg_super=%d %s" % (name, p, algo, on, opts)
            assert (kept == okept).all(), "%s: kept differs at %s" % (what, np.nonzero(kept != okept)[0][:10])
            assert (root == oroot).all(), "%s: root differs at %s" % (what, np.nonzero(root != oroot)[0][:10])
            assert st["n_kept"] == int(okept.sum()), what
            sts.append(st)
        for f in COUNTED:
            assert sts[0][f] == sts[1][f], (name, p, algo, opts, f, sts[0][f], sts[1][f])
        out.append(sts[0])
    return out


def base_of(keys, b):
    """base b of every key (2 bits: the low two of its 3-bit code)"""
    return ((keys >> np.uint64(3 * b)) & np.uint64(3)).astype(np.int64)


def super_sizes(keys, nb0, g):
    """entries per super-bin of a one-bucket input: the values of bases g .. nb0 - 1"""
    code = np.zeros(len(keys), np.int64)
    for b in range(g, nb0):
        code |= base_of(keys, b) << (2 * (b - g))
    return np.bincount(code, minlength=4 ** (nb0 - g))


def bucket_of(raw, rng, freq=None):
    """one bucket of the distinct rows of raw, in rank order"""
    umis = sorted({"".join("ACGT"[c] for c in r) for r in raw})
    rng.shuffle(umis)
    fr = np.minimum(rng.geometric(0.5, len(umis)), 40).tolist() if freq is None else freq(len(umis))
    umis, fr, _ = canonical(umis, fr)
    keys, nm = orc.encode_keys(umis)
    return keys, nm, np.array(fr, np.int32), np.array([0, len(umis)], np.uint64)


def three_classes(n):
    """7 / 3 / 1 in thirds of the rank order: at p = 0.5 two of three pairs are one-way, one in nine symmetric"""
    return [7] * (n // 3) + [3] * (n // 3) + [1] * (n - 2 * (n // 3))


@pytest.fixture(scope="module")
def l10():
    return deep_bucket(np.random.default_rng(700), 40000, 10)


@pytest.fixture(scope="module")
def l12():
    rng = np.random.default_rng(701)
    return join(deep_bucket(rng, 40000, 12), deep_bucket(rng, 20000, 12))


@pytest.mark.parametrize("bases", [0, 1, 2])
def test_l10_super_bins_of_64_16_and_4_bins(ctx, l10, bases):
    """~39,000 entries, 1,024 part-0 bins, 5 bases outside them: the planner takes g = 3 (16 super-bins of ~2,450);
    forced g = 2 and g = 1 need seg_super_min below their super-bins of ~610 and ~150"""
    sizes = super_sizes(l10[0], 5, bases or 3)
    assert sizes.min() >= 2 and sizes.max() <= 5632 * 3 // 4
    sts = on_and_off(ctx, "l10", l10, 10, seg_super_bases=bases, seg_super_min=1024 if bases == 0 else 64)
    assert all(st["n_edges"] > 0 for st in sts[:1])


def test_l12_many_small_super_bins_per_block(ctx, l12):
    """positions of ~40,000 and ~20,000: g = 1 is all that 7 bases outside the bins leave; 512 super-bins of ~156 and
    ~78 entries, more than there are CUs, in 256-thread blocks (cap 2,048) and in 1,024-thread ones (the default cap)"""
    on_and_off(ctx, "l12", l12, 12, seg_super_min=64, seg_super_cap=2048)
    on_and_off(ctx, "l12", l12, 12, seg_super_min=64, modes=MODES[:1])


def test_taken_and_not_taken_super_bins_in_one_call(ctx):
    """L = 10 with one crowded super-bin (bases 3 and 4 = AA, ~4,600 entries among fifteen of ~1,100): at cap 2,048
    it stays with the pair kernel's tiles while the others are taken, by 256-thread blocks -- both branches of the
    pair kernel's dedupe clause in one call"""
    rng = np.random.default_rng(702)
    raw = rng.integers(0, 4, (21600, 10))
    raw[18000:, 3:5] = 0
    batch = bucket_of(raw, rng)
    sizes = super_sizes(batch[0], 5, 3)
    cap = 2048
    assert (sizes > cap).sum() == 1 and (sizes <= cap).sum() == 15 and len(batch[0]) // 16 <= cap // 4 * 3
    on_and_off(ctx, "l10_mixed", batch, 10, seg_super_cap=cap)


def test_no_super_bin_taken(ctx):
    """L = 10 with base 3 fixed: four super-bins of ~4,800 entries, all above a cap of 4,096, twelve empty -- the path
    is planned (the expected super-bin is n / 16) and takes nothing"""
    rng = np.random.default_rng(703)
    raw = rng.integers(0, 4, (20000, 10))
    raw[:, 3] = 0
    batch = bucket_of(raw, rng)
    sizes = super_sizes(batch[0], 5, 3)
    assert ((sizes == 0) | (sizes > 4096)).all() and 1024 <= len(batch[0]) // 16 <= 4096 // 4 * 3
    on_and_off(ctx, "l10_none", batch, 10, seg_super_cap=4096)


def test_key_twice_in_a_super_bin(ctx):
    """a key may stand twice in the input: its super-bin is walked pair by pair, the equal keys a hit at distance 0.
    (Both copies have freq 1: a symmetric pair, so whatever removes or keeps the first copy takes the second along,
    and the reference's map from UMI to freq holds the same freq whichever copy it saw last.)"""
    rng = np.random.default_rng(704)
    keys, nm, fr, off = deep_bucket(rng, 20000, 10)  # (16 super-bins of ~1,240)
    again = rng.choice(np.nonzero(fr == 1)[0], 40, replace=False)
    k2 = np.concatenate([keys, keys[again]])
    f2 = np.concatenate([fr, np.ones(len(again), np.int32)])
    order = np.lexsort((np.arange(len(k2)), -f2))
    batch = (k2[order], np.zeros_like(k2), f2[order], np.array([0, len(k2)], np.uint64))
    assert len(np.unique(batch[0])) < len(batch[0])
    on_and_off(ctx, "l10_twice", batch, 10)
    on_and_off(ctx, "l10_twice", batch, 10, modes=MODES[:1], seg_super_bases=2, seg_super_min=64)


def test_clustered_position(ctx):
    """the clustered input of test_gpu_seg_local (a true UMI of high freq among its error copies): skewed
    super-bins of four bins; then with freqs of three classes, most pairs one-way"""
    from umi_collapse_rs_amd import synth
    st = synth.config2m(seed=31, n_reads=60000, umi_len=12, n_molecules=6000, err=0.02)
    keys = st["keys"]
    batch = (keys, np.zeros_like(keys), st["freq"], st["bucket_off"])
    on_and_off(ctx, "clustered", batch, 12, seg_super_min=16)
    one_way = (keys, np.zeros_like(keys), np.array(three_classes(len(keys)), np.int32), st["bucket_off"])
    sts = on_and_off(ctx, "clustered_one_way", one_way, 12, seg_super_min=16)
    assert sts[0]["n_edges"] > 0


def test_one_way_pairs_beyond_a_waves_slot(ctx):
    """L = 8, ~22,000 of the 65,536 keys, freqs of three classes: 16 super-bins (g = 2) of ~1,400 entries in
    256-thread blocks, 64 private slots of 512 edges in all, and more one-way pairs inside the super-bins (three in
    four pairs differ in one of the 6 bases outside the shared ones) than the slots hold: some wave overflows"""
    rng = np.random.default_rng(705)
    batch = bucket_of(rng.integers(0, 4, (26000, 8)), rng, freq=three_classes)
    n = len(batch[0])
    assert 1024 <= n // 16 <= 2048 // 4 * 3
    sts = on_and_off(ctx, "l8_dense", batch, 8, seg_super_cap=2048)
    assert sts[0]["n_edges"] * 7 // 10 > 64 * 512


def test_segments_and_calls_the_path_is_not_planned_for(ctx, l12):
    """several segments in one call of which the small ones leave 9 bases outside their bins (no super-bins there:
    the one-wave kernel and the tiles as before); a call with N and a call at k = 2 (not planned at all)"""
    rng = np.random.default_rng(706)
    batch = join(mid_buckets(rng, 4, 12, 900), deep_bucket(rng, 20000, 12), mid_buckets(rng, 2, 12, 700))
    on_and_off(ctx, "l12_mixed_segments", batch, 12, seg_super_min=64)
    with_n = deep_bucket(rng, 20000, 10, 0.005)
    assert with_n[1].any()
    on_and_off(ctx, "l10_n", with_n, 10, modes=MODES[:1])
    on_and_off(ctx, "l12_k2", deep_bucket(rng, 20000, 12), 12, k=2, modes=MODES[:1])


def test_call_without_root(ctx, l10):
    for p, algo in MODES:
        kept, _, st = call(ctx, l10, 10, 1, p, algo)
        kept_only, none, st2 = call(ctx, l10, 10, 1, p, algo, want_root=False)
        assert none is None and (kept == kept_only).all()
        for f in COUNTED:
            assert st[f] == st2[f], (f, st[f], st2[f])


def test_option_bounds(ctx):
    import umi_collapse_rs_amd as umi
    bad = {"seg_super": (-1, 2), "seg_super_bases": (-1, 5), "seg_super_cap": (0, 1, 8193, 1 << 20),
           "seg_super_min": (0, 1, 8193)}
    for name, values in bad.items():
        for v in values:
            with pytest.raises(umi.UmiHipError):
                ctx.set_option(name, v)
    for name, v in list(dict(seg_super_bases=4, seg_super_cap=8192, seg_super_min=2).items()) + list(DEFAULTS.items()):
        ctx.set_option(name, v)
