"""The segment index's part-0 sub-buckets united in LDS (seg_local_kernel, option seg_local): the
kept mask and the roots equal the oracle's with the option on and off, and the statistics that
count pairs and edges do not move.  Cases: several k and umi lengths, N bases, a forced fallback
(small seg_local_cap) and calls that mix sub-buckets above and below the cap, several segments in
one call, a config-2-sized uniform position and a clustered one (against the path without the
local kernel: the oracle is O(n^2)), and the paths the option must leave alone."""
import numpy as np
import pytest

import oracle as orc
from helpers import canonical, random_bucket

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def deep_bucket(rng, n_raw, L, n_frac=0.0):
    raw = rng.integers(0, 4, (n_raw, L))
    if n_frac:
        raw = np.where(rng.random(raw.shape) < n_frac, 4, raw)
    umis = sorted({"".join("ACGTN"[c] for c in r) for r in raw})
    rng.shuffle(umis)
    freq = np.minimum(rng.geometric(0.5, len(umis)), 40).tolist()
    umis, freq, _ = canonical(umis, freq)
    keys, nm = orc.encode_keys(umis)
    return keys, nm, np.array(freq, np.int32), np.array([0, len(umis)], np.uint64)


def mid_buckets(rng, n_buckets, L, n_mol, n_frac=0.0):
    keys, nm, fr, off = [], [], [], [0]
    for _ in range(n_buckets):
        umis, freq = random_bucket(rng, n_mol, L, err=0.05, n_frac=n_frac)
        umis, freq, _ = canonical(umis, freq)
        k, m = orc.encode_keys(umis)
        keys.append(k); nm.append(m); fr.extend(freq)
        off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


def join(*batches):
    keys = np.concatenate([b[0] for b in batches])
    nm = np.concatenate([b[1] for b in batches])
    fr = np.concatenate([b[2] for b in batches])
    off = [np.zeros(1, np.uint64)]
    for b in batches:
        off.append(off[-1][-1] + b[3][1:])
    return keys, nm, fr, np.concatenate(off).astype(np.uint64)


def run(c, batch, L, k, p=0.5, algo=0, amf=0, **opts):
    keys, nm, fr, off = batch
    for name, v in opts.items():
        c.set_option(name, v)
    return c.dedup_batch(keys, nm if nm.any() else None, fr, off, L, k, p, algo, amf)


def both_against_oracle(c, batch, L, k, p=0.5, algo=0, amf=0, **opts):
    """seg_local 1 and 0 against the oracle, bit for bit; the counted statistics equal"""
    keys, nm, fr, off = batch
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, k, p, algo, amf)
    sts = []
    try:
        for local in (1, 0):
            kept, root, st = run(c, batch, L, k, p, algo, amf, seg_local=local, **opts)
            assert (kept == okept).all(), "seg_local=%d: kept differs at %s" % (local, np.nonzero(kept != okept)[0][:10])
            assert (root == oroot).all(), "seg_local=%d: root differs at %s" % (local, np.nonzero(root != oroot)[0][:10])
            assert st["n_kept"] == int(okept.sum())
            sts.append(st)
    finally:
        c.set_option("seg_local", 1)
        c.set_option("seg_local_cap", 512)
    for f in ("n_edges", "n_pairs_evaluated", "n_kept", "n_candidates"):
        assert sts[0][f] == sts[1][f], (f, sts[0][f], sts[1][f])
    return sts[0]


@pytest.mark.parametrize("L,k,n_raw,n_frac", [(12, 1, 40000, 0.0), (12, 2, 40000, 0.0), (12, 3, 30000, 0.0),
                                              (12, 1, 40000, 0.005)])
def test_l12(ctx, L, k, n_raw, n_frac):
    rng = np.random.default_rng(400 + k + int(n_frac * 1000))
    st = both_against_oracle(ctx, deep_bucket(rng, n_raw, L, n_frac), L, k)
    assert st["n_edges"] > 0


@pytest.mark.parametrize("n_frac", [0.0, 0.01])
def test_l20_k2_with_and_without_n(ctx, n_frac):
    rng = np.random.default_rng(420 + int(n_frac * 100))
    # a deep position (bins of a few entries at L = 20) next to clustered mid-size ones
    batch = join(mid_buckets(rng, 4, 20, 700, n_frac), deep_bucket(rng, 30000, 20, n_frac))
    both_against_oracle(ctx, batch, 20, 2)


@pytest.mark.parametrize("cap", [2, 40, 64, 65, 200])
def test_forced_fallback_and_mixed_bins(ctx, cap):
    """A small cap sends some or all part-0 bins back to the pair kernel's tiles and global unions,
    in the same call as the bins the local kernel takes; several segments of 512-2,000 entries."""
    rng = np.random.default_rng(430 + cap)
    batch = join(mid_buckets(rng, 5, 12, 900), deep_bucket(rng, 40000, 12), mid_buckets(rng, 3, 10, 1500))
    both_against_oracle(ctx, batch, 12, 1, seg_local_cap=cap)
    both_against_oracle(ctx, batch, 12, 1, p=1.0, seg_local_cap=cap)


def test_clustered_position_against_oracle(ctx):
    """Clustered UMIs (a true UMI of high freq with its error copies): skewed bins, some beyond the cap."""
    from umi_collapse_rs_amd import synth
    st = synth.config2m(seed=31, n_reads=60000, umi_len=12, n_molecules=6000, err=0.02)
    keys = st["keys"]
    batch = (keys, np.zeros_like(keys), st["freq"], st["bucket_off"])
    both_against_oracle(ctx, batch, 12, 1)
    both_against_oracle(ctx, batch, 12, 1, seg_local_cap=64)


@pytest.mark.parametrize("shape", ["2", "2m"])
def test_config2_sized_positions(ctx, shape):
    """1 M reads at one position: bit for bit the path without the local kernel, same statistics,
    and the structure of a directional result."""
    from umi_collapse_rs_amd import synth
    st = synth.config2(seed=2, n_reads=1_000_000, umi_len=12) if shape == "2" else \
        synth.config2m(seed=22, n_reads=1_000_000, umi_len=12)
    keys = st["keys"]
    batch = (keys, np.zeros_like(keys), st["freq"], st["bucket_off"])
    res = []
    try:
        for local in (1, 0):
            res.append(run(ctx, batch, 12, 1, seg_local=local))
    finally:
        ctx.set_option("seg_local", 1)
    (k1, r1, s1), (k0, r0, s0) = res
    assert (k1 == k0).all() and (r1 == r0).all()
    for f in ("n_edges", "n_pairs_evaluated", "n_kept", "n_candidates"):
        assert s1[f] == s0[f], (f, s1[f], s0[f])
    idx = np.arange(len(keys), dtype=np.uint32)
    assert ((k1 == 1) == (r1 == idx)).all() and (r1[r1] == r1).all() and (r1 <= idx).all()


def test_paths_the_option_leaves_alone(ctx):
    """seg_unite = 0 (symmetric pairs through the list), adjacency, the DataStruct neighbour lists and
    the multi-GPU split's partial pairs: the same with seg_local on and off."""
    import torch
    import umi_collapse_rs_amd as umi
    rng = np.random.default_rng(450)
    batch = join(mid_buckets(rng, 3, 12, 800), deep_bucket(rng, 30000, 12))
    both_against_oracle(ctx, batch, 12, 1, seg_unite=0)
    ctx.set_option("seg_unite", 1)
    both_against_oracle(ctx, batch, 12, 1, algo=1, amf=2)
    # neighbour lists (MODE_NEIGHBOURS, one segment of ~4,000 entries): remove_near answers equal
    raw = rng.integers(0, 4, (6000, 8))
    umis = sorted({"".join("ACGT"[c] for c in r) for r in raw})
    answers = []
    for local in (1, 0):
        ctx.set_option("seg_local", local)
        d = umi.HipNaive.new({u: 1 for u in umis}, 8, 1, ctx=ctx)
        answers.append([sorted(d.remove_near(u, 1, 1 << 30)) for u in umis[::500]])
    ctx.set_option("seg_local", 1)
    assert answers[0] == answers[1] and sum(len(a) for a in answers[0]) > 0
    # the split's partial pair lists: same edges with the option on and off
    keys, nm, fr, off = batch
    dev = torch.device("cuda:0")
    t_keys = torch.from_numpy(keys.view(np.int64)).to(dev)
    t_fr = torch.from_numpy(fr).to(dev)
    cap = 1 << 22
    lists = []
    for local in (1, 0):
        ctx.set_option("seg_local", local)
        part_lists = []
        for part in range(2):
            buf = torch.zeros(cap, dtype=torch.int64, device=dev)
            ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), 0, t_fr.data_ptr(), off, 12, part, 2,
                                             buf.data_ptr(), cap, k=1)
            part_lists.append(np.sort(buf[:ne].cpu().numpy()))
        lists.append(part_lists)
    ctx.set_option("seg_local", 1)
    for a, b in zip(lists[0], lists[1]):
        assert (a == b).all()


def test_option_bounds(ctx):
    import umi_collapse_rs_amd as umi
    for bad in (0, 1, 4097, 1 << 20):
        with pytest.raises(umi.UmiHipError):
            ctx.set_option("seg_local_cap", bad)
    ctx.set_option("seg_local_cap", 2048)
    ctx.set_option("seg_local_cap", 512)
