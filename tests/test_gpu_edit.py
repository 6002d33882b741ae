"""umi_dedup_batch_edit on the device against tests/edit_model.py: the Levenshtein distance by full DP, the
collapse from its definition.  The inputs hold UMIs that differ by a shift (tests/test_edit_model_cpu.py
counts the pairs only the edit distance joins), so a kernel that computed the Hamming distance fails here."""
import numpy as np
import pytest

import edit_model as em
from edit_model import batch

pytestmark = pytest.mark.gpu

SIZES = em.SIZES
LENGTHS = (1, 2, 6, 12, 20, 21)


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype).copy()).to("cuda:0")


def call_device(ctx, keys, nm, fr, off, L, **kw):
    import torch
    t_keys, t_fr = dev(keys), dev(fr)
    t_nm = dev(nm) if nm is not None else None
    kept = torch.zeros(max(1, len(keys)), dtype=torch.uint8, device="cuda:0")
    root = torch.zeros(max(1, len(keys)), dtype=torch.int32, device="cuda:0")
    st = ctx.dedup_batch_edit_device(t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0, t_fr.data_ptr(), off, L,
                                     kept.data_ptr(), root.data_ptr(), **kw)
    torch.cuda.synchronize()
    n = len(keys)
    return kept.cpu().numpy()[:n], root.cpu().numpy()[:n].view(np.uint32), st


def ks_of(L):
    return sorted({0, 1, 2, 3, L, L + 5, 2 ** 31 - 1})


@pytest.mark.parametrize("algo,amf", [(0, 0), (1, 0), (1, 3)])
@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("L", LENGTHS)
def test_parity_with_the_model(ctx, L, n_frac, algo, amf):
    buckets, mats, (keys, nm, fr, off) = batch(L, n_frac)
    for k in ks_of(L):
        ekept, eroot = em.model_batch(buckets, k, 0.5, algo, amf, mats)
        kept, root, st = ctx.dedup_batch_edit(keys, nm if n_frac else None, fr, off, L, k=k, algo=algo, adj_max_freq=amf)
        assert kept.tolist() == ekept.tolist(), (L, k, "host")
        assert root.tolist() == eroot.tolist(), (L, k, "host")
        assert st["n_kept"] == int(ekept.sum())
        kept, root, st = call_device(ctx, keys, nm, fr, off, L, k=k, algo=algo, adj_max_freq=amf)
        assert kept.tolist() == ekept.tolist(), (L, k, "device")
        assert root.tolist() == eroot.tolist(), (L, k, "device")


@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("L", LENGTHS)
def test_cross_check_against_the_hamming_path(ctx, L, n_frac):
    """d_E == d_H wherever either is at most 1, and k >= L means every pair under both."""
    _, _, (keys, nm, fr, off) = batch(L, n_frac)
    for algo, amf in ((0, 0), (1, 3)):
        for k_e, k_h in ((0, 0), (1, 1), (L, 128), (L + 5, 128), (2 ** 31 - 1, 128)):
            kept, root, _ = ctx.dedup_batch_edit(keys, nm, fr, off, L, k=k_e, algo=algo, adj_max_freq=amf)
            hkept, hroot, _ = ctx.dedup_batch(keys, nm, fr, off, L, k=k_h, algo=algo, adj_max_freq=amf)
            assert kept.tolist() == hkept.tolist() and root.tolist() == hroot.tolist(), (L, k_e, algo)


@pytest.fixture(scope="module")
def dense():
    umis, freq = em.same_composition_bucket(12, 600)
    return umis, freq, em.edit_matrix(umis), em.pack([(umis, freq)])


@pytest.mark.parametrize("k", [2, 12])
def test_queue_pressure(ctx, dense, k):
    """Every pair passes the count filter: the LDS queue fills at the highest rate there is."""
    umis, freq, d, (keys, nm, fr, off) = dense
    for algo, amf in ((0, 0), (1, 3)):
        ekept, eroot = em.model_batch([(umis, freq)], k, 0.5, algo, amf, [d])
        kept, root, st = ctx.dedup_batch_edit(keys, None, fr, off, 12, k=k, algo=algo, adj_max_freq=amf)
        assert st["n_candidates"] == st["n_pairs_evaluated"] == 600 * 599 // 2
        assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist(), (k, algo)


def test_edge_list_growth(dense):
    import umi_collapse_rs_amd as umi
    umis, freq, d, (keys, nm, fr, off) = dense
    c = umi.Context(0)
    try:
        c.set_option("edge_capacity", 64)
        for k, algo, amf in ((12, 0, 0), (2, 0, 0), (12, 1, 3)):
            ekept, eroot = em.model_batch([(umis, freq)], k, 0.5, algo, amf, [d])
            kept, root, st = c.dedup_batch_edit(keys, None, fr, off, 12, k=k, algo=algo, adj_max_freq=amf)
            assert st["n_edges"] > 1024
            assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist(), (k, algo)
    finally:
        c.close()


def test_many_small_positions(ctx):
    rng = np.random.default_rng(99)
    buckets = []
    for _ in range(2000):
        n = int(rng.integers(1, 131))
        buckets.append(em.shifted_bucket(rng, max(1, n // 3), 12, n_frac=0.01, n_max=n))
    keys, nm, fr, off = em.pack(buckets)
    assert sum(em.shift_only_pairs(u, 2) for u, _ in buckets[:200]) > 0
    ekept, eroot = em.model_batch(buckets, 2)
    kept, root, st = ctx.dedup_batch_edit(keys, nm, fr, off, 12, k=2)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
    assert st["n_buckets"] == 2000 and st["n_pairs"] == st["n_pairs_evaluated"]
    hkept, _, _ = ctx.dedup_batch(keys, nm, fr, off, 12, k=2)
    assert kept.tolist() != hkept.tolist()   # the Hamming path sees none of the shifts


def test_stats():
    import umi_collapse_rs_amd as umi
    buckets, _, (keys, nm, fr, off) = batch(12, 0.0)
    c = umi.Context(0, profile=True)
    try:
        for algo, amf in ((0, 0), (1, 3)):
            kept, _, st = c.dedup_batch_edit(keys, None, fr, off, 12, k=2, algo=algo, adj_max_freq=amf)
            w = sum(len(u) * (len(u) - 1) // 2 for u, _ in buckets)
            assert st["n_pairs"] == st["n_pairs_evaluated"] == w
            assert 0 < st["n_candidates"] <= w
            assert st["n_kept"] == int(kept.sum())
            assert st["n_umis"] == len(keys) and st["n_buckets"] == len(off) - 1 and st["max_bucket"] == 600
            assert st["kernel_id"] == umi.UMI_KERNEL_EDIT_PAIRS == 4
            assert st["ms_kernel"] > 0 and st["n_edges"] > 0 and st["n_rounds"] >= 1
    finally:
        c.close()


def test_errors(ctx):
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd._lib import UMI_ERR_ARG, UMI_ERR_ORDER
    _, _, (keys, nm, fr, off) = batch(12, 0.05)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.dedup_batch_edit(keys, nm, fr, off, 22, k=2)
    assert e.value.code == UMI_ERR_ARG
    with pytest.raises(umi.UmiHipError) as e:
        call_device(ctx, keys, nm, fr, off, 22, k=2)
    assert e.value.code == UMI_ERR_ARG
    multi = umi.Context([0, 0])
    try:
        with pytest.raises(umi.UmiHipError) as e:
            multi.dedup_batch_edit(keys, nm, fr, off, 12, k=2)
        assert e.value.code == UMI_ERR_ARG
        with pytest.raises(umi.UmiHipError) as e:
            call_device(multi, keys, nm, fr, off, 12, k=2)
        assert e.value.code == UMI_ERR_ARG
    finally:
        multi.close()
    rising = fr.copy()
    s = int(off[-3])   # the bucket of 600 (an empty one follows it)
    assert int(off[-2]) - s == 600
    rising[s + 5] = rising[s + 4] + 1
    with pytest.raises(umi.UmiHipError) as e:
        ctx.dedup_batch_edit(keys, nm, rising, off, 12, k=2)
    assert e.value.code == UMI_ERR_ORDER
    # an N code that a given nmask does not cover
    assert nm.any()
    with pytest.raises(umi.UmiHipError) as e:
        ctx.dedup_batch_edit(keys, np.zeros_like(nm), fr, off, 12, k=2)
    assert e.value.code == UMI_ERR_ORDER
    # ... and the same keys without any nmask are fine: code 100 is N
    kept, root, _ = ctx.dedup_batch_edit(keys, None, fr, off, 12, k=2)
    kept2, root2, _ = ctx.dedup_batch_edit(keys, nm, fr, off, 12, k=2)
    assert kept.tolist() == kept2.tolist() and root.tolist() == root2.tolist()


def test_with_a_deferred_call_out(ctx):
    """The edit call lets a deferred umi_dedup_batch_device_begin end first; its result still waits."""
    import torch
    rng = np.random.default_rng(5)
    small = [em.shifted_bucket(rng, 10, 12, n_max=40) for _ in range(300)]   # every position the fused kernel's
    skeys, snm, sfr, soff = em.pack(small)
    t = [dev(skeys), dev(snm), dev(sfr)]
    dkept = torch.zeros(len(skeys), dtype=torch.uint8, device="cuda:0")
    droot = torch.zeros(len(skeys), dtype=torch.int32, device="cuda:0")
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t[0].data_ptr(), t[1].data_ptr(), t[2].data_ptr(), soff, 12, dkept.data_ptr(),
                                 droot.data_ptr(), k=1, stream=stream.cuda_stream)
    buckets, mats, (keys, nm, fr, off) = batch(12, 0.05)
    ekept, eroot = em.model_batch(buckets, 2, mats=mats)
    kept, root, _ = ctx.dedup_batch_edit(keys, nm, fr, off, 12, k=2)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
    kept, root, _ = call_device(ctx, keys, nm, fr, off, 12, k=2)
    assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
    st = ctx.dedup_batch_end()
    stream.synchronize()
    hkept, hroot, hst = ctx.dedup_batch(skeys, snm, sfr, soff, 12, k=1)
    assert st["n_kept"] == hst["n_kept"] == int(hkept.sum())
    assert dkept.cpu().numpy().tolist() == hkept.tolist()
    assert droot.cpu().numpy().view(np.uint32).tolist() == hroot.tolist()
