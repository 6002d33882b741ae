"""umi_dedup_batch_edit pair by pair and at every k: the distance edit_pair_kernel takes between two keys is read off
through sweeps of k over buckets of two entries (the first k at which a pair merges is its distance), whole buckets
are compared with the model at every k of 0..L, and n_edges / n_candidates are compared with exact counts in every
call.  The inputs (tests/edit_model.py: adversarial_pairs, mixed_bucket, all_strings_bucket) hold pairs at every
distance 1..L in both orders -- the first entry of a pair is the row, Myers' pattern; the second the column, its
text -- pairs on the filter's bound and pairs that pass the filter and fail the check at every k;
tests/test_edit_model_cpu.py states what they hold.  Everything is integer equality."""
import functools

import numpy as np
import pytest

import cluster_model as cm
import edit_model as em

pytestmark = pytest.mark.gpu

DIR, ADJ, CLUSTER = 0, 1, 2
LENGTHS = (1, 2, 3, 6, 12, 20, 21)
ALGOS = {"directional": (DIR, 0), "adjacency": (ADJ, 3), "cluster": (CLUSTER, 0)}


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(np.int64 if a.dtype == np.uint64 else a.dtype).copy()).to("cuda:0")


def call(ctx, device, keys, nm, fr, off, L, **kw):
    """(kept, root, stats) of one call, by the host form or by dedup_batch_edit_device; nm may be None"""
    if not device:
        return ctx.dedup_batch_edit(keys, nm, fr, off, L, **kw)
    import torch
    n = len(keys)
    t_keys, t_fr = dev(keys), dev(fr)
    t_nm = dev(nm) if nm is not None else None
    kept = torch.zeros(max(1, n), dtype=torch.uint8, device="cuda:0")
    root = torch.zeros(max(1, n), dtype=torch.int32, device="cuda:0")
    st = ctx.dedup_batch_edit_device(t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0, t_fr.data_ptr(), off, L,
                                     kept.data_ptr(), root.data_ptr(), **kw)
    torch.cuda.synchronize()
    return kept.cpu().numpy()[:n], root.cpu().numpy()[:n].view(np.uint32), st


@functools.lru_cache(maxsize=None)
def pair_case(L):
    pairs = em.adversarial_pairs(L)
    d = np.array([em.levenshtein(a, b) for a, b in pairs])
    l1 = np.array([em.count_l1(a, b) for a, b in pairs])
    never = np.array([em.PAIR_FREQS[i % len(em.PAIR_FREQS)] == (3, 3) for i in range(len(pairs))])
    return pairs, d, l1, never, em.pair_buckets(pairs)


@pytest.mark.parametrize("L", LENGTHS)
def test_every_pair_distance_read_off_by_k(ctx, L):
    """One bucket per pair of adversarial_pairs(L), one directional call at p = 0.5 per k of 0..L+1 in ascending
    order: a (2, 1) or (1, 1) bucket merges iff d_E(a, b) <= k, so the first k at which it does is the distance
    the kernel took, row a against column b; a (3, 3) bucket never merges and still goes through filter and check.
    Odd k run the device form; nmask is given at k = 0, 1 mod 4 and NULL at 2, 3."""
    pairs, d, l1, never, (keys, nm, fr, off) = pair_case(L)
    n = len(pairs)
    first = np.full(n, -1)
    before = np.zeros(n, bool)
    stats_wrong = []   # (the pairs are named first: the counts are asserted behind the sweep)
    for k in range(L + 2):
        kept, root, st = call(ctx, k % 2 == 1, keys, nm if k % 4 < 2 else None, fr, off, L, k=k)
        kept, root = kept.reshape(n, 2), root.reshape(n, 2)
        merged = kept[:, 1] == 0
        assert kept[:, 0].all(), (L, k)
        assert not merged[never].any(), (L, k, [pairs[i] for i in np.nonzero(merged & never)[0][:5]])
        assert (root[:, 0] == 2 * np.arange(n)).all(), (L, k)
        assert (root[:, 1] == 2 * np.arange(n) + np.where(merged, 0, 1)).all(), (L, k)
        assert not (before & ~merged).any(), (L, k, [pairs[i] for i in np.nonzero(before & ~merged)[0][:5]])
        first[merged & ~before] = k
        before = merged
        expected = dict(n_edges=int((~never & (d <= k)).sum()), n_candidates=int((l1 <= 2 * min(k, L)).sum()), n_pairs=n,
                        n_pairs_evaluated=n, n_kept=int(kept.sum()))
        print("L=%d k=%d: n_edges %d (model %d), n_candidates %d (model %d)" % (
            L, k, st["n_edges"], expected["n_edges"], st["n_candidates"], expected["n_candidates"]))
        stats_wrong += [(k, name, st[name], e) for name, e in expected.items() if st[name] != e]
    wrong = [(a, b, int(first[i]), int(d[i])) for i, (a, b) in enumerate(pairs) if not never[i] and first[i] != d[i]]
    assert not wrong, "%d pairs (a, b, got, expected), the first: %s" % (len(wrong), wrong[:10])
    assert not stats_wrong, "(k, counter, got, expected): %s" % stats_wrong[:10]


@functools.lru_cache(maxsize=None)
def whole_case(name):
    """[(L, buckets, distance matrices, count_l1 matrices, packed call)] of a case: one call of mixed buckets of
    every size for a length, or every string of length 4 and of length 3 as two calls of one bucket"""
    if name == "all_strings":
        return [(L,) + em.all_strings_batch(L) for L in (4, 3)]
    return [(int(name),) + em.whole_batch(int(name))]


@functools.lru_cache(maxsize=None)
def whole_model(name, algo_name):
    """per call of the case and k of 0..L: kept, root, n_edges, n_candidates"""
    algo, amf = ALGOS[algo_name]
    out = []
    for L, buckets, mats, l1s, (keys, nm, fr, off) in whole_case(name):
        per_k = []
        for k in range(L + 1):
            ekept, eroot = cm.batch(mats, off, k) if algo == CLUSTER else em.model_batch(buckets, k, 0.5, algo, amf, mats)
            per_k.append((ekept, eroot,
                          sum(em.permitted_pairs(m, f, k, 0.5, algo, amf) for m, (_, f) in zip(mats, buckets)),
                          sum(em.filter_hits(u, k, l1) for l1, (u, _) in zip(l1s, buckets))))
        out.append(per_k)
    return out


@pytest.mark.parametrize("algo_name", list(ALGOS))
@pytest.mark.parametrize("name", ["6", "12", "20", "21", "all_strings"])
def test_whole_buckets_at_every_k(ctx, name, algo_name):
    """em.whole_batch: mixed buckets of 2, 63, 64, 65, 129 and 330 entries (one row tile less one, one, one and an
    entry, two and an entry, five and a part) with empty buckets between them, at every k of 0..L; the case
    all_strings is every string of length 4 (625) and of length 3 (125), a bucket each, which hold every pair there
    is.  Result, n_kept, n_edges and n_candidates against the model."""
    algo, amf = ALGOS[algo_name]
    for (L, buckets, mats, l1s, (keys, nm, fr, off)), per_k in zip(whole_case(name), whole_model(name, algo_name)):
        w = sum(len(u) * (len(u) - 1) // 2 for u, _ in buckets)
        for k, (ekept, eroot, e_edges, e_cand) in enumerate(per_k):
            kept, root, st = call(ctx, False, keys, nm if k % 2 == 0 else None, fr, off, L, k=k, algo=algo, adj_max_freq=amf)
            what = (name, L, algo_name, k)
            print("%s: n_edges %d (model %d), n_candidates %d (model %d)" % (what, st["n_edges"], e_edges, st["n_candidates"], e_cand))
            assert kept.tolist() == ekept.tolist(), what
            assert root.tolist() == eroot.tolist(), what
            assert st["n_kept"] == int(ekept.sum()), what
            assert st["n_edges"] == e_edges, what
            assert st["n_candidates"] == e_cand, what
            assert st["n_pairs"] == st["n_pairs_evaluated"] == w, what


def test_edge_list_redo_at_a_middle_k():
    """A first edge list of 1,024 (edge_capacity 64 is raised to that) against the 330-entry bucket of L = 12 at
    k = 6, cluster: the pair kernel runs twice, and the second run's counts replace the first's; the context keeps the
    longer list, so its next call runs the kernel once."""
    import umi_collapse_rs_amd as umi
    umis, freq = em.mixed_bucket(12, 330, seed=330)
    d, l1 = em.edit_matrix(umis), em.count_l1_matrix(umis)
    keys, nm, fr, off = em.pack([(umis, freq)])
    ekept, eroot = cm.batch([d], off, 6)
    e_edges, e_cand = em.permitted_pairs(d, freq, 6, algo=CLUSTER), em.filter_hits(umis, 6, l1)
    assert e_edges > 1024
    c = umi.Context(0)
    try:
        c.set_option("edge_capacity", 64)
        for launches in (2, 1):
            kept, root, st = c.dedup_batch_edit(keys, nm, fr, off, 12, k=6, algo=CLUSTER)
            print("n_pair_launches %d, n_edges %d (model %d), n_candidates %d (model %d)" % (
                st["n_pair_launches"], st["n_edges"], e_edges, st["n_candidates"], e_cand))
            assert st["n_pair_launches"] >= 2 if launches == 2 else st["n_pair_launches"] == 1, st
            assert st["n_edges"] == e_edges and st["n_candidates"] == e_cand, st
            assert kept.tolist() == ekept.tolist() and root.tolist() == eroot.tolist()
            assert st["n_kept"] == int(ekept.sum())
    finally:
        c.close()
