"""tests/cluster_model.py, the definition of `--algo cluster` / UMI_ALGO_CLUSTER, checked on the CPU:
union-find against breadth-first search, both against the oracle's directional mode at percentage = inf (equal
while freq < 2^31 - 1, and a case at 2^31 - 1 where they differ: why the model is the definition and not the
oracle), and the package's Cluster class over a plain-Python DataStruct."""
import numpy as np
import pytest

import cluster_model as cm
import edit_model as em
import oracle as orc
from helpers import canonical, clustered_bucket, hamming_matrix

INF = float("inf")
SIZES = (1, 2, 3, 17, 64, 65, 128, 200)


def buckets_of(L, n_frac, seed, top=None):
    """Buckets of SIZES entries (fewer where 4^L runs out) in rank order; top: the largest freq, given to rank 0
    of every bucket."""
    rng = np.random.default_rng(7100 + 10 * L + seed)
    out = []
    for n in SIZES:
        umis, freq = clustered_bucket(rng, min(n, 4 ** L // 2), L, n_frac)
        if top:
            freq = [top] + freq[1:]
        out.append((umis, freq))
    return out


def assemble(buckets, wide):
    umis = [u for b in buckets for u in b[0]]
    fr = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    keys, nm = (orc.encode_keys_wide if wide else orc.encode_keys)(umis)
    return keys, nm, fr, off


@pytest.mark.parametrize("k", [0, 1, 2, 3])
@pytest.mark.parametrize("n_frac", [0.0, 0.3])
@pytest.mark.parametrize("L", [4, 5, 6, 7, 8, 9, 10, 11, 12, 24])
def test_model_two_formulations_and_the_oracle_at_p_inf(L, n_frac, k):
    """Union-find = BFS = orc.dedup_batch[_wide](percentage = inf, algo = 0), kept and root, with freq up to
    2^31 - 2; the character-level Hamming matrix and the word arithmetic give the same graph."""
    buckets = buckets_of(L, n_frac, k, top=2 ** 31 - 2)
    keys, nm, fr, off = assemble(buckets, L > 21)
    assert int(fr.max()) == 2 ** 31 - 2
    mats = [hamming_matrix(b[0]) for b in buckets]
    kept, root = cm.batch(mats, off, k)
    for b, d in enumerate(mats):
        s = int(off[b])
        assert np.array_equal(cm.components_bfs(d, k) + s, root[s:s + len(d)])
        assert np.array_equal(cm.word_distance(keys[s:s + len(d)], nm[s:s + len(d)]), d)
    assert np.array_equal(root[kept == 1], np.nonzero(kept)[0])
    run = orc.dedup_batch_wide if L > 21 else orc.dedup_batch
    okept, oroot, _ = run(keys, nm if nm.any() else None, fr, off, L, k, INF, 0)
    assert np.array_equal(okept, kept) and np.array_equal(oroot, root)
    assert (n_frac > 0) == bool(nm.any())
    if k >= 1 and L <= 8:
        assert kept.sum() < len(kept)  # (something is removed at all)


def test_model_edit_distance_matrix():
    """The model takes any distance matrix: over edit_matrix the two formulations agree, and at k = 2 the edit
    graph joins entries the Hamming graph leaves apart."""
    rng = np.random.default_rng(7201)
    umis, _ = em.shifted_bucket(rng, 40, 12, n_max=150)
    de, dh = em.edit_matrix(umis), em.hamming_matrix(umis)
    for k in (0, 1, 2, 3):
        assert np.array_equal(cm.components(de, k), cm.components_bfs(de, k))
    assert np.array_equal(cm.components(de, 1), cm.components(dh, 1))
    assert cm.kept_of(cm.components(de, 2)).sum() < cm.kept_of(cm.components(dh, 2)).sum()


def test_oracle_differs_at_int32_max():
    """freq = 2^31 - 1: freq + 1 wraps in the reference, inf * (a negative number) saturates to INT32_MIN, and
    the oracle's directional entry removes nothing.  The component does not care."""
    umis, fr = ["ACGTACGT", "ACGTACGA"], np.array([2 ** 31 - 1, 5], np.int32)
    keys, _ = orc.encode_keys(umis)
    off = np.array([0, 2], np.uint64)
    okept, _, _ = orc.dedup_batch(keys, None, fr, off, 8, 1, INF, 0)
    kept, root = cm.batch([hamming_matrix(umis)], off, 1)
    assert okept.tolist() == [1, 1]
    assert kept.tolist() == [1, 0] and root.tolist() == [0, 0]


@pytest.mark.parametrize("k", [1, 2])
@pytest.mark.parametrize("n", [50, 300])
def test_cluster_class_over_a_python_datastruct(n, k):
    """umi_collapse_rs_amd.Cluster.apply with a plain-Python DataStruct: the reads it returns are the model's
    kept entries in rank order, the tracked clusters the model's components."""
    from umi_collapse_rs_amd import Cluster, ReadFreq
    rng = np.random.default_rng(7300 + n + k)
    umis, freq = clustered_bucket(rng, n, 8, 0.0)
    perm = rng.permutation(len(umis)).tolist()  # (first-appearance order is not rank order)
    reads = {umis[i]: ReadFreq("read%d" % i, freq[i]) for i in perm}
    ranked, _, _ = canonical([umis[i] for i in perm], [freq[i] for i in perm])
    root = cm.components(hamming_matrix(ranked), k)
    exp = [reads[ranked[i]].read for i in np.nonzero(cm.kept_of(root))[0]]
    naive = cm.PyNaive.of(lambda a, b: sum(x != y for x, y in zip(a, b)))
    tracker = {}
    got = Cluster(k=k, percentage=float("nan"), track_cluster=True).apply(reads, tracker, 8, data_struct=naive)
    assert got == exp
    members = {ranked[r]: sorted(ranked[i] for i in np.nonzero(root == r)[0]) for r in np.nonzero(cm.kept_of(root))[0]}
    assert {u: sorted(v) for u, v in tracker.items()} == members
