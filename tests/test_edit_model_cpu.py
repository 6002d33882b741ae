"""The Levenshtein model of tests/edit_model.py and what the edit-distance kernel rests on, without a GPU:
known answers, d_E against d_H, the count filter's bound, the bit-vector recurrence restated in Python,
the test inputs (they must hold pairs that only the edit distance joins), and the program's refusals."""
import os
import subprocess

import numpy as np
import pytest

import edit_model as em
from helpers import brute_directional

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def random_pairs(seed, n):
    """Seeded pairs of equal-length UMIs over ATCGN, lengths 1..21: half unrelated, half a few substitutions
    and window shifts apart."""
    rng = np.random.default_rng(seed)
    letters = "ACGTN"
    out = []
    for _ in range(n):
        L = int(rng.integers(1, 22))
        a = "".join(letters[c] for c in rng.integers(0, 5, L))
        if rng.random() < 0.5:
            b = list(a)
            for _ in range(int(rng.integers(0, 4))):
                i = int(rng.integers(0, L))
                r = rng.random()
                c = letters[int(rng.integers(0, 5))]
                if r < 0.33:
                    b[i] = c
                elif r < 0.66:
                    b = b[:i] + b[i + 1:] + [c]
                else:
                    b = (b[:i] + [c] + b[i:])[:L]
            b = "".join(b)
        else:
            b = "".join(letters[c] for c in rng.integers(0, 5, L))
        out.append((a, b))
    return out


PAIRS = random_pairs(20260, 4000)


def test_known_answers():
    assert em.levenshtein("ACGTACGTACGT", "CGTACGTACGTA") == 2   # one base lost: d_H is 12
    assert em.hamming("ACGTACGTACGT", "CGTACGTACGTA") == 12
    assert em.levenshtein("N", "N") == 0
    assert em.levenshtein("N", "A") == 1
    assert em.levenshtein("A", "A") == 0 and em.levenshtein("A", "C") == 1   # L = 1
    a = "ACGTACGTACGTACGTACGTA"                                               # L = 21
    assert em.levenshtein(a, a) == 0
    assert em.levenshtein(a, a[1:] + "C") == 2
    assert em.levenshtein(a, "T" + a[:-1]) == 2
    assert em.levenshtein(a, "C" * 21) == 16
    assert em.levenshtein("ACNT", "ACGT") == 1 and em.levenshtein("ANNT", "ANNT") == 0
    assert em.levenshtein("AAAACCCC", "CCCCAAAA") == 8
    assert em.levenshtein("ACGT", "") == 4


def test_matrix_is_the_scalar_recurrence():
    rng = np.random.default_rng(3)
    for L in (1, 2, 7, 12, 21):
        umis = ["".join("ACGTN"[c] for c in rng.integers(0, 5, L)) for _ in range(12)]
        d = em.edit_matrix(umis)
        for i, a in enumerate(umis):
            for j, b in enumerate(umis):
                assert d[i, j] == em.levenshtein(a, b)


def test_edit_never_exceeds_hamming_and_equals_it_up_to_one():
    n_le1 = 0
    for a, b in PAIRS:
        d_e, d_h = em.levenshtein(a, b), em.hamming(a, b)
        assert d_e <= d_h
        if d_h <= 1 or d_e <= 1:
            assert d_e == d_h, (a, b)
            n_le1 += 1
    assert n_le1 > 100


def test_count_filter_is_a_lower_bound():
    """L1 of the A, C, G, T counts is at most 2 d_E: the filter rejects L1 > 2 k."""
    tight = 0
    for a, b in PAIRS:
        d = em.levenshtein(a, b)
        assert em.count_l1(a, b) <= 2 * d, (a, b)
        tight += em.count_l1(a, b) == 2 * d and d > 0
    assert tight > 0   # (the bound is reached: 2 k cannot be lowered)


def test_bit_vector_recurrence_is_the_dp():
    for a, b in PAIRS:
        assert em.myers_global(a, b) == em.levenshtein(a, b), (a, b)
    for L in (1, 2, 20, 21):   # the register's ends
        for a, b in (("A" * L, "A" * L), ("A" * L, "C" * L), ("N" * L, "N" * L), ("N" * L, "A" * L),
                     (("AC" * 11)[:L], ("CA" * 11)[:L])):
            assert em.myers_global(a, b) == em.levenshtein(a, b), (a, b)


def test_generators_hold_pairs_only_the_edit_distance_joins():
    rng = np.random.default_rng(11)
    for L, k in ((6, 2), (12, 2), (12, 3), (20, 2), (21, 3)):
        umis, freq = em.shifted_bucket(rng, 60, L, n_frac=0.02)
        assert len(set(umis)) == len(umis) and freq == sorted(freq, reverse=True)
        assert em.shift_only_pairs(umis, k) > 0, (L, k)
    umis, freq = em.same_composition_bucket(12, 600)
    assert len(set(umis)) == 600 and freq == sorted(freq, reverse=True)
    assert all(em.letter_counts(u) == [6, 6, 0, 0] for u in umis)
    d = em.edit_matrix(umis)
    assert em.shift_only_pairs(umis, 2, d) > 0
    assert ((d <= 2).sum() - 600) // 2 > 0 and (d > 2).any()   # k = 2 decides: some pairs in, some out


def test_model_differs_from_the_hamming_model_at_k2():
    rng = np.random.default_rng(12)
    differ = 0
    for _ in range(5):
        umis, freq = em.shifted_bucket(rng, 50, 12)
        surv_e, _ = em.brute_directional_edit(umis, freq, 2, 0.5)
        surv_h, _ = brute_directional(umis, freq, 2, 0.5)
        assert set(surv_e) <= set(surv_h)   # d_E <= d_H: more edges, no fewer removals
        differ += surv_e != surv_h
        # ... and k = 1 is the Hamming result
        assert em.brute_directional_edit(umis, freq, 1, 0.5) == brute_directional(umis, freq, 1, 0.5)
    assert differ > 0


def test_encode_decode_round_trip():
    umis = ["ACGTN", "NNNNN", "TTTTT"]
    keys, nm = em.encode(umis)
    assert em.decode(keys, 5) == umis
    import oracle as orc
    ok, om = orc.encode_keys(umis)
    assert (keys == ok).all() and (nm == om).all()


@pytest.mark.parametrize("argv", [
    ["--distance", "levenshtein"],
    ["--distance", "levenshtein", "-i", "in.bam", "-o", "out.bam"],
    ["-m", "fastq", "--distance", "edit", "-i", "in.fq", "-o", "out.fq"],
    ["--distance", "edit", "--devices", "0,1", "-i", "in.bam", "-o", "out.bam"],
    ["--distance", "edit", "-u", "22", "-i", "in.bam", "-o", "out.bam"],
])
def test_program_refuses_before_the_gpu(argv, tmp_path):
    r = subprocess.run([CLI] + argv, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 101, r.stderr
    assert "--distance" in r.stderr
    assert not os.listdir(tmp_path)


def test_program_refuses_a_long_whitelist(tmp_path):
    wl = tmp_path / "wl.txt"
    wl.write_text("ACGTACGTACGTACGTACGTAC\n")
    r = subprocess.run([CLI, "--distance", "edit", "--umi-whitelist", str(wl), "-i", "in.bam", "-o", "out.bam"],
                       cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 101 and "21 bases" in r.stderr, r.stderr


def test_help_names_the_flag_and_the_k_note():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--distance" in r.stdout and "hamming or edit" in r.stdout and "-k 2" in r.stdout


def test_library_exports_the_edit_entry_points():
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    lib = umi.load()
    for name in ("umi_dedup_batch_edit", "umi_dedup_batch_edit_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    assert umi.UMI_KERNEL_EDIT_PAIRS == 4


# ---- what tests/test_gpu_edit_distances.py rests on ----------------------------------------------------------
SWEEP_LENGTHS = (1, 2, 3, 6, 12, 20, 21)


@pytest.fixture(scope="module")
def sweep():
    """per length: the pairs, their distances by the DP and their count_l1"""
    out = {}
    for L in SWEEP_LENGTHS:
        pairs = em.adversarial_pairs(L)
        out[L] = (pairs, np.array([em.levenshtein(a, b) for a, b in pairs]),
                  np.array([em.count_l1(a, b) for a, b in pairs]))
    return out


@pytest.mark.parametrize("L", SWEEP_LENGTHS)
def test_adversarial_pairs_are_well_formed(sweep, L):
    pairs, d, _ = sweep[L]
    assert len(set(pairs)) == len(pairs)
    for a, b in pairs:
        assert a != b and len(a) == len(b) == L and set(a + b) <= set("ACGTN"), (a, b)
    assert em.adversarial_pairs(L) is pairs   # (made once)
    listed = set(pairs)
    for d_ in range(1, L + 1):   # the families that are spelt out, in both orders
        for x in "ACGTN":
            for y in "ACGTN":
                if x != y:
                    for b in (y * d_ + x * (L - d_), x * (L - d_) + y * d_):
                        assert (x * L, b) in listed and (b, x * L) in listed
    for s in range(1, L):
        base = ("ACGT" * 6)[:L]
        if base[s:] + base[:s] != base:
            assert (base, base[s:] + base[:s]) in listed and (base[s:] + base[:s], base) in listed
    for a, b in pairs[:8 * L]:   # the substitution family leads the list: d_H is the number of places changed
        assert em.hamming(a, b) >= em.levenshtein(a, b) >= 1


@pytest.mark.parametrize("L", SWEEP_LENGTHS)
def test_every_distance_occurs_in_at_least_20_pairs(sweep, L):
    _, d, _ = sweep[L]
    for x in range(1, L + 1):
        assert int((d == x).sum()) >= 20, (L, x)


@pytest.mark.parametrize("L", SWEEP_LENGTHS)
def test_the_filter_bound_is_met_at_every_distance(sweep, L):
    """count_l1 == 2 d == 2 d_E: the pair passes the filter at k = d by equality and is within k."""
    _, d, l1 = sweep[L]
    for x in range(1, L + 1):
        assert int(((d == x) & (l1 == 2 * x)).sum()) >= 10, (L, x)


@pytest.mark.parametrize("L", SWEEP_LENGTHS[1:])
def test_pairs_pass_the_filter_and_fail_the_check_at_every_k(sweep, L):
    """count_l1 <= 2 k < 2 d_E: only the exact check keeps these pairs apart."""
    _, d, l1 = sweep[L]
    for k in range(L):
        assert int(((l1 <= 2 * k) & (d > k)).sum()) >= 10, (L, k)


@pytest.mark.parametrize("L", SWEEP_LENGTHS)
def test_bit_vector_recurrence_is_the_dp_on_the_adversarial_pairs(sweep, L):
    pairs, d, _ = sweep[L]
    listed = {p: int(x) for p, x in zip(pairs, d)}
    for (a, b), x in listed.items():
        assert em.myers_global(a, b) == x, (a, b)
        assert em.myers_global(b, a) == (listed[(b, a)] if (b, a) in listed else em.levenshtein(b, a)) == x, (b, a)


@pytest.mark.parametrize("L", SWEEP_LENGTHS)
def test_pair_buckets(sweep, L):
    pairs, d, l1 = sweep[L]
    keys, nm, fr, off = em.pair_buckets(pairs)
    assert off.tolist() == list(range(0, 2 * len(pairs) + 1, 2))
    assert fr.reshape(-1, 2).tolist() == [list(em.PAIR_FREQS[i % 3]) for i in range(len(pairs))]
    assert em.decode(keys, L) == [s for p in pairs for s in p]
    assert nm.tolist() == em.encode([s for p in pairs for s in p])[1].tolist()
    # the three frequency patterns under the directional rule at p = 0.5: two merge whenever the pair is near, one never
    assert [em.permitted_pairs([[0, 1], [1, 0]], list(f), 1) for f in em.PAIR_FREQS] == [1, 1, 0]
    # the n_candidates the GPU test expects per call, from count_l1, is the sum of filter_hits over the buckets
    for k in sorted({0, 1, L // 2, L - 1, L, L + 1}):
        assert sum(em.filter_hits([a, b], k) for a, b in pairs) == int((l1 <= 2 * min(k, L)).sum())
    # every distance is seen under each merging pattern and in the pattern that never merges
    for x in range(1, L + 1):
        at = np.nonzero(d == x)[0]
        assert {int(i) % 3 for i in at} == {0, 1, 2}, (L, x)
    # ... and in both orders, (a, b) and (b, a), under a pattern that merges
    at = {p: i for i, p in enumerate(pairs)}
    both = {int(d[i]) for (a, b), i in at.items() if i % 3 != 2 and at.get((b, a), 2) % 3 != 2}
    assert both == set(range(1, L + 1)), L


def test_filter_hits_and_permitted_pairs_against_the_scalar_definitions():
    for L, n, seed in ((6, 40, 1), (12, 70, 2), (21, 65, 3)):
        umis, freq = em.mixed_bucket(L, n, seed)
        assert len(umis) == n == len(set(umis)) and freq == sorted(freq, reverse=True)
        d = em.edit_matrix(umis)
        for k in (0, 2, L - 1, L, L + 3):
            assert em.filter_hits(umis, k) == sum(em.count_l1(umis[i], umis[j]) <= 2 * min(k, L)
                                                  for i in range(n) for j in range(i + 1, n))
            thr = [int(np.float32(0.5) * np.float32(f + 1)) for f in freq]
            near = [(i, j) for i in range(n) for j in range(i + 1, n) if d[i, j] <= k]
            assert em.permitted_pairs(d, freq, k, 0.5, 0, 0) == sum(freq[j] <= thr[i] or freq[i] <= thr[j] for i, j in near)
            assert em.permitted_pairs(d, freq, k, 0.5, 1, 3) == sum(freq[j] <= 3 for i, j in near)
            assert em.permitted_pairs(d, freq, k, 0.5, 2, 0) == len(near)
    assert em.filter_hits([], 3) == em.filter_hits(["ACG"], 3) == 0 and em.permitted_pairs(np.zeros((1, 1)), [4], 3) == 0


def test_all_strings_bucket():
    for L in (1, 3, 4):
        umis, freq = em.all_strings_bucket(L)
        assert len(set(umis)) == len(umis) == 5 ** L and freq == [1] * 5 ** L and all(len(u) == L for u in umis)


@pytest.mark.parametrize("L", [12, 21])
def test_a_tile_of_the_largest_mixed_bucket_drains_the_queue_mid_tile(L):
    """edit_pair_kernel's tiling of a bucket: row tiles start at multiples of 64 from the bucket's start; the column
    tiles of a row tile start at its first row and step by 64; only pairs with row < column count.  The LDS queue
    holds 1,024 hits and is worked off in whole groups of 64 once more than 960 wait, and emptied at the end of a
    tile.  A tile with 961..4,095 filter hits therefore drains in the middle of the tile, at a fill level that the
    hits of its columns set and that is no multiple of 64 unless they happen to add up to one, and not every pair of
    it passes."""
    umis, freq = em.mixed_bucket(L, 330, seed=330)
    assert len(umis) == 330
    l1 = em.count_l1_matrix(umis)
    found = {}
    for k in range(L):
        tiles = em.tile_hits(l1, k, L)
        assert sorted(tiles) == [(r0, c0) for r0 in range(0, 330, 64) for c0 in range(r0, 330, 64)]
        assert sum(tiles.values()) == em.filter_hits(umis, k, l1)
        found[k] = [t for t, v in tiles.items() if 961 <= v <= 4095]
    assert any(found.values()), L
    if L == 12:   # the k of test_edge_list_redo_at_a_middle_k: such tiles, and more pairs than the first list of 1,024
        assert found[6] and em.permitted_pairs(em.edit_matrix(umis), freq, 6, algo=2) > 1024


def test_whole_batch_sizes():
    for L in (6, 12, 20, 21):
        buckets, mats, l1s, (keys, nm, fr, off) = em.whole_batch(L)
        assert [len(u) for u, _ in buckets] == [n for s in em.WHOLE_SIZES for n in (min(s, len(em.distinct_strings(L))), 0)]
        assert len(keys) == int(off[-1]) and all(len(m) == len(u) for m, (u, _) in zip(mats, buckets))
    assert [len(u) for u, _ in em.whole_batch(12)[0]][::2] == list(em.WHOLE_SIZES)
