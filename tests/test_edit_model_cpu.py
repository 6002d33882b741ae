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
