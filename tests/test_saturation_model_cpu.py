"""tests/saturation_model.py (the definition of umi_saturation_curve and --saturation-curve) on the CPU: the hash's known
answers, the properties that make the definition trustworthy, the model against its restatement in plain loops, the
text of the saturation column, and every refusal of the program's three flags (status 101 before the GPU is woken)."""
import os
import subprocess

import numpy as np
import pytest

import gene_model
import saturation_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


# ---- the hash ---------------------------------------------------------------------------------------------

def test_known_answers():
    for (seed, i), h, level in sm.KNOWN:
        assert sm.read_hash(seed, i) == h, (seed, i, hex(sm.read_hash(seed, i)))
        assert sm.read_level(seed, i, 10) == level


def test_reads_per_level():
    assert np.bincount(sm.levels(0, 100_000, 10), minlength=10).tolist() == sm.KNOWN_PER_LEVEL


def test_the_vectorised_levels_are_the_scalar_ones():
    for seed in (0, 1, 7, sm.M64):
        for L in (1, 2, 10, 31, 32):
            lev = sm.levels(seed, 300, L)
            assert lev.tolist() == [sm.read_level(seed, i, L) for i in range(300)]
            assert lev.min() >= 0 and lev.max() < L
    assert sm.read_level(0, 2 ** 32 - 1, 10) == 7


# ---- the properties -----------------------------------------------------------------------------------------

def test_columns_0_to_5_never_decrease():
    m = sm.fuzz()
    for mask in (None, (np.arange(30) % 3 != 0).astype(np.uint8)):
        for L in (1, 5, 10, 32):
            c = sm.model_of(m, 30, L, 5, mask).astype(np.int64)
            assert (np.diff(c[:, :6], axis=0) >= 0).all()


def test_the_last_row_does_not_depend_on_the_seed_and_counts_what_it_says():
    m = sm.fuzz()
    last = [sm.model_of(m, 30, 10, seed)[-1] for seed in (0, 1, 12345, sm.M64)]
    assert all((row == last[0]).all() for row in last)
    assert len({tuple(sm.model_of(m, 30, 10, seed)[0]) for seed in (0, 1, 12345)}) > 1  # (the other rows do)
    staged = m["read_entry"][m["read_entry"] != sm.UNSTAGED].astype(np.int64)
    r = m["root"].astype(np.int64)[staged]
    counted = r[m["kept"][r] != 0]
    with_read = np.zeros(len(m["kept"]), bool)
    with_read[counted] = True
    assert int(last[0][0]) == len(counted)
    assert int(last[0][1]) == int(with_read.sum()) == int(np.count_nonzero((m["kept"] != 0) & with_read))
    assert int(with_read.sum()) < int(np.count_nonzero(m["kept"]))  # (there are molecules without any read)
    # count_model's pairs that hold a molecule with a read
    row, col, mol, _ = gene_model.count_model(with_read.astype(np.uint8), np.ones(len(with_read), np.int32), m["off"], m["row"], m["col"])
    assert int(last[0][2]) == int(np.count_nonzero(mol)) and int(last[0][2]) < len(mol)


@pytest.mark.parametrize("L", [1, 5, 10, 16])
def test_row_j_at_L_is_row_2j_plus_1_at_2L(L):
    m = sm.fuzz()
    mask = (np.arange(30) % 4 != 1).astype(np.uint8)
    for seed in (0, 9):
        for cm in (None, mask):
            assert (sm.model_of(m, 30, L, seed, cm) == sm.model_of(m, 30, 2 * L, seed, cm)[1::2]).all()


# ---- the model against its restatement -----------------------------------------------------------------------

def restated(m, n_cols, L, seed, mask):
    return sm.saturation_restated(m["read_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], n_cols, L, seed, mask)


def test_model_against_restatement_on_the_fuzz_input():
    m = sm.fuzz()
    assert (sm.model_of(m, 30, 10, 0) == restated(m, 30, 10, 0, None)).all()
    mask = np.zeros(40, np.uint8)  # (columns 30..39 hold nothing, and some of them are selected)
    mask[[0, 3, 4, 9, 17, 31, 35]] = 1
    assert (sm.model_of(m, 40, 4, 2, mask) == restated(m, 40, 4, 2, mask)).all()


@pytest.mark.parametrize("case", range(6))
def test_model_against_restatement_on_small_inputs(case):
    rng = np.random.default_rng(case)
    sizes = [int(x) for x in rng.choice([0, 1, 2, 3, 9, 33], 40)]
    n_rows, n_cols = [(5, 4), (1, 1), (3, 9)][case % 3]
    m = sm.make(case, sizes, n_rows, n_cols, readless=0.2, filtered=0.3)
    for L, seed in ((1, 0), (3, 1), (10, 7), (32, sm.M64)):
        for mask in (None, np.zeros(n_cols, np.uint8), np.ones(n_cols, np.uint8), (np.arange(n_cols) % 2).astype(np.uint8)):
            a, b = sm.model_of(m, n_cols, L, seed, mask), restated(m, n_cols, L, seed, mask)
            assert (a == b).all(), (L, seed, mask)
            if mask is not None and not mask.any():
                assert not a[:, 3:].any()


def test_no_reads_and_no_buckets():
    m = sm.make(1, [3, 4], 2, 2)
    none = dict(m, read_entry=np.zeros(0, np.uint32))
    assert not sm.model_of(none, 2).any()
    assert not sm.saturation_model(np.zeros(0, np.uint32), np.zeros(0, np.uint8), np.zeros(0, np.uint32), [0], [], [], 3, 4).any()


# ---- the file ---------------------------------------------------------------------------------------------------

def test_saturation_text():
    assert sm.saturation_text(0, 0) == "0.0000"
    assert sm.saturation_text(1, 1) == "0.0000"
    assert sm.saturation_text(7, 7) == "0.0000"
    assert sm.saturation_text(3, 1) == "0.6666"
    assert sm.saturation_text(10000, 1) == "0.9999"
    assert sm.saturation_text(2 ** 40, 1) == "0.9999"
    assert sm.saturation_text(1, 0) == "1.0000"


def test_curve_file():
    curve = np.array([[0, 0, 0, 0, 0, 0, 0, 0], [3, 2, 2, 1, 2, 2, 2, 2]], np.uint64)
    assert sm.curve_file(curve) == (sm.HEADER + "1/2\t0\t0\t0.0000\t0\t0\t0\t0\t0\t0\n2/2\t3\t2\t0.3333\t2\t1\t2\t2\t2\t2\n").encode()
    assert sm.HEADER.split() == ["depth", "reads", "molecules", "saturation", "pairs", "cells", "molecules_in_cells", "pairs_in_cells",
                                 "median_molecules", "median_genes"]


# ---- the program's refusals -------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def refused(tmp_path, flags, left=()):
    """the program's message for a run that must end with status 101 before the GPU is woken; `left`: what it may
    leave in the directory"""
    r = subprocess.run([CLI, "-i", "in.bam", "-o", "out.bam"] + flags, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert sorted(os.listdir(tmp_path)) == sorted(left)
    return r.stderr


BASE = ["--umi-tag", "UB", "--per-cell", "--per-gene", "--count-matrix", "m"]


def test_the_flag_wants_the_matrix(built, tmp_path):
    assert "--saturation-curve goes with --count-matrix DIR only" in refused(tmp_path, ["--umi-tag", "UB", "--per-gene", "--saturation-curve", "c.tsv"])


def test_the_flag_does_not_go_with_stage_gpu(built, tmp_path):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "c.tsv", "--stage", "gpu"])
    assert "--stage gpu does not go with --saturation-curve" in msg


def test_the_companions_want_the_flag(built, tmp_path):
    assert "--saturation-points goes with --saturation-curve only" in refused(tmp_path, BASE + ["--saturation-points", "5"])
    assert "--saturation-seed goes with --saturation-curve only" in refused(tmp_path, BASE + ["--saturation-seed", "5"])


@pytest.mark.parametrize("value", ["0", "33", "-1", "ten", "1.5", "", "99999999999999999999999", " 4", "4 "])
def test_points_outside_1_to_32(built, tmp_path, value):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "c.tsv", "--saturation-points", value])
    assert "--saturation-points want" in msg


@pytest.mark.parametrize("value", ["-1", "18446744073709551616", "seed", "1e3", "", "0x10", "+5"])
def test_a_seed_outside_64_bits(built, tmp_path, value):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "c.tsv", "--saturation-seed", value])
    assert "--saturation-seed want" in msg


def test_given_twice_with_different_values(built, tmp_path):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "a.tsv", "--saturation-curve", "b.tsv"])
    assert "--saturation-curve given twice with different values: 'a.tsv' and 'b.tsv'" in msg
    msg = refused(tmp_path, BASE + ["--saturation-curve", "a.tsv", "--saturation-points", "4", "--saturation-points", "5"])
    assert "--saturation-points given twice with different values: '4' and '5'" in msg
    msg = refused(tmp_path, BASE + ["--saturation-curve", "a.tsv", "--saturation-seed", "4", "--saturation-seed", "5"])
    assert "--saturation-seed given twice with different values: '4' and '5'" in msg


def test_twice_with_one_value_and_the_largest_values_are_taken(built, tmp_path):
    # what ends the run is the input that is not there
    msg = refused(tmp_path, BASE + ["--saturation-curve", "a.tsv", "--saturation-curve", "a.tsv", "--saturation-points", "32",
                                    "--saturation-points", "32", "--saturation-seed", "18446744073709551615", "--saturation-seed",
                                    "18446744073709551615"], left=["m", "a.tsv"])
    assert "in.bam" in msg and "saturation" not in msg
    msg = refused(tmp_path, ["--umi-tag", "UB", "--per-gene", "--count-matrix", "m", "--saturation-curve", "a.tsv", "--saturation-points", "1",
                             "--saturation-seed", "0"], left=["m", "a.tsv"])
    assert "in.bam" in msg and "saturation" not in msg  # (without --per-cell too)


def test_a_file_that_cannot_be_created(built, tmp_path):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "no_such_dir/c.tsv"], left=["m"])
    assert "cannot make no_such_dir/c.tsv for --saturation-curve" in msg


def test_help_names_the_flags(built):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--saturation-curve", "--saturation-points", "--saturation-seed"):
        assert flag in r.stdout
