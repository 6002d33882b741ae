"""tests/barcode_multi_model.py without a GPU: its two models agree on every input of the GPU tests, the inputs hold
what they are meant to hold, the first three statuses are barcode_model's, the weight table equals its formula,
and the program refuses what --cell-whitelist-multi's flags can get wrong before it looks for a GPU."""
import os
import subprocess

import numpy as np
import pytest

import barcode_model as bm
import barcode_multi_model as mm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
FIELDS = ("match", "status", "counts", "exact_reads")


def same(a, b):
    for f in FIELDS:
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), f


def test_the_table_equals_its_formula():
    assert mm.table_from_formula() == mm.T and len(mm.T) == 41
    assert mm.T[0] == 67108864 and mm.T[40] == 6711


@pytest.mark.parametrize("name", sorted(mm.gpu_inputs()))
def test_the_two_models_agree(name):
    _, L, wl, reads, quals = mm.gpu_inputs()[name]
    same(mm.correct_multi_bruteforce(reads, quals, L, wl), mm.expected(name))
    for permille, pseudo in ((1000, 0), (500, 1)):
        if len(reads) // L <= 3000:
            same(mm.correct_multi_bruteforce(reads, quals, L, wl, permille, pseudo), mm.expected(name, permille, pseudo))


@pytest.mark.parametrize("name", sorted(mm.gpu_inputs()))
def test_what_the_inputs_hold(name):
    kind, L, wl, reads, quals = mm.gpu_inputs()[name]
    got = mm.expected(name)
    first = bm.correct(reads, L, wl, 1)
    assert len(quals) == len(reads) and quals.min() >= 33 and quals.max() <= 126
    if kind == "all":
        assert all(int(c) >= 8 for c in got["counts"]), got["counts"]
    # exact, corrected and none are barcode_model's; ambiguous splits into ambiguous and resolved
    for s in (bm.EXACT, bm.CORRECTED, bm.NONE):
        assert ((got["status"] == s) == (first["status"] == s)).all()
        assert (got["match"][first["status"] == s] == first["match"][first["status"] == s]).all()
    assert int(got["counts"][3] + got["counts"][4]) == int(first["counts"][3])
    assert ((first["status"] == bm.AMBIGUOUS) == (got["status"] >= 3)).all()
    assert (got["match"][got["status"] == mm.RESOLVED] >= 0).all() and (got["match"][got["status"] == mm.AMBIGUOUS] == -1).all()
    assert int(got["exact_reads"].sum()) == int(got["counts"][0])


def test_the_special_inputs():
    assert len({len(mm.gpu_inputs()[n][3]) // mm.gpu_inputs()[n][1] for n in mm.gpu_inputs()} & {10000}) == 1
    # L = 32: ambiguous reads with candidates in the first pass of 64 variants only, the second only, and both
    _, L, wl, reads, quals = mm.gpu_inputs()["two_pass_L32"]
    index = {bytes(w): i for i, w in enumerate(wl)}
    seen = set()
    for r in (bytes(r) for r in reads.reshape(-1, L)):
        if r in index:
            continue
        pos = [p for p in range(L) for c in b"ACGT" if c != r[p] and r[:p] + bytes([c]) + r[p + 1:] in index]
        var = [3 * p + (("ACGT".index(chr(c)) - "ACGT".index(chr(r[p])) - 1) % 4) for p in range(L) for c in b"ACGT"
               if c != r[p] and r[:p] + bytes([c]) + r[p + 1:] in index]
        assert len(pos) >= 2
        seen.add((any(v < 64 for v in var), any(v >= 64 for v in var)))
    assert seen == {(True, False), (False, True), (True, True)}
    got = mm.expected("two_pass_L32")
    assert int(got["counts"][3]) >= 8 and int(got["counts"][4]) >= 8
    # one N on a full list: four candidates, one quality; some resolved, some not
    got = mm.expected("full3_one_n")
    assert int(got["counts"][3]) >= 8 and int(got["counts"][4]) >= 8
    # the hot barcode
    assert int(mm.expected("hot")["exact_reads"].max()) >= 8000
    # no exact read: nothing has weight without a pseudocount; with one, the qualities alone decide
    got0, got1 = mm.expected("no_exact"), mm.expected("no_exact", 975, 1)
    assert int(got0["counts"][0]) == 0 and int(got0["counts"][4]) == 0 and int(got0["counts"][3]) >= 8
    assert int(got1["counts"][4]) >= 8 and int(got1["counts"][3]) >= 8


def test_hand_made_cases():
    for name, (wl, reads, quals, permille, pseudo, status, match) in {**mm.hand_cases(), **mm.hand_quality_cases()}.items():
        L = len(wl[0])
        q = b"".join(quals) if quals is not None else bytes([33 + 30]) * (L * len(reads))
        raw = "".join(reads).encode()
        for model in (mm.correct_multi, mm.correct_multi_bruteforce):
            got = model(raw, q, L, wl, permille, pseudo)
            assert (int(got["status"][-1]), int(got["match"][-1])) == (status, match), name


# ---- the program's refusals that need no GPU ----------------------------------------------------------------

@pytest.fixture(scope="module")
def files(tmp_path_factory):
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])
    d = tmp_path_factory.mktemp("multi_cli")
    lst = str(d / "cells.txt")
    with open(lst, "w") as f:
        f.write("ACGTACGTACGTACGT\nACGTACGTACGTACGA\n")
    return str(d / "in.bam"), str(d / "out.bam"), lst  # (the input is never opened: the flags are refused first)


BASE = ["--per-cell", "--cell-tag", "CR", "--umi-tag", "UR"]


@pytest.mark.parametrize("flags, word", [
    (["--cell-whitelist-multi"], "--cell-whitelist only"),
    (["--cell-quality-tag", "CY"], "--cell-whitelist only"),
    (["--cell-whitelist-min-posterior", "0.9"], "--cell-whitelist only"),
    (["--cell-whitelist-pseudocount", "1"], "--cell-whitelist only"),
    (["--cell-whitelist", "LIST", "--cell-quality-tag", "CY"], "--cell-whitelist-multi only"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-min-posterior", "0.9"], "--cell-whitelist-multi only"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-pseudocount", "1"], "--cell-whitelist-multi only"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-whitelist-max-mismatches", "0"], "max-mismatches 0"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-quality-tag", "C"], "two characters"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-quality-tag", "CYY"], "two characters"),
    (["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-quality-tag", "1Y"], "two characters"),
] + [(["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-whitelist-min-posterior", p], "at most three decimals")
     for p in ("", "0.9755", "1.001", "2", "-0.5", "0,9", "abc", "0.", ".5", "1e-1", "0.9 ", "+0.9", "00.9")]
  + [(["--cell-whitelist", "LIST", "--cell-whitelist-multi", "--cell-whitelist-pseudocount", n], "0..1000")
     for n in ("", "-1", "1001", "1.5", "x", "+1", " 1", "99999999999999999999")],
    ids=lambda v: " ".join(v)[-60:] if isinstance(v, list) else None)
def test_refused_with_status_101_and_nothing_written(files, flags, word):
    src, dst, lst = files
    r = subprocess.run([CLI, "-i", src, "-o", dst] + BASE + [lst if x == "LIST" else x for x in flags], capture_output=True,
                       text=True, timeout=60)
    assert r.returncode == 101 and word in r.stderr, r.stderr
    assert not os.path.exists(dst)


@pytest.mark.parametrize("p", ["0", "1", "0.5", "0.975", "1.0", "1.000", "0.000"])
def test_well_formed_values_pass_the_flags(files, p):
    # (the run ends at the input file, which is not there: the flags were accepted)
    src, dst, lst = files
    r = subprocess.run([CLI, "-i", src, "-o", dst] + BASE + ["--cell-whitelist", lst, "--cell-whitelist-multi",
                       "--cell-whitelist-min-posterior", p, "--cell-whitelist-pseudocount", "1000", "--cell-quality-tag", "QY"],
                       capture_output=True, text=True, timeout=60)
    assert "at most three decimals" not in r.stderr and "0..1000" not in r.stderr and "go with" not in r.stderr
    assert r.returncode != 0 and not os.path.exists(dst)
