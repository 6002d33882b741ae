"""--cell-whitelist / umi_correct_barcodes, the parts that need no GPU: the two forms of the model
(tests/barcode_model.py) against each other and against hand-worked cases, what the GPU tests' inputs hold,
every refusal of the program (argument and list checking come before the GPU is woken), and the argument
errors of the C entry points that are decided on the host (the context is looked at last, so a NULL one
reaches them all)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import barcode_model as bm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def same(a, b):
    for f in ("match", "status", "counts"):
        assert a[f].shape == b[f].shape and (a[f] == b[f]).all(), f


# ---- the model ------------------------------------------------------------------------------------

@pytest.mark.parametrize("L,n_wl,seed", [(1, 3, 1), (2, 9, 2), (5, 200, 3), (16, 300, 4), (32, 150, 5), (17, 64, 6)])
@pytest.mark.parametrize("mm", [0, 1])
def test_the_two_forms_agree(L, n_wl, seed, mm):
    rng = np.random.default_rng(seed)
    wl, pairs = bm.random_list(rng, n_wl, L)
    reads = bm.listed_reads(rng, wl, 800, pairs)
    a = bm.correct(reads, L, wl, mm)
    same(a, bm.correct_bruteforce(reads, L, wl, mm))
    same(a, bm.correct_bruteforce(reads, L, wl, mm, chunk=37))
    assert int(a["counts"].sum()) == 800
    if mm == 0:
        assert a["counts"][bm.CORRECTED] == 0 and a["counts"][bm.AMBIGUOUS] == 0


@pytest.mark.parametrize("where", ["low", "high"])
def test_the_two_forms_agree_on_a_clustered_list(where):
    wl, pairs = bm.clustered_list(9, where)
    assert len(wl) == 4096 and len(set(map(bytes, wl))) == 4096
    codes = [sum(b"ACGT".index(c) << (2 * b) for b, c in enumerate(bytes(r))) for r in wl]
    fixed = (4 ** 9 - 1) ^ (4 ** 6 - 1 if where == "low" else (4 ** 6 - 1) << 6)
    assert len({c & fixed for c in codes}) == 1  # the keys differ in the low (high) 12 bits only
    reads = bm.listed_reads(np.random.default_rng(9), wl, 400, pairs)
    same(bm.correct(reads, 9, wl), bm.correct_bruteforce(reads, 9, wl))


def one(read, wl, mm=1):
    r = bm.correct([read], len(read), wl, mm)
    assert int(r["counts"][r["status"][0]]) == 1 and int(r["counts"].sum()) == 1
    same(r, bm.correct_bruteforce([read], len(read), wl, mm))
    return int(r["status"][0]), int(r["match"][0])


def test_known_answers():
    wl = ["ACGT", "TTTT", "ACCA"]
    assert one("TTTT", wl) == (bm.EXACT, 1)
    assert one("TTTT", wl, 0) == (bm.EXACT, 1)
    assert one("TTTA", wl) == (bm.CORRECTED, 1)      # the last base
    assert one("GTTT", wl) == (bm.CORRECTED, 1)      # the first base
    assert one("TTTA", wl, 0) == (bm.NONE, -1)
    assert one("GGGG", wl) == (bm.NONE, -1)
    assert one("TTAA", wl) == (bm.NONE, -1)          # two away from TTTT
    # an N differs from every listed base: never exact, and its candidates are the four letters there
    assert one("NCGT", wl) == (bm.CORRECTED, 0)      # N at the first base
    assert one("ACGN", wl) == (bm.CORRECTED, 0)      # N at the last base
    assert one("ACGN", wl, 0) == (bm.NONE, -1)
    assert one("NCGA", wl) == (bm.NONE, -1)          # an N and a substitution
    assert one("NNGT", wl) == (bm.NONE, -1)          # two N: no candidates
    assert one("TTNN", wl) == (bm.NONE, -1)
    assert one("ACNA", wl) == (bm.CORRECTED, 2)
    assert one("ACNT", wl) == (bm.CORRECTED, 0)


def test_ambiguous_pairs_made_on_purpose():
    wl, read = bm.AMBIGUOUS_SAME_POSITION
    assert (wl, read) == (["AAAA", "CAAA"], "GAAA")
    assert one(read, wl) == (bm.AMBIGUOUS, -1)
    assert one(read, wl, 0) == (bm.NONE, -1)
    assert one("NAAA", wl) == (bm.AMBIGUOUS, -1)
    wl, read = bm.AMBIGUOUS_DIFFERENT_POSITIONS
    assert (wl, read) == (["AA", "CC"], "CA")
    assert one(read, wl) == (bm.AMBIGUOUS, -1)
    assert one("AC", wl) == (bm.AMBIGUOUS, -1)
    assert one("AG", wl) == (bm.CORRECTED, 0)


def test_full_list():
    wl, _ = bm.full_list(2)
    assert len(wl) == 16
    assert one("GT", wl) == (bm.EXACT, 2 + 4 * 3)
    assert one("NT", wl) == (bm.AMBIGUOUS, -1)
    assert one("NN", wl) == (bm.NONE, -1)


def test_every_gpu_input_holds_what_it_is_meant_to():
    seen_kinds = set()
    for name, (kind, L, wl, reads) in bm.gpu_inputs().items():
        assert len(set(map(bytes, wl))) == len(wl), name
        counts = bm.expected(name, 1)["counts"]
        seen_kinds.add(kind)
        if kind == "all":
            assert all(int(c) >= 8 for c in counts), (name, counts)
            c0 = bm.expected(name, 0)["counts"]
            assert int(c0[bm.EXACT]) >= 8 and int(c0[bm.NONE]) >= 8 and int(c0[1]) == int(c0[3]) == 0
        elif kind == "full":  # no "none" by construction (and so nothing to correct either)
            assert int(counts[bm.NONE]) == 0 and int(counts[bm.CORRECTED]) == 0
            assert int(counts[bm.EXACT]) >= 8 and int(counts[bm.AMBIGUOUS]) >= 8
        else:
            assert L <= 2 or len(wl) <= 2
            assert int(counts[bm.EXACT]) >= 8
    assert seen_kinds == {"all", "full", "small"}
    # the read counts of the sweep are prefixes of one input; the whole of it is of kind "all" (above)
    assert bm.gpu_inputs()["reads10000"][0] == "all" and len(bm.gpu_inputs()["reads10000"][3]) == 10000 * 16
    # the lengths and list sizes the GPU tests are to cover
    Ls = {v[1] for v in bm.gpu_inputs().values()}
    sizes = {len(v[2]) for v in bm.gpu_inputs().values()}
    assert {1, 2, 15, 16, 17, 31, 32} <= Ls and {1, 2, 64, 4096, 4999, 5003} <= sizes


# ---- the program's refusals ------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


@pytest.fixture
def files(tmp_path):
    good = tmp_path / "cells.txt"
    good.write_text("# a kit\nACGTACGTACGTACGT\n\nTTTTACGTACGTACGT\r\nGGGGCCCCACGTACGT\n")
    src = tmp_path / "in.bam"
    src.write_bytes(b"not read before the refusal")
    return str(src), str(tmp_path / "out.bam"), str(good), tmp_path


def refused(args, word):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert word in r.stderr, r.stderr
    return r.stderr


@pytest.mark.parametrize("extra,word", [
    ([], "--per-cell"),                                   # the flag without --per-cell
    (["--per-cell", "-m", "fastq"], "fastq"),
    (["--per-cell", "--two-pass"], "--two-pass"),
    (["--per-cell", "--dump-staging", "x.bin"], "--dump-staging"),
    (["--per-cell", "--passthrough"], "--passthrough"),
    (["--per-cell", "--cell-whitelist-max-mismatches", "2"], "--cell-whitelist-max-mismatches"),
    (["--per-cell", "--cell-whitelist-max-mismatches", "-1"], "--cell-whitelist-max-mismatches"),
    (["--per-cell", "--cell-whitelist-max-mismatches", "x"], "--cell-whitelist-max-mismatches"),
    (["--per-cell", "--cell-whitelist-max-mismatches", ""], "--cell-whitelist-max-mismatches"),
])
def test_flags_that_do_not_go_with_a_cell_whitelist(files, extra, word):
    src, dst, wl, _ = files
    refused(["-i", src, "-o", dst, "--cell-whitelist", wl] + extra, word)
    assert not os.path.exists(dst)


@pytest.mark.parametrize("extra", [["--cell-whitelist-max-mismatches", "0"], ["--cell-whitelist-metrics", "m.tsv"]])
def test_the_companion_flags_need_the_list(files, extra):
    src, dst, _, _ = files
    refused(["-i", src, "-o", dst, "--per-cell"] + extra, "--cell-whitelist only")


@pytest.mark.parametrize("text,word", [
    ("", "holds no barcode"),
    ("# only a comment\n\n", "holds no barcode"),
    ("ACGT\nACGTA\n", "line 2: 5 bases, the barcodes before it have 4"),
    ("ACGT\nACNT\n", "outside ACGT"),
    ("ACGT\nacgt\n", "outside ACGT"),
    ("ACGT-1\nGGGG-1\n", "outside ACGT"),                 # Cell Ranger's suffix
    ("ACGT\nGGGG\nACGT\n", "duplicate entry ACGT"),
    ("A" * 33 + "\n", "more than 32"),
])
def test_malformed_lists(files, text, word):
    src, dst, _, tmp = files
    bad = tmp / "bad.txt"
    bad.write_text(text)
    err = refused(["-i", src, "-o", dst, "--per-cell", "--cell-whitelist", str(bad)], word)
    assert "cell barcode whitelist" in err


def test_missing_list_file(files):
    src, dst, _, tmp = files
    refused(["-i", src, "-o", dst, "--per-cell", "--cell-whitelist", str(tmp / "nothing.txt")], "cannot open")


def test_a_list_of_32_bases_is_read(files):
    # (it gets past the list checks: the next thing to fail is the input, which is no BAM file)
    src, dst, _, tmp = files
    ok = tmp / "long.txt"
    ok.write_text("A" * 32 + "\n" + "T" * 32 + "\n")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--per-cell", "--cell-whitelist", str(ok)], capture_output=True, text=True,
                       timeout=60)
    assert r.returncode != 0 and "whitelist" not in r.stderr


def test_help_names_the_flags():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
    for f in ("--cell-whitelist", "--cell-whitelist-max-mismatches", "--cell-whitelist-metrics"):
        assert f in out


# ---- the library ---------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import umi_collapse_rs_amd as umi
    return umi.load()


def test_the_library_exports_both_symbols(lib):
    assert lib.umi_correct_barcodes and lib.umi_correct_barcodes_device
    assert lib.umi_abi_version() == 2


def call(lib, device_form, bc=b"ACGT", n=1, bc_len=4, wl=b"ACGTTTTT", n_wl=2, mm=1, match=True, counts=True):
    """the call with a NULL context: every argument check comes before the context is looked at"""
    from umi_collapse_rs_amd import _lib
    ub = np.frombuffer(bc, np.uint8) if bc is not None else None
    wb = np.frombuffer(wl, np.uint8) if wl is not None else None
    m = np.zeros(max(1, n), np.int32) if match else None
    c = np.zeros(4, np.uint64) if counts else None
    if device_form:  # (host addresses stand in for device pointers: nothing is dereferenced before the refusal)
        rc = lib.umi_correct_barcodes_device(None, ub.ctypes.data if ub is not None else None, n, bc_len,
                                             _lib.ptr(wb, C.c_uint8), n_wl, mm, m.ctypes.data if match else None, None,
                                             _lib.ptr(c, C.c_uint64), None)
    else:
        rc = lib.umi_correct_barcodes(None, _lib.ptr(ub, C.c_uint8), n, bc_len, _lib.ptr(wb, C.c_uint8), n_wl, mm,
                                      _lib.ptr(m, C.c_int32), None, _lib.ptr(c, C.c_uint64))
    return rc, lib.umi_last_error().decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_argument_errors(lib, device_form):
    from umi_collapse_rs_amd import _lib
    ARG, CHAR = _lib.UMI_ERR_ARG, _lib.UMI_ERR_CHAR
    for kw, code, word in [
        (dict(n_wl=0), ARG, "empty"),
        (dict(n_wl=(1 << 24) + 1), ARG, "whitelist"),
        (dict(wl=None), ARG, "whitelist_ascii"),
        (dict(bc=None), ARG, "NULL"),
        (dict(match=False), ARG, "NULL"),
        (dict(counts=False), ARG, "counts"),
        (dict(mm=-1), ARG, "max_mismatches"),
        (dict(mm=2), ARG, "max_mismatches"),
        (dict(bc_len=0), ARG, "bc_len"),
        (dict(bc_len=33), ARG, "bc_len"),
        (dict(bc_len=-3), ARG, "bc_len"),
        (dict(n=1 << 30), ARG, "30-bit"),
        (dict(wl=b"ACGTTNTT"), CHAR, "Unknown character in whitelist: 78 (entry 1)"),
        (dict(wl=b"aCGTTTTT"), CHAR, "Unknown character in whitelist: 97 (entry 0)"),
        (dict(), ARG, "ctx is NULL"),            # everything else in order: only now the context
        (dict(n=0, bc=None, match=False), ARG, "ctx is NULL"),
    ]:
        rc, msg = call(lib, device_form, **kw)
        assert rc == code and word in msg, (kw, rc, msg)


def test_python_wrapper_refuses_ragged_input():
    import umi_collapse_rs_amd as umi
    c = umi.Context.__new__(umi.Context)  # (no device: the wrapper's own checks come first)
    with pytest.raises(ValueError):
        umi.Context.correct_barcodes(c, np.zeros(7, np.uint8), 4, ["ACGT"])
    with pytest.raises(ValueError):
        umi.Context.correct_barcodes(c, np.zeros(8, np.uint8), 4, ["ACGT", "ACG"])
