"""--umi-whitelist / umi_correct_umis, the parts that need no GPU: the numpy model against hand-worked
cases, every refusal of the program (argument and whitelist checking come before the GPU is woken),
and the argument errors of the C entry points that are decided on the host (the context is looked at
last, so a NULL one reaches them all)."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import whitelist_model as wm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


# ---- the model, by hand --------------------------------------------------------------------------

def one(read, wl, **kw):
    r = wm.correct([read], len(read), wl, **kw)
    return int(r["match"][0]), int(r["best"][0]), int(r["second"][0]), r["out"].tobytes().decode(), list(map(int, r["counts"]))


def test_exact_and_one_mismatch():
    wl = ["AAAA", "CCCC", "GGTT"]
    assert one("CCCC", wl) == (1, 0, 4, "CCCC", [1, 0, 0])
    assert one("GGTA", wl) == (2, 1, 3, "GGTT", [0, 1, 0])   # AAAA is 3 away
    assert one("ACGT", wl) == (-1, 3, 3, "ACGT", [0, 0, 1])  # every listed UMI is 3 away


def test_tie_gives_the_lower_index_and_second_equals_best():
    wl = ["AAAA", "AATT", "CCCC"]
    # halfway: AAAT is 1 from AAAA and 1 from AATT
    assert one("AAAT", wl, min_distance=0) == (0, 1, 1, "AAAA", [0, 1, 0])
    assert one("AAAT", wl, min_distance=1) == (-1, 1, 1, "AAAT", [0, 0, 1])
    # the same list the other way round: still the lower index
    assert one("AAAT", wl[::-1], min_distance=0)[0] == 1


def test_duplicate_entry_makes_second_equal_best():
    assert one("ACGT", ["ACGT", "TTTT", "ACGT"], min_distance=0) == (0, 0, 0, "ACGT", [1, 0, 0])
    assert one("ACGT", ["ACGT", "TTTT", "ACGT"], min_distance=1)[0] == -1


def test_single_entry_list():
    assert one("ACGA", ["ACGT"]) == (0, 1, 5, "ACGT", [0, 1, 0])      # second = umi_len + 1
    assert one("ACGA", ["ACGT"], min_distance=4)[0] == 0              # 5 - 1 >= 4
    assert one("ACGA", ["ACGT"], min_distance=5)[0] == -1
    assert one("TTTT", ["ACGT"], max_mismatches=2) == (-1, 3, 5, "TTTT", [0, 0, 1])


def test_n_mismatches_every_listed_base():
    wl = ["ACGT", "TTTT"]
    assert one("ACNT", wl) == (0, 1, 3, "ACGT", [0, 1, 0])
    assert one("NNNN", wl, max_mismatches=4, min_distance=0) == (0, 4, 4, "ACGT", [0, 1, 0])
    assert one("ACNT", wl, max_mismatches=0)[0] == -1


def test_max_mismatches_zero_and_beyond_the_length():
    wl = ["ACGT", "GGGG"]
    assert one("ACGT", wl, max_mismatches=0)[0] == 0
    assert one("ACGA", wl, max_mismatches=0) == (-1, 1, 3, "ACGA", [0, 0, 1])
    for mm in (4, 5, 1000):  # any distance passes the first condition
        assert one("TTTT", wl, max_mismatches=mm) == (0, 3, 4, "ACGT", [0, 1, 0])
        assert one("TGTG", wl, max_mismatches=mm) == (1, 2, 4, "GGGG", [0, 1, 0])
    assert one("TTTT", wl, max_mismatches=2)[0] == -1


def test_min_distance_zero_one_two():
    wl = ["AAAA", "AACC", "GGGG"]
    # AAAC: 1 from AAAA, 1 from AACC; AAAA itself: 0 and 2
    assert [one("AAAC", wl, min_distance=d)[0] for d in (0, 1, 2)] == [0, -1, -1]
    assert [one("AAAA", wl, min_distance=d)[0] for d in (0, 1, 2, 3)] == [0, 0, 0, -1]
    # GGGA: 1 from GGGG, 3 from AAAA
    assert [one("GGGA", wl, min_distance=d)[0] for d in (0, 1, 2, 3)] == [2, 2, 2, -1]


def test_model_counts_and_chunking_agree():
    rng = np.random.default_rng(5)
    wl = wm.random_list(rng, 40, 9)
    reads = wm.noisy_reads(rng, wl, 9, 700)
    a = wm.correct(reads, 9, wl, 2, 1)
    b = wm.correct(reads, 9, wl, 2, 1, chunk=13)
    for f in a:
        assert (a[f] == b[f]).all(), f
    assert int(a["counts"].sum()) == 700 and all(int(c) > 0 for c in a["counts"])
    assert (a["match"] >= 0).sum() == int(a["counts"][0] + a["counts"][1])


# ---- the program's refusals ------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


@pytest.fixture
def files(tmp_path):
    good = tmp_path / "wl.txt"
    good.write_text("# a kit\nACGTACGT\n\nTTTTACGT\r\nGGGGCCCC\n")
    src = tmp_path / "in.bam"
    src.write_bytes(b"not read before the refusal")
    return str(src), str(tmp_path / "out.bam"), str(good), tmp_path


def refused(args, word):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert word in r.stderr, r.stderr
    return r.stderr


@pytest.mark.parametrize("extra,word", [
    (["-m", "fastq"], "fastq"),
    (["--two-pass"], "--two-pass"),
    (["--dump-staging", "x.bin"], "--dump-staging"),
    (["--passthrough"], "--passthrough"),
    (["-u", "9"], "-u 9"),
])
def test_flags_that_do_not_go_with_a_whitelist(files, extra, word):
    src, dst, wl, _ = files
    refused(["-i", src, "-o", dst, "--umi-whitelist", wl] + extra, word)
    assert not os.path.exists(dst)


@pytest.mark.parametrize("extra", [
    ["--whitelist-max-mismatches", "2"],
    ["--whitelist-min-distance", "2"],
    ["--whitelist-metrics", "m.tsv"],
])
def test_the_other_whitelist_flags_need_the_whitelist(files, extra):
    src, dst, _, _ = files
    refused(["-i", src, "-o", dst] + extra, "--umi-whitelist")


@pytest.mark.parametrize("flag", ["--whitelist-max-mismatches", "--whitelist-min-distance"])
@pytest.mark.parametrize("value", ["-1", "x", "1.5", ""])
def test_whitelist_numbers_must_be_numbers(files, flag, value):
    src, dst, wl, _ = files
    refused(["-i", src, "-o", dst, "--umi-whitelist", wl, flag, value], flag)


@pytest.mark.parametrize("text,word", [
    ("", "holds no UMI"),
    ("# only a comment\n\n", "holds no UMI"),
    ("ACGT\nACGTA\n", "line 2: 5 bases"),
    ("ACGT\nACNT\n", "outside ACGT"),
    ("ACGT\nacgt\n", "outside ACGT"),
    ("ACGT\nGGGG\nACGT\n", "duplicate entry ACGT"),
    ("A" * 86 + "\n", "more than 85"),
])
def test_malformed_whitelists(files, text, word):
    src, dst, _, tmp = files
    bad = tmp / "bad.txt"
    bad.write_text(text)
    refused(["-i", src, "-o", dst, "--umi-whitelist", str(bad)], word)


def test_missing_whitelist_file(files):
    src, dst, _, tmp = files
    refused(["-i", src, "-o", dst, "--umi-whitelist", str(tmp / "nothing.txt")], "cannot open")


def test_a_whitelist_of_85_bases_is_read(files):
    # (it gets past the whitelist checks: the next thing to fail is the input, which is no BAM file)
    src, dst, _, tmp = files
    ok = tmp / "long.txt"
    ok.write_text("A" * 85 + "\n" + "C" * 85 + "\n")
    r = subprocess.run([CLI, "-i", src, "-o", dst, "--umi-whitelist", str(ok)], capture_output=True, text=True, timeout=60)
    assert r.returncode != 0 and "whitelist" not in r.stderr


def test_help_names_the_flags():
    out = subprocess.run([CLI, "--help"], capture_output=True, text=True).stdout
    for f in ("--umi-whitelist", "--whitelist-max-mismatches", "--whitelist-min-distance", "--whitelist-metrics"):
        assert f in out


# ---- the entry points' host-side argument errors ---------------------------------------------------

@pytest.fixture(scope="module")
def lib():
    import umi_collapse_rs_amd as umi
    return umi.load()


def call(lib, device_form, umi=b"ACGT", n=1, umi_len=4, wl=b"ACGTTTTT", n_wl=2, mm=1, md=1, match=True, counts=True):
    """the call with a NULL context: every argument check comes before the context is looked at"""
    from umi_collapse_rs_amd import _lib
    ub = np.frombuffer(umi, np.uint8) if umi is not None else None
    wb = np.frombuffer(wl, np.uint8) if wl is not None else None
    m = np.zeros(max(1, n), np.int32) if match else None
    c = np.zeros(3, np.uint64) if counts else None
    if device_form:  # (host addresses stand in for device pointers: nothing is dereferenced before the refusal)
        rc = lib.umi_correct_umis_device(None, ub.ctypes.data if ub is not None else None, n, umi_len,
                                         _lib.ptr(wb, C.c_uint8), n_wl, mm, md, None, m.ctypes.data if match else None,
                                         None, None, _lib.ptr(c, C.c_uint64), None)
    else:
        rc = lib.umi_correct_umis(None, _lib.ptr(ub, C.c_uint8), n, umi_len, _lib.ptr(wb, C.c_uint8), n_wl, mm, md, None,
                                  _lib.ptr(m, C.c_int32), None, None, _lib.ptr(c, C.c_uint64))
    return rc, lib.umi_last_error().decode()


@pytest.mark.parametrize("device_form", [False, True])
def test_argument_errors(lib, device_form):
    from umi_collapse_rs_amd import _lib
    ARG, CHAR = _lib.UMI_ERR_ARG, _lib.UMI_ERR_CHAR
    for kw, code, word in [
        (dict(n_wl=0), ARG, "empty"),
        (dict(n_wl=(1 << 24) + 1), ARG, "whitelist"),
        (dict(wl=None), ARG, "whitelist_ascii"),
        (dict(umi=None), ARG, "NULL"),
        (dict(match=False), ARG, "NULL"),
        (dict(counts=False), ARG, "counts"),
        (dict(mm=-1), ARG, "max_mismatches"),
        (dict(md=-1), ARG, "min_distance"),
        (dict(umi_len=0), ARG, "umi_len"),
        (dict(umi_len=86), ARG, "umi_len"),
        (dict(umi_len=-3), ARG, "umi_len"),
        (dict(n=1 << 30), ARG, "30-bit"),
        (dict(wl=b"ACGTTNTT"), CHAR, "Unknown character in whitelist: 78 (entry 1)"),
        (dict(wl=b"aCGTTTTT"), CHAR, "Unknown character in whitelist: 97 (entry 0)"),
        (dict(), ARG, "ctx is NULL"),            # everything else in order: only now the context
        (dict(n=0, umi=None, match=False), ARG, "ctx is NULL"),
    ]:
        rc, msg = call(lib, device_form, **kw)
        assert rc == code and word in msg, (kw, rc, msg)


def test_python_wrapper_refuses_ragged_input():
    import umi_collapse_rs_amd as umi
    with pytest.raises(ValueError):
        umi.Context._whitelist_bytes(["ACGT", "ACG"], 4)
    with pytest.raises(ValueError):
        umi.Context._whitelist_bytes(np.zeros(7, np.uint8), 4)
