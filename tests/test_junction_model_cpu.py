"""tests/junction_model.py (the definition of umi_junction_matrix and --junction-matrix) on the CPU: the model against
hand-written answers, the junction walk the kernels run (csrc/umihip_junction_walk.hpp) under AddressSanitizer + UBSan
against vectors the model writes, and the program's refusals (status 101 before the GPU is woken)."""
import os
import subprocess

import numpy as np
import pytest

import junction_model as jm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
TOP = 2 ** 31 - 1


def junctions(pos, text):
    return jm.read_junctions(pos, jm.cigar_words(text))


# ---- the junctions of a read -------------------------------------------------------------------------------------

def test_each_op_code():
    assert junctions(100, "10M5N10M") == [(110, 115)]
    assert junctions(100, "10=5N10X") == [(110, 115)]
    assert junctions(100, "10M2D3M5N10M") == [(115, 120)]            # D extends the block
    assert junctions(100, "10M2I3M5N10M") == [(113, 118)]            # I consumes nothing
    assert junctions(100, "3S10M5N10M4S") == [(110, 115)]
    assert junctions(100, "2H3S10M5N10M4S1H") == [(110, 115)]
    assert junctions(100, "10M1P5N2P10M") == [(110, 115)]
    assert junctions(100, "10M") == [] and junctions(100, "") == [] and junctions(100, "5S") == []
    for op in range(9, 16):
        with pytest.raises(jm.BadOp):
            jm.read_junctions(100, jm.cigar_words([(10, "M"), (5, op), (3, "M")]))


def test_leading_trailing_and_zero_length_N():
    assert junctions(100, "5N10M") == [] and junctions(100, "10M5N") == [] and junctions(100, "5N10M7N") == []
    assert junctions(100, "10M0N10M") == []                          # two abutting blocks, an empty gap
    assert junctions(100, "5N10M3N10M7N") == [(115, 118)]
    assert junctions(100, "10M0N0N5N0N10M") == [(110, 115)]


def test_several_N_form_one_junction():
    assert junctions(100, "10M5N3I7N10M") == [(110, 122)]           # N I N
    assert junctions(100, "10M5N0M7N10M") == [(110, 122)]           # an empty block between them is left out
    assert junctions(100, "10M5N2S1H1P7N10M") == [(110, 122)]
    assert junctions(100, "10M5N1M7N10M") == [(110, 115), (116, 123)]


def test_N_beside_D():
    assert junctions(100, "10M2D5N10M") == [(112, 117)]
    assert junctions(100, "10M5N2D10M") == [(110, 115)]
    assert junctions(100, "10M5N2D") == [(110, 115)]                 # a block of a deletion alone is a block
    assert junctions(100, "10M50D10M") == []                         # a D never makes a junction


def test_positions_near_the_top():
    assert junctions(TOP - 30, "10M20N1M") == [(TOP - 20, TOP)]      # a gap ending at 2^31 - 1
    assert junctions(TOP - 30, "10M21N1M") == []                     # ... and one beyond it
    assert junctions(TOP - 40, "5M2N5M3N5M40N5M3N5M") == [(TOP - 35, TOP - 33), (TOP - 28, TOP - 25)]
    assert junctions(0, "1M" + "268435455N" * 8 + "6N1M") == [(1, TOP)]
    assert junctions(0, "1M" + "268435455N" * 8 + "7N1M") == []
    assert junctions(-5, "3M4N10M") == []                            # a block that ends before 0
    assert junctions(-5, "6M4N10M") == [(1, 5)]


def test_a_read_of_300_junctions():
    got = junctions(1000, "5M" + "3N5M" * 300)
    assert len(got) == 300 and got[0] == (1005, 1008) and got[-1] == (1005 + 8 * 299, 1008 + 8 * 299)
    assert got == sorted(set(got))


# ---- the table, the triplets, the counts ----------------------------------------------------------------------------

def bucketed(reads, entry, kept, root, off, col):
    words, woff = [], [0]
    for _, _, c in reads:
        words += jm.cigar_words(c)
        woff.append(len(words))
    return jm.junction_matrix(np.array([r[0] for r in reads], np.int32), np.array([r[1] for r in reads], np.int32), np.array(words, np.uint32),
                              np.array(woff, np.uint64), np.array(entry, np.uint32), np.array(kept, np.uint8), np.array(root, np.uint32),
                              np.array(off, np.uint64), np.array(col, np.uint32))


def lists(result):
    jn, trip, counts = result
    return list(zip(*(a.tolist() for a in jn))), list(zip(*(a.tolist() for a in trip))), counts.tolist()


def test_kept_removed_unstaged_and_filtered_out_reads():
    # entries 0..5 of one bucket: 1 and 2 hang on 0 (kept), 4 hangs on 3 (a root the filter removed), 5 of its own
    reads = [(0, 10, "5M10N5M"), (0, 10, "5M10N5M"), (0, 10, "5M10N5M"), (0, 10, "5M20N5M"), (0, 10, "5M20N5M"), (0, 10, "5M30N5M"),
             (0, 10, "5M40N5M"), (0, 10, "5M")]
    table, trip, counts = lists(bucketed(reads, [0, 1, 2, 3, 4, 5, jm.UNSTAGED, 5], [1, 0, 0, 0, 0, 1], [0, 0, 0, 3, 3, 5], [0, 6], [0]))
    assert table == [(0, 15, 25), (0, 15, 45)]
    assert trip == [(0, 0, 1, 3), (1, 0, 1, 1)]
    assert counts == [4, 4, 2, 2]


def test_one_molecule_with_the_same_junction_in_five_reads():
    table, trip, counts = lists(bucketed([(2, 10, "5M10N5M")] * 5, [0, 1, 1, 0, 1], [1, 0], [0, 0], [0, 2], [3]))
    assert table == [(2, 15, 25)] and trip == [(0, 3, 1, 5)] and counts == [5, 5, 1, 1]


def test_one_junction_in_two_columns_and_the_order_of_the_table():
    reads = [(1, 10, "5M10N5M"), (0, 90, "5M10N5M"), (0, 10, "5M11N5M"), (0, 10, "5M10N5M"), (0, 10, "5M10N5M"), (0, 10, "5M10N5M")]
    # four buckets of one entry each; buckets 1 and 3 share column 0
    table, trip, counts = lists(bucketed(reads, [0, 1, 2, 3, 1, 2], [1, 1, 1, 1], [0, 1, 2, 3], [0, 1, 2, 3, 4], [2, 0, 1, 0]))
    assert table == [(0, 15, 25), (0, 15, 26), (0, 95, 105), (1, 15, 25)]  # (ref, start, end) ascending
    assert trip == [(0, 0, 2, 2), (2, 0, 1, 1), (0, 1, 1, 1), (1, 1, 1, 1), (3, 2, 1, 1)]  # by column, then junction
    assert counts == [6, 6, 4, 5]


def test_the_filtered_renumbering_and_the_files():
    reads = [(1, 10, "5M10N5M"), (0, 90, "5M10N5M"), (0, 10, "5M11N5M"), (0, 10, "5M10N5M")]
    jn, trip, _ = bucketed(reads, [0, 1, 2, 3], [1, 1, 1, 1], [0, 1, 2, 3], [0, 1, 2, 3, 4], [2, 0, 1, 3])
    fjn, ftrip = jm.filter_columns(jn, trip, [1, 2])
    assert list(zip(*(a.tolist() for a in fjn))) == [(0, 15, 26), (1, 15, 25)]
    assert list(zip(*(a.tolist() for a in ftrip))) == [(0, 0, 1, 1), (1, 1, 1, 1)]
    files = jm.directory_files(fjn, ftrip, 2, ["chrA", "chrB"])
    assert files["features.tsv"] == b"chrA\t16\t26\nchrB\t16\t25\n"  # the intron's first and last base, 1-based
    assert files["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n2 2 2\n1 1 1\n2 2 1\n" == files["reads.mtx"]
    none = jm.filter_columns(jn, trip, [])
    assert all(len(a) == 0 for a in none[0] + none[1])
    assert jm.directory_files(none[0], none[1], 0, [])["matrix.mtx"] == b"%%MatrixMarket matrix coordinate integer general\n0 0 0\n"


def test_the_generated_inputs_hold_what_the_gpu_tests_need():
    m = jm.make_inputs(5, [0, 1, 1, 2, 3, 5, 8, 32, 33, 40] * 12 + [257, 0, 1], 9)
    jn, trip, counts = jm.model_of(m)
    assert int(trip[3].sum()) == int(counts[1]) and (trip[2] <= trip[3]).all() and len(set(zip(trip[1].tolist(), trip[0].tolist()))) == len(trip[0])
    ops = set((m["cigar"] & 15).tolist())
    assert ops == {0, 1, 2, 3, 4, 5, 6, 7, 8}
    assert int((~jm.counted_reads(m)).sum()) > 100
    assert int(jm.model_of(jm.make_inputs(3, [3, 40, 1, 33, 7] * 40, 5, total=4097))[2][1]) == 4097


# ---- the walk the kernels run ------------------------------------------------------------------------------------

def walk_vectors():
    rng = np.random.default_rng(12)
    pool = jm.make_pool(rng)
    reads = []
    for text, pos in (("10M5N10M", 100), ("5N10M", 100), ("10M5N", 100), ("10M0N10M", 100), ("10M5N3I7N10M", 100), ("10M2D5N10M", 100),
                      ("10M50D10M", 100), ("10M20N1M", TOP - 30), ("10M21N1M", TOP - 30), ("5M" + "3N5M" * 300, 1000), ("", 5), ("4S", 5),
                      ("3M4N10M", -5), ("6M4N10M", -5), ("1M" + "268435455N" * 8 + "6N1M", 0), ("1M" + "268435455N" * 8 + "7N1M5N1M", 0)):
        reads.append((pos, jm.cigar_words(text)))
    for op in (9, 12, 15):
        reads.append((100, jm.cigar_words([(10, "M"), (5, "N"), (3, "M"), (2, op), (5, "N"), (3, "M")])))
        reads.append((100, jm.cigar_words([(2, op)])))
    for _ in range(400):
        r = pool[int(rng.integers(0, len(pool)))]
        k = int(rng.integers(0, 6))
        reads.append(jm.spliced_read(rng, r, int(rng.integers(0, len(r) - k + 1)), k))
    lines = []
    for pos, words in reads:
        try:
            js = jm.read_junctions(pos, words)
            tail = [len(js)] + [x for j in js for x in j]
        except jm.BadOp:
            tail = [-1]
        lines.append(" ".join(str(x) for x in [pos, len(words)] + list(words) + tail))
    return lines


def test_junction_walk_under_sanitizers(tmp_path):
    table = str(tmp_path / "junction_walk.txt")
    lines = walk_vectors()
    with open(table, "w") as f:
        f.write("\n".join(lines) + "\n")
    exe = str(tmp_path / "test_junction_walk")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           "-fno-omit-frame-pointer", "-o", exe, os.path.join(ROOT, "tests", "cpp", "test_junction_walk.cpp")])
    r = subprocess.run([exe, table], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout, r.stderr[-2000:])
    assert r.stdout.startswith("%d reads, " % len(lines)) and " 6 bad op codes, 0 failures" in r.stdout


# ---- the program's refusals -----------------------------------------------------------------------------------------

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
    assert "--junction-matrix goes with --count-matrix DIR only" in refused(tmp_path, ["--umi-tag", "UB", "--per-gene", "--junction-matrix"])


def test_the_flag_does_not_go_with_stage_gpu(built, tmp_path):
    assert "--stage gpu does not go with --junction-matrix" in refused(tmp_path, BASE + ["--junction-matrix", "--stage", "gpu"])


def test_the_other_refusals_keep_their_words(built, tmp_path):
    msg = refused(tmp_path, BASE + ["--saturation-curve", "c.tsv", "--stage", "gpu", "--junction-matrix"])
    assert "--stage gpu does not go with --saturation-curve (a read's entry is kept by the host staging alone)" in msg
    assert "--per-gene" in refused(tmp_path, ["--umi-tag", "UB", "--count-matrix", "m", "--junction-matrix"])  # (--count-matrix's own)


def test_directories_that_cannot_be_made(built, tmp_path):
    os.mkdir(tmp_path / "m")
    (tmp_path / "m" / "junctions").write_text("a file")
    msg = refused(tmp_path, BASE + ["--junction-matrix"], left=["m"])
    assert "cannot make the directory m/junctions for --junction-matrix" in msg
    os.remove(tmp_path / "m" / "junctions")
    os.mkdir(tmp_path / "m" / "junctions")
    (tmp_path / "m" / "junctions" / "filtered").write_text("a file")
    msg = refused(tmp_path, BASE + ["--junction-matrix", "--cell-filter", "min-molecules", "--cell-min-molecules", "3"], left=["m"])
    assert "cannot make the directory m/junctions/filtered for --junction-matrix" in msg


def test_the_flag_is_taken_with_everything_it_goes_with(built, tmp_path):
    # what ends the run is the input that is not there
    msg = refused(tmp_path, BASE + ["--junction-matrix", "--junction-matrix", "--umi-filtering", "multi-gene", "--saturation-curve", "a.tsv",
                                    "--cell-filter", "min-molecules", "--cell-min-molecules", "3", "--stage", "auto"], left=["m", "a.tsv"])
    assert "in.bam" in msg and "junction" not in msg
    assert sorted(os.listdir(tmp_path / "m")) == ["filtered", "junctions"] and os.listdir(tmp_path / "m" / "junctions") == ["filtered"]
    msg = refused(tmp_path, ["--umi-tag", "UB", "--per-gene", "--count-matrix", "m", "--junction-matrix", "--stage", "host"], left=["m", "a.tsv"])
    assert "in.bam" in msg and "junction" not in msg  # (without --per-cell too)


def test_without_the_flag_no_junction_line(built, tmp_path):
    # a run that stages nothing and touches no GPU: the summary of --dump-staging on an empty BAM
    import bamio
    import tag_model
    tag_model.write_bam(str(tmp_path / "in.bam"), bamio.make_header([("chrA", 1000)]), [])
    r = subprocess.run([CLI, "-i", "in.bam", "-o", "out.bam", "--umi-tag", "UB", "--per-gene", "--dump-staging", "staged.bin"], cwd=tmp_path,
                       capture_output=True, text=True, timeout=60)
    assert r.returncode == 0, r.stderr
    assert "Number of" in r.stderr and "unction" not in r.stderr
    assert not os.path.exists(tmp_path / "junctions")


def test_help_names_the_flag(built):
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0 and "--junction-matrix" in r.stdout
