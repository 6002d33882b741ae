"""--cell-filter without a GPU: tests/cells_model.py against a brute force over Python ints, the rule's corners by
hand, the generated inputs against the properties they are named for, the program's inputs against what the GPU tests
need of them, and the refusals that end a run with status 101 before the GPU is woken."""
import os
import subprocess

import numpy as np
import pytest

import cells_model as cm
import gene_model as gm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SEED = 33  # the seed tests/test_gpu_cell_filter_cli.py runs the program on


def brute(case, rule, expect_cells=3000, percentile_permille=990, max_min_ratio=10, min_molecules=1):
    """the statement of the issue, triplet by triplet over Python ints and a list sort"""
    T, R, G = [0] * case.n_cols, [0] * case.n_cols, [0] * case.n_cols
    for r, c, m, rd in zip(case.row.tolist(), case.col.tolist(), case.molecules.tolist(), case.reads.tolist()):
        T[c] += m
        R[c] += rd
        G[c] += m > 0
    S = sorted((t for t in T if t >= 1), reverse=True)
    n = len(S)
    m = 0
    if n == 0:
        t = 0
    elif rule == cm.CR22:
        m = S[min(n - 1, expect_cells * (1000 - percentile_permille) // 1000)]
        t = max(1, (2 * m + max_min_ratio) // (2 * max_min_ratio))
    elif rule == cm.TOP:
        t = S[min(n - 1, expect_cells - 1)]
    else:
        t = max(1, min_molecules)
    called = [int(T[c] >= 1 and T[c] >= t) for c in range(case.n_cols)]
    new_col, k = [], 0
    for c in range(case.n_cols):
        new_col.append(k if called[c] else cm.NOT_CALLED)
        k += called[c]
    trip = [(r, new_col[c], mo, rd) for r, c, mo, rd in
            zip(case.row.tolist(), case.col.tolist(), case.molecules.tolist(), case.reads.tolist()) if called[c] and mo > 0]
    med = lambda v: sorted(v)[(len(v) - 1) // 2] if v else 0
    in_cells = [c for c in range(case.n_cols) if called[c]]
    counts = [n, k, t, m, sum(T[c] for c in in_cells), sum(R[c] for c in in_cells), sum(T), sum(R), med([T[c] for c in in_cells]),
              med([G[c] for c in in_cells])]
    return (T, R, G, called, new_col), trip, dict(zip(cm.COUNTS, counts))


def same_as_brute(case, **rule):
    per, trip, counts = cm.call_model(case, **rule)
    (T, R, G, called, new_col), btrip, bcounts = brute(case, **rule)
    assert [per[k].tolist() for k in ("cell_molecules", "cell_reads", "cell_genes", "called", "new_col")] == [T, R, G, called, new_col]
    assert list(zip(*(a.tolist() for a in trip))) == btrip
    assert counts == bcounts
    assert per["cell_molecules"].dtype == per["cell_reads"].dtype == trip[3].dtype == np.uint64
    assert per["cell_genes"].dtype == per["new_col"].dtype == trip[0].dtype == trip[1].dtype == trip[2].dtype == np.uint32
    assert per["called"].dtype == np.uint8
    return counts


RULESETS = [dict(rule=cm.CR22), dict(rule=cm.CR22, expect_cells=10, percentile_permille=900, max_min_ratio=3),
            dict(rule=cm.CR22, expect_cells=7, percentile_permille=0, max_min_ratio=1), dict(rule=cm.TOP, expect_cells=5),
            dict(rule=cm.TOP, expect_cells=1), dict(rule=cm.MIN, min_molecules=9), dict(rule=cm.MIN, min_molecules=0)]


@pytest.mark.parametrize("seed", range(4))
def test_model_is_the_brute_force(seed):
    some_called = some_not = 0
    for nnz in (0, 1, 2, 65, 700):
        for case in (cm.random_case(seed, nnz), cm.one_column(seed, nnz), cm.one_each(seed, nnz)):
            for rule in RULESETS:
                c = same_as_brute(case, **rule)
                some_called += c["called"] > 0
                some_not += c["called"] < c["candidates"]
    for rule in RULESETS:
        same_as_brute(cm.big_case(), **rule)
        same_as_brute(cm.runs_case(seed, [1, 2, 64, 65, 130, 1, 3]), **rule)
    assert some_called > 10 and some_not > 10


def call(totals, **rule):
    per, _, counts = cm.call_model(cm.totals_case(totals), **rule)
    return counts, per["called"].tolist()


def test_the_rules_corners_by_hand():
    # the defaults: i = floor(3000 * 10 / 1000) = 30
    totals = list(range(1000, 900, -1))  # S[30] = 970, t = 97
    c, called = call(totals, rule=cm.CR22)
    assert (c["knee"], c["threshold"], c["called"], c["candidates"]) == (970, 97, 100, 100)
    c, called = call(totals + [97, 96], rule=cm.CR22)
    assert (c["knee"], c["threshold"], c["called"]) == (970, 97, 101) and called[-2:] == [1, 0]
    assert cm.threshold(totals, cm.CR22) == (97, 970)
    # n = 1
    for rule in RULESETS:
        c, called = call([7], **rule)
        assert c["candidates"] == 1 and called == [int(rule.get("min_molecules", 1) <= 7)]
    # N beyond n: the last candidate is the knee
    c, called = call([50, 40, 0, 30], rule=cm.CR22, expect_cells=1000, percentile_permille=0, max_min_ratio=1)
    assert (c["knee"], c["threshold"], c["candidates"], called) == (30, 30, 3, [1, 1, 0, 1])
    c, called = call([50, 40, 0, 30], rule=cm.TOP, expect_cells=4)
    assert (c["threshold"], c["knee"], called) == (30, 0, [1, 1, 0, 1])
    # P = 1000: i = 0
    c, called = call([5, 100, 40, 9], rule=cm.CR22, percentile_permille=1000)
    assert (c["knee"], c["threshold"], called) == (100, 10, [0, 1, 1, 0])
    # m < R / 2: t = 1, and m = R / 2 rounds up to 1 as well
    for m in (1, 4, 5):
        c, called = call([m, 1, 0], rule=cm.CR22, expect_cells=1, percentile_permille=1000, max_min_ratio=10)
        assert (c["knee"], c["threshold"], called) == (m, 1, [1, 1, 0])
    # half up: 15 / 10 -> 2, 14 / 10 -> 1, 25 / 10 -> 3
    assert [cm.threshold([m], cm.CR22)[0] for m in (14, 15, 24, 25)] == [1, 2, 2, 3]
    # ties at t are called whole
    c, called = call([9, 7, 7, 7, 3], rule=cm.TOP, expect_cells=2)
    assert (c["threshold"], c["called"], called) == (7, 4, [1, 1, 1, 1, 0])
    c, called = call([9, 7, 7, 7, 3], rule=cm.MIN, min_molecules=7)
    assert (c["called"], c["median_molecules"]) == (4, 7)
    # nothing: t = 0
    c, called = call([0, 0], rule=cm.TOP, expect_cells=1)
    assert (c["candidates"], c["called"], c["threshold"], c["median_molecules"], called) == (0, 0, 0, 0, [0, 0])
    # lower medians
    assert [cm.lower_median(v) for v in ([], [4], [4, 9], [9, 4, 6], [1, 2, 3, 4])] == [0, 4, 4, 6, 2]


def test_totals_above_32_bits():
    case = cm.big_case()
    per, trip, c = cm.call_model(case, rule=cm.TOP, expect_cells=1)
    assert int(per["cell_molecules"][1]) == 3 * 0xFFFFFFFF > 2 ** 32 and c["threshold"] == 3 * 0xFFFFFFFF
    assert int(per["cell_reads"][1]) > 2 ** 41 and per["called"].tolist() == [0, 1, 0, 0, 0, 0]
    assert trip[1].tolist() == [0, 0, 0] and c["median_molecules"] == 3 * 0xFFFFFFFF
    # a column of zeros has reads and is no candidate
    assert int(per["cell_molecules"][3]) == 0 and int(per["cell_reads"][3]) == 10 and c["candidates"] == 4
    per, _, c = cm.call_model(case, rule=cm.MIN, min_molecules=1)
    assert per["called"].tolist() == [1, 1, 1, 0, 1, 0] and per["new_col"].tolist() == [0, 1, 2, cm.NOT_CALLED, 3, cm.NOT_CALLED]
    assert c["median_genes"] == 1 and c["median_molecules"] == 3


def sorted_and_distinct(case):
    pairs = list(zip(case.col.tolist(), case.row.tolist()))
    return all(a < b for a, b in zip(pairs, pairs[1:])) and all(c < case.n_cols and r < case.n_rows for c, r in pairs)


def test_generated_inputs_have_the_properties_they_are_named_for():
    for nnz in (0, 1, 2, 63, 64, 65, 255, 256, 257, 1500):
        for case in (cm.random_case(1, nnz), cm.one_column(2, nnz), cm.one_each(3, nnz)):
            assert len(case.row) == len(case.col) == len(case.molecules) == len(case.reads) == nnz
            assert sorted_and_distinct(case)
        assert cm.one_column(2, nnz).n_cols == 1
        assert len(set(cm.one_each(3, nnz).col.tolist())) == nnz
    case = cm.random_case(4, 1500)
    assert (case.molecules == 0).any() and (case.reads >= case.molecules).all() and (case.reads > 0).all()
    runs = [5, 64, 65, 130, 1030, 2500, 1, 1, 3]
    case = cm.runs_case(5, runs)
    assert sorted_and_distinct(case)
    cols, lengths = np.unique(case.col, return_counts=True)
    assert lengths.tolist() == runs
    assert len(cols) < int(cols.max()) + 1 < case.n_cols  # gaps in the ids, and empty columns behind the last
    start = np.concatenate([[0], np.cumsum(runs)])
    inside = [(a // 64 == (b - 1) // 64) for a, b in zip(start[:-1], start[1:])]
    blocks = [(b - 1) // 1024 - a // 1024 for a, b in zip(start[:-1], start[1:])]
    assert any(inside) and not all(inside) and 1 in blocks and max(blocks) >= 2  # one wave, waves, a block's edge, several blocks
    # ties at the threshold under a rule of each kind
    case = cm.tied_case(6)
    assert sorted_and_distinct(case) and (case.molecules == 0).any()
    for rule, t in zip(cm.TIED_RULES, (40, 4, 40)):
        per, _, c = cm.call_model(case, **rule)
        assert c["threshold"] == t and int((per["cell_molecules"] == np.uint64(t)).sum()) == 3
        assert sorted(per["cell_molecules"].tolist()) == sorted(cm.TIED_TOTALS)
        assert c["called"] == int((per["cell_molecules"] >= np.uint64(t)).sum()) < c["candidates"]
        same_as_brute(case, **rule)


@pytest.fixture(scope="module")
def raw_files():
    """what --per-cell --per-gene --count-matrix writes for the CLI tests' BAM, by the model"""
    header, recs, cells = cm.cells_bam(SEED)
    _, st, kept = gm.expected_output(recs, per_cell=True)
    return gm.expected_matrix(st, kept), cells


def test_cli_inputs_split_the_cells_under_each_rule(raw_files):
    files, cells = raw_files
    case, names = cm.case_of_files(files)
    assert sorted(names) == sorted(c.encode() + b"-1" for c in cells)
    for name, (flags, rule) in cm.CLI_RULES.items():
        per, trip, c = cm.call_model(case, **rule)
        assert c["called"] >= 2 and c["candidates"] - c["called"] >= 2, (name, c)
        # (the deepest cell's doubled UMI is a molecule under either gene)
        assert c["candidates"] == len(cm.DEPTHS) and sorted(per["cell_molecules"].tolist()) == sorted((cm.DEPTHS[0] + 1,) + cm.DEPTHS[1:])
        out, counts = cm.files_model(files, **rule)
        assert counts == c and len(out["filtered/barcodes.tsv"].splitlines()) == c["called"]
        assert len(out["cells.tsv"].splitlines()) == 1 + c["candidates"]
    per, _, c = cm.call_model(case, **cm.CLI_RULES["top-cells"][1])
    assert int((per["cell_molecules"] == np.uint64(c["threshold"])).sum()) >= 2 and c["called"] > 3  # a tie at the threshold


IO = ["-i", "in.bam", "-o", "out.bam"]
FULL = IO + ["--umi-tag", "UB", "--per-cell", "--per-gene", "--count-matrix", "m"]
REFUSALS = [
    (IO + ["--umi-tag", "UB", "--per-gene", "--count-matrix", "m", "--cell-filter", "cr2.2"], "--cell-filter"),
    (IO + ["--umi-tag", "UB", "--per-cell", "--count-matrix", "m", "--cell-filter", "cr2.2"], "--count-matrix"),
    (IO + ["--umi-tag", "UB", "--per-cell", "--per-gene", "--cell-filter", "cr2.2"], "--cell-filter"),
    (FULL + ["--cell-filter", "knee"], "--cell-filter wants"),
    (FULL + ["--expect-cells", "5"], "--expect-cells"),
    (FULL + ["--cell-filter-percentile", "0.9"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter-ratio", "5"], "--cell-filter-ratio"),
    (FULL + ["--cell-min-molecules", "5"], "--cell-min-molecules"),
    (FULL + ["--cell-filter", "min-molecules", "--cell-min-molecules", "5", "--expect-cells", "5"], "--expect-cells"),
    (FULL + ["--cell-filter", "top-cells", "--expect-cells", "5", "--cell-filter-percentile", "0.9"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter", "top-cells", "--expect-cells", "5", "--cell-filter-ratio", "3"], "--cell-filter-ratio"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-min-molecules", "5"], "--cell-min-molecules"),
    (FULL + ["--cell-filter", "top-cells"], "--expect-cells"),
    (FULL + ["--cell-filter", "min-molecules"], "--cell-min-molecules"),
    (FULL + ["--cell-filter", "cr2.2", "--expect-cells", "0"], "--expect-cells"),
    (FULL + ["--cell-filter", "cr2.2", "--expect-cells", "-3"], "--expect-cells"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter-ratio", "0"], "--cell-filter-ratio"),
    (FULL + ["--cell-filter", "min-molecules", "--cell-min-molecules", "0"], "--cell-min-molecules"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter-percentile", "1.1"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter-percentile", "-0.5"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter-percentile", "0.9905"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter-percentile", "99e-2"], "--cell-filter-percentile"),
    (FULL + ["--cell-filter", "cr2.2", "--cell-filter", "top-cells", "--expect-cells", "3"], "--cell-filter given twice"),
]


@pytest.mark.parametrize("argv,names", REFUSALS, ids=[str(i) for i in range(len(REFUSALS))])
def test_program_refuses_before_the_gpu(argv, names, tmp_path):
    r = subprocess.run([CLI] + argv, cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 101, r.stderr
    assert names in r.stderr
    assert not os.listdir(tmp_path)


def test_program_refuses_a_filtered_directory_that_cannot_be_made(tmp_path):
    (tmp_path / "m").mkdir()
    (tmp_path / "m" / "filtered").write_text("in the way\n")
    r = subprocess.run([CLI] + FULL + ["--cell-filter", "cr2.2"], cwd=tmp_path, capture_output=True, text=True)
    assert r.returncode == 101 and "--cell-filter" in r.stderr and "m/filtered" in r.stderr, r.stderr
    assert os.listdir(tmp_path) == ["m"] and os.listdir(tmp_path / "m") == ["filtered"]


def test_the_same_rule_twice_is_one_rule(tmp_path):
    """(refused for the input that is not there, not for the flags)"""
    r = subprocess.run([CLI] + FULL + ["--cell-filter", "cr2.2", "--cell-filter", "cr2.2"], cwd=tmp_path, capture_output=True, text=True)
    assert "given twice" not in r.stderr and "in.bam" in r.stderr


def test_help_names_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--cell-filter", "--expect-cells", "--cell-filter-percentile", "--cell-filter-ratio", "--cell-min-molecules", "cr2.2",
                 "top-cells", "min-molecules"):
        assert flag in r.stdout, flag


def test_library_exports_the_entry_points_and_the_rules():
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    lib = umi.load()
    assert lib.umi_call_cells and lib.umi_call_cells_device
    assert (umi.UMI_CELLS_CR22, umi.UMI_CELLS_TOP, umi.UMI_CELLS_MIN) == (cm.CR22, cm.TOP, cm.MIN) == (0, 1, 2)
    assert umi.Context.CELLS_COUNTS == cm.COUNTS
    text = open(os.path.join(ROOT, "include", "umihip.h")).read()
    assert "#define UMI_CELLS_CR22 0" in text and "#define UMI_CELLS_TOP 1" in text and "#define UMI_CELLS_MIN 2" in text
    assert "umi_call_cells" in _lib.SIGNATURES and "umi_call_cells_device" in _lib.SIGNATURES
