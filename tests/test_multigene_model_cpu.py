"""--umi-filtering multi-gene without a GPU: tests/multigene_model.py against its own brute-force statement, the
planted cases of multigene_bam, the model's invariants on it, and the refusals that end a run with status 101 before
the GPU is woken."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import gene_model as gm
import multigene_model as mm
import stats_model as sm
import tag_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SEED = 21  # the seed tests/test_gpu_multigene_cli.py runs the program on


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


@pytest.fixture(scope="module")
def expected():
    return mm.expected(mm.multigene_bam(SEED)[1])


def random_case(seed):
    """buckets of 0 to 6 entries over a pool of few UMIs (N among their letters, garbage above them), a forest per
    bucket, few groups"""
    rng = np.random.default_rng(seed)
    L = int(rng.choice([3, 12, 21, 22, 43]))
    nb = int(rng.integers(1, 40))
    sizes = rng.integers(0, 7, nb) * (rng.random(nb) < 0.8)
    n = int(sizes.sum())
    pool = ["".join("ACGTN"[x] for x in rng.choice(5, L, p=[.24, .24, .24, .24, .04])) for _ in range(max(2, n // 3))]
    keys = sm.encode([pool[int(rng.integers(0, len(pool)))] for _ in range(n)], L)
    nw = sm.n_words_of(L)
    top = 3 * L - 64 * (nw - 1)
    if top < 64 and n:
        keys.reshape(-1, nw)[:, nw - 1] |= rng.integers(0, 2 ** 63, n, dtype=np.uint64) << np.uint64(top)
    kept, root = np.zeros(n, np.uint8), np.zeros(n, np.uint32)
    base = 0
    for size in sizes:
        if size:
            k = rng.random(size) < 0.6
            k[int(rng.integers(0, size))] = True
            idx = np.flatnonzero(k)
            kept[base:base + size] = np.where(k, rng.integers(1, 256, size), 0)
            root[base:base + size] = [base + (i if k[i] else int(idx[rng.integers(0, len(idx))])) for i in range(size)]
        base += size
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n_groups = int(rng.integers(1, 4))
    return keys, rng.integers(1, 4, n).astype(np.int32), kept, root, off, rng.integers(0, n_groups, nb).astype(np.uint32), L


@pytest.mark.parametrize("seed", range(40))
def test_model_agrees_with_the_brute_force_statement(seed):
    case = random_case(seed)
    a, b = mm.filter_model(*case), mm.brute_filter(*case)
    assert (a[0] == b[0]).all() and (a[1] == b[1]).all() and a[2] == b[2]
    kept = case[2]
    assert not (a[0] & (kept == 0)).any() and set(np.unique(a[0]).tolist()) <= {0, 1}
    assert a[2]["removed"] + int(a[0].sum()) == int(np.count_nonzero(kept))
    assert int(a[1].astype(np.int64).sum()) + a[2]["removed_reads"] == int(case[1].astype(np.int64).sum())


def test_the_random_cases_reach_every_outcome():
    seen = {"runs": 0, "removed": 0, "survivor in a run": 0, "run without survivor": 0}
    for seed in range(40):
        case = random_case(seed)
        kept_out, _, counts = mm.filter_model(*case)
        seen["runs"] += counts["runs"]
        seen["removed"] += counts["removed"]
        mols, _ = mm._molecules(case[0], case[1], case[2], case[3], case[4], case[5], case[6], None)
        runs = {}
        for i, g, u, _ in mols:
            runs.setdefault((g, u), []).append(i)
        for members in runs.values():
            if len(members) > 1:
                alive = sum(int(kept_out[i]) for i in members)
                assert alive <= 1
                seen["survivor in a run" if alive else "run without survivor"] += 1
    assert all(v > 10 for v in seen.values()), seen


def test_model_edges():
    z = np.zeros(0)
    k, f, c = mm.filter_model(z, z, z, z, [0], z, 5)
    assert len(k) == 0 and len(f) == 0 and c == {"runs": 0, "removed": 0, "removed_reads": 0}
    k, f, c = mm.filter_model(z, z, z, z, [0, 0, 0], [7, 7], 5)
    assert len(k) == 0 and c["runs"] == 0
    # two buckets of one group with the same UMI: 2^31 - 1 three times against once
    big = 2 ** 31 - 1
    keys = sm.encode(["ACG", "ACG", "ACG", "ACG"], 3)
    k, f, c = mm.filter_model(keys, [big, big, big, big], [1, 0, 0, 9], [0, 0, 0, 3], [0, 3, 4], [0, 0], 3)
    assert k.tolist() == [1, 0, 0, 0] and f.tolist() == [big, big, big, 0] and c == {"runs": 1, "removed": 1, "removed_reads": big}
    # ... in two groups: nothing is joined
    k, f, c = mm.filter_model(keys, [big, big, big, big], [1, 0, 0, 9], [0, 0, 0, 3], [0, 3, 4], [0, 1], 3)
    assert k.tolist() == [1, 0, 0, 1] and c["runs"] == 0


def test_every_planted_case_occurs(expected):
    assert mm.classes(expected) == set(mm.CLASSES)


def test_the_filter_changes_the_output_and_the_counts_add_up(expected):
    e = expected
    unfiltered = [i for i in np.nonzero(e["kept"])[0]]
    assert 0 < len(e["records"]) < len(unfiltered)
    assert e["counts"]["removed"] + len(e["records"]) == len(unfiltered)
    assert e["counts"]["runs"] >= 6 and e["counts"]["removed_reads"] > 0
    # the matrix: no zero lines, the histogram of the records, the reads of the survivors
    mol, reads = gm.parse_matrix(e["files"])
    assert all(v > 0 for v in mol.values())
    assert mol == gm.histogram(e["records"], per_cell=True)
    assert sum(reads.values()) == int(e["st"]["freq"].sum()) - e["counts"]["removed_reads"]
    plain = gm.expected_matrix(e["st"], e["kept"])
    assert plain["features.tsv"] == e["files"]["features.tsv"] and plain["barcodes.tsv"] == e["files"]["barcodes.tsv"]
    # ... one line fewer: the pair that lost all its molecules is left out, of NNZ as well
    lines, plain_lines = e["files"]["matrix.mtx"].splitlines(), plain["matrix.mtx"].splitlines()
    assert len(lines) == len(plain_lines) - 1 and int(lines[1].split()[2]) == len(lines) - 2 == int(plain_lines[1].split()[2]) - 1
    assert len(e["files"]["reads.mtx"].splitlines()) == len(lines)


def test_without_per_cell_the_one_cell_joins_more(expected):
    one = mm.expected(mm.multigene_bam(SEED)[1], per_cell=False)
    assert one["counts"]["runs"] > 0 and mm.CLASSES[6] not in mm.classes(one)
    assert one["files"]["barcodes.tsv"] == b"all\n"


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def small_file(tmp_path):
    header = bamio.make_header([("chr1", 100000)])
    z = tag_model.aux_z
    tags = z("UB", "ACGTACGTAC") + z("CB", "AAAC-1") + z("GX", "G1")
    recs = [bamio.make_record("r%d" % i, 0, 0, 500 + 200 * i, 60, [("M", 50)], 50, bytes([30] * 50), tags=tags) for i in range(2)]
    src = str(tmp_path / "in.bam")
    tag_model.write_bam(src, header, recs)
    return src


REFUSALS = [
    (["--umi-filtering", "multi-gene"], "--umi-filtering multi-gene goes with --per-gene only"),
    (["--per-cell", "--umi-filtering", "multi-gene"], "--umi-filtering multi-gene goes with --per-gene only"),
    (["--per-gene", "--umi-filtering", "multigene"], "--umi-filtering wants none or multi-gene"),
    (["--per-gene", "--umi-filtering", ""], "--umi-filtering wants none or multi-gene"),
    (["--umi-filtering", "MultiGeneUMI_CR"], "--umi-filtering wants none or multi-gene"),
    (["--per-gene", "--umi-filtering", "none", "--umi-filtering", "multi-gene"], "--umi-filtering given twice with different values"),
    (["--per-gene", "--umi-filtering", "multi-gene", "--umi-filtering", "none"], "--umi-filtering given twice with different values"),
]


@pytest.mark.parametrize("flags,text", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_refusals(tmp_path, flags, text):
    src = small_file(tmp_path)
    matrix = ["--count-matrix", str(tmp_path / "m")] if "--per-gene" in flags else []  # (refused itself without --per-gene)
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB"] + matrix + flags)
    assert r.returncode == 101, r.stderr
    assert text in r.stderr and "--umi-filtering" in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "m")) and not os.path.exists(str(tmp_path / "o.bam"))


def test_a_value_is_required(tmp_path):
    r = run(["-i", small_file(tmp_path), "-o", str(tmp_path / "o.bam"), "--per-gene", "--umi-filtering"])
    assert r.returncode == 101 and "--umi-filtering" in r.stderr and not os.path.exists(str(tmp_path / "o.bam")), r.stderr


def test_help_names_the_flag_and_its_values():
    r = run(["--help"])
    assert r.returncode == 0
    at = r.stdout.index("--umi-filtering")
    assert "none" in r.stdout[at:at + 200] and "multi-gene" in r.stdout[at:at + 200]


def test_dump_staging_is_unaffected(tmp_path):
    """the exit before the collapse: the same staging file with and without the flag"""
    header, recs = mm.multigene_bam(SEED)
    src = str(tmp_path / "in.bam")
    tag_model.write_bam(src, header, recs)
    dumps = []
    for name, flags in (("a", []), ("b", ["--umi-filtering", "multi-gene"]), ("c", ["--umi-filtering", "none"])):
        out = str(tmp_path / name)
        r = run(["-i", src, "-o", str(tmp_path / "unused.bam"), "--umi-tag", "UB", "--per-cell", "--per-gene", "--dump-staging", out] + flags)
        assert r.returncode == 0, r.stderr
        assert "UMI filtering" not in r.stderr
        dumps.append(open(out, "rb").read())
    assert dumps[0] == dumps[1] == dumps[2] and len(dumps[0]) > 32
