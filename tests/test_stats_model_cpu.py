"""tests/stats_model.py against hand-worked buckets, the column identity umihip_stats.hip counts by against the
model's all-pairs sum, pick() beyond 32 bits against exact arithmetic, the tables' invariants -- and the refusals of
umicollapse --output-stats, which need no GPU."""
import os
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import oracle as orc
import stats_model as sm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def one_bucket(umis, kept=None, freq=None, seed=0, **kw):
    L = len(umis[0])
    n = len(umis)
    kept = [1] * n if kept is None else kept
    first = kept.index(1) if 1 in kept else 0
    root = [i if kept[i] else first for i in range(n)]
    return sm.stats_model(sm.encode(umis, L), freq or [1] * n, kept, root, [0, n], L, seed=seed, **kw)


def test_hand_worked_buckets():
    # ACG / ACT / TTT: pair by pair 1 (ACG-ACT), 3 (ACG-TTT), 2 (ACT-TTT), S = 6 and P = 3: bin 2.  (The feature's
    # write-up works this bucket with S = 5; either sum rounds up to bin 2.)
    assert sm.pair_sum(["ACG", "ACT", "TTT"]) == sm.column_sum(["ACG", "ACT", "TTT"]) == 6
    assert sm.bin_of(["ACG", "ACT", "TTT"], 3) == 2
    assert sm.bin_of(["ACG", "ACT", "TTA"], 3) == 3  # S = 1 + 3 + 3 = 7, ceil(7 / 3)
    assert sm.bin_of(["ACG", "ACG"], 3) == 0         # two equal picks
    assert sm.bin_of(["ACG"], 3) == 4                # "single"
    assert sm.bin_of([], 3) is None
    res = one_bucket(["ACG", "ACT", "TTT"], kept=[1, 0, 1])
    assert res["dist"][0].tolist() == [0, 0, 1, 0, 0]
    assert res["dist"][2].tolist() == [0, 0, 0, 1, 0]  # ACG / TTT: 3
    assert int(res["dist"][1].sum()) == int(res["dist"][3].sum()) == 1
    res = one_bucket(["ACG", "ACT", "TTT"], kept=[1, 0, 0])
    assert res["dist"][2].tolist() == [0, 0, 0, 0, 1] and res["dist"][3].tolist() == [0, 0, 0, 0, 1]
    # an empty bucket contributes nothing, wherever it lies
    keys = sm.encode(["AC", "AT"], 2)
    res = sm.stats_model(keys, [3, 1], [1, 0], [0, 0], [0, 0, 2, 2], 2)
    assert res["dist"].sum(axis=1).tolist() == [1, 1, 1, 1]
    assert res["count_pre"][[1, 3]].tolist() == [1, 1] and int(res["count_post"][4]) == 1 and int(res["count_post"].sum()) == 1
    # N is a letter of its own
    assert sm.pair_sum(["AN", "AA"]) == 1 and sm.pair_sum(["AN", "AN"]) == 0


def test_codes_and_straddling_bases():
    rng = np.random.default_rng(3)
    for L in (1, 21, 22, 42, 43, 64, 85):
        u = "".join("ACGTN"[x] for x in rng.integers(0, 5, L))
        keys = sm.encode([u], L)
        assert len(keys) == sm.n_words_of(L) and sm.decode(keys, 0, L, len(keys)) == u
    # the oracle's encoding is the same one
    assert int(orc.encode_keys(["ACGTNACGTACG"])[0][0]) == int(sm.encode(["ACGTNACGTACG"], 12)[0])


@pytest.mark.parametrize("n", [2, 3, 65, 600])
@pytest.mark.parametrize("L", [1, 12, 22, 85])
def test_column_identity_against_all_pairs(n, L):
    rng = np.random.default_rng(n * 100 + L)
    pool = ["".join("ACGTN"[x] for x in rng.choice(5, L, p=[0.3, 0.3, 0.2, 0.15, 0.05])) for _ in range(max(2, n // 3))]
    umis = [pool[int(rng.integers(0, len(pool)))] for _ in range(n)]  # a multiset: equal UMIs among them
    assert sm.pair_sum(umis) == sm.column_sum(umis)


def test_pick_beyond_32_bits():
    freq = [3, 2 ** 30, 1, 7, 2 ** 31 - 1, 2, 2 ** 31 - 1, 5]
    cum = list(np.cumsum(np.array(freq, dtype=object)))
    R = sum(freq)
    assert R > 2 ** 32
    hit = set()
    for seed in (0, 2 ** 64 - 1, 12345):
        for i in range(200):
            x = (seed + 0x9E3779B97F4A7C15 * (i + 1)) % 2 ** 64
            x ^= x >> 30
            x = x * 0xBF58476D1CE4E5B9 % 2 ** 64
            x ^= x >> 27
            x = x * 0x94D049BB133111EB % 2 ** 64
            x ^= x >> 31
            t = int(Fraction(x * R, 2 ** 64))  # floor
            exp = next(e for e in range(len(freq)) if sum(freq[:e + 1]) > t)
            assert sm.pick(i, seed, cum) == exp
            hit.add(exp)
    assert {1, 4, 6} <= hit  # the heavy entries take the draws


def random_call(seed, L=9, n_buckets=14, n_frac=0.05):
    """seeded buckets, the oracle's directional collapse on them"""
    rng = np.random.default_rng(seed)
    umis, freq, off = [], [], [0]
    for b in range(n_buckets):
        size = int(rng.integers(0, 9)) if b % 4 else 0
        centre = rng.integers(0, 4, L)
        seen = {}
        for _ in range(size * 2):
            u = centre.copy()
            for at in rng.integers(0, L, int(rng.integers(0, 3))):
                u[at] = rng.integers(0, 4)
            text = "".join("ACGT"[x] for x in u)
            if rng.random() < n_frac:
                at = int(rng.integers(0, L))
                text = text[:at] + "N" + text[at + 1:]
            seen[text] = seen.get(text, 0) + int(rng.integers(1, 6))
        order = sorted(seen, key=lambda t: -seen[t])  # rank order: freq descending, ties by first appearance
        umis += order
        freq += [seen[t] for t in order]
        off.append(len(umis))
    keys = sm.encode(umis, L)
    nmask = np.zeros_like(keys)
    for i, u in enumerate(umis):
        nmask[i] = sum(7 << (3 * b) for b, ch in enumerate(u) if ch == "N")
    freq, off = np.array(freq, np.int32), np.array(off, np.uint64)
    kept, root, _ = orc.dedup_batch(keys, nmask, freq, off, L, 1)
    return keys, freq, kept, root, off, L


@pytest.mark.parametrize("seed", range(4))
def test_invariants(seed):
    keys, freq, kept, root, off, L = random_call(seed)
    res = sm.stats_model(keys, freq, kept, root, off, L, seed=seed, hist_bins=64)
    non_empty = int(np.count_nonzero(np.diff(off.astype(np.int64))))
    reads = int(freq.astype(np.int64).sum())
    assert non_empty > 3 and res["dist"].sum(axis=1).tolist() == [non_empty] * 4
    c = np.arange(64, dtype=np.int64)
    assert int(res["count_pre"][63]) == int(res["count_post"][63]) == 0  # (nothing reached the last bin)
    assert int((c * res["count_pre"].astype(np.int64)).sum()) == int((c * res["count_post"].astype(np.int64)).sum()) == reads
    assert int(res["count_post"].sum()) == int(np.count_nonzero(kept)) and int(res["count_pre"].sum()) == len(freq)
    assert int(res["reads_post"].sum()) == int(res["reads_pre"].sum()) == reads
    assert int(res["times_pre"].sum()) == len(freq) and int(res["times_post"].sum()) == int(np.count_nonzero(kept))
    ints = [sm.key_int(keys, int(e), 1) for e in res["umi_entry"]]
    assert ints == sorted(set(sm.key_int(keys, i, 1) for i in range(len(freq))))
    assert int(res["count_pre"][0]) == int(res["count_post"][0]) == 0
    # the last bin collects what lies at or above it
    low = sm.stats_model(keys, freq, kept, root, off, L, seed=seed, hist_bins=3, per_umi=False)
    assert int(low["count_pre"].sum()) == len(freq) and int(low["count_pre"][2]) == int(np.count_nonzero(freq >= 2))
    assert "umi_entry" not in low


def test_the_writers():
    keys, freq, kept, root, off, L = random_call(1)
    a, b, c = sm.stats_files(keys, freq, kept, root, off, L, "dir", seed=4)
    assert a.splitlines()[0] == "counts\tinstances_pre\tinstances_post" and "+" not in a
    rows = b.splitlines()
    assert rows[0] == "edit_distance\tunique\tunique_null\tdir\tdir_null"
    assert [r.split("\t")[0] for r in rows[1:]] == [str(j) for j in range(L + 1)] + ["Single_UMI"]
    assert c.splitlines()[0].split("\t")[0] == "UMI" and all(len(r.split("\t")[0]) == L for r in c.splitlines()[1:])
    assert sm.per_position_text(np.array([0, 1, 2], np.uint64), np.array([0, 0, 1], np.uint64)) == \
        "counts\tinstances_pre\tinstances_post\n1\t1\t0\n2+\t2\t1\n"


# ---- the program's refusals: status 101 with --output-stats in the message (an unknown flag is 101 as well)
def run(flags):
    return subprocess.run([CLI] + flags, capture_output=True, text=True, timeout=120)


@pytest.mark.parametrize("flags", [
    ["-m", "fastq", "--output-stats", "P"],
    ["--two-pass", "--output-stats", "P"],
    ["--dump-staging", "S", "--output-stats", "P"],
    ["--passthrough", "--output-stats", "P"],
    ["--output-stats-seed", "3"],
    ["--output-stats", "P", "--output-stats-seed", "-1"],
    ["--output-stats", "P", "--output-stats-seed", "18446744073709551616"],
    ["--output-stats", "P", "--output-stats-seed", "1.5"],
    ["--output-stats", "P", "--output-stats-seed", ""],
], ids=["fastq", "two-pass", "dump-staging", "passthrough", "seed alone", "negative seed", "seed 2^64", "fraction", "empty seed"])
def test_refusals(tmp_path, flags):
    flags = [str(tmp_path / f) if f in ("P", "S") else f for f in flags]
    r = run(["-i", str(tmp_path / "missing.bam"), "-o", str(tmp_path / "o.bam")] + flags)
    assert r.returncode == 101 and "--output-stats" in r.stderr and "unexpected argument" not in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "P_per_umi.tsv"))


def test_unwritable_prefix_ends_the_run_before_the_input_is_read(tmp_path):
    r = run(["-i", str(tmp_path / "missing.bam"), "-o", str(tmp_path / "o.bam"), "--output-stats", str(tmp_path / "no" / "dir" / "p")])
    assert r.returncode == 101 and "--output-stats" in r.stderr and "_per_umi_per_position.tsv" in r.stderr, r.stderr
    # another refusal wins over the files: nothing is made
    r = run(["-i", str(tmp_path / "missing.bam"), "-o", str(tmp_path / "o.bam"), "--output-stats", str(tmp_path / "p"), "--algo", "cc"])
    assert r.returncode == 101 and "Invalid algorithm combination" in r.stderr
    assert not os.path.exists(str(tmp_path / "p_per_umi.tsv"))


def test_help_names_the_flag():
    r = run(["--help"])
    assert r.returncode == 0 and "--output-stats <PREFIX>" in r.stdout and "--output-stats-seed" in r.stdout
