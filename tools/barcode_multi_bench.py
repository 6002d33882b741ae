"""umi_correct_barcodes_multi_device on resident data, beside umi_correct_barcodes_device on the same arrays.  One
JSON line per shape on stdout and, with --record, appended to profiles/barcode_multi_bench.jsonl.

  lists: 737,280 and 6,794,880 distinct barcodes of 16 bases (the sizes of the 10x lists), random, a tenth of
      them another entry with two substitutions -- what an ambiguous read is made from;
  reads: 10^7 -- 93 % exact, 3 % one substitution, 1 % one N, 1 % random and 2 % halfway between two listed
      barcodes two bases apart (ambiguous under 1MM) -- with random qualities 2..40; with --skew F a fraction F of
      the reads is one barcode's exact reads (a deep cell: the histogram's hot address).
  Both calls are timed with device events (they synchronise inside): median of --reps calls after a warm-up call.

usage: python tools/barcode_multi_bench.py [--reps 50] [--reads N] [--skew F] [--min-list N] [--max-list N] [--record]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context  # noqa: E402

L = 16
LISTS = [737_280, 6_794_880]
ACGT = np.frombuffer(b"ACGT", np.uint8)


def letters(codes):
    return ACGT[((codes[:, None] >> (2 * np.arange(L, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.intp)]


def near_list(rng, n_wl):
    """(codes uint64 [n_wl], half): a tenth of the entries is another entry with other letters at two positions, and
    half holds, per such pair, the unlisted barcode with one of the two letters changed: one base from both"""
    m = n_wl // 10
    base = rng.permutation(np.unique(rng.integers(0, 4 ** L, int(n_wl * 1.01) + 16, dtype=np.uint64)))[:n_wl]
    j = rng.choice(n_wl - m, m, replace=False)
    p_j = rng.integers(0, L, m)
    p_k = (p_j + rng.integers(1, L, m)) % L
    half = base[j] ^ (rng.integers(1, 4, m).astype(np.uint64) << (2 * p_j).astype(np.uint64))
    far = half ^ (rng.integers(1, 4, m).astype(np.uint64) << (2 * p_k).astype(np.uint64))
    _, first = np.unique(far, return_index=True)
    ok = np.zeros(m, bool)
    ok[first] = True
    ok &= ~np.isin(far, base) & ~np.isin(half, base)
    j, half, far = j[ok], half[ok], far[ok]
    codes = base.copy()
    k = n_wl - m + np.arange(len(far))  # (the sources lie before n_wl - m)
    codes[k] = far
    assert len(np.unique(codes)) == n_wl
    return codes, half


def make_reads(rng, codes, half, n, skew):
    u = letters(codes[rng.integers(0, len(codes), n)])
    r = rng.random(n)
    sub = np.flatnonzero(r < 0.03)
    at = rng.integers(0, L, len(sub))
    u[sub, at] = ACGT[(np.searchsorted(ACGT, u[sub, at]) + rng.integers(1, 4, len(sub))) % 4]
    with_n = np.flatnonzero((r >= 0.03) & (r < 0.04))
    u[with_n, rng.integers(0, L, len(with_n))] = ord("N")
    rnd = np.flatnonzero((r >= 0.04) & (r < 0.05))
    u[rnd] = ACGT[rng.integers(0, 4, (len(rnd), L))]
    amb = np.flatnonzero((r >= 0.05) & (r < 0.07))
    u[amb] = letters(half[rng.integers(0, len(half), len(amb))])
    if skew:
        u[rng.random(n) < skew] = letters(codes[:1])[0]
    q = rng.integers(33 + 2, 33 + 41, n * L).astype(np.uint8)
    return u.reshape(-1), q


def timed(call, reps):
    import torch
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts = call()
        e1.record()
        torch.cuda.synchronize()
        if r:  # (the first call grows the workspace and loads the code object)
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), [int(c) for c in counts]


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--skew", type=float, default=0.0)
    ap.add_argument("--max-list", type=int, default=LISTS[-1])
    ap.add_argument("--min-list", type=int, default=0)
    ap.add_argument("--note", default="")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/barcode_multi_bench.jsonl")
    a = ap.parse_args()
    ctx = Context(0)
    n = a.reads
    for n_wl in [x for x in LISTS if a.min_list <= x <= a.max_list]:
        rng = np.random.default_rng(n_wl)
        codes, half = near_list(rng, n_wl)
        wl = letters(codes)
        reads, quals = make_reads(rng, codes, half, n, a.skew)
        d_in, d_q = torch.from_numpy(reads).to("cuda:0"), torch.from_numpy(quals).to("cuda:0")
        d_match = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        d_exact = torch.empty(n_wl, dtype=torch.int32, device="cuda:0")
        plain, plain_min, plain_counts = timed(lambda: ctx.correct_barcodes_device(
            d_in.data_ptr(), n, L, wl, 1, d_match.data_ptr(), d_status.data_ptr()), a.reps)
        multi, multi_min, counts = timed(lambda: ctx.correct_barcodes_multi_device(
            d_in.data_ptr(), d_q.data_ptr(), n, L, wl, 975, 0, d_match.data_ptr(), d_status.data_ptr(), d_exact.data_ptr()),
            a.reps)
        assert plain_counts[:3] == counts[:3] and plain_counts[3] == counts[3] + counts[4]
        line = {"what": "umi_correct_barcodes_multi_device", "reads": n, "bases": L, "listed": n_wl, "skew": a.skew,
                "reps": a.reps, "ms_multi_median": round(multi, 3), "ms_multi_min": round(multi_min, 3),
                "ms_plain_median": round(plain, 3), "ms_plain_min": round(plain_min, 3), "ratio": round(multi / plain, 3),
                "counts": counts, "max_exact_reads": int(d_exact.max().item())}
        if a.note:
            line["note"] = a.note
        s = json.dumps(line)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "barcode_multi_bench.jsonl"), "a") as f:
                f.write(s + "\n")
        del d_in, d_q, d_match, d_status, d_exact
    ctx.close()


if __name__ == "__main__":
    main()
