"""umi_correct_barcodes_device on resident data, beside umi_correct_umis_device(1, 1) where that finishes in a few
seconds.  One JSON line per measurement on stdout and, with --record, appended to profiles/barcode_bench.jsonl.

  lists: 4,096, 65,536, 737,280 and 6,794,880 random distinct barcodes of 16 bases (the last two are the sizes
      of the 10x lists); reads: 10^6 and 10^7, 95 % exact, 3 % one substitution, 1 % one N, 1 % random.
  The call is timed with device events (it synchronises inside): median of --reps calls after a warm-up call.
  The index is built in every call, so the same call on the first 64 reads is timed beside it -- the list packed
  on the host, its upload, the table's fill, the two host looks, with next to no lookups: "build" -- and the
  difference is what the lookups cost: "lookup".

usage: python tools/barcode_bench.py [--reps 7] [--record] [--max-list N]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context  # noqa: E402

L = 16
LISTS = [4096, 65536, 737_280, 6_794_880]
READS = [1_000_000, 10_000_000]
ALL_PAIRS_UP_TO = 65536  # the all-against-all call is measured up to this many entries
ACGT = np.frombuffer(b"ACGT", np.uint8)


def random_list(rng, n_wl):
    codes = np.unique(rng.integers(0, 4 ** L, int(n_wl * 1.01) + 16, dtype=np.uint64))
    codes = rng.permutation(codes)[:n_wl]
    assert len(codes) == n_wl
    return ACGT[((codes[:, None] >> (2 * np.arange(L, dtype=np.uint64))[None, :]) & np.uint64(3)).astype(np.intp)]


def make_reads(rng, wl, n):
    u = wl[rng.integers(0, len(wl), n)].copy()
    r = rng.random(n)
    sub = np.flatnonzero(r < 0.03)
    at = rng.integers(0, L, len(sub))
    u[sub, at] = ACGT[(np.searchsorted(ACGT, u[sub, at]) + rng.integers(1, 4, len(sub))) % 4]
    with_n = np.flatnonzero((r >= 0.03) & (r < 0.04))
    u[with_n, rng.integers(0, L, len(with_n))] = ord("N")
    rnd = np.flatnonzero((r >= 0.04) & (r < 0.05))
    u[rnd] = ACGT[rng.integers(0, 4, (len(rnd), L))]
    return u.reshape(-1)


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
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/barcode_bench.jsonl")
    ap.add_argument("--max-list", type=int, default=LISTS[-1])
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "barcode_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    for n_wl in [x for x in LISTS if x <= a.max_list]:
        rng = np.random.default_rng(n_wl)
        wl = random_list(rng, n_wl)
        for n in READS:
            reads = make_reads(rng, wl, n)
            d_in = torch.from_numpy(reads).to("cuda:0")
            d_match = torch.empty(n, dtype=torch.int32, device="cuda:0")
            d_status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
            med, best, counts = timed(lambda: ctx.correct_barcodes_device(d_in.data_ptr(), n, L, wl, 1, d_match.data_ptr(),
                                                                          d_status.data_ptr()), a.reps)
            build, _, _ = timed(lambda: ctx.correct_barcodes_device(d_in.data_ptr(), 64, L, wl, 1, d_match.data_ptr(),
                                                                    d_status.data_ptr()), a.reps)
            line = {"what": "umi_correct_barcodes_device", "reads": n, "bases": L, "listed": n_wl,
                    "ms_call_median": round(med, 3), "ms_call_min": round(best, 3), "ms_build_median": round(build, 3),
                    "ms_lookup": round(med - build, 3), "reads_per_s_lookup": n / (max(med - build, 1e-6) * 1e-3),
                    "counts": counts}
            if n_wl <= ALL_PAIRS_UP_TO:
                ref_match = torch.empty(n, dtype=torch.int32, device="cuda:0")
                ref, _, _ = timed(lambda: ctx.correct_umis_device(d_in.data_ptr(), n, L, wl, 1, 1, 0, ref_match.data_ptr()),
                                  a.reps)
                line["ms_all_pairs_call_median"] = round(ref, 3)
                line["same_match"] = bool((ref_match == d_match).all().item())
            emit(line)
            del d_in, d_match, d_status
    ctx.close()


if __name__ == "__main__":
    main()
