"""umi_dedup_stats_device on resident data, beside umi_dedup_batch_device with root[] on the same arrays.  One JSON
line per shape on stdout and, with --record, appended to profiles/stats_bench.jsonl.

  shapes: "one position" -- 10^6 entries in one bucket (counted in pieces by the whole grid); "positions" -- 10^7
      entries in 10^5 buckets of 100 (a wave each); "many small" -- 2 x 10^7 buckets of 1 to 3 entries, what a
      single-cell sample gives (a lane each).  UMIs of 12 random bases, freq falling inside a bucket.
  The arrays stay on the device; kept[] and root[] are what the dedup call wrote.  Every shape is warmed up (a call
  of each kind, which grows the workspaces and loads the code objects); then --reps rounds of three calls in turn --
  the dedup call with root[], the stats call with the per-UMI table, the stats call without -- each between device
  events (all three synchronise inside); the medians and minima are reported.  The stats call's time holds its walk
  of the bucket table on the host and the table's upload, as the dedup call's does.  On "many small" the family-size
  part alone is also timed on the host (np.bincount and np.add.at on the downloaded arrays, once, by the host's
  clock), and compared with the device's two histograms.
  --scale shrinks the shapes (a rehearsal).

usage: python tools/stats_bench.py [--reps 50] [--record] [--scale 1.0]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

UMI_LEN, HIST_BINS = 12, 65536
CODES = np.array([0, 5, 6, 3], np.uint64)  # A, T, C, G in the batched call's 3 bits per base


def make_shape(rng, n_buckets, lo, hi):
    sizes = rng.integers(lo, hi + 1, n_buckets)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    keys = np.zeros(n, np.uint64)
    for b in range(UMI_LEN):
        keys |= CODES[rng.integers(0, 4, n, dtype=np.uint8)] << np.uint64(3 * b)
    at = np.arange(n, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), sizes)
    freq = (np.repeat(sizes, sizes) - at).astype(np.int32)  # (falling inside a bucket, as the call's contract asks)
    return keys, freq, off


def host_family_sizes(freq, kept, root):
    pre = np.bincount(np.minimum(freq, HIST_BINS - 1), minlength=HIST_BINS).astype(np.uint64)
    total = np.zeros(len(freq), np.int64)
    np.add.at(total, root.astype(np.int64), freq.astype(np.int64))
    post = np.bincount(np.minimum(total[kept != 0], HIST_BINS - 1), minlength=HIST_BINS).astype(np.uint64)
    return pre, post


def timed(call):
    import torch
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    out = call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1), out


def main():
    import torch
    from umi_collapse_rs_amd import Context
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/stats_bench.jsonl")
    ap.add_argument("--scale", type=float, default=1.0)
    a = ap.parse_args()
    shapes = [("one position", 1, int(1_000_000 * a.scale)), ("positions", int(100_000 * a.scale), 100),
              ("many small", int(20_000_000 * a.scale), None)]
    ctx = Context(0)
    for name, nb, size in shapes:
        rng = np.random.default_rng(nb + 7)
        keys, freq, off = make_shape(rng, nb, size or 1, size or 3)
        n = len(freq)
        dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x).to("cuda:0")
        d_keys, d_freq = dev(keys), dev(freq)
        d_kept = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
        d_root = torch.zeros(n, dtype=torch.int32, device="cuda:0")
        pre, post = (torch.zeros(HIST_BINS, dtype=torch.int64, device="cuda:0") for _ in range(2))
        dist = torch.zeros(4 * (UMI_LEN + 2), dtype=torch.int64, device="cuda:0")
        t32 = [torch.zeros(n, dtype=torch.int32, device="cuda:0") for _ in range(3)]
        t64 = [torch.zeros(n, dtype=torch.int64, device="cuda:0") for _ in range(2)]
        dedup = lambda: ctx.dedup_batch_device(d_keys.data_ptr(), 0, d_freq.data_ptr(), off, UMI_LEN, d_kept.data_ptr(),
                                               d_root.data_ptr(), k=1)
        stats = lambda table: ctx.dedup_stats_device(
            d_keys.data_ptr(), d_freq.data_ptr(), d_kept.data_ptr(), d_root.data_ptr(), off, UMI_LEN, pre.data_ptr(),
            post.data_ptr(), dist.data_ptr(), seed=1, hist_bins=HIST_BINS,
            **(dict(d_umi_entry=t32[0].data_ptr(), d_times_pre=t32[1].data_ptr(), d_reads_pre=t64[0].data_ptr(),
                    d_times_post=t32[2].data_ptr(), d_reads_post=t64[1].data_ptr()) if table else {}))
        dedup(), stats(True), stats(False)  # the warm-up
        ms = {"dedup": [], "table": [], "plain": []}
        rows = 0
        for _ in range(a.reps):
            ms["dedup"].append(timed(dedup)[0])
            t, rows = timed(lambda: stats(True))
            ms["table"].append(t)
            ms["plain"].append(timed(lambda: stats(False))[0])
        d = dist.cpu().numpy().reshape(4, UMI_LEN + 2)
        kept = d_kept.cpu().numpy()
        line = {"what": "umi_dedup_stats_device", "shape": name, "buckets": nb, "entries": n, "umi_len": UMI_LEN, "reps": a.reps,
                "kept": int(np.count_nonzero(kept)), "distinct_umis": int(rows),
                "ms_stats_with_table_median": round(float(np.median(ms["table"])), 3),
                "ms_stats_with_table_min": round(float(np.min(ms["table"])), 3),
                "ms_stats_median": round(float(np.median(ms["plain"])), 3), "ms_stats_min": round(float(np.min(ms["plain"])), 3),
                "ms_dedup_batch_device_root_median": round(float(np.median(ms["dedup"])), 3),
                "ms_dedup_batch_device_root_min": round(float(np.min(ms["dedup"])), 3),
                "dist_rows_sum_to_buckets": bool((d.sum(axis=1) == nb).all()),
                "entries_per_s_stats": n / (float(np.median(ms["plain"])) * 1e-3)}
        if name == "many small":
            root = d_root.cpu().numpy().view(np.uint32)
            t0 = time.perf_counter()
            h_pre, h_post = host_family_sizes(freq, kept, root)
            line["ms_host_numpy_family_sizes"] = round((time.perf_counter() - t0) * 1e3, 1)
            line["family_sizes_same_as_host"] = bool((pre.cpu().numpy().view(np.uint64) == h_pre).all() and
                                                     (post.cpu().numpy().view(np.uint64) == h_post).all())
        s = json.dumps(line)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "stats_bench.jsonl"), "a") as f:
                f.write(s + "\n")
        del d_keys, d_freq, d_kept, d_root, pre, post, dist, t32, t64
    ctx.close()


if __name__ == "__main__":
    main()
