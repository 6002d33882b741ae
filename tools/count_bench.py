"""umi_count_matrix_device on resident data, beside umi_dedup_batch_device on the same arrays and a host baseline
(np.lexsort + np.add.reduceat on the same input).  One JSON line per shape on stdout and, with --record, appended
to profiles/count_bench.jsonl.

  shapes: "many small" -- 2 x 10^7 buckets of 1 to 3 entries over 10^4 cells x 3 x 10^4 genes, what a single-cell
      sample gives (buckets may share a pair); "few large" -- 10^5 buckets of 100 entries over the same matrix.
  Both device calls synchronise inside and are timed with device events around them: median and minimum of --reps
  calls after a warm-up call that grows the workspace and loads the code objects.  The count's time holds its walk
  of the bucket table on the host and the table's upload, as the dedup call's does.  The host baseline is timed by
  the host's clock, once; its result is what the device's is compared with (exact equality of all four arrays).
  --scale shrinks both shapes (a rehearsal); --host-only stops before the first device call.

usage: python tools/count_bench.py [--reps 5] [--record] [--scale 1.0] [--host-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CELLS, N_GENES, UMI_LEN = 10_000, 30_000, 12
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
    kept = (rng.random(n) < 0.8).astype(np.uint8)
    row = rng.integers(0, N_GENES, n_buckets).astype(np.uint32)
    col = rng.integers(0, N_CELLS, n_buckets).astype(np.uint32)
    return keys, freq, kept, off, row, col


def host_count(kept, freq, off, row, col):
    """(rows, cols, molecules, reads) by a sort of the buckets and sums over equal neighbours (no bucket is empty)"""
    starts = off[:-1].astype(np.int64)
    mol = np.add.reduceat((kept != 0).astype(np.int64), starts)
    reads = np.add.reduceat(freq.astype(np.int64), starts)
    order = np.lexsort((row, col))
    r, c = row[order], col[order]
    head = np.flatnonzero(np.concatenate([[True], (r[1:] != r[:-1]) | (c[1:] != c[:-1])]))
    return r[head], c[head], np.add.reduceat(mol[order], head).astype(np.uint32), np.add.reduceat(reads[order], head).astype(np.uint64)


def timed(call, reps):
    import torch
    ms, out = [], None
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        out = call()
        e1.record()
        torch.cuda.synchronize()
        if r:
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/count_bench.jsonl")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    shapes = [("many small", int(20_000_000 * a.scale), 1, 3), ("few large", int(100_000 * a.scale), 100, 100)]
    ctx = None
    for name, nb, lo, hi in shapes:
        rng = np.random.default_rng(nb)
        keys, freq, kept, off, row, col = make_shape(rng, nb, lo, hi)
        t0 = time.perf_counter()
        exp = host_count(kept, freq, off, row, col)
        host_ms = (time.perf_counter() - t0) * 1e3
        line = {"what": "umi_count_matrix_device", "shape": name, "buckets": nb, "entries": int(off[-1]), "rows": N_GENES,
                "cols": N_CELLS, "nnz": int(len(exp[0])), "ms_host_lexsort_reduceat": round(host_ms, 1)}
        if not a.host_only:
            import torch
            from umi_collapse_rs_amd import Context
            ctx = ctx or Context(0)
            dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)
                                             if x.dtype == np.uint32 else x).to("cuda:0")
            d_keys, d_freq, d_kept, d_row, d_col = dev(keys), dev(freq), dev(kept), dev(row), dev(col)
            d_dedup_kept = torch.zeros(len(keys), dtype=torch.uint8, device="cuda:0")
            outs = [torch.zeros(nb, dtype=torch.int32, device="cuda:0") for _ in range(3)]
            o_reads = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
            med, best, nnz = timed(lambda: ctx.count_matrix_device(d_kept.data_ptr(), d_freq.data_ptr(), off, d_row.data_ptr(),
                                                                   d_col.data_ptr(), N_GENES, N_CELLS, outs[0].data_ptr(),
                                                                   outs[1].data_ptr(), outs[2].data_ptr(), o_reads.data_ptr()),
                                   a.reps)
            got = [t.cpu().numpy().view(np.uint32)[:nnz] for t in outs] + [o_reads.cpu().numpy().view(np.uint64)[:nnz]]
            same = nnz == len(exp[0]) and all((g == e).all() for g, e in zip(got, exp))
            d_med, d_best, _ = timed(lambda: ctx.dedup_batch_device(d_keys.data_ptr(), 0, d_freq.data_ptr(), off, UMI_LEN,
                                                                    d_dedup_kept.data_ptr(), k=1), max(1, a.reps // 2))
            line.update({"ms_count_median": round(med, 3), "ms_count_min": round(best, 3), "same_as_host": bool(same),
                         "ms_dedup_batch_device_median": round(d_med, 3), "ms_dedup_batch_device_min": round(d_best, 3),
                         "buckets_per_s_count": nb / (med * 1e-3)})
            del d_keys, d_freq, d_kept, d_row, d_col, d_dedup_kept, outs, o_reads
        s = json.dumps(line)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "count_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    if ctx:
        ctx.close()


if __name__ == "__main__":
    main()
