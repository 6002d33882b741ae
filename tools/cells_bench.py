"""umi_call_cells_device on resident data, beside umi_count_matrix_device on arrays of the same size and the rule in
numpy on the host.  One JSON line per shape on stdout and, with --record, appended to profiles/cells_bench.jsonl.

  shapes: "droplets" -- 2 x 10^7 triplets over 7 x 10^5 columns of a 3 x 10^4-row matrix, 5 x 10^3 of them deep (3,000
      triplets each, the cells) and the others shallow (about 7 each, the ambient droplets), what the raw matrix of a
      10x run looks like; "one column" -- 10^6 triplets in a single column, the matrix without --per-cell.
  The call synchronises inside; it is timed by the host's clock around it, so its host work counts: median and
  minimum of --reps calls after a warm-up call that grows the workspace and loads the code objects.  The rule is
  cr2.2 with its defaults.  umi_count_matrix_device is timed the same way on as many buckets of one entry as there
  are triplets, with the triplets' rows and columns.  The host baseline (np.add.reduceat, np.sort, boolean masks) is
  timed once; its result is what the device's is compared with (exact equality of every output array and count).
  --scale shrinks both shapes (a rehearsal); --host-only stops before the first device call.

usage: python tools/cells_bench.py [--reps 50] [--record] [--scale 1.0] [--host-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_ROWS = 30_000
RULE = dict(rule=0, expect_cells=3000, percentile_permille=990, max_min_ratio=10, min_molecules=1)


def make_shape(rng, sizes, n_rows):
    """triplets sorted by column, then row: column c holds sizes[c] of them at distinct rows"""
    sizes = np.asarray(sizes, np.int64)
    nnz = int(sizes.sum())
    col = np.repeat(np.arange(len(sizes), dtype=np.uint32), sizes)
    start = np.concatenate([[0], np.cumsum(sizes)])[:-1]
    at = np.arange(nnz, dtype=np.int64) - np.repeat(start, sizes)
    per = np.repeat(sizes, sizes)
    lo, hi = at * n_rows // per, (at + 1) * n_rows // per  # (one stratum each, sizes <= n_rows: rising, distinct)
    row = lo + (rng.random(nnz) * (hi - lo)).astype(np.int64)
    mol = rng.integers(0, 4, nnz).astype(np.uint32)
    reads = mol.astype(np.uint64) + rng.integers(1, 6, nnz).astype(np.uint64)
    return row.astype(np.uint32), col, mol, reads


def host_call(row, col, mol, reads, n_cols, rule, expect_cells, percentile_permille, max_min_ratio, min_molecules):
    head = np.flatnonzero(np.concatenate([[True], col[1:] != col[:-1]]))
    T, R, G = np.zeros(n_cols, np.uint64), np.zeros(n_cols, np.uint64), np.zeros(n_cols, np.uint32)
    T[col[head]] = np.add.reduceat(mol.astype(np.uint64), head)
    R[col[head]] = np.add.reduceat(reads, head)
    G[col[head]] = np.add.reduceat((mol != 0).astype(np.uint32), head)
    S = np.sort(T[T >= 1])[::-1]
    n = len(S)
    m = int(S[min(n - 1, expect_cells * (1000 - percentile_permille) // 1000)]) if n else 0
    t = max(1, (2 * m + max_min_ratio) // (2 * max_min_ratio)) if n else 0
    called = (T >= 1) & (T >= np.uint64(t))
    new_col = np.full(n_cols, 0xFFFFFFFF, np.uint32)
    k = int(called.sum())
    new_col[called] = np.arange(k, dtype=np.uint32)
    keep = called[col] & (mol != 0)
    med = lambda v: int(np.sort(v)[(len(v) - 1) // 2]) if len(v) else 0
    counts = [n, k, t, m, int(T[called].sum()), int(R[called].sum()), int(T.sum()), int(R.sum()), med(T[called]), med(G[called])]
    return (T, R, G, called.astype(np.uint8), new_col), (row[keep], new_col[col[keep]], mol[keep], reads[keep]), counts


def timed(call, reps):
    import torch
    ms, out = [], None
    for r in range(reps + 1):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = call()
        torch.cuda.synchronize()
        if r:
            ms.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ms)), float(np.min(ms)), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/cells_bench.jsonl")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    rng = np.random.default_rng(5)
    deep, cols = int(5_000 * a.scale), int(700_000 * a.scale)
    shallow = rng.poisson(5_000_000 / 695_000 - 1, cols - deep) + 1
    shallow[-1] += max(0, int(20_000_000 * a.scale) - deep * 3_000 - int(shallow.sum()))
    droplets = rng.permutation(np.concatenate([np.full(deep, 3_000), shallow]))
    shapes = [("droplets", droplets, N_ROWS), ("one column", np.array([int(1_000_000 * a.scale)]), int(1_000_000 * a.scale))]
    ctx = None
    for name, sizes, n_rows in shapes:
        n_cols = len(sizes)
        row, col, mol, reads = make_shape(rng, sizes, n_rows)
        nnz = len(row)
        t0 = time.perf_counter()
        exp = host_call(row, col, mol, reads, n_cols, **RULE)
        host_ms = (time.perf_counter() - t0) * 1e3
        line = {"what": "umi_call_cells_device", "shape": name, "triplets": nnz, "rows": n_rows, "cols": n_cols, "rule": "cr2.2",
                "candidates": exp[2][0], "called": exp[2][1], "threshold": exp[2][2], "nnz_out": int(len(exp[1][0])),
                "ms_host_numpy": round(host_ms, 1)}
        if not a.host_only:
            import torch
            from umi_collapse_rs_amd import Context
            ctx = ctx or Context(0)
            dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)
                                             if x.dtype == np.uint32 else x).to("cuda:0")
            d_row, d_col, d_mol, d_reads = dev(row), dev(col), dev(mol), dev(reads)
            z = lambda n, dt: torch.zeros(max(n, 1), dtype=dt, device="cuda:0")
            per = [z(n_cols, torch.int64), z(n_cols, torch.int64), z(n_cols, torch.int32), z(n_cols, torch.uint8), z(n_cols, torch.int32)]
            outs = [z(nnz, torch.int32), z(nnz, torch.int32), z(nnz, torch.int32), z(nnz, torch.int64)]
            med, best, (nnz_out, counts) = timed(lambda: ctx.call_cells_device(
                d_row.data_ptr(), d_col.data_ptr(), d_mol.data_ptr(), d_reads.data_ptr(), nnz, n_rows, n_cols,
                *(t.data_ptr() for t in per), *(t.data_ptr() for t in outs), **RULE), a.reps)
            views = (np.uint64, np.uint64, np.uint32, np.uint8, np.uint32)
            same = nnz_out == len(exp[1][0]) and list(counts.values()) == exp[2]
            same = same and all((t.cpu().numpy().view(v)[:n_cols] == e).all() for t, v, e in zip(per, views, exp[0]))
            same = same and all((t.cpu().numpy().view(v)[:nnz_out] == e).all()
                                for t, v, e in zip(outs, (np.uint32, np.uint32, np.uint32, np.uint64), exp[1]))
            # umi_count_matrix_device on as many buckets of one entry, with the triplets' ids
            off = np.arange(nnz + 1, dtype=np.uint64)
            d_kept, d_freq = z(nnz, torch.uint8) + 1, z(nnz, torch.int32) + 1
            c_med, c_best, _ = timed(lambda: ctx.count_matrix_device(d_kept.data_ptr(), d_freq.data_ptr(), off, d_row.data_ptr(),
                                                                     d_col.data_ptr(), n_rows, n_cols, outs[0].data_ptr(),
                                                                     outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr()),
                                     max(1, a.reps // 5))
            line.update({"ms_call_cells_median": round(med, 3), "ms_call_cells_min": round(best, 3), "same_as_host": bool(same),
                         "ms_count_matrix_device_median": round(c_med, 3), "ms_count_matrix_device_min": round(c_best, 3),
                         "triplets_per_s": nnz / (med * 1e-3), "reps": a.reps})
            del d_row, d_col, d_mol, d_reads, per, outs, d_kept, d_freq
        s = json.dumps(line)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "cells_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    if ctx:
        ctx.close()


if __name__ == "__main__":
    main()
