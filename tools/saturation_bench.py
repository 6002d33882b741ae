"""umi_saturation_curve_device on resident data, beside umi_velocity_matrix_device on the same arrays in the same process
(the same scatter and reduce shape) and a numpy computation of the same curve on the host.  One JSON line per shape on
stdout and, with --record, appended to profiles/saturation_bench.jsonl.

  shapes: velocity_bench's two -- "many small", 2 x 10^7 buckets of 1 to 3 entries, and "few large", 10^5 buckets of 100
      entries, over 10^4 cells x 3 x 10^4 genes, three reads per entry with their entry drawn (the reads come in no
      order), a fifth of the entries hanging on their bucket's first -- and "deep molecule": one molecule of 2^17 reads
      among the few large buckets'.  L = 10, seed 0, no cell mask (every column with a molecule is selected).
  Both device calls synchronise inside and are timed with device events around them: median and minimum of --reps
      calls after a warm-up call that grows the workspace and loads the code objects.  The saturation call with option
      "saturation_skip" 0 and 1, in turn; its curve is compared with the host's, value for value.  The host computation
      is timed by the host's clock, once.  "saturation_over_velocity" is the ratio of the medians with both skip options
      at their defaults (off).
  Not measured here: the program end to end, and the host-buffer form (its copies of the arrays).
  --scale shrinks every shape (a rehearsal); --host-only stops before the first device call.

usage: python tools/saturation_bench.py [--reps 10] [--record] [--scale 1.0] [--host-only]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_bench as cb  # noqa: E402

LEVELS, SEED = 10, 0


def levels(seed, n_reads, n_levels):
    """the level of reads 0 .. n_reads-1 (include/umihip.h has the hash), in numpy's wrapping 64-bit arithmetic"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n_reads, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (((z >> np.uint64(32)) * np.uint64(n_levels)) >> np.uint64(32)).astype(np.int64)


def host_curve(entry, kept, root, off, row, col, n_cols, n_levels, seed):
    """the curve on the host: a sort of (molecule, level) for the molecules' levels, minima per bucket, count_bench's sort
    of the buckets and minima over equal neighbours, per-column tables and their sorted columns (no bucket is empty, every
    read is staged, no cell mask)"""
    L, n = n_levels, len(kept)
    lev = levels(seed, len(entry), L)
    r = root[entry].astype(np.int64)
    counted = kept[r] != 0
    reads = np.bincount(lev[counted], minlength=L)
    first = np.unique(r[counted] * 32 + lev[counted])  # sorted: a molecule's smallest level comes first
    mol, at = np.unique(first >> 5, return_index=True)
    mol_level = np.full(n, L, np.int64)
    mol_level[mol] = first[at] & 31
    molecules = np.bincount(mol_level[mol], minlength=L)
    starts = off[:-1].astype(np.int64)
    blev = np.minimum.reduceat(mol_level, starts)
    order = np.lexsort((row, col))
    rr, cc = row[order], col[order]
    head = np.flatnonzero(np.concatenate([[True], (rr[1:] != rr[:-1]) | (cc[1:] != cc[:-1])]))
    plev, pcol = np.minimum.reduceat(blev[order], head), cc[head].astype(np.int64)
    pairs = np.bincount(plev[plev < L], minlength=L)
    mcol = np.repeat(col.astype(np.int64), np.diff(off.astype(np.int64)))[mol]
    col_m = np.bincount(mcol * L + mol_level[mol], minlength=n_cols * L).reshape(n_cols, L)
    col_p = np.bincount(pcol[plev < L] * L + plev[plev < L], minlength=n_cols * L).reshape(n_cols, L)
    sel = col_m.sum(axis=1) > 0
    cum_m, cum_p = np.cumsum(col_m[sel], axis=1), np.cumsum(col_p[sel], axis=1)
    n_sel = int(sel.sum())
    curve = np.zeros((L, 8), np.uint64)
    curve[:, 0], curve[:, 1], curve[:, 2] = np.cumsum(reads), np.cumsum(molecules), np.cumsum(pairs)
    curve[:, 3] = (cum_m > 0).sum(axis=0)
    curve[:, 4], curve[:, 5] = cum_m.sum(axis=0), cum_p.sum(axis=0)
    if n_sel:
        curve[:, 6], curve[:, 7] = np.sort(cum_m, axis=0)[(n_sel - 1) // 2], np.sort(cum_p, axis=0)[(n_sel - 1) // 2]
    return curve


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/saturation_bench.jsonl")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--host-only", action="store_true")
    a = ap.parse_args()
    shapes = [("many small", int(20_000_000 * a.scale), 1, 3), ("few large", int(100_000 * a.scale), 100, 100)]
    ctx = None
    for name, nb, lo, hi in shapes:
        rng = np.random.default_rng(nb)
        _, _, kept, off, row, col = cb.make_shape(rng, nb, lo, hi)
        n = int(off[-1])
        first = np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
        root = np.where(rng.random(n) < 0.2, first, np.arange(n)).astype(np.uint32)
        kept = np.where(root == np.arange(n), kept, 0).astype(np.uint8)
        entry = rng.integers(0, n, 3 * n).astype(np.uint32)
        variants = [("plain", entry)]
        if name == "few large":  # one molecule of 2^17 reads among them
            deep = int(root[n // 2])
            kept[deep] = 1
            variants.append(("deep molecule", np.concatenate([entry, np.full(1 << 17, deep, np.uint32)])[rng.permutation(3 * n + (1 << 17))]))
        for what, v_entry in variants:
            t0 = time.perf_counter()
            exp = host_curve(v_entry, kept, root, off, row, col, cb.N_CELLS, LEVELS, SEED)
            host_ms = (time.perf_counter() - t0) * 1e3
            line = {"what": "umi_saturation_curve_device", "shape": name, "variant": what, "buckets": nb, "entries": n,
                    "reads": int(len(v_entry)), "rows": cb.N_GENES, "cols": cb.N_CELLS, "levels": LEVELS, "seed": SEED, "reps": a.reps,
                    "curve_last": [int(x) for x in exp[-1]], "ms_host_numpy": round(host_ms, 1)}
            if not a.host_only:
                import torch
                from umi_collapse_rs_amd import Context
                ctx = ctx or Context(0)
                dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
                cls = rng.choice(np.array([1, 2, 3, 4], np.uint8), len(v_entry), p=[0.6, 0.2, 0.1, 0.1])
                d_entry, d_cls, d_kept, d_root, d_row, d_col = dev(v_entry), dev(cls), dev(kept), dev(root), dev(row), dev(col)
                outs = [torch.zeros(nb, dtype=torch.int32, device="cuda:0") for _ in range(5)]
                ctx.set_option("velocity_skip", 0)
                v_med, v_min, _ = cb.timed(lambda: ctx.velocity_matrix_device(
                    d_entry.data_ptr(), d_cls.data_ptr(), len(v_entry), d_kept.data_ptr(), d_root.data_ptr(), off, d_row.data_ptr(),
                    d_col.data_ptr(), cb.N_GENES, cb.N_CELLS, *(t.data_ptr() for t in outs)), a.reps)
                line.update({"ms_velocity_matrix_median": round(v_med, 3), "ms_velocity_matrix_min": round(v_min, 3)})
                for skip in (0, 1, 0, 1):  # (in turn, twice: the later pair is what is kept)
                    ctx.set_option("saturation_skip", skip)
                    med, best, got = cb.timed(lambda: ctx.saturation_curve_device(
                        d_entry.data_ptr(), len(v_entry), d_kept.data_ptr(), d_root.data_ptr(), off, d_row.data_ptr(), d_col.data_ptr(),
                        cb.N_GENES, cb.N_CELLS, LEVELS, SEED), a.reps)
                    key = "skip" if skip else "no_skip"
                    line.update({"ms_saturation_%s_median" % key: round(med, 3), "ms_saturation_%s_min" % key: round(best, 3),
                                 "same_as_host_%s" % key: bool((got == exp).all())})
                ctx.set_option("saturation_skip", 0)
                line["saturation_over_velocity"] = round(line["ms_saturation_no_skip_median"] / v_med, 3)
                line["skip_over_no_skip"] = round(line["ms_saturation_skip_median"] / line["ms_saturation_no_skip_median"], 3)
                line["host_over_device"] = round(host_ms / line["ms_saturation_no_skip_median"], 1)
                del d_entry, d_cls, d_kept, d_root, d_row, d_col, outs
            s = json.dumps(line)
            print(s, flush=True)
            if a.record:
                with open(os.path.join(ROOT, "profiles", "saturation_bench.jsonl"), "a") as f:
                    f.write(s + "\n")
    if ctx:
        ctx.close()


if __name__ == "__main__":
    main()
