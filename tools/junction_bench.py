"""umi_junction_matrix_device on resident data, beside umi_velocity_matrix_device on the same entries, reads and buckets in
the same process: the yardstick, a call of the same scatter-then-sort-and-reduce shape.  One JSON line per shape and
spliced share on stdout and, with --record, appended to profiles/junction_bench.jsonl.

  velocity_bench's two bucket shapes ("many small": 2 x 10^7 buckets of 1 to 3 entries; "few large": 10^5 buckets of 100),
  three reads per entry (their entry drawn, so that the reads come in no order; a fifth of the entries hang on their
  bucket's first).  An eighth of the reads, and then all of them, are spliced: xM yN zM over one junction drawn from a
  pool of 3 x 10^5 on 25 references; the others are one M word.  For the yardstick a spliced read is a JUNCTION read
  and the others EXONIC.  Device events around the calls, medians of --reps after a warm-up call.  The four counts of
  every call and, after the last call, the seven output arrays are compared with a numpy computation.
  --scale shrinks every shape (a rehearsal).

usage: python tools/junction_bench.py [--reps 10] [--scale 1.0] [--shares 0.125,1.0] [--shapes "many small,few large"] [--record]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_bench as cb  # noqa: E402
from umi_collapse_rs_amd import Context, UMI_READ_CLASS_EXONIC, UMI_READ_CLASS_JUNCTION  # noqa: E402

POOL, REFS = 300_000, 25


def make_pool(rng):
    """POOL distinct junctions in the order of (ref, start, end)"""
    ref = np.sort(rng.integers(0, REFS, POOL)).astype(np.int32)
    start = rng.integers(1000, 200_000_000, POOL).astype(np.int64)
    end = start + rng.integers(50, 100_000, POOL)
    order = np.lexsort((end, start, ref))
    ref, start, end = ref[order], start[order], end[order]
    keep = np.concatenate([[True], (ref[1:] != ref[:-1]) | (start[1:] != start[:-1]) | (end[1:] != end[:-1])])
    return ref[keep], start[keep], end[keep]


def make_reads(rng, n_reads, share, pool):
    """(read_ref, read_pos, cigar, cigar_off, junction: the pool's index of a spliced read's junction, -1 for the others)"""
    p_ref, p_start, p_end = pool
    spliced = rng.random(n_reads) < share
    jn = np.where(spliced, rng.integers(0, len(p_ref), n_reads), -1)
    a, b = rng.integers(1, 60, n_reads), rng.integers(1, 60, n_reads)
    j = np.maximum(jn, 0)
    ref = np.where(spliced, p_ref[j], rng.integers(0, REFS, n_reads)).astype(np.int32)
    pos = np.where(spliced, p_start[j] - a, rng.integers(0, 200_000_000, n_reads)).astype(np.int32)
    off = np.concatenate([[0], np.cumsum(1 + 2 * spliced.astype(np.int64))]).astype(np.uint64)
    words = np.zeros(int(off[-1]), np.uint32)
    at = off[:-1].astype(np.int64)
    words[at] = (a << 4).astype(np.uint32)  # xM (the whole read where it is not spliced)
    s = at[spliced]
    words[s + 1] = (((p_end[j] - p_start[j])[spliced] << 4) | 3).astype(np.uint32)
    words[s + 2] = (b[spliced] << 4).astype(np.uint32)
    return ref, pos, words, off, jn


def host_junctions(jn, entry, kept, root, off, col, pool):
    """the table, the triplets and the counts on the host: np.unique over packed keys"""
    n = len(kept)
    r = root[entry].astype(np.int64)
    counted = (jn >= 0) & (kept[r] != 0)
    j, r = jn[counted], r[counted]
    c = np.repeat(col.astype(np.int64), np.diff(off.astype(np.int64)))[r]
    used, rank = np.unique(j, return_inverse=True)  # (the pool is in table order)
    n_jn = max(1, len(used))
    pair = c * n_jn + rank
    pairs, reads = np.unique(pair, return_counts=True)
    mol_pair = np.unique(pair * n + r) // n
    _, molecules = np.unique(mol_pair, return_counts=True)
    table = tuple(np.asarray(x[used], np.int32) for x in pool)
    trip = ((pairs % n_jn).astype(np.uint32), (pairs // n_jn).astype(np.uint32), molecules.astype(np.uint32), reads.astype(np.uint64))
    return table, trip, [int(counted.sum()), int(counted.sum()), len(used), len(pairs)]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--shares", default="0.125,1.0")
    ap.add_argument("--shapes", default="many small,few large")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/junction_bench.jsonl")
    a = ap.parse_args()
    import torch

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "junction_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
    shapes = [("many small", int(20_000_000 * a.scale), 1, 3), ("few large", int(100_000 * a.scale), 100, 100)]
    for name, nb, lo, hi in shapes:
        if name not in a.shapes.split(","):
            continue
        rng = np.random.default_rng(nb)
        _, _, kept, off, row, col = cb.make_shape(rng, nb, lo, hi)
        n = int(off[-1])
        first = np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
        hang = rng.random(n) < 0.2
        root = np.where(hang, first, np.arange(n)).astype(np.uint32)
        kept = np.where(root == np.arange(n), kept, 0).astype(np.uint8)
        entry = rng.integers(0, n, 3 * n).astype(np.uint32)
        pool = make_pool(rng)
        d_kept, d_root, d_row, d_col, d_entry = dev(kept), dev(root), dev(row), dev(col), dev(entry)
        v_outs = [torch.zeros(nb, dtype=torch.int32, device="cuda:0") for _ in range(5)]
        for share in (float(x) for x in a.shares.split(",")):
            ref, pos, words, woff, jn = make_reads(rng, 3 * n, share, pool)
            exp_table, exp_trip, exp_counts = host_junctions(jn, entry, kept, root, off, col, pool)
            cap = exp_counts[1]
            cls = np.where(jn >= 0, UMI_READ_CLASS_JUNCTION, UMI_READ_CLASS_EXONIC).astype(np.uint8)
            d_ref, d_pos, d_words, d_woff, d_cls = dev(ref), dev(pos), dev(words), dev(woff), dev(cls)
            outs = [torch.zeros(max(1, cap), dtype=torch.int32, device="cuda:0") for _ in range(6)]
            o_reads = torch.zeros(max(1, cap), dtype=torch.int64, device="cuda:0")
            same_counts = []

            def junctions():
                counts = ctx.junction_matrix_device(d_ref.data_ptr(), d_pos.data_ptr(), d_words.data_ptr(), d_woff.data_ptr(),
                                                    d_entry.data_ptr(), 3 * n, d_kept.data_ptr(), d_root.data_ptr(), off, d_col.data_ptr(),
                                                    cb.N_CELLS, cap, *(t.data_ptr() for t in outs), o_reads.data_ptr())
                same_counts.append([int(x) for x in counts] == exp_counts)
                return counts
            med, best, counts = cb.timed(junctions, a.reps)
            got_table = [t.cpu().numpy()[:exp_counts[2]] for t in outs[:3]]
            got_trip = [t.cpu().numpy().view(np.uint32)[:exp_counts[3]] for t in outs[3:]] + [o_reads.cpu().numpy().view(np.uint64)[:exp_counts[3]]]
            same = all(same_counts) and all((g == e).all() for g, e in zip(got_table + got_trip, exp_table + exp_trip))
            v_med, v_best, v_nnz = cb.timed(lambda: ctx.velocity_matrix_device(
                d_entry.data_ptr(), d_cls.data_ptr(), 3 * n, d_kept.data_ptr(), d_root.data_ptr(), off, d_row.data_ptr(), d_col.data_ptr(),
                cb.N_GENES, cb.N_CELLS, *(t.data_ptr() for t in v_outs)), a.reps)
            emit({"what": "umi_junction_matrix_device", "shape": name, "spliced_share": share, "buckets": nb, "entries": n, "reads": 3 * n,
                  "cigar_words": int(len(words)), "pool": int(len(pool[0])), "cols": cb.N_CELLS, "spliced_reads_counted": exp_counts[0],
                  "occurrences": exp_counts[1], "junctions": exp_counts[2], "nnz": exp_counts[3], "reps": a.reps,
                  "ms_junction_matrix_median": round(med, 3), "ms_junction_matrix_min": round(best, 3),
                  "ms_velocity_matrix_median": round(v_med, 3), "ms_velocity_matrix_min": round(v_best, 3), "velocity_nnz": int(v_nnz),
                  "junction_over_velocity": round(med / v_med, 3), "same_as_host_every_call_counts_last_call_arrays": bool(same)})
            del d_ref, d_pos, d_words, d_woff, d_cls, outs, o_reads
        del d_kept, d_root, d_row, d_col, d_entry, v_outs
    ctx.close()


if __name__ == "__main__":
    main()
