"""The two calls of --velocity on resident data.  One JSON line per shape on stdout and, with --record, appended to
profiles/velocity_bench.jsonl.

  classes: umi_assign_genes_classes_device beside umi_assign_genes_introns_device, called in turn in one process on the
      same arrays -- introns_bench's annotation and its 10^7 reads, sorted and shuffled, under exon-first and under all.
      Host-clock medians of --reps calls after a warm-up, each full call followed by the same call on the first 64
      reads ("build": the index made and uploaded -- for the classes call with the prefix arrays and the genes' own
      exons -- and next to no lookups), as introns_bench times them.  The kernels' own times come from a kernel trace of
      this tool taken in a run of its own (--series classes --reps 16 --shapes <one shape> --modes exon_first; the
      dispatches of the full calls, no counters).
  matrix: umi_velocity_matrix_device beside umi_count_matrix_device on count_bench's two bucket shapes with three
      reads per entry (their entry drawn, so that the reads come in no order; a fifth of the entries hang on their
      bucket's first), device events around the calls; the result is compared with a host computation.  Then one
      molecule of 2^17 reads among the "few large" shape's.  Everything with option "velocity_skip" 1 (a lane loads its
      molecule's evidence first and leaves the atomic out where its bit is set) and 0, the default (an atomic per read
      with evidence); "velocity_over_count_matrix" is the ratio with the option on.
  --scale shrinks every shape (a rehearsal).

usage: python tools/velocity_bench.py [--series classes,matrix] [--reps 50] [--matrix-reps 10] [--reads 10000000]
                                      [--shapes sorted,shuffled] [--modes exon_first,all] [--scale 1.0] [--record]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import count_bench as cb  # noqa: E402
import genes_bench as gb  # noqa: E402
import introns_bench as ib  # noqa: E402
from umi_collapse_rs_amd import (Context, UMI_READ_CLASS_EXONIC, UMI_READ_CLASS_INTRONIC, UMI_READ_CLASS_JUNCTION,  # noqa: E402
                                 UMI_READ_CLASS_SPANNING, UMI_STRAND_FORWARD)


def classes_series(ctx, a, emit):
    import torch
    rng = np.random.default_rng(2026)
    n = int(a.reads * a.scale)
    ex, g_start, nested = ib.annotation(rng, gb.GENES, gb.LINES)
    base, intronic = ib.make_reads(rng, ex, g_start, n)
    orders = {"sorted": lambda: np.lexsort((base["pos"], base["ref"])), "shuffled": lambda: rng.permutation(n)}
    n_genes = int(ex["gene"].max()) + 1
    for name in a.shapes.split(","):
        reads = gb.ordered(base, orders[name]())
        ref, pos, rev, words, off = gb.packed(reads)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ref, pos, rev, words.view(np.int32), off.view(np.int64))]
        d_gene = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status, d_tier, d_cls = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(3))
        line = {"what": "umi_assign_genes_classes_device", "shape": name, "reads": n, "exon_lines": int(len(ex["gene"])),
                "genes": n_genes, "genes_nested": round(nested, 4), "reads_intronic": round(intronic, 4),
                "spliced": float((reads["n_words"] == 3).mean()), "reps": a.reps}
        for mode_name in a.modes.split(","):
            mode = ib.MODES[mode_name]

            def introns(m):
                return ctx.assign_genes_introns_device(ex, n_genes, UMI_STRAND_FORWARD, mode, *(t.data_ptr() for t in d), m,
                                                       d_gene.data_ptr(), d_status.data_ptr(), d_tier.data_ptr())

            def classes(m):
                return ctx.assign_genes_classes_device(ex, n_genes, UMI_STRAND_FORWARD, mode, *(t.data_ptr() for t in d), m,
                                                       d_gene.data_ptr(), d_status.data_ptr(), d_tier.data_ptr(), d_cls.data_ptr())
            res_i, counts_i = ib.paired(lambda: introns(n), lambda: introns(64), a.reps)
            theirs = (d_gene.cpu().numpy(), d_status.cpu().numpy(), d_tier.cpu().numpy())
            res_c, (counts_c, class_counts) = ib.paired(lambda: classes(n), lambda: classes(64), a.reps)
            ours = (d_gene.cpu().numpy(), d_status.cpu().numpy(), d_tier.cpu().numpy())
            res_i["counts"] = [int(c) for c in counts_i]
            res_c["counts"], res_c["class_counts"] = [int(c) for c in counts_c], [int(c) for c in class_counts]
            res_c["same_gene_status_tier_counts"] = bool(all((x == y).all() for x, y in zip(ours, theirs)) and
                                                         res_i["counts"] == res_c["counts"])
            res_c["call_over_introns_call"] = round(res_c["ms_call_median"] / res_i["ms_call_median"], 3)
            res_c["build_over_introns_build"] = round(res_c["ms_build_median"] / res_i["ms_build_median"], 3)
            line[mode_name + "_introns"], line[mode_name + "_classes"] = res_i, res_c
        emit(line)
        del d, d_gene, d_status, d_tier, d_cls


def host_layers(entry, cls, kept, root, off, row, col):
    """(rows, cols, spliced, unspliced, ambiguous) on the host: the evidence OR-ed per root, the kept entries by their
    evidence, count_bench's sort of the buckets and sums over equal neighbours (no bucket is empty)"""
    n = len(kept)
    ev = np.zeros(n, np.uint8)
    r = root[entry]
    np.bitwise_or.at(ev, r[cls == UMI_READ_CLASS_JUNCTION], 1)
    np.bitwise_or.at(ev, r[(cls == UMI_READ_CLASS_SPANNING) | (cls == UMI_READ_CLASS_INTRONIC)], 2)
    starts = off[:-1].astype(np.int64)
    k = kept != 0
    layers = [np.add.reduceat((k & (ev == 1)).astype(np.int64), starts), np.add.reduceat((k & (ev == 2)).astype(np.int64), starts),
              np.add.reduceat((k & (ev != 1) & (ev != 2)).astype(np.int64), starts)]
    order = np.lexsort((row, col))
    rr, cc = row[order], col[order]
    head = np.flatnonzero(np.concatenate([[True], (rr[1:] != rr[:-1]) | (cc[1:] != cc[:-1])]))
    return (rr[head], cc[head]) + tuple(np.add.reduceat(v[order], head).astype(np.uint32) for v in layers)


def matrix_series(ctx, a, emit):
    import torch
    shapes = [("many small", int(20_000_000 * a.scale), 1, 3), ("few large", int(100_000 * a.scale), 100, 100)]
    dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32) if x.dtype == np.uint32 else x).to("cuda:0")
    for name, nb, lo, hi in shapes:
        rng = np.random.default_rng(nb)
        _, freq, kept, off, row, col = cb.make_shape(rng, nb, lo, hi)
        n = int(off[-1])
        first = np.repeat(off[:-1].astype(np.int64), np.diff(off.astype(np.int64)))
        hang = rng.random(n) < 0.2
        root = np.where(hang, first, np.arange(n)).astype(np.uint32)
        kept = np.where(root == np.arange(n), kept, 0).astype(np.uint8)
        entry = rng.integers(0, n, 3 * n).astype(np.uint32)
        cls = rng.choice(np.array([UMI_READ_CLASS_EXONIC, UMI_READ_CLASS_JUNCTION, UMI_READ_CLASS_SPANNING, UMI_READ_CLASS_INTRONIC],
                                  np.uint8), 3 * n, p=[0.6, 0.2, 0.1, 0.1])
        variants = [("plain", entry, cls)]
        if name == "few large":  # one molecule of 2^17 reads among them
            deep = int(root[n // 2])
            variants.append(("deep molecule", np.concatenate([entry, np.full(1 << 17, deep, np.uint32)])[rng.permutation(3 * n + (1 << 17))],
                             None))
        d_freq, d_kept, d_root, d_row, d_col = dev(freq), dev(kept), dev(root), dev(row), dev(col)
        outs = [torch.zeros(nb, dtype=torch.int32, device="cuda:0") for _ in range(5)]
        o_reads = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
        c_med, c_min, _ = cb.timed(lambda: ctx.count_matrix_device(d_kept.data_ptr(), d_freq.data_ptr(), off, d_row.data_ptr(),
                                                                   d_col.data_ptr(), cb.N_GENES, cb.N_CELLS, outs[0].data_ptr(),
                                                                   outs[1].data_ptr(), outs[2].data_ptr(), o_reads.data_ptr()), a.matrix_reps)
        for what, v_entry, v_cls in variants:
            if v_cls is None:
                v_cls = rng.choice(np.array([1, 2, 3, 4], np.uint8), len(v_entry))
            exp = host_layers(v_entry, v_cls, kept, root, off, row, col)
            d_entry, d_cls = dev(v_entry), dev(v_cls)
            line = {"what": "umi_velocity_matrix_device", "shape": name, "variant": what, "buckets": nb, "entries": n,
                    "reads": int(len(v_entry)), "rows": cb.N_GENES, "cols": cb.N_CELLS, "nnz": int(len(exp[0])), "reps": a.matrix_reps,
                    "ms_count_matrix_median": round(c_med, 3), "ms_count_matrix_min": round(c_min, 3)}
            for skip in (1, 0):
                ctx.set_option("velocity_skip", skip)
                med, best, nnz = cb.timed(lambda: ctx.velocity_matrix_device(
                    d_entry.data_ptr(), d_cls.data_ptr(), len(v_entry), d_kept.data_ptr(), d_root.data_ptr(), off, d_row.data_ptr(),
                    d_col.data_ptr(), cb.N_GENES, cb.N_CELLS, *(t.data_ptr() for t in outs)), a.matrix_reps)
                got = [t.cpu().numpy().view(np.uint32)[:nnz] for t in outs]
                same = nnz == len(exp[0]) and all((g == e).all() for g, e in zip(got, exp))
                key = "skip" if skip else "no_skip"
                line.update({"ms_velocity_%s_median" % key: round(med, 3), "ms_velocity_%s_min" % key: round(best, 3),
                             "same_as_host_%s" % key: bool(same)})
            ctx.set_option("velocity_skip", 0)
            line["velocity_over_count_matrix"] = round(line["ms_velocity_skip_median"] / c_med, 3)
            line["skip_over_no_skip"] = round(line["ms_velocity_skip_median"] / line["ms_velocity_no_skip_median"], 3)
            emit(line)
            del d_entry, d_cls
        del d_freq, d_kept, d_root, d_row, d_col, outs, o_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--series", default="classes,matrix")
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--matrix-reps", type=int, default=10)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="sorted,shuffled")
    ap.add_argument("--modes", default="exon_first,all")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/velocity_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "velocity_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    if "classes" in a.series.split(","):
        classes_series(ctx, a, emit)
    if "matrix" in a.series.split(","):
        matrix_series(ctx, a, emit)
    ctx.close()


if __name__ == "__main__":
    main()
