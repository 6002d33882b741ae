"""umi_assign_genes_introns_device on resident data, beside umi_assign_genes_device on the same arrays: the call, the
host's index build alone, and the walk ("kernel") under exon-first and under all, with both tiers' tops in LDS, with
the exons' alone (option "gene_body_top" 0) and with none (option "gene_top" 0).  One JSON line per shape on stdout
and, with --record, appended to profiles/introns_bench.jsonl.  Follows tools/genes_bench.py, whose read maker, packing
and clock it uses.

  annotation: genes_bench's human-size synthetic one (GENES genes, LINES exon lines, a gene's SLOTS exon places
      SLOT_STEP apart, strand by the gene's number), with NESTED of the genes moved into another gene's introns: gene g
      starts NEST_SHIFT bases behind gene g - 2 (same reference, same strand), so that its exon places fall between
      its host's and the two bodies lie over one another almost whole.
  reads: 10^7 of 90 bases.  Half are genes_bench's (85 % from a drawn exon line, a quarter of all spliced, 15 %
      anywhere); the other half are intronic: they start 5 to 225 bases behind the longest exon a drawn line's place can
      hold and end before the gene's next place.  90 % on their gene's strand.  Sorted by (reference, position), and
      the same reads shuffled.
  Timing as genes_bench: medians of --reps calls after a warm-up, each full call followed by the same call on the
  first 64 reads ("build": bodies derived, four tables made and uploaded, next to no lookups); "kernel" is the median of
  the differences and lies inside the build's noise at this size, so the kernels' own times come from a kernel trace
  of this tool taken in a run of its own (--reps 15 --shapes <one shape>; the dispatches of the full calls).

usage: python tools/introns_bench.py [--reps 50] [--reads 10000000] [--record] [--shapes sorted,shuffled]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
import genes_bench as gb  # noqa: E402
from umi_collapse_rs_amd import (Context, UMI_INTRONS_ALL, UMI_INTRONS_EXON_FIRST, UMI_STRAND_FORWARD)  # noqa: E402

NESTED, NEST_SHIFT = 0.10, 300
MODES = {"exon_first": UMI_INTRONS_EXON_FIRST, "all": UMI_INTRONS_ALL}
TOPS = {"tops": (1, 1), "exon_top_only": (1, 0), "no_top": (0, 0)}


def annotation(rng, genes, lines):
    g_ref = rng.integers(0, gb.REFS, genes).astype(np.int32)
    g_start = rng.integers(0, gb.REF_LEN - gb.SLOTS * gb.SLOT_STEP - 1000 - NEST_SHIFT, genes).astype(np.int64)
    nested = np.flatnonzero(rng.random(genes) < NESTED)
    nested = nested[(nested >= 2) & ~np.isin(nested - 2, nested)]  # (a host is not nested itself)
    g_ref[nested], g_start[nested] = g_ref[nested - 2], g_start[nested - 2] + NEST_SHIFT
    gene = np.sort(rng.integers(0, genes, lines)).astype(np.int32)
    slot = rng.integers(0, gb.SLOTS, lines)
    start = g_start[gene] + slot * gb.SLOT_STEP
    length = 80 + (gene.astype(np.int64) * 31 + slot * 17) % 200
    strand = np.where(gene % 2 == 0, ord("+"), ord("-")).astype(np.uint8)
    return {"ref": g_ref[gene], "start": start.astype(np.int32), "end": (start + length).astype(np.int32), "strand": strand,
            "gene": gene}, g_start, len(nested) / genes


def make_reads(rng, ex, g_start, n):
    reads = gb.make_reads(rng, ex, g_start, n)
    intronic = rng.random(n) < 0.5
    line = rng.integers(0, len(ex["gene"]), n)
    pos = ex["start"][line].astype(np.int64) + 285 + rng.integers(0, 220, n)  # (an exon is at most 279 long, a place 600)
    rev = ((ex["strand"][line] == ord("-")) ^ (rng.random(n) < 0.1)).astype(np.uint8)
    reads["ref"] = np.where(intronic, ex["ref"][line], reads["ref"]).astype(np.int32)
    reads["pos"] = np.where(intronic, pos, reads["pos"]).astype(np.int32)
    reads["rev"] = np.where(intronic, rev, reads["rev"]).astype(np.uint8)
    reads["words"][intronic, 0] = gb.READ_LEN << 4
    reads["n_words"] = np.where(intronic, 1, reads["n_words"])
    return reads, float(intronic.mean())


def paired(full_call, build_call, reps):
    """medians of the full call, of the build-only call behind it, and of their difference"""
    full, build = [], []
    full_call(), build_call()
    for _ in range(reps):  # (in turn: what the host's build drifts by is in both)
        t0 = time.perf_counter()
        counts = full_call()
        t1 = time.perf_counter()
        build_call()
        t2 = time.perf_counter()
        full.append((t1 - t0) * 1e3)
        build.append((t2 - t1) * 1e3)
    full, build = np.array(full), np.array(build)
    return {"ms_call_median": round(float(np.median(full)), 3), "ms_build_median": round(float(np.median(build)), 3),
            "ms_kernel_median": round(float(np.median(full - build)), 3), "ms_kernel_min": round(float(np.min(full - build)), 3)}, counts


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="sorted,shuffled")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/introns_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "introns_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    rng = np.random.default_rng(2026)
    n = a.reads
    ex, g_start, nested = annotation(rng, gb.GENES, gb.LINES)
    base, intronic = make_reads(rng, ex, g_start, n)
    orders = {"sorted": lambda: np.lexsort((base["pos"], base["ref"])), "shuffled": lambda: rng.permutation(n)}
    n_genes = int(ex["gene"].max()) + 1
    for name in a.shapes.split(","):
        reads = gb.ordered(base, orders[name]())
        ref, pos, rev, words, off = gb.packed(reads)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ref, pos, rev, words.view(np.int32), off.view(np.int64))]
        d_gene = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        d_tier = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        line = {"what": "umi_assign_genes_introns_device", "shape": name, "reads": n, "exon_lines": int(len(ex["gene"])),
                "genes": n_genes, "genes_nested": round(nested, 4), "reads_intronic": round(intronic, 4),
                "spliced": float((reads["n_words"] == 3).mean()), "reps": a.reps}

        def plain(m):
            return ctx.assign_genes_device(ex, n_genes, UMI_STRAND_FORWARD, *(t.data_ptr() for t in d), m, d_gene.data_ptr(),
                                           d_status.data_ptr())
        line["assign_genes"], counts = paired(lambda: plain(n), lambda: plain(64), a.reps)
        line["assign_genes"]["counts"] = [int(c) for c in counts]
        for mode_name, mode in MODES.items():
            def call(m):
                return ctx.assign_genes_introns_device(ex, n_genes, UMI_STRAND_FORWARD, mode, *(t.data_ptr() for t in d), m,
                                                       d_gene.data_ptr(), d_status.data_ptr(), d_tier.data_ptr())
            first = None
            for key, (top, body_top) in TOPS.items():
                ctx.set_option("gene_top", top)
                ctx.set_option("gene_body_top", body_top)
                res, counts = paired(lambda: call(n), lambda: call(64), a.reps)
                res["counts"] = [int(c) for c in counts]
                got = (d_gene.cpu().numpy(), d_status.cpu().numpy(), d_tier.cpu().numpy())
                if first is None:
                    first = got
                else:
                    res["same_as_with_tops"] = bool(all((x == y).all() for x, y in zip(got, first)))
                line[mode_name + "_" + key] = res
            ctx.set_option("gene_top", 1)
            ctx.set_option("gene_body_top", 1)
        emit(line)
        del d, d_gene, d_status, d_tier
    ctx.close()


if __name__ == "__main__":
    main()
