"""umi_assign_genes_transcripts_classes_device on resident arrays, beside its two yardsticks called in turn on the same
arrays in the same process: umi_assign_genes_transcripts_device (the transcript kernel) and
umi_assign_genes_classes_device (the gene-level two-tier class kernel).  One JSON line per shape on stdout and, with
--record, appended to profiles/transcript_classes_bench.jsonl.

  annotation: tools/transcripts_bench.py's (about 2 x 10^5 transcripts, 1.4 x 10^6 exon lines).
  reads: its 10^7 reads, half of them moved into introns as tools/introns_bench.py moves them: one block of 90 bases that
      starts 285 to 504 bases behind a drawn line's start.  Sorted by (reference, position) and shuffled.
  The calls synchronise inside: medians of --reps calls after a warm-up, the full call and the same call on 64 reads (the
  host's index build and its upload, next to no lookups) in turn.  The kernels' own times come from a kernel trace of
  `--trace 16` (16 dispatches of every kernel and setting, nothing else timed), a run of its own with no counters.
  numpy: the rule restated for this input (reads of one block or two, a gene on one reference and strand) on --sample
  reads, under exon-first and all.

usage: python tools/transcript_classes_bench.py [--reps 50] [--reads 10000000] [--record] [--shapes sorted,shuffled] [--trace N]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import transcripts_bench as tb  # noqa: E402
from genes_bench import GENES, READ_LEN, SLOTS  # noqa: E402
from umi_collapse_rs_amd import Context, UMI_INTRONS_ALL, UMI_INTRONS_EXON_FIRST, UMI_STRAND_FORWARD  # noqa: E402

MODES = {"exon_first": UMI_INTRONS_EXON_FIRST, "all": UMI_INTRONS_ALL}
BODY_MAX = 7000  # (no gene's body is that long: ten places of 600 bases)


def into_introns(rng, ex, reads):
    n = len(reads["ref"])
    intronic = rng.random(n) < 0.5
    line = rng.integers(0, len(ex["gene"]), n)
    pos = ex["start"][line].astype(np.int64) + 285 + rng.integers(0, 220, n)  # (an exon is at most 279 long, a place 600)
    rev = ((ex["strand"][line] == ord("-")) ^ (rng.random(n) < 0.1)).astype(np.uint8)
    reads["ref"] = np.where(intronic, ex["ref"][line], reads["ref"]).astype(np.int32)
    reads["pos"] = np.where(intronic, pos, reads["pos"]).astype(np.int32)
    reads["rev"] = np.where(intronic, rev, reads["rev"]).astype(np.uint8)
    reads["words"][intronic, 0] = READ_LEN << 4
    reads["n_words"] = np.where(intronic, 1, reads["n_words"])
    return reads, float(intronic.mean())


# ---- the rule in numpy, for this input ---------------------------------------------------------------------

def numpy_classify(ex, reads, n_genes, mode):
    """(gene, status, tier, cls) under forward.  G is transcripts_bench.numpy_assign's; a gene lies on one reference and
    strand, so it has one body, and its exons are its distinct lines"""
    n = len(reads["ref"])
    g_fit, s_fit = tb.numpy_assign(ex, reads)
    ref, pos, w = reads["ref"].astype(np.int64), reads["pos"].astype(np.int64), reads["words"].astype(np.int64)
    two = reads["n_words"] == 3
    b = np.zeros((n, 2, 2), np.int64)  # blocks, cut to [0, 2^31)
    b[:, 0, 0], b[:, 0, 1] = pos, pos + (w[:, 0] >> 4)
    b[:, 1, 0] = np.where(two, b[:, 0, 1] + (w[:, 1] >> 4), 0)
    b[:, 1, 1] = np.where(two, b[:, 1, 0] + (w[:, 2] >> 4), 0)
    b = np.clip(b, 0, 1 << 31)
    # the genes' bodies and their exons (at most SLOTS a gene)
    lo, hi = np.full(n_genes, 1 << 40, np.int64), np.zeros(n_genes, np.int64)
    np.minimum.at(lo, ex["gene"], ex["start"])
    np.maximum.at(hi, ex["gene"], ex["end"])
    g_ref, g_minus = np.zeros(n_genes, np.int64), np.zeros(n_genes, bool)
    g_ref[ex["gene"]], g_minus[ex["gene"]] = ex["ref"], ex["strand"] == ord("-")
    lines = np.unique(np.c_[ex["gene"], ex["start"], ex["end"]].astype(np.int64), axis=0)
    at = np.arange(len(lines)) - np.searchsorted(lines[:, 0], lines[:, 0], "left")
    xs, xe = np.zeros((n_genes, SLOTS), np.int64), np.zeros((n_genes, SLOTS), np.int64)
    xs[lines[:, 0], at], xe[lines[:, 0], at] = lines[:, 1], lines[:, 2]
    # B: the bodies of the read's strand and reference that share a base with a block; its first gene and whether there is another
    first, several = np.full(n, -1, np.int64), np.zeros(n, bool)
    used = np.flatnonzero(hi > 0)
    for rev in (0, 1):
        genes = used[g_minus[used] == bool(rev)]
        key = (g_ref[genes] << 32) | lo[genes]
        o = np.argsort(key, kind="stable")
        genes, key = genes[o], key[o]
        r = np.flatnonzero(reads["rev"] == rev)
        for j in (0, 1):
            s, e = b[r, j, 0], b[r, j, 1]
            a0 = np.searchsorted(key, (ref[r] << 32) | np.maximum(s - BODY_MAX, 0), "left")
            a1 = np.searchsorted(key, (ref[r] << 32) | e, "left")  # (bodies that start before e)
            for k in range(int((a1 - a0).max(initial=0))):
                i = np.minimum(a0 + k, len(key) - 1)
                g = genes[i]
                hit = (a0 + k < a1) & (e > s) & (g_ref[g] == ref[r]) & (lo[g] < e) & (s < hi[g])
                several[r] |= hit & (first[r] >= 0) & (first[r] != g)
                first[r] = np.where(hit & (first[r] < 0), g, first[r])
    fits = s_fit == 0
    if mode == UMI_INTRONS_EXON_FIRST:
        by_body = (s_fit == 1) & (first >= 0) & ~several
        status = np.where(fits, 0, np.where(s_fit == 2, 2, np.where(first < 0, 1, np.where(several, 2, 0))))
        gene = np.where(fits, g_fit, np.where(by_body, first, -1))
    else:
        status = np.where(s_fit == 2, 2, np.where(first < 0, 1, np.where(several, 2, 0)))
        by_body = (status == 0) & ~fits
        gene = np.where(status == 0, first, -1)
    tier = by_body.astype(np.uint8)
    # classes: by a transcript from the blocks' number; by a body from the cover of the blocks by the gene's exons
    g = np.maximum(gene, 0)
    cover = np.zeros(n, np.int64)
    for j in (0, 1):
        cover += np.clip(np.minimum(b[:, j, 1, None], xe[g]) - np.maximum(b[:, j, 0, None], xs[g]), 0, None).sum(1)
    length = (b[:, :, 1] - b[:, :, 0]).sum(1)
    gap_s, gap_e = b[:, 0, 1], b[:, 1, 0]
    gap_own = ((xs[g] <= gap_s[:, None]) & (gap_e[:, None] <= xe[g]) & (xe[g] > xs[g])).any(1) | (gap_e <= gap_s)
    body_cls = np.where(cover == 0, 4, np.where(cover < length, 3, np.where(two & ~gap_own, 2, 1)))
    cls = np.where(status != 0, 0, np.where(by_body, body_cls, np.where(two, 2, 1)))
    return gene.astype(np.int32), status.astype(np.uint8), tier, cls.astype(np.uint8)


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genes", type=int, default=GENES)
    ap.add_argument("--sample", type=int, default=100_000)
    ap.add_argument("--shapes", default="sorted,shuffled")
    ap.add_argument("--trace", type=int, default=0, help="N dispatches of each kernel and setting, nothing else (for a kernel trace)")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/transcript_classes_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "transcript_classes_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    rng = np.random.default_rng(2026)
    n = a.reads
    ex = tb.annotation(rng, a.genes)
    base, intronic = into_introns(rng, ex, tb.make_reads(rng, ex, n))
    shapes = {"sorted": tb.ordered(base, np.lexsort((base["pos"], base["ref"]))), "shuffled": tb.ordered(base, rng.permutation(n))}
    n_genes, n_tr = a.genes, int(ex["transcript"].max()) + 1
    for name in a.shapes.split(","):
        reads = shapes[name]
        ref, pos, rev, words, off = tb.packed(reads)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ref, pos, rev, words.view(np.int32), off.view(np.int64))]
        d_gene = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status, d_tier, d_cls = (torch.empty(n, dtype=torch.uint8, device="cuda:0") for _ in range(3))
        ins = [t.data_ptr() for t in d]

        def ours(mode, classes):
            return lambda m: ctx.assign_genes_transcripts_classes_device(ex, n_genes, n_tr, UMI_STRAND_FORWARD, mode, *ins, m, d_gene.data_ptr(),
                                                                         d_status.data_ptr(), d_tier.data_ptr(), d_cls.data_ptr(), classes=classes)
        calls = {"transcripts": lambda m: ctx.assign_genes_transcripts_device(ex, n_genes, n_tr, UMI_STRAND_FORWARD, *ins, m, d_gene.data_ptr(),
                                                                              d_status.data_ptr())}
        for mode_name, mode in MODES.items():
            calls["gene_classes_" + mode_name] = (lambda mode: lambda m: ctx.assign_genes_classes_device(
                ex, n_genes, UMI_STRAND_FORWARD, mode, *ins, m, d_gene.data_ptr(), d_status.data_ptr(), d_tier.data_ptr(), d_cls.data_ptr()))(mode)
            calls[mode_name + "_classes"] = ours(mode, True)
            calls[mode_name + "_plain"] = ours(mode, False)
        if a.trace:
            for what, call in calls.items():
                for _ in range(a.trace):
                    call(n)
            print("traced %s: %d dispatches each of %s, in this order" % (name, a.trace, ", ".join(calls)), flush=True)
            continue
        line = {"what": "umi_assign_genes_transcripts_classes_device beside umi_assign_genes_transcripts_device and umi_assign_genes_classes_device",
                "shape": name, "reads": n, "exon_lines": int(len(ex["gene"])), "genes": n_genes, "transcripts": n_tr,
                "reads_moved_into_introns": round(intronic, 4), "reps": a.reps}
        kept = {}
        for what, call in calls.items():
            full, build = [], []
            call(n), call(64)
            for _ in range(a.reps):  # (in turn: what the host's build drifts by is in both)
                t0 = time.perf_counter()
                out = call(n)
                t1 = time.perf_counter()
                call(64)
                t2 = time.perf_counter()
                full.append((t1 - t0) * 1e3)
                build.append((t2 - t1) * 1e3)
            full, build = np.array(full), np.array(build)
            line["ms_call_median_" + what] = round(float(np.median(full)), 3)
            line["ms_call_64_reads_median_" + what] = round(float(np.median(build)), 3)
            line["ms_difference_median_" + what] = round(float(np.median(full - build)), 3)
            if what.endswith("_classes") and not what.startswith("gene_"):
                line["counts_" + what], line["class_counts_" + what] = [int(c) for c in out[0]], [int(c) for c in out[1]]
                kept[what] = [t.cpu().numpy() for t in (d_gene, d_status, d_tier, d_cls)]
            if what.endswith("_plain"):
                mine = kept[what[:-6] + "_classes"]
                line["same_without_classes_" + what[:-6]] = bool(all((t.cpu().numpy() == m).all() for t, m in zip((d_gene, d_status, d_tier), mine)))
        for mode_name in MODES:
            for yard in ("transcripts", "gene_classes_" + mode_name):
                for mine in (mode_name + "_classes", mode_name + "_plain"):
                    line["ratio_call_%s_to_%s" % (mine, yard)] = round(line["ms_call_median_" + mine] / line["ms_call_median_" + yard], 3)
                    line["ratio_difference_%s_to_%s" % (mine, yard)] = round(line["ms_difference_median_" + mine] / line["ms_difference_median_" + yard], 3)
        pick = np.sort(rng.choice(n, min(a.sample, n), replace=False))
        sample = tb.ordered(reads, pick)
        line["sample"] = int(len(pick))
        for mode_name, mode in MODES.items():
            want = numpy_classify(ex, sample, n_genes, mode)
            line["same_as_numpy_on_sample_" + mode_name] = bool(all((w == g[pick]).all() for w, g in zip(want, kept[mode_name + "_classes"])))
        emit(line)
        del d, d_gene, d_status, d_tier, d_cls
    ctx.close()


if __name__ == "__main__":
    main()
