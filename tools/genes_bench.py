"""umi_assign_genes_device on resident data: the index build and the kernel apart, the kernel with and without the
sampled top in LDS (option "gene_top"), the same rule on the host in numpy, and umi_correct_barcodes_device on as many
reads as the yardstick.  One JSON line per shape on stdout and, with --record, appended to profiles/genes_bench.jsonl.

  annotation: synthetic, of human size -- GENES genes on REFS references of REF_LEN bases, LINES exon lines; a gene
      has SLOTS exon places SLOT_STEP apart, a line is a (gene, place) drawn at random, so places repeat the way one
      exon repeats over a gene's transcripts; a gene lies on + or - by its number.  The small one: 10^3 lines.
  reads: 10^7 of 90 bases, 85 % starting inside a drawn exon line (a quarter of all spliced: they leave the exon
      after 10 to 80 bases and go on at the gene's next place), 15 % anywhere; 90 % on their gene's strand.  Sorted by
      (reference, position) as a coordinate-sorted BAM has them, and the same reads shuffled.
  The call synchronises inside and is timed by the host's clock: medians of --reps calls after a warm-up call, all
  shapes in one process.  The index is built on the host by every call, so the same call on the first 64 reads is
  timed beside each full call ("build": the two tables made and uploaded, next to no lookups) and the median of the
  differences is what the walk and the lookups cost ("kernel"), with the top and without it.  At human size the
  build takes some 90 ms and the kernel under 1 ms, so that difference lies inside the build's noise: the kernel's own
  time there comes from a kernel trace of this tool (--reps 15 --shapes <one shape>; the dispatches of the full calls).
  numpy: segment tables made here by the same cut (for the result's sake: gene and status are compared with the
  device's) and the lookups as two searchsorted per block; only the lookups are timed.

usage: python tools/genes_bench.py [--reps 50] [--reads 10000000] [--record] [--shapes sorted,shuffled,small]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context, UMI_STRAND_FORWARD  # noqa: E402

GENES, LINES, REFS, REF_LEN = 60_000, 1_400_000, 24, 120_000_000
SLOTS, SLOT_STEP, READ_LEN = 10, 600, 90
MULTI = -2


def annotation(rng, genes, lines):
    g_ref = rng.integers(0, REFS, genes).astype(np.int32)
    g_start = rng.integers(0, REF_LEN - SLOTS * SLOT_STEP - 1000, genes).astype(np.int64)
    gene = np.sort(rng.integers(0, genes, lines)).astype(np.int32)
    slot = rng.integers(0, SLOTS, lines)
    start = g_start[gene] + slot * SLOT_STEP
    length = 80 + (gene.astype(np.int64) * 31 + slot * 17) % 200  # (a place's exon is the same on every line that names it)
    strand = np.where(gene % 2 == 0, ord("+"), ord("-")).astype(np.uint8)
    return {"ref": g_ref[gene], "start": start.astype(np.int32), "end": (start + length).astype(np.int32), "strand": strand,
            "gene": gene}, g_start


def make_reads(rng, ex, g_start, n):
    line = rng.integers(0, len(ex["gene"]), n)
    ref = ex["ref"][line].astype(np.int32)
    s, e, g = ex["start"][line].astype(np.int64), ex["end"][line].astype(np.int64), ex["gene"][line].astype(np.int64)
    u = rng.random(n)
    pos = s + rng.integers(0, 60, n)
    spliced = u < 0.25
    first = rng.integers(10, 81, n)
    slot = (s - g_start[g]) // SLOT_STEP
    gap = g_start[g] + (slot + 1) * SLOT_STEP - e  # to the gene's next place (the last place: into what lies behind)
    pos = np.where(spliced, e - first, pos)
    anywhere = u >= 0.85
    pos = np.where(anywhere, rng.integers(0, REF_LEN, n), pos)
    ref = np.where(anywhere, rng.integers(0, REFS, n), ref).astype(np.int32)
    rev = ((ex["strand"][line] == ord("-")) ^ (rng.random(n) < 0.1)).astype(np.uint8)
    words = np.zeros((n, 3), np.uint32)
    words[:, 0] = np.where(spliced, first << 4, READ_LEN << 4)
    words[:, 1] = (np.maximum(gap, 1) << 4 | 3).astype(np.uint32)
    words[:, 2] = ((READ_LEN - first) << 4).astype(np.uint32)
    n_words = np.where(spliced, 3, 1)
    return {"ref": ref, "pos": pos.astype(np.int32), "rev": rev, "words": words, "n_words": n_words}


def ordered(reads, order):
    return {k: v[order] for k, v in reads.items()}


def packed(reads):
    n_words = reads["n_words"]
    keep = np.arange(3)[None, :] < n_words[:, None]
    off = np.concatenate([[0], np.cumsum(n_words)]).astype(np.uint64)
    return reads["ref"], reads["pos"], reads["rev"], reads["words"][keep], off


# ---- the rule in numpy --------------------------------------------------------------------------------------

def numpy_table(ex, take):
    """start, end, label, run of the covered elementary segments of the exons whose strand is in `take`"""
    m = np.isin(ex["strand"], take)
    ks = (ex["ref"][m].astype(np.int64) << 32) | ex["start"][m]
    ke = (ex["ref"][m].astype(np.int64) << 32) | ex["end"][m]
    gene = ex["gene"][m].astype(np.int64)
    if not len(ks):
        z = np.zeros(0, np.int64)
        return z, z, z, z
    # a gene's exons united, so that a gene is open once wherever it is open
    o = np.lexsort((ks, gene))
    ks, ke, gene = ks[o], ke[o], gene[o]
    lift = gene << 40  # (a key has 37 bits: a later gene's keys lie above everything an earlier one reaches)
    reach = np.maximum.accumulate(ke + lift)
    new = np.r_[True, (ks + lift)[1:] > reach[:-1]]
    u_s, u_e, u_g = ks[new], np.maximum.reduceat(ke, np.flatnonzero(new)), gene[new]
    cuts = np.unique(np.concatenate([u_s, u_e]))
    d_count, d_sum = np.zeros(len(cuts) + 1, np.int64), np.zeros(len(cuts) + 1, np.int64)
    i_s, i_e = np.searchsorted(cuts, u_s), np.searchsorted(cuts, u_e)
    np.add.at(d_count, i_s, 1)
    np.add.at(d_count, i_e, -1)
    np.add.at(d_sum, i_s, u_g)
    np.add.at(d_sum, i_e, -u_g)
    count, idsum = np.cumsum(d_count)[:-2], np.cumsum(d_sum)[:-2]
    covered = count > 0
    start, end = cuts[:-1][covered], cuts[1:][covered]
    label = np.where(count[covered] == 1, idsum[covered], MULTI)
    run = np.cumsum(np.r_[True, (label[1:] != label[:-1]) | (label[1:] == MULTI)])
    return start, end, label, run


def numpy_blocks(table, ref, s, e, live):
    """per block: a gene, -1 none, MULTI several (live: the blocks that exist)"""
    start, end, label, run = table
    out = np.full(len(ref), -1, np.int64)
    if not len(start):
        return out
    ks, ke = (ref.astype(np.int64) << 32) | s, (ref.astype(np.int64) << 32) | e
    lo = np.searchsorted(end, ks, "right")
    hi = np.searchsorted(start, ke, "left") - 1
    hit = live & (lo <= hi)
    lo_c, hi_c = np.minimum(lo, len(start) - 1), np.maximum(hi, 0)
    several = (label[lo_c] == MULTI) | (run[lo_c] != run[hi_c])
    out[hit] = np.where(several, MULTI, label[lo_c])[hit]
    return out


def numpy_assign(tables, reads):
    """(gene, status) by the rule; forward: a read on + asks the + table"""
    ref, pos = reads["ref"], reads["pos"].astype(np.int64)
    w = reads["words"].astype(np.int64)
    spliced = reads["n_words"] == 3
    e1 = pos + (w[:, 0] >> 4)
    s2 = e1 + (w[:, 1] >> 4)
    e2 = s2 + (w[:, 2] >> 4)
    gene = np.full(len(ref), -1, np.int64)
    status = np.ones(len(ref), np.uint8)
    for rev in (0, 1):
        m = reads["rev"] == rev
        a = numpy_blocks(tables[rev], ref[m], pos[m], e1[m], np.ones(int(m.sum()), bool))
        b = numpy_blocks(tables[rev], ref[m], s2[m], e2[m], spliced[m])
        several = (a == MULTI) | (b == MULTI) | ((a >= 0) & (b >= 0) & (a != b))
        g = np.where(several, -1, np.maximum(a, b))
        gene[m] = g
        status[m] = np.where(several, 2, np.where(g >= 0, 0, 1))
    return gene.astype(np.int32), status


def clocked(call, reps):
    ms = []
    for r in range(reps + 1):
        t0 = time.perf_counter()
        out = call()
        if r:  # (the first call grows the workspace and loads the code object)
            ms.append((time.perf_counter() - t0) * 1e3)
    return np.array(ms), out


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--shapes", default="sorted,shuffled,small")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/genes_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "genes_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    rng = np.random.default_rng(2025)
    n = a.reads
    big, big_start = annotation(rng, GENES, LINES)
    small, small_start = annotation(rng, 100, 1000)
    base = make_reads(rng, big, big_start, n)
    shapes = {"sorted": (big, ordered(base, np.lexsort((base["pos"], base["ref"])))),
              "shuffled": (big, ordered(base, rng.permutation(n)))}
    few = make_reads(rng, small, small_start, n)
    shapes["small"] = (small, ordered(few, np.lexsort((few["pos"], few["ref"]))))
    # the yardstick: 16-base barcodes of as many reads against a list of 737,280
    acgt = np.frombuffer(b"ACGT", np.uint8)
    wl = acgt[rng.integers(0, 4, (737_280, 16))]
    wl = wl[np.unique(wl.view("S16").ravel(), return_index=True)[1]]
    d_bc = torch.from_numpy(wl[rng.integers(0, len(wl), n)].reshape(-1)).to("cuda:0")
    d_match = torch.empty(n, dtype=torch.int32, device="cuda:0")
    bc_ms, _ = clocked(lambda: ctx.correct_barcodes_device(d_bc.data_ptr(), n, 16, wl, 1, d_match.data_ptr()), min(a.reps, 20))
    del d_bc, d_match
    for name in a.shapes.split(","):
        ex, reads = shapes[name]
        ref, pos, rev, words, off = packed(reads)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ref, pos, rev, words.view(np.int32), off.view(np.int64))]
        d_gene = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        n_genes = int(ex["gene"].max()) + 1

        def call(m):
            return ctx.assign_genes_device(ex, n_genes, UMI_STRAND_FORWARD, *(t.data_ptr() for t in d), m, d_gene.data_ptr(),
                                           d_status.data_ptr())
        line = {"what": "umi_assign_genes_device", "shape": name, "reads": n, "exon_lines": int(len(ex["gene"])), "genes": n_genes,
                "spliced": float((reads["n_words"] == 3).mean()), "reps": a.reps}
        for top in (1, 0):
            ctx.set_option("gene_top", top)
            full, build = [], []
            call(n), call(64)
            for _ in range(a.reps):  # (in turn: what the host's build drifts by is in both)
                t0 = time.perf_counter()
                counts = call(n)
                t1 = time.perf_counter()
                call(64)
                t2 = time.perf_counter()
                full.append((t1 - t0) * 1e3)
                build.append((t2 - t1) * 1e3)
            full, build = np.array(full), np.array(build)
            key = "top" if top else "no_top"
            line["ms_call_median_" + key] = round(float(np.median(full)), 3)
            line["ms_build_median_" + key] = round(float(np.median(build)), 3)
            line["ms_kernel_median_" + key] = round(float(np.median(full - build)), 3)
            line["ms_kernel_min_" + key] = round(float(np.min(full - build)), 3)
            line["counts"] = [int(c) for c in counts]
            if top:
                g_top, s_top = d_gene.cpu().numpy(), d_status.cpu().numpy()
            else:
                line["same_without_top"] = bool((d_gene.cpu().numpy() == g_top).all() and (d_status.cpu().numpy() == s_top).all())
        ctx.set_option("gene_top", 1)
        tables = [numpy_table(ex, [ord("+"), ord(".")]), numpy_table(ex, [ord("-"), ord(".")])]
        line["segments"] = [int(len(t[0])) for t in tables]
        np_ms, (g_np, s_np) = clocked(lambda: numpy_assign(tables, reads), 3)
        line["ms_numpy_lookups_median"] = round(float(np.median(np_ms)), 1)
        line["same_as_numpy"] = bool((g_np == g_top).all() and (s_np == s_top).all())
        line["ms_barcodes_call_median"] = round(float(np.median(bc_ms)), 3)
        emit(line)
        del d, d_gene, d_status
    ctx.close()


if __name__ == "__main__":
    main()
