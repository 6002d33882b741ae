"""umi_assign_genes_transcripts_device beside umi_assign_genes_device (the yardstick) on the same resident arrays, in one
process: call time by the host's clock, the same call on 64 reads (the host-side index build and its upload, next to no
lookups), the kernel with and without the sampled top in LDS (option "gene_top"), the verdicts against numpy on a
sample, and the walk back of the shared lookup counted on the host.  One JSON line per shape on stdout and, with
--record, appended to profiles/transcripts_bench.jsonl.

  annotation: tools/genes_bench.py's genes and exon places (GENES genes on REFS references, SLOTS places a gene), with
      transcripts added: a gene has 1 to 6 transcripts (about 2 x 10^5 in all), each a subset of the gene's places, so
      an exon is shared between a gene's transcripts; about 1.4 x 10^6 exon lines.
  reads: 10^7 of 90 bases, 85 % starting inside a drawn exon line (a quarter of all spliced: they leave that exon at its
      end after 10 to 80 bases and go on at the start of their transcript's next exon), 15 % anywhere; 90 % on their
      gene's strand.  Sorted by (reference, position) and shuffled.
  The calls synchronise inside: medians of --reps calls after a warm-up, the full call and the 64-read call in turn; the
  median of their differences is what the walks and lookups cost by the host's clock.  The kernels' own times come from
  a kernel trace of `--trace 16` (16 dispatches of each kernel per shape and setting, nothing else timed), a run of its
  own.
  numpy: the rule for reads of one or two blocks, over the distinct exons and the instances, on --sample reads.
  walk back: build/test_transcript_index (make trtest) reads the annotation and the sample and counts the distinct exons
      the lookup steps over per read; it also checks the device's verdicts once more, on the CPU.

usage: python tools/transcripts_bench.py [--reps 50] [--reads 10000000] [--record] [--shapes sorted,shuffled] [--trace N]"""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from genes_bench import GENES, READ_LEN, REF_LEN, REFS, SLOT_STEP, SLOTS  # noqa: E402
from umi_collapse_rs_amd import Context, UMI_STRAND_FORWARD  # noqa: E402


def annotation(rng, genes):
    """exon lines transcript-major and ascending: dict of ref, start, end, strand, gene, transcript"""
    g_ref = rng.integers(0, REFS, genes).astype(np.int32)
    g_start = rng.integers(0, REF_LEN - SLOTS * SLOT_STEP - 1000, genes).astype(np.int64)
    n_tr = rng.integers(1, 7, genes)
    tr_gene = np.repeat(np.arange(genes), n_tr)
    keep = rng.random((len(tr_gene), SLOTS)) < 0.7
    keep[:, 0] |= keep.sum(1) < 2
    keep[:, 1] |= keep.sum(1) < 2
    tr, slot = np.nonzero(keep)
    gene = tr_gene[tr]
    start = g_start[gene] + slot * SLOT_STEP
    length = 80 + (gene.astype(np.int64) * 31 + slot * 17) % 200  # (a place's exon is the same in every transcript that has it)
    strand = np.where(gene % 2 == 0, ord("+"), ord("-")).astype(np.uint8)
    return {"ref": g_ref[gene], "start": start.astype(np.int32), "end": (start + length).astype(np.int32), "strand": strand,
            "gene": gene.astype(np.int32), "transcript": tr.astype(np.int32)}


def make_reads(rng, ex, n):
    lines = len(ex["gene"])
    line = rng.integers(0, lines, n)
    nxt = np.minimum(line + 1, lines - 1)
    has_next = (line + 1 < lines) & (ex["transcript"][nxt] == ex["transcript"][line])
    s, e = ex["start"][line].astype(np.int64), ex["end"][line].astype(np.int64)
    u = rng.random(n)
    spliced = u < 0.25
    first = rng.integers(10, 81, n)
    gap = np.where(has_next, ex["start"][nxt].astype(np.int64) - e, 1)  # (a transcript's last exon: on into what lies behind)
    pos = np.where(spliced, e - first, s + rng.integers(0, 60, n))
    anywhere = u >= 0.85
    pos = np.where(anywhere, rng.integers(0, REF_LEN, n), pos)
    ref = np.where(anywhere, rng.integers(0, REFS, n), ex["ref"][line]).astype(np.int32)
    rev = ((ex["strand"][line] == ord("-")) ^ (rng.random(n) < 0.1)).astype(np.uint8)
    words = np.zeros((n, 3), np.uint32)
    words[:, 0] = np.where(spliced, first << 4, READ_LEN << 4)
    words[:, 1] = (np.maximum(gap, 1) << 4 | 3).astype(np.uint32)
    words[:, 2] = ((READ_LEN - first) << 4).astype(np.uint32)
    return {"ref": ref, "pos": pos.astype(np.int32), "rev": rev, "words": words, "n_words": np.where(spliced, 3, 1)}


def ordered(reads, order):
    return {k: v[order] for k, v in reads.items()}


def packed(reads):
    keep = np.arange(3)[None, :] < reads["n_words"][:, None]
    off = np.concatenate([[0], np.cumsum(reads["n_words"])]).astype(np.uint64)
    return reads["ref"], reads["pos"], reads["rev"], reads["words"][keep], off


# ---- the rule in numpy, for reads of one block or two (no exon here touches another of its transcript) ----------

def numpy_assign(ex, reads):
    """(gene, status) under forward: a read on + asks the transcripts on +"""
    n = len(reads["ref"])
    ref, pos, w = reads["ref"].astype(np.int64), reads["pos"].astype(np.int64), reads["words"].astype(np.int64)
    two = reads["n_words"] == 3
    e1 = pos + (w[:, 0] >> 4)
    s2 = e1 + (w[:, 1] >> 4)
    e2 = s2 + (w[:, 2] >> 4)
    gene, status = np.full(n, -1, np.int64), np.ones(n, np.uint8)
    lines = len(ex["gene"])
    nxt = np.minimum(np.arange(lines) + 1, lines - 1)
    has_next = (np.arange(lines) + 1 < lines) & (ex["transcript"][nxt] == ex["transcript"])
    for rev in (0, 1):
        m = np.flatnonzero((ex["strand"] == (ord("-") if rev else ord("+"))))
        ks = (ex["ref"][m].astype(np.int64) << 32) | ex["start"][m]
        o = np.argsort(ks, kind="stable")
        m, ks = m[o], ks[o]
        ke = (ex["ref"][m].astype(np.int64) << 32) | ex["end"][m]
        g = ex["gene"][m].astype(np.int64)
        n_ok, n_s, n_e = has_next[m], ex["start"][nxt[m]].astype(np.int64), ex["end"][nxt[m]].astype(np.int64)
        r = np.flatnonzero(reads["rev"] == rev)
        k1, k1e = (ref[r] << 32) | np.maximum(pos[r], 0), (ref[r] << 32) | e1[r]
        lo = np.searchsorted(ks, k1 - 300, "left")  # (no exon is 300 bases long)
        hi = np.searchsorted(ks, k1, "right")
        found, several = np.full(len(r), -1, np.int64), np.zeros(len(r), bool)
        for k in range(int((hi - lo).max(initial=0))):
            i = np.minimum(lo + k, len(ks) - 1)
            fit = (lo + k < hi) & (pos[r] >= 0) & (ks[i] <= k1)
            fit &= np.where(two[r], (ke[i] == k1e) & n_ok[i] & (n_s[i] == s2[r]) & (n_e[i] >= e2[r]), ke[i] >= k1e)
            several |= fit & (found >= 0) & (found != g[i])
            found = np.where(fit & (found < 0), g[i], found)
        gene[r] = np.where(several, -1, found)
        status[r] = np.where(several, 2, np.where(found >= 0, 0, 1))
    return gene.astype(np.int32), status


def walk_back(ex, reads, gene, status):
    """(mean, max) distinct exons stepped over per read, counted by the shared lookup in build/test_transcript_index,
    which also compares the verdicts given with its own; None where the program is not built"""
    exe = os.path.join(ROOT, "build", "test_transcript_index")
    if not os.path.exists(exe):
        return None
    n = len(reads["ref"])
    with tempfile.TemporaryDirectory() as d:
        path = os.path.join(d, "bench.txt")
        with open(path, "w") as f:
            f.write("case %d %d %d bench\n" % (len(ex["gene"]), int(ex["transcript"].max()) + 1, n))
            for r, s, e, st, g, t in zip(ex["ref"].tolist(), ex["start"].tolist(), ex["end"].tolist(), ex["strand"].tolist(),
                                         ex["gene"].tolist(), ex["transcript"].tolist()):
                f.write("%d %d %d %c %d %d\n" % (r, s, e, st, g, t))
            for i in range(n):
                k = int(reads["n_words"][i])
                f.write("%d %d %d %d 0 0 %d 0 0 %d %s\n" % (reads["ref"][i], reads["pos"][i], reads["rev"][i], status[i], gene[i], k,
                                                            " ".join(str(int(x)) for x in reads["words"][i][:k])))
        out = subprocess.run([exe, path, "forward"], capture_output=True, text=True)
    m = re.search(r"walk back: reads (\d+), mean ([0-9.]+), max (\d+)", out.stdout)
    if out.returncode != 0 or not m:
        raise SystemExit("test_transcript_index: " + out.stdout[-500:] + out.stderr[-2000:])
    return float(m.group(2)), int(m.group(3))


def main():
    import torch
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--genes", type=int, default=GENES)
    ap.add_argument("--sample", type=int, default=100_000)
    ap.add_argument("--shapes", default="sorted,shuffled")
    ap.add_argument("--trace", type=int, default=0, help="N dispatches of each kernel and setting, nothing else (for a kernel trace)")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/transcripts_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "transcripts_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    rng = np.random.default_rng(2026)
    n = a.reads
    ex = annotation(rng, a.genes)
    base = make_reads(rng, ex, n)
    shapes = {"sorted": ordered(base, np.lexsort((base["pos"], base["ref"]))), "shuffled": ordered(base, rng.permutation(n))}
    n_genes, n_tr = a.genes, int(ex["transcript"].max()) + 1
    for name in a.shapes.split(","):
        reads = shapes[name]
        ref, pos, rev, words, off = packed(reads)
        d = [torch.from_numpy(np.ascontiguousarray(x)).to("cuda:0") for x in (ref, pos, rev, words.view(np.int32), off.view(np.int64))]
        d_gene = torch.empty(n, dtype=torch.int32, device="cuda:0")
        d_status = torch.empty(n, dtype=torch.uint8, device="cuda:0")
        calls = {
            "transcripts": lambda m: ctx.assign_genes_transcripts_device(ex, n_genes, n_tr, UMI_STRAND_FORWARD, *(t.data_ptr() for t in d), m,
                                                                         d_gene.data_ptr(), d_status.data_ptr()),
            "overlap": lambda m: ctx.assign_genes_device(ex, n_genes, UMI_STRAND_FORWARD, *(t.data_ptr() for t in d), m, d_gene.data_ptr(),
                                                         d_status.data_ptr()),
        }
        if a.trace:
            for what, call in calls.items():
                for top in (1, 0):
                    ctx.set_option("gene_top", top)
                    for _ in range(a.trace):
                        call(n)
            ctx.set_option("gene_top", 1)
            print("traced %s: %d dispatches of gene_transcripts_kernel<true>, <false>, gene_assign_kernel<true>, <false>, in this order"
                  % (name, a.trace), flush=True)
            continue
        line = {"what": "umi_assign_genes_transcripts_device beside umi_assign_genes_device", "shape": name, "reads": n,
                "exon_lines": int(len(ex["gene"])), "genes": n_genes, "transcripts": n_tr,
                "distinct_exons": int(len(np.unique(np.c_[ex["ref"], ex["start"], ex["end"]], axis=0))),
                "spliced": float((reads["n_words"] == 3).mean()), "reps": a.reps}
        for what, call in calls.items():
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
                key = what + ("_top" if top else "_no_top")
                line["ms_call_median_" + key] = round(float(np.median(full)), 3)
                line["ms_call_64_reads_median_" + key] = round(float(np.median(build)), 3)
                line["ms_difference_median_" + key] = round(float(np.median(full - build)), 3)
                line["counts_" + what] = [int(c) for c in counts]
                if what == "transcripts":
                    if top:
                        g_top, s_top = d_gene.cpu().numpy(), d_status.cpu().numpy()
                    else:
                        line["same_without_top"] = bool((d_gene.cpu().numpy() == g_top).all() and (d_status.cpu().numpy() == s_top).all())
        ctx.set_option("gene_top", 1)
        pick = np.sort(rng.choice(n, min(a.sample, n), replace=False))
        sample = ordered(reads, pick)
        g_np, s_np = numpy_assign(ex, sample)
        line["sample"] = int(len(pick))
        line["same_as_numpy_on_sample"] = bool((g_np == g_top[pick]).all() and (s_np == s_top[pick]).all())
        steps = walk_back(ex, sample, g_top[pick], s_top[pick])
        if steps is not None:
            line["walk_back_mean"], line["walk_back_max"] = round(steps[0], 3), steps[1]
        emit(line)
        del d, d_gene, d_status
    ctx.close()


if __name__ == "__main__":
    main()
