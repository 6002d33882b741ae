"""umi_filter_multigene_device on resident data, beside umi_dedup_batch_device with root[] and umi_count_matrix_device on
the same arrays and a host route (np.lexsort + a grouped maximum on the same input).  One JSON line per shape on stdout
and, with --record, appended to profiles/multigene_bench.jsonl.

  shapes: "many small" -- 2 x 10^7 buckets of 1 to 3 entries over 10^4 cells x 3 x 10^4 genes, 12-base UMIs, one bucket
      in 200 given its predecessor's cell and first UMI, so that about 1 % of the molecules share; "few large" -- 10^5
      buckets of 100 entries; "one run" -- one cell, one UMI in 10^6 one-entry buckets, and "runs of one" -- as many
      molecules with a UMI each, to set it against; "many small, 22 bases" -- the first shape with keys of two words,
      for the word-by-word sort.
  kept[] / root[] are the dedup call's own where it takes the keys (one word), else every entry kept.  The three
  device calls synchronise inside and are timed with device events around them: median and minimum of --reps calls
  after a warm-up call that grows the workspace and loads the code objects.  The filter's time holds its walk of the
  bucket table on the host and the table's upload, as the other calls' do.  The host route is timed by the host's clock,
  once; its result is what the device's is compared with (exact equality of kept_out, freq_out and the counts).
  --scale shrinks the shapes (a rehearsal); --host-only stops before the first device call; --only NAME runs one shape.

usage: python tools/multigene_bench.py [--reps 50] [--record] [--scale 1.0] [--host-only] [--only NAME]"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

N_CELLS, N_GENES = 10_000, 30_000
CODES = np.array([0, 5, 6, 3], np.uint64)  # A, T, C, G in the batched call's 3 bits per base


def random_keys(rng, n, umi_len):
    """[n, n_words] keys of random bases"""
    nw = (3 * umi_len + 63) // 64
    keys = np.zeros((n, nw), np.uint64)
    for b in range(umi_len):
        code = CODES[rng.integers(0, 4, n, dtype=np.uint8)]
        w, sh = 3 * b // 64, 3 * b % 64
        keys[:, w] |= code << np.uint64(sh)
        if sh > 61:
            keys[:, w + 1] |= code >> np.uint64(64 - sh)
    return keys


def make_shape(rng, n_buckets, lo, hi, umi_len, n_cells, share, one_umi=False):
    sizes = rng.integers(lo, hi + 1, n_buckets)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    keys = random_keys(rng, n, umi_len)
    if one_umi:
        keys[:] = keys[0]
    at = np.arange(n, dtype=np.int64) - np.repeat(off[:-1].astype(np.int64), sizes)
    freq = (np.repeat(sizes, sizes) - at).astype(np.int32)  # (falling inside a bucket, as the call's contract asks)
    if lo == hi == 1:
        freq = rng.integers(1, 4, n).astype(np.int32)
    cell = rng.integers(0, n_cells, n_buckets).astype(np.uint32)
    gene = rng.integers(0, N_GENES, n_buckets).astype(np.uint32)
    if share:  # a bucket in `share`: its predecessor's cell, and that bucket's first UMI as its own first
        b = np.arange(share, n_buckets, share)
        cell[b] = cell[b - 1]
        keys[off[b].astype(np.int64)] = keys[off[b - 1].astype(np.int64)]
    return keys, freq, off, cell, gene


def host_filter(keys, freq, kept, root, off, cell):
    """(kept_out, freq_out, counts) by a sort of the molecules and a maximum over equal neighbours"""
    n = len(freq)
    total = np.bincount(root.astype(np.int64), weights=freq.astype(np.float64), minlength=n).astype(np.int64)  # (exact below 2^53)
    mol = np.flatnonzero(kept)
    bucket = np.searchsorted(off, mol, side="right") - 1
    g, k, t = cell[bucket], keys[mol], total[mol]
    order = np.lexsort(tuple(k[:, w] for w in range(k.shape[1])) + (g,))
    g, k, t = g[order], k[order], t[order]
    head = np.concatenate([[True], (g[1:] != g[:-1]) | (k[1:] != k[:-1]).any(axis=1)]) if len(mol) else np.zeros(0, bool)
    starts = np.flatnonzero(head)
    length = np.diff(np.concatenate([starts, [len(mol)]]))
    top = np.maximum.reduceat(t, starts) if len(mol) else t
    run = np.cumsum(head) - 1
    holds = t == top[run]
    ties = np.add.reduceat(holds.astype(np.int64), starts) if len(mol) else holds
    alive = (length[run] == 1) | (holds & (ties[run] == 1))
    kept_out = np.zeros(n, np.uint8)
    kept_out[mol[order][alive]] = 1
    freq_out = np.where(kept_out[root.astype(np.int64)] != 0, freq, 0).astype(np.int32)
    counts = {"runs": int((length > 1).sum()), "removed": int((~alive).sum()), "removed_reads": int(t[~alive].sum())}
    return kept_out, freq_out, counts


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/multigene_bench.jsonl")
    ap.add_argument("--scale", type=float, default=1.0)
    ap.add_argument("--host-only", action="store_true")
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    sc = lambda v: max(1, int(v * a.scale))
    shapes = [("many small", sc(20_000_000), 1, 3, 12, N_CELLS, 200, False), ("few large", sc(100_000), 100, 100, 12, N_CELLS, 200, False),
              ("one run", sc(1_000_000), 1, 1, 12, 1, 0, True), ("runs of one", sc(1_000_000), 1, 1, 12, 1, 0, False),
              ("many small, 22 bases", sc(20_000_000), 1, 3, 22, N_CELLS, 200, False)]
    ctx = None
    for name, nb, lo, hi, umi_len, n_cells, share, one_umi in shapes:
        if a.only and a.only != name:
            continue
        rng = np.random.default_rng(nb + umi_len)
        keys, freq, off, cell, gene = make_shape(rng, nb, lo, hi, umi_len, n_cells, share, one_umi)
        n, nw = len(freq), keys.shape[1]
        kept, root = np.ones(n, np.uint8), np.arange(n, dtype=np.uint32)
        line = {"what": "umi_filter_multigene_device", "shape": name, "buckets": nb, "entries": n, "umi_len": umi_len, "groups": n_cells,
                "reps": a.reps}
        if not a.host_only:
            import torch
            from umi_collapse_rs_amd import Context
            ctx = ctx or Context(0)
            dev = lambda x: torch.from_numpy(x.view(np.int64) if x.dtype == np.uint64 else x.view(np.int32)
                                             if x.dtype == np.uint32 else x).to("cuda:0")
            d_keys, d_freq, d_cell, d_gene = dev(keys.reshape(-1)), dev(freq), dev(cell), dev(gene)
            d_kept = torch.ones(n, dtype=torch.uint8, device="cuda:0")
            d_root = torch.arange(n, dtype=torch.int32, device="cuda:0")
            if nw == 1 and not one_umi:  # (the collapse's own arrays; equal UMIs side by side are not a staged bucket)
                d_med, d_best, _ = timed(lambda: ctx.dedup_batch_device(d_keys.data_ptr(), 0, d_freq.data_ptr(), off, umi_len,
                                                                        d_kept.data_ptr(), d_root.data_ptr(), k=1), max(1, a.reps // 5))
                line.update({"ms_dedup_batch_device_root_median": round(d_med, 3), "ms_dedup_batch_device_root_min": round(d_best, 3)})
                kept, root = d_kept.cpu().numpy(), d_root.cpu().numpy().view(np.uint32)
            k_out = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
            f_out = torch.zeros(n, dtype=torch.int32, device="cuda:0")
            med, best, counts = timed(lambda: ctx.filter_multigene_device(d_keys.data_ptr(), d_freq.data_ptr(), d_kept.data_ptr(),
                                                                         d_root.data_ptr(), off, d_cell.data_ptr(), n_cells, umi_len,
                                                                         k_out.data_ptr(), d_freq_out=f_out.data_ptr(), n_words=nw), a.reps)
            outs = [torch.zeros(nb, dtype=torch.int32, device="cuda:0") for _ in range(3)]
            o_reads = torch.zeros(nb, dtype=torch.int64, device="cuda:0")
            c_med, c_best, _ = timed(lambda: ctx.count_matrix_device(k_out.data_ptr(), f_out.data_ptr(), off, d_gene.data_ptr(),
                                                                     d_cell.data_ptr(), N_GENES, n_cells, outs[0].data_ptr(),
                                                                     outs[1].data_ptr(), outs[2].data_ptr(), o_reads.data_ptr()),
                                     max(1, a.reps // 5))
            line.update({"ms_filter_median": round(med, 3), "ms_filter_min": round(best, 3), "ms_count_matrix_median": round(c_med, 3),
                         "ms_count_matrix_min": round(c_best, 3), "entries_per_s_filter": n / (med * 1e-3)})
            got = (k_out.cpu().numpy(), f_out.cpu().numpy(), counts)
            del d_keys, d_freq, d_cell, d_gene, d_kept, d_root, k_out, f_out, outs, o_reads
        t0 = time.perf_counter()
        exp = host_filter(keys, freq, kept, root, off, cell)
        line.update({"ms_host_lexsort_max": round((time.perf_counter() - t0) * 1e3, 1), "molecules": int(np.count_nonzero(kept)),
                     "runs": exp[2]["runs"], "removed": exp[2]["removed"]})
        if not a.host_only:
            line["same_as_host"] = bool((got[0] == exp[0]).all() and (got[1] == exp[1]).all() and got[2] == exp[2])
        s = json.dumps(line)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "multigene_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    if ctx:
        ctx.close()


if __name__ == "__main__":
    main()
