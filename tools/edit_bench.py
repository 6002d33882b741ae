"""umi_dedup_batch_edit_device on resident data, with umi_dedup_batch_device on the same arrays beside it.
One JSON line per measurement on stdout and, with --record, appended to profiles/edit_bench.jsonl.

  shapes: 10 M reads in 100,000 positions (the molecule model of the main workload), and one position of
      20,000, 100,000 and 1,000,000 uniform-random entries; 12 bp, k = 2.
  Each call is timed with device events (it synchronises inside): median of --reps calls after a warm-up
      call.  A shape whose warm-up call says the repetitions would pass --time-limit seconds runs fewer of
      them, one at least, and its line says how many ("reps").
  Quoted: pairs per second of the call (W / median), n_candidates / n_pairs_evaluated (what the count filter
      lets through), and the share of the pair kernel's time that is the exact check -- 1 - ms_kernel(k = 0)
      / ms_kernel(k = 2) from a context with "profile" on: at k = 0 the filter passes equal letter counts
      only, so that call's kernel time is the filter's, the loads' and the queue's.
  No threshold: the Hamming call on the same build is the context figure.

usage: python tools/edit_bench.py [--reps 7] [--time-limit 120] [--only NAME] [--record]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context, synth  # noqa: E402

UMI_LEN, K = 12, 2


def one_position(n_entries, seed):
    st = synth.config2(seed=seed, n_reads=n_entries + n_entries // 8 + 1000, umi_len=UMI_LEN)
    assert len(st["keys"]) >= n_entries  # (rank order: the first n entries are a bucket in rank order too)
    return dict(keys=st["keys"][:n_entries], freq=st["freq"][:n_entries], bucket_off=np.array([0, n_entries], np.uint64))


SHAPES = [("10M_reads_100k_positions", lambda: synth.config3()),
          ("one_position_20k", lambda: one_position(20_000, 20)),
          ("one_position_100k", lambda: one_position(100_000, 100)),
          ("one_position_1M", lambda: one_position(1_000_000, 1000))]


def timed(call, reps, limit_s):
    """(median ms, min ms, repetitions run, last stats) of call() after one warm-up call"""
    import torch

    def once():
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), st
    warm, st = once()  # (grows the workspace and the edge list, loads the code object)
    reps = max(1, min(reps, int(limit_s * 1e3 / max(warm, 1e-3))))
    ms = []
    for _ in range(reps):
        t, st = once()
        ms.append(t)
    return float(np.median(ms)), float(np.min(ms)), reps, st


def measure(name, st, reps, limit_s):
    import torch
    keys = torch.from_numpy(st["keys"].view(np.int64).copy()).to("cuda:0")
    freq = torch.from_numpy(np.ascontiguousarray(st["freq"], np.int32)).to("cuda:0")
    off = np.ascontiguousarray(st["bucket_off"], np.uint64)
    n = len(st["keys"])
    kept = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    root = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ctx, prof = Context(0), Context(0, profile=True)
    args = (keys.data_ptr(), 0, freq.data_ptr(), off, UMI_LEN, kept.data_ptr(), root.data_ptr())
    e_med, e_min, e_reps, e_st = timed(lambda: ctx.dedup_batch_edit_device(*args, k=K), reps, limit_s)
    kept_edit = int(e_st["n_kept"])
    h_med, h_min, h_reps, h_st = timed(lambda: ctx.dedup_batch_device(*args, k=K), reps, limit_s)
    # the pair kernel alone, with and without an exact check worth the name
    p2 = prof.dedup_batch_edit_device(*args, k=K)
    p2 = prof.dedup_batch_edit_device(*args, k=K)
    p0 = prof.dedup_batch_edit_device(*args, k=0)
    p0 = prof.dedup_batch_edit_device(*args, k=0)
    ctx.close()
    prof.close()
    w = int(e_st["n_pairs"])
    return {"what": "umi_dedup_batch_edit_device", "shape": name, "entries": n, "positions": len(off) - 1, "bases": UMI_LEN,
            "k": K, "pairs": w, "reps": e_reps, "reps_asked": reps,
            "ms_edit_median": round(e_med, 3), "ms_edit_min": round(e_min, 3),
            "pairs_per_s_edit": w / (e_med * 1e-3) if w else 0.0,
            "n_pairs_evaluated": int(e_st["n_pairs_evaluated"]), "n_candidates": int(e_st["n_candidates"]),
            "filter_pass_rate": round(e_st["n_candidates"] / max(1, e_st["n_pairs_evaluated"]), 4),
            "n_edges_edit": int(e_st["n_edges"]), "kept_edit": kept_edit,
            "ms_kernel_k2": round(float(p2["ms_kernel"]), 3), "ms_kernel_k0": round(float(p0["ms_kernel"]), 3),
            "filter_pass_rate_k0": round(p0["n_candidates"] / max(1, p0["n_pairs_evaluated"]), 5),
            "exact_check_share_of_kernel": round(1.0 - float(p0["ms_kernel"]) / max(float(p2["ms_kernel"]), 1e-6), 3),
            "ms_hamming_median": round(h_med, 3), "ms_hamming_min": round(h_min, 3), "reps_hamming": h_reps,
            "pairs_per_s_hamming": w / (h_med * 1e-3) if w else 0.0,
            "n_pairs_evaluated_hamming": int(h_st["n_pairs_evaluated"]), "kept_hamming": int(h_st["n_kept"]),
            "edit_over_hamming": round(e_med / max(h_med, 1e-6), 2)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--time-limit", type=float, default=120.0, help="seconds of timed repetitions per shape and call")
    ap.add_argument("--only", default="", help="one shape's name")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/edit_bench.jsonl")
    a = ap.parse_args()

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "edit_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    for name, make in SHAPES:
        if a.only and a.only != name:
            continue
        emit(measure(name, make(), a.reps, a.time_limit))


if __name__ == "__main__":
    main()
