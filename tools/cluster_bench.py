"""umi_dedup_batch_device with algo = cluster, beside the two directional calls it is to be compared with, on
resident data.  One JSON line per shape and want_root on stdout and, with --record, appended to
profiles/cluster_bench.jsonl.

  shapes (synth.py, 12 bp, k = 1): config 2 -- 1 M reads, one position; config 3 -- 10 M reads in 100,000
      positions; 2m -- one deep position from the molecule model (bench.py's 2m).
  variants: algo = cluster; algo = dir, percentage = inf (the same result through the directional path: the
      yardstick); algo = dir, percentage = 0.5 (the shipped default, for scale).
  method: one process, one context per variant, each warmed up, then the three called in turn --reps times
      (at least 50), every call timed with device events (it synchronises inside); medians and minima.  Both
      want_root values.  The outputs of the first two are compared in the same run (kept, and root where asked
      for): a line with "equal": false is a failed run, and the exit status says so.
  acceptance: against the dir, percentage = inf variant, never against the cluster path itself -- the cluster
      median must not exceed it by more than the spread that variant shows between repetitions of the whole
      script on the same build ("--run R" tags a line with the repetition it belongs to; the spread is taken
      over the lines' ms_dir_inf_median by whoever reads the file).
  where the time goes: umi_stats of one more call of the first two variants on contexts with "profile" on
      (ms_prep / ms_pairs / ms_collapse / ms_finalize, n_rounds, n_edges).

usage: python tools/cluster_bench.py [--reps 50] [--only NAME] [--run R] [--record]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import UMI_ALGO_CLUSTER, UMI_ALGO_DIRECTIONAL, Context, synth  # noqa: E402

UMI_LEN, K = 12, 1
SHAPES = [("config2_1M_reads_one_position", lambda: synth.config2()),
          ("config3_10M_reads_100k_positions", lambda: synth.config3()),
          ("2m_molecule_model_deep_position", lambda: synth.config2m())]
VARIANTS = [("cluster", UMI_ALGO_CLUSTER, 0.5), ("dir_inf", UMI_ALGO_DIRECTIONAL, float("inf")),
            ("dir_0.5", UMI_ALGO_DIRECTIONAL, 0.5)]
PHASES = ("ms_prep", "ms_pairs", "ms_collapse", "ms_finalize", "ms_total")


def measure(name, st, want_root, reps, run):
    import torch
    keys = torch.from_numpy(st["keys"].view(np.int64).copy()).to("cuda:0")
    freq = torch.from_numpy(np.ascontiguousarray(st["freq"], np.int32)).to("cuda:0")
    off = np.ascontiguousarray(st["bucket_off"], np.uint64)
    n = len(st["keys"])
    assert int(st["freq"].max()) < 2 ** 31 - 1  # (dir at p = inf is the same result only below that)
    out = {v: (torch.zeros(n, dtype=torch.uint8, device="cuda:0"), torch.zeros(n, dtype=torch.int32, device="cuda:0"))
           for v, _, _ in VARIANTS}
    ctxs = {v: Context(0) for v, _, _ in VARIANTS}

    def call(ctx, v, algo, p):
        kept, root = out[v]
        return ctx.dedup_batch_device(keys.data_ptr(), 0, freq.data_ptr(), off, UMI_LEN, kept.data_ptr(),
                                      root.data_ptr() if want_root else 0, k=K, percentage=p, algo=algo)

    def once(v, algo, p):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        s = call(ctxs[v], v, algo, p)
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), s
    stats = {}
    for v, algo, p in VARIANTS:  # warm-up: workspace, edge list, code objects; twice, the second with everything in place
        once(v, algo, p)
        _, stats[v] = once(v, algo, p)
    ms = {v: [] for v, _, _ in VARIANTS}
    for _ in range(reps):
        for v, algo, p in VARIANTS:
            t, stats[v] = once(v, algo, p)
            ms[v].append(t)
    equal = bool(torch.equal(out["cluster"][0], out["dir_inf"][0]))
    if want_root:
        equal = equal and bool(torch.equal(out["cluster"][1], out["dir_inf"][1]))
    equal = equal and stats["cluster"]["n_kept"] == stats["dir_inf"]["n_kept"]
    phases = {}
    for v, algo, p in VARIANTS[:2]:
        prof = Context(0, profile=True)
        call(prof, v, algo, p)
        s = call(prof, v, algo, p)
        phases[v] = {f: round(float(s[f]), 4) for f in PHASES}
        prof.close()
    for c in ctxs.values():
        c.close()
    line = {"what": "umi_dedup_batch_device, algo cluster against dir", "shape": name, "run": run, "entries": n,
            "positions": len(off) - 1, "bases": UMI_LEN, "k": K, "want_root": bool(want_root), "reps": reps,
            "equal": equal, "pairs": int(stats["cluster"]["n_pairs"])}
    for v, _, _ in VARIANTS:
        tag = v.replace(".", "")
        line["ms_%s_median" % tag] = round(float(np.median(ms[v])), 4)
        line["ms_%s_min" % tag] = round(float(np.min(ms[v])), 4)
        line["n_kept_%s" % tag] = int(stats[v]["n_kept"])
        line["n_edges_%s" % tag] = int(stats[v]["n_edges"])
        line["n_rounds_%s" % tag] = int(stats[v]["n_rounds"])
    line["cluster_over_dir_inf"] = round(line["ms_cluster_median"] / max(line["ms_dir_inf_median"], 1e-9), 4)
    line["phases_cluster"], line["phases_dir_inf"] = phases["cluster"], phases["dir_inf"]
    return line


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="", help="one shape's name")
    ap.add_argument("--run", type=int, default=0, help="which repetition of the whole script this is")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/cluster_bench.jsonl")
    a = ap.parse_args()
    if a.reps < 50:
        ap.error("--reps must be at least 50")
    ok = True
    for name, make in SHAPES:
        if a.only and a.only != name:
            continue
        st = make()
        for want_root in (True, False):
            line = measure(name, st, want_root, a.reps, a.run)
            ok = ok and line["equal"]
            s = json.dumps(line)
            print(s, flush=True)
            if a.record:
                with open(os.path.join(ROOT, "profiles", "cluster_bench.jsonl"), "a") as f:
                    f.write(s + "\n")
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
