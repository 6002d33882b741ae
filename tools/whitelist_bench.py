"""umi_correct_umis_device on resident data, and umicollapse end to end with and without --umi-whitelist.
One JSON line per measurement on stdout and, with --record, appended to profiles/whitelist_bench.jsonl.

  library: reads x bases x listed UMIs of 1e7 x 12 x 96, 1e7 x 12 x 4096, 1e6 x 24 x 65536.  The call is timed
      with device events (it synchronises inside): median of --reps calls after a warm-up call.  The same
      call with a list of ONE entry is timed beside it -- the check pass over the reads, the two host looks
      and the stores, with next to no comparisons -- and the difference is what the comparisons cost;
      comparisons per second are quoted on both.
  cli: a 2 M-read BAM whose UMIs are listed ones with errors; wall time of the process, plain and with
      --umi-whitelist, alternating.

usage: python tools/whitelist_bench.py [--reps 7] [--skip-cli] [--record]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import whitelist_model as wm  # noqa: E402
from umi_collapse_rs_amd import Context  # noqa: E402

CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SHAPES = [(10_000_000, 12, 96), (10_000_000, 12, 4096), (1_000_000, 24, 65536)]
PAIR_STEP = {"pairs": 4.7e11, "ms": 33.0}  # the brute-force pair step of the main workload (README), one key word


def timed(ctx, d_in, n, umi_len, wl, d_match, reps):
    import torch
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        counts = ctx.correct_umis_device(d_in.data_ptr(), n, umi_len, wl, 1, 1, 0, d_match.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if r:  # (the first call grows the workspace and loads the code object)
            ms.append(e0.elapsed_time(e1))
    return float(np.median(ms)), float(np.min(ms)), [int(c) for c in counts]


def library_leg(ctx, n, umi_len, n_wl, reps):
    import torch
    rng = np.random.default_rng(n_wl)
    wl = wm.random_list(rng, n_wl, umi_len)
    reads = wm.noisy_reads(rng, wl, umi_len, n)
    d_in = torch.from_numpy(reads).to("cuda:0")
    d_match = torch.empty(n, dtype=torch.int32, device="cuda:0")
    med, best, counts = timed(ctx, d_in, n, umi_len, wl, d_match, reps)
    med1, _, _ = timed(ctx, d_in, n, umi_len, wl[:umi_len], d_match, reps)
    words = (umi_len + 15) // 16
    cmp_ms = max(med - med1, 1e-6)
    pair_rate = PAIR_STEP["pairs"] / (PAIR_STEP["ms"] * 1e-3)
    return {"what": "umi_correct_umis_device", "reads": n, "bases": umi_len, "listed": n_wl, "words_per_key": words,
            "comparisons": n * n_wl, "ms_call_median": round(med, 3), "ms_call_min": round(best, 3),
            "ms_call_one_entry_median": round(med1, 3), "ms_compare": round(cmp_ms, 3),
            "comparisons_per_s_call": n * n_wl / (med * 1e-3), "comparisons_per_s_compare": n * n_wl / (cmp_ms * 1e-3),
            "pair_step_pairs_per_s": pair_rate,
            "slower_than_pair_step_per_key_word": round(pair_rate / (n * n_wl * words / (cmp_ms * 1e-3)), 2),
            "counts": counts}


def write_bam(path, n_reads, n_positions, wl, umi_len, seed=1):
    import bamio
    rng = np.random.default_rng(seed)
    header = bamio.make_header([("chr1", 250_000_000)])
    rpp = n_reads // n_positions
    with open(path, "wb") as f:
        buf, idx = bytearray(header), 0
        for p0 in range(0, n_positions, 2000):
            npos = min(2000, n_positions - p0)
            letters = wm.noisy_reads(rng, wl, umi_len, npos * rpp).reshape(-1, umi_len)
            quals = rng.integers(20, 41, (npos * rpp, 50)).astype(np.uint8)
            for i in range(npos * rpp):
                buf += bamio.make_record("r%d_%s" % (idx, letters[i].tobytes().decode()), 0, 0, 1000 + 10 * (p0 + i // rpp), 60,
                                         [("M", 50)], 50, quals[i].tobytes())
                idx += 1
            f.write(bamio.bgzf_compress(bytes(buf), level=1)[:-28])  # (no EOF marker between chunks)
            buf = bytearray()
        f.write(bytes.fromhex("1f8b08040000000000ff0600424302001b0003000000000000000000"))


def cli_leg(out_dir, reps, emit):
    rng = np.random.default_rng(3)
    wl = wm.random_list(rng, 4096, 12)
    src, lst = os.path.join(out_dir, "wl_2m.bam"), os.path.join(out_dir, "wl_4096.txt")
    write_bam(src, 2_000_000, 20_000, wl, 12)
    with open(lst, "w") as f:
        f.write("\n".join(bytes(r).decode() for r in wl.reshape(-1, 12)) + "\n")
    walls = {"plain": [], "whitelist": []}
    for r in range(reps + 1):
        for side, extra in (("plain", []), ("whitelist", ["--umi-whitelist", lst])):  # (alternating)
            t = time.perf_counter()
            p = subprocess.run([CLI, "-i", src, "-o", os.path.join(out_dir, "wl_out.bam"), "-k", "0", "--num-threads", "16"] + extra,
                               capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t
            if p.returncode != 0:
                print(p.stderr, file=sys.stderr)
                sys.exit(p.returncode)
            if r:  # (the first round warms the page cache)
                walls[side].append(wall)
    emit({"what": "cli", "reads": 2_000_000, "positions": 20_000, "bases": 12, "listed": 4096, "k": 0,
          "wall_s_plain_median": round(float(np.median(walls["plain"])), 3),
          "wall_s_whitelist_median": round(float(np.median(walls["whitelist"])), 3),
          "wall_s_plain": [round(w, 3) for w in walls["plain"]], "wall_s_whitelist": [round(w, 3) for w in walls["whitelist"]]})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--record", action="store_true", help="append the lines to profiles/whitelist_bench.jsonl")
    ap.add_argument("--out", default=os.path.join(ROOT, "build", "whitelist_bench"))
    a = ap.parse_args()
    os.makedirs(a.out, exist_ok=True)

    def emit(d):
        s = json.dumps(d)
        print(s, flush=True)
        if a.record:
            with open(os.path.join(ROOT, "profiles", "whitelist_bench.jsonl"), "a") as f:
                f.write(s + "\n")
    ctx = Context(0)
    for n, umi_len, n_wl in SHAPES:
        emit(library_leg(ctx, n, umi_len, n_wl, a.reps))
    ctx.close()
    if not a.skip_cli:
        cli_leg(a.out, 3, emit)


if __name__ == "__main__":
    main()
