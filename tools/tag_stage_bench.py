"""Measures --umi-tag / --per-cell: the grouped device staging against the plain one,
and umicollapse --per-cell --umi-tag UB against name mode end to end.  Needs the GPU.

  python tools/tag_stage_bench.py [--reads 10000000] [--e2e-reads 2000000] [--repeats 3] [--out result.json]

1. umi_stage_reads_device against umi_stage_reads_grouped_device with group_key_bits = 0 (the same inputs, the
   two alternating): the no-regression check.
2. the grouped form with a 17-bit cell key, 10 M reads over 100,000 positions and 5,000 cells, with an
   alignment key of 17 bits (the composed key still fits) and of 36 bits (a genome's: extra passes).
3. a synthetic BAM of --e2e-reads reads that carry their UMI in the name and in UB, and a barcode in CB:
   umicollapse in name mode against --per-cell --umi-tag UB, alternating, wall time of the process.
Every time is the median of --repeats runs after one warm-up run."""
import argparse
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def staging_inputs(n, n_positions, n_cells, umi_len, seed=5):
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, n_positions, n)).astype(np.uint64)
    cell = rng.integers(0, n_cells, n).astype(np.uint64)
    pool = rng.integers(0, 4, (4096, umi_len))
    umis = np.frombuffer(b"ACGT", np.uint8)[pool[rng.integers(0, 4096, n)]].reshape(-1)
    score = rng.integers(0, 60, n).astype(np.int32)
    return pos, cell, umis, score


def bench_staging(args, result):
    import torch
    import umi_collapse_rs_amd as umi
    ctx = umi.Context(0)
    dev = torch.device("cuda:0")
    n, umi_len = args.reads, 12
    pos, cell, umis, score = staging_inputs(n, 100_000, 5000, umi_len)
    d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
    d_cell = torch.from_numpy(cell.view(np.int64)).to(dev)
    d_umi = torch.from_numpy(umis).to(dev)
    d_score = torch.from_numpy(score).to(dev)
    outs = [torch.empty(n, dtype=torch.int64, device=dev) for _ in range(3)]
    d_freq = torch.empty(n, dtype=torch.int32, device=dev)
    d_boff = torch.empty(n + 1, dtype=torch.int64, device=dev)
    d_keys, d_nmask, d_rep = (t.data_ptr() for t in outs)

    def plain(abits):
        return lambda: ctx.stage_reads_device(d_pos.data_ptr(), d_umi.data_ptr(), d_score.data_ptr(), n, umi_len, d_keys,
                                              d_nmask, d_freq.data_ptr(), d_rep, d_boff.data_ptr(), merge=1,
                                              align_key_bits=abits)

    def grouped(abits, gbits):
        return lambda: ctx.stage_reads_grouped_device(d_pos.data_ptr(), d_cell.data_ptr(), d_umi.data_ptr(),
                                                      d_score.data_ptr(), n, umi_len, d_keys, d_nmask, d_freq.data_ptr(),
                                                      d_rep, d_boff.data_ptr(), merge=1, align_key_bits=abits,
                                                      group_key_bits=gbits)

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3, r

    cases = [("plain_a17", plain(17)), ("grouped0_a17", grouped(17, 0)), ("grouped17_a17", grouped(17, 17)),
             ("plain_a36", plain(36)), ("grouped0_a36", grouped(36, 0)), ("grouped17_a36", grouped(36, 17))]
    times = {name: [] for name, _ in cases}
    counts = {}
    for _, fn in cases:  # warm-up (code objects, workspace)
        timed(fn)
    for _ in range(args.repeats):
        for name, fn in cases:
            ms, r = timed(fn)
            times[name].append(ms)
            counts[name] = r
    result["staging"] = {name: dict(median_ms=float(np.median(v)), runs_ms=v, entries=counts[name][0],
                                    buckets=counts[name][1]) for name, v in times.items()}
    result["staging_reads"] = n
    ctx.close()


def tagged_bam(path, n, n_positions, n_cells, seed=9):
    """fixed-size records built column by column: name r<9 digits>_<12-base UMI>, 50M, UB:Z, CB:Z"""
    import bamio
    rng = np.random.default_rng(seed)
    pos = np.sort(rng.integers(0, n_positions, n)) * 10 + 1000
    pool = rng.integers(0, 4, (4096, 12))
    ub = np.frombuffer(b"ACGT", np.uint8)[pool[rng.integers(0, 4096, n)]]
    cells = np.frombuffer(b"ACGT", np.uint8)[rng.integers(0, 4, (n_cells, 16))]
    cb = cells[rng.integers(0, n_cells, n)]
    l_name, l_seq = 24, 50
    body = 32 + l_name + 4 + 25 + l_seq + (3 + 13) + (3 + 19)
    rec = np.zeros((n, 4 + body), np.uint8)
    i32 = lambda col, v: rec.__setitem__((slice(None), slice(col, col + 4)), np.asarray(v, "<i4").view(np.uint8).reshape(-1, 4))
    i32(0, np.full(n, body))
    i32(4, np.zeros(n))
    i32(8, pos)
    rec[:, 12] = l_name
    rec[:, 13] = rng.integers(0, 61, n)
    rec[:, 14:16] = np.frombuffer(np.uint16(4680).tobytes(), np.uint8)
    rec[:, 16:18] = np.frombuffer(np.uint16(1).tobytes(), np.uint8)
    i32(20, np.full(n, l_seq))
    i32(24, np.full(n, -1))
    i32(28, np.full(n, -1))
    o = 36
    idx = np.arange(n)
    rec[:, o] = ord("r")
    for d in range(9):
        rec[:, o + 1 + d] = ord("0") + (idx // 10 ** (8 - d)) % 10
    rec[:, o + 10] = ord("_")
    rec[:, o + 11:o + 23] = ub
    o += l_name
    rec[:, o:o + 4] = np.frombuffer(np.uint32((50 << 4) | 0).tobytes(), np.uint8)
    o += 4 + 25
    rec[:, o:o + l_seq] = rng.integers(20, 41, (n, l_seq))
    o += l_seq
    rec[:, o:o + 3] = np.frombuffer(b"UBZ", np.uint8)
    rec[:, o + 3:o + 15] = ub
    o += 16
    rec[:, o:o + 3] = np.frombuffer(b"CBZ", np.uint8)
    rec[:, o + 3:o + 19] = cb
    rec[:, o + 19:o + 21] = np.frombuffer(b"-1", np.uint8)
    header = bamio.make_header([("chr1", 200_000_000)])
    with open(path, "wb") as f:
        f.write(bamio.bgzf_compress(header + rec.tobytes(), level=1))


def bench_e2e(args, result):
    cli = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
    with tempfile.TemporaryDirectory() as d:
        src = os.path.join(d, "in.bam")
        tagged_bam(src, args.e2e_reads, 100_000, 5000)
        modes = {"name": [], "per_cell_umi_tag_UB": ["--per-cell", "--umi-tag", "UB"]}
        times = {m: [] for m in modes}
        logs = {}
        for rnd in range(args.repeats + 1):
            for m, flags in modes.items():
                t0 = time.perf_counter()
                r = subprocess.run([cli, "-i", src, "-o", os.path.join(d, "o.bam"), "--num-threads", "16"] + flags,
                                   capture_output=True, text=True, timeout=600)
                wall = time.perf_counter() - t0
                if r.returncode != 0:
                    raise SystemExit("umicollapse %s failed: %s" % (m, r.stderr))
                if rnd:
                    times[m].append(wall)
                logs[m] = [l for l in r.stderr.splitlines() if l.startswith(("Number", "phases"))]
        result["e2e"] = {m: dict(median_s=float(np.median(v)), runs_s=v, log=logs[m]) for m, v in times.items()}
        result["e2e_reads"] = args.e2e_reads


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=10_000_000)
    ap.add_argument("--e2e-reads", type=int, default=2_000_000)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    result = {}
    bench_staging(args, result)
    bench_e2e(args, result)
    text = json.dumps(result, indent=1)
    print(text)
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
