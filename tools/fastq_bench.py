"""Fastq mode's long-key path on shapes F1-F3: umi_dedup_seqs timed with device events (call and pair
kernel), pairs evaluated against W = sum n(n-1)/2, umi_stage_seqs_device on resident data timed with
device events, and the umicollapse CLI end to end with its phase split, --stage host and --stage gpu
alternating.  One JSON line per shape and measurement on stdout.

  F1: 1 M reads, 150 bp, ~300 k molecules, 0.5 % substitutions, k = 1
  F2: F1 with the last 75 bases constant (one heavy bin: part 1 is shared by most of the bucket)
  F3: 1 M reads, lengths 18-150, 1 % N

--consensus: instead, per shape, umi_consensus_seqs_device on resident data (staged and collapsed on the
device just before), timed with device events, next to the stage and collapse calls of the same data, with
the bytes the call must move at the least and that traffic over the time as a share of the HBM rate.

usage: python tools/fastq_bench.py [--shapes F1,F2,F3] [--reps 5] [--out DIR] [--consensus]"""
import argparse
import json
import os
import re
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context, synth, to_bitset_seq  # noqa: E402

CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SHAPES = {
    "F1": dict(n_reads=1_000_000, n_molecules=300_000, length=150, err=0.005),
    "F2": dict(n_reads=1_000_000, n_molecules=300_000, length=150, err=0.005, const_suffix=75),
    "F3": dict(n_reads=1_000_000, n_molecules=300_000, lengths=list(range(18, 151)), err=0.005, n_frac=0.01),
}


def stage(seqs):
    buckets = {}
    for s in seqs:
        d = buckets.setdefault(len(s), {})
        d[s] = d.get(s, 0) + 1
    ent, off, blen = [], [0], []
    for L, d in buckets.items():
        items = sorted(d.items(), key=lambda kv: -kv[1])
        ent += items
        off.append(len(ent))
        blen.append(L)
    return ent, off, blen


def stage_leg(ctx, name, seqs, quals, reps):
    """umi_stage_seqs_device (merge avgqual, entry_of_read on) on data already on the device, timed with
    device events around the call (which synchronises inside)"""
    import torch
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.uint32)
    pos = np.zeros(n, np.uint64)
    pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    pos = np.concatenate([pos, pos + np.uint64(int(lens.sum()))])
    w = max(1, (3 * int(lens.max()) + 63) // 64)
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(b"".join(seqs) + b"".join(quals), np.uint8).copy()).to(dev)
    d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_keys, d_nm = (torch.empty(n * w, dtype=torch.int64, device=dev) for _ in range(2))
    d_freq, d_eor = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(2))
    d_rep = torch.empty(n, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        _, blen, ne, any_n = ctx.stage_seqs_device(d_text.data_ptr(), d_pos.data_ptr(), d_pos.data_ptr() + 8 * n,
                                                   d_len.data_ptr(), n, w, d_keys.data_ptr(), d_nm.data_ptr(),
                                                   d_freq.data_ptr(), d_rep.data_ptr(), d_eor.data_ptr(), merge=1)
        e1.record()
        torch.cuda.synchronize()
        if r:  # (the first call grows the workspace)
            ms.append(e0.elapsed_time(e1))
    return {"shape": name, "what": "umi_stage_seqs_device", "reads": n, "n_words": w, "entries": ne,
            "buckets": len(blen), "any_n": any_n, "ms_median": float(np.median(ms)), "ms_min": float(np.min(ms))}


HBM_MEASURED = 6.29e12  # bytes per second, a float4 copy on the MI355X


def consensus_leg(ctx, name, seqs, quals, reps):
    """stage -> collapse -> consensus, all on device pointers; device events around each call (each
    synchronises inside)"""
    import ctypes as C
    import torch
    from umi_collapse_rs_amd._lib import Stats, check, load, ptr
    n = len(seqs)
    lens = np.array([len(s) for s in seqs], np.uint32)
    total = int(lens.sum())
    pos = np.zeros(n, np.uint64)
    pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    pos = np.concatenate([pos, pos + np.uint64(total)])
    w = max(1, (3 * int(lens.max()) + 63) // 64)
    dev = torch.device("cuda", 0)
    d_text = torch.from_numpy(np.frombuffer(b"".join(seqs) + b"".join(quals), np.uint8).copy()).to(dev)
    d_pos = torch.from_numpy(pos.view(np.int64)).to(dev)
    d_len = torch.from_numpy(lens.view(np.int32)).to(dev)
    d_keys, d_nm = (torch.empty(n * w, dtype=torch.int64, device=dev) for _ in range(2))
    d_freq, d_eor, d_root, d_cr = (torch.empty(n, dtype=torch.int32, device=dev) for _ in range(4))
    d_rep, d_coff = (torch.empty(n, dtype=torch.int64, device=dev) for _ in range(2))
    d_kept = torch.empty(n, dtype=torch.uint8, device=dev)
    d_cs, d_cq = (torch.empty(total + 8, dtype=torch.uint8, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ms = {"stage": [], "dedup": [], "consensus": []}
    for r in range(reps + 1):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
        ev[0].record()
        boff, blen, ne, any_n = ctx.stage_seqs_device(d_text.data_ptr(), d_pos.data_ptr(), d_pos.data_ptr() + 8 * n,
                                                      d_len.data_ptr(), n, w, d_keys.data_ptr(), d_nm.data_ptr(),
                                                      d_freq.data_ptr(), d_rep.data_ptr(), d_eor.data_ptr(), merge=1)
        ev[1].record()
        st = Stats()
        check(load().umi_dedup_seqs_device(ctx._h, d_keys.data_ptr(), d_nm.data_ptr() if any_n else None, w,
                                           d_freq.data_ptr(), ptr(boff, C.c_uint64), ptr(blen, C.c_int32), len(blen), 1,
                                           0.5, 0, 0, d_kept.data_ptr(), d_root.data_ptr(), None, C.byref(st)))
        ev[2].record()
        cons_bytes = ctx.consensus_seqs_device(d_text.data_ptr(), d_pos.data_ptr(), d_pos.data_ptr() + 8 * n,
                                               d_len.data_ptr(), n, d_eor.data_ptr(), d_freq.data_ptr(), d_kept.data_ptr(),
                                               d_root.data_ptr(), ne, boff, blen, d_cs.data_ptr(), d_cq.data_ptr(),
                                               d_coff.data_ptr(), d_cr.data_ptr())
        ev[3].record()
        torch.cuda.synchronize()
        if r:  # (the first round grows the workspaces)
            for j, k in enumerate(("stage", "dedup", "consensus")):
                ms[k].append(ev[j].elapsed_time(ev[j + 1]))
    kept = int(st.n_kept)
    # the least the call moves: base and quality of every read once, the consensus written, per read its two
    # offsets, length and entry, per entry freq, kept, root, per kept entry its offset and count
    min_bytes = 2 * total + 2 * cons_bytes + n * (8 + 8 + 4 + 4) + ne * (4 + 1 + 4) + kept * (8 + 4)
    med = float(np.median(ms["consensus"]))
    return {"shape": name, "what": "umi_consensus_seqs_device", "reads": n, "entries": ne, "clusters": kept,
            "largest_cluster": int(d_cr[:ne][d_kept[:ne].bool()].max()), "bases": total, "cons_bytes": cons_bytes,
            "ms_median": med, "ms_min": float(np.min(ms["consensus"])), "min_bytes": int(min_bytes),
            "gb_per_s": round(min_bytes / med / 1e6, 1), "share_of_hbm_measured": round(min_bytes / (med * 1e-3) / HBM_MEASURED, 4),
            "ms_stage_median": float(np.median(ms["stage"])), "ms_dedup_median": float(np.median(ms["dedup"]))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="F1,F2,F3")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=None, help="also keep the FASTQ files here (default: a temp dir)")
    ap.add_argument("--consensus", action="store_true", help="time umi_consensus_seqs_device on the shapes instead")
    a = ap.parse_args()
    out = a.out or os.path.join(ROOT, "build", "fastq_bench")
    os.makedirs(out, exist_ok=True)
    ctx = Context(0, profile=True)
    for name in a.shapes.split(","):
        t0 = time.time()
        seqs, quals = synth.fastq_reads(hash(name) & 0xFFFF, **SHAPES[name])
        if a.consensus:
            print(json.dumps(consensus_leg(ctx, name, seqs, quals, a.reps)), flush=True)
            continue
        ent, off, blen = stage(seqs)
        w = max(1, max((3 * L + 63) // 64 for L in blen))
        keys, nm = to_bitset_seq([e[0] for e in ent], w)
        freq = np.array([e[1] for e in ent], np.int32)
        nmask = nm if nm.any() else None
        gen_s = time.time() - t0
        runs = []
        for r in range(a.reps + 1):
            t = time.perf_counter()
            kept, _, st = ctx.dedup_seqs(keys, nmask, freq, off, blen, k=1)
            wall = (time.perf_counter() - t) * 1e3
            if r:  # (the first call grows the workspace)
                runs.append((wall, st))
        st = runs[-1][1]
        print(json.dumps({
            "shape": name, "what": "umi_dedup_seqs", "reads": len(seqs), "entries": len(ent), "buckets": len(blen),
            "max_bucket": int(st["max_bucket"]), "W": int(st["n_pairs"]), "pairs_evaluated": int(st["n_pairs_evaluated"]),
            "candidates": int(st["n_candidates"]), "edges": int(st["n_edges"]), "kept": int(st["n_kept"]),
            "ms_call_wall_median": float(np.median([x[0] for x in runs])),
            "ms_total_median": float(np.median([x[1]["ms_total"] for x in runs])),
            "ms_prep_median": float(np.median([x[1]["ms_prep"] for x in runs])),
            "ms_kernel_median": float(np.median([x[1]["ms_kernel"] for x in runs])),
            "ms_collapse_median": float(np.median([x[1]["ms_collapse"] for x in runs])),
            "kernel_id": int(st["kernel_id"]), "gen_s": round(gen_s, 1)}), flush=True)
        print(json.dumps(stage_leg(ctx, name, seqs, quals, a.reps)), flush=True)
        path = os.path.join(out, name + ".fq")
        with open(path, "wb") as f:
            f.write(synth.fastq_text(seqs, quals))
        for r in range(3):
            for side in ("host", "gpu"):  # (alternating: the two sides see the same machine state)
                t = time.perf_counter()
                p = subprocess.run([CLI, "-m", "fastq", "-i", path, "-o", os.path.join(out, name + ".out.fq"), "-k", "1",
                                    "--stage", side], capture_output=True, text=True, timeout=600)
                wall = time.perf_counter() - t
                if p.returncode != 0:
                    print(p.stderr, file=sys.stderr)
                    sys.exit(p.returncode)
                m = re.search(r"phases: read\+parse ([0-9.]+) s, staging \((host|gpu)\) ([0-9.]+) s, gpu init ([0-9.]+) s, "
                              r"hot path \(H2D\+GPU\+D2H\) ([0-9.]+) s .*write ([0-9.]+) s", p.stderr)
                print(json.dumps({"shape": name, "what": "cli", "stage": m.group(2), "run": r, "wall_s": round(wall, 3),
                                  "read_parse_s": float(m.group(1)), "staging_s": float(m.group(3)),
                                  "gpu_init_s": float(m.group(4)), "gpu_call_s": float(m.group(5)),
                                  "write_s": float(m.group(6))}), flush=True)
    ctx.close()


if __name__ == "__main__":
    main()
