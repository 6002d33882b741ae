"""umi_consensus_bam_device on two shapes, timed with device events around the call on resident data (it
synchronises twice inside), with the bytes the call must move at the least and that traffic over the time as
a share of the HBM rate; beside it umi_consensus_seqs_device (fastq_bench.consensus_leg) on the same reads
as text; then the umicollapse CLI end to end on the 2 M-read file bench.py uses, without and with
--call-consensus, alternating.  One JSON line per measurement on stdout and in
profiles/consensus_bam_bench.jsonl.

  small: 200,000 clusters of 5 reads of 150 bases
  deep:  one cluster of 50,000 reads of 150 bases

The reads of a cluster are copies of its molecule without errors, so that the FASTQ call (whose clusters are
what its own collapse finds) sees the same clusters.  The vote kernel's own time is a rocprofv3
--kernel-trace --stats run of this script (a run of its own: tracing slows the host).

usage: python tools/consensus_bam_bench.py [--shapes small,deep] [--reps 5] [--no-cli] [--parent-cli PATH]"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))
from umi_collapse_rs_amd import Context  # noqa: E402

CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
SHAPES = {"small": dict(n_clusters=200_000, copies=5, length=150), "deep": dict(n_clusters=1, copies=50_000, length=150)}
HBM_MEASURED = 6.29e12  # bytes per second, a float4 copy on the MI355X


def make(seed, n_clusters, copies, length):
    """(base ids [n_clusters, length], qualities [n, length], cluster of every read), reads shuffled"""
    rng = np.random.default_rng(seed)
    mol = rng.integers(0, 4, (n_clusters, length), dtype=np.uint8)
    cluster = rng.permutation(np.repeat(np.arange(n_clusters, dtype=np.uint32), copies))
    qual = rng.integers(2, 42, (len(cluster), length), dtype=np.uint8)
    return mol, qual, cluster


def bam_leg(ctx, name, mol, qual, cluster, reps):
    import torch
    n, L = qual.shape
    nc = len(mol)
    nib = (1 << mol[cluster]).astype(np.uint8)
    if L & 1:
        nib = np.concatenate([nib, np.zeros((n, 1), np.uint8)], axis=1)
    rows = np.concatenate([np.full((n, 3), 0x5A, np.uint8), (nib[:, 0::2] << 4) | nib[:, 1::2], qual], axis=1)
    stride, sb = rows.shape[1], (L + 1) // 2
    at = 3 + stride * np.arange(n, dtype=np.int64)
    dev = torch.device("cuda", 0)
    d_data = torch.from_numpy(rows.reshape(-1)).to(dev)
    d_sp, d_qp = torch.from_numpy(at).to(dev), torch.from_numpy(at + sb).to(dev)
    d_len = torch.full((n,), L, dtype=torch.int32, device=dev)
    d_cl = torch.from_numpy(cluster.view(np.int32).copy()).to(dev)
    d_clen = torch.full((nc,), L, dtype=torch.int32, device=dev)
    o_seq = torch.empty(nc * sb + 8, dtype=torch.uint8, device=dev)
    o_qual = torch.empty(nc * L + 8, dtype=torch.uint8, device=dev)
    o_so, o_qo = (torch.empty(nc, dtype=torch.int64, device=dev) for _ in range(2))
    o_d, o_e = (torch.empty(nc, dtype=torch.int32, device=dev) for _ in range(2))
    torch.cuda.synchronize()
    ms = []
    for r in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ctx.consensus_bam_device(d_data.data_ptr(), d_sp.data_ptr(), d_qp.data_ptr(), d_len.data_ptr(), d_cl.data_ptr(), n,
                                 d_clen.data_ptr(), nc, o_seq.data_ptr(), o_qual.data_ptr(), o_so.data_ptr(), o_qo.data_ptr(),
                                 o_d.data_ptr(), o_e.data_ptr())
        e1.record()
        torch.cuda.synchronize()
        if r:  # (the first call grows the workspace)
            ms.append(e0.elapsed_time(e1))
    assert int(o_d.sum()) == n and int(o_e.sum()) == 0  # every read voted, and they agree
    # the least the call moves: 1.5 bytes per voter base, the consensus written, per read its two offsets,
    # length and cluster, per cluster its length, two offsets, depth and disagree
    min_bytes = n * (sb + L) + nc * (sb + L) + n * (8 + 8 + 4 + 4) + nc * (4 + 8 + 8 + 4 + 4)
    med = float(np.median(ms))
    return {"shape": name, "what": "umi_consensus_bam_device", "reads": n, "clusters": nc, "length": L, "ms_median": med,
            "ms_min": float(np.min(ms)), "min_bytes": int(min_bytes), "gb_per_s": round(min_bytes / med / 1e6, 1),
            "share_of_hbm_measured": round(min_bytes / (med * 1e-3) / HBM_MEASURED, 4), "ms_vote_kernel": None}


def cli_leg(parent_cli, reps):
    """the file of bench.py's end-to-end run; this build without and with the flag (and the parent build's
    program without it, where one is given), alternating"""
    out = os.path.join(ROOT, "build", "consensus_bam_bench")
    os.makedirs(out, exist_ok=True)
    src = os.path.join(out, "in.bam")
    subprocess.check_call([sys.executable, os.path.join(ROOT, "tools", "make_bam.py"), src, "--reads", "2000000", "--positions",
                           "20000"], stdout=subprocess.DEVNULL, stderr=subprocess.DEVNULL)
    sides = [("plain", CLI, []), ("call-consensus", CLI, ["--call-consensus"])]
    if parent_cli:
        sides.insert(0, ("parent plain", parent_cli, []))
    for r in range(reps + 1):
        for side, cli, extra in sides:
            time.sleep(1.0)  # (the driver puts the context of the process before away in the background)
            t = time.perf_counter()
            p = subprocess.run([cli, "-i", src, "-o", os.path.join(out, "out.bam"), "--merge", "avgqual", "--num-threads", "16"]
                               + extra, capture_output=True, text=True, timeout=600)
            wall = time.perf_counter() - t
            if p.returncode != 0:
                print(p.stderr, file=sys.stderr)
                sys.exit(p.returncode)
            phases = [l for l in p.stderr.splitlines() if l.startswith("phases:")]
            yield {"what": "cli", "side": side, "run": r, "warm_up": r == 0, "wall_s": round(wall, 3), "phases": phases[0][8:]}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shapes", default="small,deep")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cli", action="store_true")
    ap.add_argument("--parent-cli", default=None, help="bin/umicollapse of the parent commit's build, to run beside this one")
    a = ap.parse_args()
    log = open(os.path.join(ROOT, "profiles", "consensus_bam_bench.jsonl"), "w")

    def emit(rec):
        line = json.dumps(rec)
        print(line, flush=True)
        log.write(line + "\n")
        log.flush()

    ctx = Context(0)
    for name in a.shapes.split(","):
        mol, qual, cluster = make(17, **SHAPES[name])
        emit(bam_leg(ctx, name, mol, qual, cluster, a.reps))
        from fastq_bench import consensus_leg
        letters = np.frombuffer(b"ACGT", np.uint8)[mol]
        seqs = [letters[c].tobytes() for c in cluster]
        quals = [(q + 33).tobytes() for q in qual]
        emit(consensus_leg(ctx, name, seqs, quals, a.reps))
    ctx.close()
    if not a.no_cli:
        for rec in cli_leg(a.parent_cli, a.reps):
            emit(rec)


if __name__ == "__main__":
    main()
