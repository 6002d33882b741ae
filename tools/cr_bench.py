"""umi_dedup_batch_cr_device on resident data, with umi_dedup_batch_device (algo dir, k = 1) on the same arrays
beside it: the directional call is the yardstick, called in turn in the same process.  One JSON line per measurement
on stdout and, with --record, appended to profiles/cr_bench.jsonl (--out: another file).

  shapes: 2 x 10^7 buckets of one to three entries; 10^5 buckets of 100 entries; one position of 10^6 entries;
      12-base UMIs without N, seeded, one-mismatch neighbours planted in every bucket.
  Each call is timed with device events around it (it synchronises inside): median of --reps calls after a warm-up
      call, the two calls alternating.  The yardstick's median is taken three times; the largest difference between
      the three is the run-to-run spread quoted.
  "cr_small_max": 32, 128 and 512 on the 10^5 x 100 shape (the tiny buckets lie under every candidate, the single
      position above every one).
  Checked, not timed: target[] of a sample of entries (whole buckets of the first two shapes) against the rule
      stated over a dict of the bucket in numpy / Python.

usage: python tools/cr_bench.py [--reps 50] [--only NAME] [--scale 1.0] [--record] [--out FILE]"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from umi_collapse_rs_amd import Context  # noqa: E402

UMI_LEN = 12
CODE = np.array([0, 6, 3, 5], np.uint64)  # A C G T in the keys' 3-bit code; two bits a base here, base 0 lowest


def keys_of(v):
    """3-bit keys of UMIs held as 24-bit numbers, two bits a base"""
    k = np.zeros(len(v), np.uint64)
    for b in range(UMI_LEN):
        k |= CODE[(v >> np.uint32(2 * b)) & np.uint32(3)] << np.uint64(3 * b)
    return k


def mutate(v, pos, rng):
    """another base at position pos of every UMI"""
    add = rng.integers(1, 4, len(v)).astype(np.uint32)
    old = (v >> (2 * pos)) & np.uint32(3)
    return (v & ~(np.uint32(3) << (2 * pos))) | (((old + add) & np.uint32(3)) << (2 * pos))


def tiny_buckets(n_buckets, seed):
    """buckets of one to three entries: a random UMI, and copies of it with one base changed (half of them) or three
    (the rest), at places that keep the entries distinct; counts that fall or tie along the bucket"""
    rng = np.random.default_rng(seed)
    size = rng.integers(1, 4, n_buckets)
    off = np.zeros(n_buckets + 1, np.uint64)
    off[1:] = np.cumsum(size)
    n = int(off[-1])
    bucket = np.repeat(np.arange(n_buckets), size)
    rank = (np.arange(n) - off[:-1].astype(np.int64)[bucket]).astype(np.uint32)
    first = rng.integers(0, 1 << 24, n_buckets, dtype=np.uint32)[bucket]
    p1 = rng.integers(0, UMI_LEN, n_buckets).astype(np.uint32)[bucket]
    pos = (p1 + np.uint32(5) * (rank == 2)) % np.uint32(UMI_LEN)   # the third entry's place: another one
    v = np.where(rank > 0, mutate(first, pos, rng), first)
    three = (rng.random(n) < 0.5) & (rank > 0)
    for d in (1, 2):
        v = np.where(three, mutate(v, (pos + np.uint32(d)) % np.uint32(UMI_LEN), rng), v)
    f0 = rng.integers(1, 5, n_buckets)[bucket]
    step = rng.integers(0, 2, n_buckets)[bucket]
    freq = np.maximum(1, f0 - step * rank.astype(np.int64)).astype(np.int32)
    return dict(v=v, keys=keys_of(v), freq=freq, bucket_off=off)


def hundred_buckets(n_buckets, seed):
    """buckets of 100: 25 molecules, told apart by their last three bases, each with three copies that differ from
    it in one of the first nine; the molecules' counts are drawn, the copies have one read; rank order"""
    rng = np.random.default_rng(seed)
    n = 100 * n_buckets
    mol = np.tile(np.repeat(np.arange(25, dtype=np.uint32), 4), n_buckets)
    copy = np.tile(np.arange(4, dtype=np.uint32), 25 * n_buckets)
    centre = np.repeat(rng.integers(0, 1 << 18, 25 * n_buckets, dtype=np.uint32), 4) | (mol << np.uint32(18))
    p = np.repeat(rng.integers(0, 3, 25 * n_buckets).astype(np.uint32), 4) + np.uint32(3) * (copy - (copy > 0))
    v = np.where(copy > 0, mutate(centre, p, rng), centre)
    freq = np.where(copy > 0, 1, np.repeat(rng.integers(1, 20, 25 * n_buckets), 4)).astype(np.int32)
    order = np.lexsort((-freq, np.arange(n) // 100))
    off = (np.arange(n_buckets + 1, dtype=np.uint64) * np.uint64(100))
    return dict(v=v[order], keys=keys_of(v[order]), freq=freq[order], bucket_off=off)


def one_position(n, seed):
    rng = np.random.default_rng(seed)
    v = rng.choice(1 << 24, n, replace=False).astype(np.uint32)
    freq = np.sort(rng.geometric(0.3, n).astype(np.int32))[::-1].copy()
    return dict(v=v, keys=keys_of(v), freq=freq, bucket_off=np.array([0, n], np.uint64))


def string_of(v):
    return tuple((int(v) >> (2 * b)) & 3 for b in range(UMI_LEN))   # A < C < G < T, base 0 first


def rule_targets(v, freq, start, end, sample):
    """target (call index) of the sampled entries of the bucket [start, end): the rule over a dict of the bucket"""
    at = {int(x): start + i for i, x in enumerate(v[start:end])}
    out = {}
    for i in sample:
        s = int(v[i])
        best = (int(freq[i]), string_of(s), i)
        for b in range(UMI_LEN):
            for c in range(4):
                t = (s & ~(3 << (2 * b))) | (c << (2 * b))
                j = at.get(t)
                if j is not None and t != s:
                    best = max(best, (int(freq[j]), string_of(t), j))
        out[i] = best[2]
    return out


def timed(calls, reps):
    """medians (ms) of the calls, alternating, after a warm-up round; and the last stats of each"""
    import torch

    def once(call):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        st = call()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1), st
    for c in calls:
        once(c)
    ms, st = [[] for _ in calls], [None] * len(calls)
    for _ in range(reps):
        for i, c in enumerate(calls):
            t, st[i] = once(c)
            ms[i].append(t)
    return [float(np.median(m)) for m in ms], [float(np.min(m)) for m in ms], st


def measure(name, d, reps, small_maxes, sample_buckets):
    import torch
    keys = torch.from_numpy(d["keys"].view(np.int64).copy()).to("cuda:0")
    freq = torch.from_numpy(np.ascontiguousarray(d["freq"], np.int32)).to("cuda:0")
    off = np.ascontiguousarray(d["bucket_off"], np.uint64)
    n = len(d["keys"])
    kept = torch.zeros(n, dtype=torch.uint8, device="cuda:0")
    root = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    target = torch.zeros(n, dtype=torch.int32, device="cuda:0")
    ctx = Context(0)
    yard = lambda: ctx.dedup_batch_device(keys.data_ptr(), 0, freq.data_ptr(), off, UMI_LEN, kept.data_ptr(), root.data_ptr(), k=1)
    cr = lambda: ctx.dedup_batch_cr_device(keys.data_ptr(), 0, freq.data_ptr(), off, UMI_LEN, kept.data_ptr(), root.data_ptr(),
                                           target.data_ptr())
    out = {"what": "umi_dedup_batch_cr_device", "shape": name, "entries": n, "buckets": len(off) - 1, "bases": UMI_LEN, "reps": reps}
    yard_medians = []
    for small_max in small_maxes:
        if small_max is not None:
            ctx.set_option("cr_small_max", small_max)
        (m_cr, m_y), (lo_cr, lo_y), (st_cr, st_y) = timed([cr, yard], reps)
        yard_medians.append(m_y)
        tag = "" if small_max is None else "_small_max_%d" % small_max
        out["ms_cr_median" + tag] = round(m_cr, 3)
        out["ms_cr_min" + tag] = round(lo_cr, 3)
        out["cr_over_dir" + tag] = round(m_cr / max(m_y, 1e-6), 3)
    while len(yard_medians) < 3:   # (three medians of the yardstick for its spread)
        yard_medians.append(timed([yard], reps)[0][0])
    out["ms_dir_medians"] = [round(x, 3) for x in yard_medians]
    out["ms_dir_spread"] = round(max(yard_medians) - min(yard_medians), 3)
    out.update(n_kept_cr=int(st_cr["n_kept"]), n_edges_cr=int(st_cr["n_edges"]), n_kept_dir=int(st_y["n_kept"]),
               n_pairs=int(st_cr["n_pairs"]))
    # the outputs against the rule, on a sample
    cr()
    torch.cuda.synchronize()
    got_t = target.cpu().numpy().view(np.uint32)
    got_k = kept.cpu().numpy()
    rng = np.random.default_rng(1)
    checked = wrong = 0
    nb = len(off) - 1
    if nb == 1:
        sample = [int(x) for x in rng.choice(n, 2000, replace=False)]
        want = rule_targets(d["v"], d["freq"], 0, n, sample)
        wrong = sum(int(got_t[i]) != want[i] for i in sample)
        checked = len(sample)
    else:
        for b in (int(x) for x in rng.choice(nb, sample_buckets, replace=False)):
            s, e = int(off[b]), int(off[b + 1])
            want = rule_targets(d["v"], d["freq"], s, e, range(s, e))
            wrong += sum(int(got_t[i]) != want[i] for i in range(s, e))
            wrong += sum(int(got_k[i]) != int(i in set(want.values())) for i in range(s, e))
            checked += e - s
    out.update(sample_entries=checked, sample_mismatches=wrong)
    ctx.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--only", default="", help="one shape's name")
    ap.add_argument("--scale", type=float, default=1.0, help="shrink every shape (a rehearsal)")
    ap.add_argument("--record", action="store_true", help="append the lines to the output file")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "cr_bench.jsonl"))
    a = ap.parse_args()
    sc = lambda x: max(1, int(x * a.scale))
    shapes = [("20M_buckets_of_1_to_3", lambda: tiny_buckets(sc(20_000_000), 1), [None], 2000),
              ("100k_buckets_of_100", lambda: hundred_buckets(sc(100_000), 2), [32, 128, 512], 50),
              ("one_position_1M", lambda: one_position(sc(1_000_000), 3), [None], 0)]
    for name, make, small_maxes, sample in shapes:
        if a.only and a.only != name:
            continue
        s = json.dumps(measure(name, make(), a.reps, small_maxes, sample))
        print(s, flush=True)
        if a.record:
            with open(a.out, "a") as f:
                f.write(s + "\n")


if __name__ == "__main__":
    main()
