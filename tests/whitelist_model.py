"""Test-side model of umi_correct_umis (include/umihip.h) in plain numpy: every read's UMI is
byte-compared with every listed UMI, chunked over the reads.

    d(u, w)  positions whose bytes differ (the list holds ACGT only, so an N of a read differs from
             every listed base)
    best     the smallest d over the list; idx the smallest index that reaches it
    second   the smallest d over every entry other than idx; umi_len + 1 with one listed UMI
    matched  best <= max_mismatches and second - best >= min_distance

Also the generators of the tests' inputs: lists of distinct random UMIs, and reads that are listed
UMIs with a few substitutions, some with an N, some random."""
import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)


def as_rows(buf, umi_len):
    if isinstance(buf, (list, tuple)):
        buf = b"".join(x.encode() if isinstance(x, str) else bytes(x) for x in buf)
    if isinstance(buf, (bytes, bytearray)):
        buf = np.frombuffer(bytes(buf), np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1, umi_len)


def correct(umis, umi_len, whitelist, max_mismatches=1, min_distance=1, chunk=None):
    """dict(out, match, best, second, counts) as Context.correct_umis returns it"""
    u = as_rows(umis, umi_len)
    w = as_rows(whitelist, umi_len)
    n, n_wl = len(u), len(w)
    assert n_wl >= 1 and max_mismatches >= 0 and min_distance >= 0
    assert np.isin(w, ACGT).all() and np.isin(u, np.frombuffer(b"ACGTN", np.uint8)).all()
    best = np.zeros(n, np.int64)
    idx = np.zeros(n, np.int64)
    second = np.full(n, umi_len + 1, np.int64)
    chunk = chunk or max(1, (1 << 25) // (n_wl * umi_len))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = (u[lo:hi, None, :] != w[None, :, :]).sum(axis=2)  # [reads, entries]
        i = d.argmin(axis=1)  # (the first of equal minima: the smallest index)
        rows = np.arange(hi - lo)
        best[lo:hi] = d[rows, i]
        idx[lo:hi] = i
        if n_wl > 1:
            d[rows, i] = umi_len + 1
            second[lo:hi] = d.min(axis=1)
    matched = (best <= max_mismatches) & (second - best >= min_distance)
    match = np.where(matched, idx, -1).astype(np.int32)
    out = np.where(matched[:, None], w[idx], u).astype(np.uint8).reshape(-1)
    counts = np.array([(matched & (best == 0)).sum(), (matched & (best > 0)).sum(), (~matched).sum()], np.uint64)
    return {"out": out, "match": match, "best": best.astype(np.uint8), "second": second.astype(np.uint8),
            "counts": counts}


def random_list(rng, n_wl, umi_len):
    """n_wl distinct UMIs where 4 ** umi_len allows it (else with repeats), uint8 [n_wl * umi_len]"""
    if 4 ** min(umi_len, 16) < 4 * n_wl:  # short UMIs: draw from all of them
        codes = np.arange(4 ** umi_len)
        rng.shuffle(codes)
        codes = np.resize(codes, n_wl)
        digits = (codes[:, None] >> (2 * np.arange(umi_len))[None, :]) & 3
        return ACGT[digits].reshape(-1)
    w = ACGT[rng.integers(0, 4, (n_wl, umi_len))]
    while True:
        _, first = np.unique(w, axis=0, return_index=True)
        dup = np.setdiff1d(np.arange(n_wl), first)
        if not len(dup):
            return w.reshape(-1)
        w[dup] = ACGT[rng.integers(0, 4, (len(dup), umi_len))]


def noisy_reads(rng, whitelist, umi_len, n, n_frac=0.03, random_frac=0.05):
    """listed UMIs with 0 to 3 substitutions, n_frac of them with an N, random_frac random; uint8 [n * umi_len]"""
    w = as_rows(whitelist, umi_len)
    u = w[rng.integers(0, len(w), n)].copy()
    n_sub = rng.integers(0, 4, n)
    for s in range(3):
        hit = np.flatnonzero(n_sub > s)
        at = rng.integers(0, umi_len, len(hit))
        u[hit, at] = ACGT[(np.searchsorted(ACGT, u[hit, at]) + rng.integers(1, 4, len(hit))) % 4]
    rnd = rng.random(n) < random_frac
    u[rnd] = ACGT[rng.integers(0, 4, (int(rnd.sum()), umi_len))]
    with_n = np.flatnonzero(rng.random(n) < n_frac)
    u[with_n, rng.integers(0, umi_len, len(with_n))] = ord("N")
    return u.reshape(-1)
