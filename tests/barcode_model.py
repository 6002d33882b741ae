"""Test-side model of umi_correct_barcodes (include/umihip.h), twice, and the makers of the tests' inputs.

The function (STARsolo's 1MM rule).  Barcodes have L bases; the list holds ACGT only, without duplicates; reads
hold ACGTN; max_mismatches is 0 or 1.  Per read a status, a match and (implied) a distance:

    exact (0)      the barcode is listed: match = its index
    corrected (1)  not exact, max_mismatches 1, exactly one listed barcode differs from the read in exactly one
                   position (an N differs from every listed base): match = that barcode's index
    none (2)       neither, and no listed barcode within max_mismatches: match = -1
    ambiguous (3)  max_mismatches 1, not exact, two or more listed barcodes at distance 1: match = -1

correct() is that definition with a dict of the listed strings and the substitutions written out;
correct_bruteforce() takes all-pairs Hamming distances in numpy and reads the verdict off them."""
import functools

import numpy as np

ACGT = np.frombuffer(b"ACGT", np.uint8)
EXACT, CORRECTED, NONE, AMBIGUOUS = 0, 1, 2, 3


def as_rows(buf, L):
    if isinstance(buf, (list, tuple)):
        buf = b"".join(x.encode() if isinstance(x, str) else bytes(x) for x in buf)
    if isinstance(buf, (bytes, bytearray)):
        buf = np.frombuffer(bytes(buf), np.uint8)
    return np.ascontiguousarray(buf, dtype=np.uint8).reshape(-1, L)


def _result(match, status):
    match, status = np.asarray(match, np.int32), np.asarray(status, np.uint8)
    return {"match": match, "status": status, "counts": np.bincount(status, minlength=4).astype(np.uint64)}


def correct(reads, L, whitelist, max_mismatches=1):
    """dict(match, status, counts) as Context.correct_barcodes returns it, from the definition"""
    assert max_mismatches in (0, 1) and 1 <= L <= 32
    wl = [bytes(r) for r in as_rows(whitelist, L)]
    index = {w: i for i, w in enumerate(wl)}
    assert len(index) == len(wl) >= 1 and all(set(w) <= set(b"ACGT") for w in wl)
    match, status = [], []
    for r in (bytes(r) for r in as_rows(reads, L)):
        assert set(r) <= set(b"ACGTN")
        if r in index:
            match.append(index[r]); status.append(EXACT)
            continue
        found = set()
        n_count = r.count(b"N")
        if max_mismatches == 1 and n_count <= 1:
            # (with an N in the read every other position's substitution leaves the N, which matches nothing)
            for p in ([r.index(b"N")] if n_count else range(L)):
                for c in b"ACGT":
                    if c != r[p]:
                        v = r[:p] + bytes([c]) + r[p + 1:]
                        if v in index:
                            found.add(index[v])
        if len(found) == 1:
            match.append(found.pop()); status.append(CORRECTED)
        else:
            match.append(-1); status.append(AMBIGUOUS if found else NONE)
    return _result(match, status)


def correct_bruteforce(reads, L, whitelist, max_mismatches=1, chunk=None):
    """the same from the Hamming distance of every read to every entry"""
    u, w = as_rows(reads, L), as_rows(whitelist, L)
    n, n_wl = len(u), len(w)
    match, status = np.full(n, -1, np.int32), np.full(n, NONE, np.uint8)
    chunk = chunk or max(1, (1 << 25) // (n_wl * L))
    for lo in range(0, n, chunk):
        hi = min(n, lo + chunk)
        d = (u[lo:hi, None, :] != w[None, :, :]).sum(axis=2)
        zero, one = d == 0, d == 1
        is_exact = zero.any(axis=1)
        n_one = one.sum(axis=1) if max_mismatches == 1 else np.zeros(hi - lo, np.int64)
        st = np.where(is_exact, EXACT, np.where(n_one == 1, CORRECTED, np.where(n_one > 1, AMBIGUOUS, NONE)))
        m = np.where(is_exact, zero.argmax(axis=1), np.where(n_one == 1, one.argmax(axis=1), -1))
        match[lo:hi], status[lo:hi] = m, st
    return _result(match, status)


# ---- inputs -----------------------------------------------------------------------------------------------

def _substitute(rng, rows, at):
    """another letter at column at[i] of row i (rows of ACGT)"""
    i = np.arange(len(rows))
    rows[i, at] = ACGT[(np.searchsorted(ACGT, rows[i, at]) + rng.integers(1, 4, len(rows))) % 4]


def random_list(rng, n_wl, L, near=0.3):
    """(uint8 [n_wl, L] of distinct barcodes, pairs): a fraction `near` of the entries is another entry with one
    or two substitutions, and pairs lists those (i, j) -- what an ambiguous read is made from.  Where 4 ** L is
    small the list is drawn from all barcodes and the pairs are found by comparing all entries."""
    if 4 ** min(L, 16) < 4 * n_wl or n_wl <= 64:
        if 4 ** min(L, 16) < 4 * n_wl:
            codes = rng.permutation(4 ** L)[:n_wl]
            assert len(codes) == n_wl, "more barcodes than there are"
            w = ACGT[(codes[:, None] >> (2 * np.arange(L))[None, :]) & 3]
        else:
            while True:
                w = _distinct(rng, n_wl, L)
                for k in range(1, n_wl, 3):  # every third entry next to the one before it
                    w[k] = w[k - 1]
                    for p in rng.choice(L, size=min(L, 1 + k % 2), replace=False):
                        w[k, p] = ACGT[(np.searchsorted(ACGT, w[k, p]) + 1) % 4]
                if len(set(map(bytes, w))) == n_wl:
                    break
        d = (w[:, None, :] != w[None, :, :]).sum(axis=2)
        ii, jj = np.nonzero((d >= 1) & (d <= 2))
        return w, [(int(i), int(j)) for i, j in zip(ii, jj) if i < j]
    w = _distinct(rng, n_wl, L)
    seen = set(map(bytes, w))
    pairs = []
    for k in rng.choice(n_wl, size=int(near * n_wl), replace=False):
        src = int(rng.integers(0, n_wl))
        if src == k:
            continue
        v = w[src].copy()
        for p in rng.choice(L, size=int(rng.integers(1, 3)), replace=False):
            v[p] = ACGT[(np.searchsorted(ACGT, v[p]) + rng.integers(1, 4)) % 4]
        if bytes(v) in seen:
            continue
        seen.discard(bytes(w[k]))
        # (an earlier pair that used k as its source is stale now: dropped below by looking again)
        w[k] = v
        seen.add(bytes(v))
        pairs.append((int(k), src))
    pairs = [(i, j) for i, j in pairs if 1 <= int((w[i] != w[j]).sum()) <= 2]
    assert len(set(map(bytes, w))) == n_wl
    return w, pairs


def _distinct(rng, n_wl, L):
    w = ACGT[rng.integers(0, 4, (n_wl, L))]
    while True:
        _, first = np.unique(w, axis=0, return_index=True)
        dup = np.setdiff1d(np.arange(n_wl), first)
        if not len(dup):
            return w
        w[dup] = ACGT[rng.integers(0, 4, (len(dup), L))]


def clustered_list(L, where):
    """every 4 ** 6 variant of the first ('low') or the last ('high') 6 bases under a fixed remainder: the packed
    keys differ only in their low or only in their high bits.  Entries c and c ^ 1 are one base apart."""
    assert L >= 7 and where in ("low", "high")
    rest = ACGT[(np.arange(L - 6) * 7 + 3) % 4]
    var = ACGT[(np.arange(4 ** 6)[:, None] >> (2 * np.arange(6))[None, :]) & 3]
    rest = np.broadcast_to(rest, (4 ** 6, L - 6))
    w = np.concatenate([var, rest] if where == "low" else [rest, var], axis=1)
    return np.ascontiguousarray(w), [(c, c ^ 1) for c in range(0, 4 ** 6, 2)]


def full_list(L):
    """all 4 ** L barcodes, L <= 4"""
    assert L <= 4
    return np.ascontiguousarray(ACGT[(np.arange(4 ** L)[:, None] >> (2 * np.arange(L))[None, :]) & 3]), []


def listed_reads(rng, wl, n, pairs=(), one_n=0.06, two_n=0.03, random_frac=0.1, ambiguous=0.1):
    """uint8 [n * L]: listed barcodes with 0, 1 or 2 substitutions (about 50 / 30 / 20 %), random_frac of them
    random, one_n / two_n of them with one / two N on top, and a fraction `ambiguous` made from a pair of listed
    barcodes one or two bases apart so that both are one substitution away"""
    w = np.asarray(wl, np.uint8)
    L = w.shape[1]
    u = w[rng.integers(0, len(w), n)].copy()
    n_sub = rng.choice(3, size=n, p=[0.5, 0.3, 0.2])
    for s in range(2):
        hit = np.flatnonzero(n_sub > s)
        rows = u[hit]
        _substitute(rng, rows, rng.integers(0, L, len(hit)))
        u[hit] = rows
    rnd = rng.random(n) < random_frac
    u[rnd] = ACGT[rng.integers(0, 4, (int(rnd.sum()), L))]
    r = rng.random(n)
    for i in np.flatnonzero(r < one_n + two_n):
        k = 1 if r[i] < one_n else min(2, L)
        u[i, rng.choice(L, size=k, replace=False)] = ord("N")
    if len(pairs):
        for i in np.flatnonzero(rng.random(n) < ambiguous):
            a, b = pairs[int(rng.integers(0, len(pairs)))]
            diff = np.flatnonzero(w[a] != w[b])
            u[i] = w[a]
            if len(diff) == 1:  # through the same position: a third letter there
                u[i, diff[0]] = [c for c in ACGT if c not in (w[a, diff[0]], w[b, diff[0]])][int(rng.integers(0, 2))]
            else:               # through different positions: halfway between the two
                u[i, diff[1]] = w[b, diff[1]]
    return u.reshape(-1)


# the hand-made ambiguous pairs: (list, read)
AMBIGUOUS_SAME_POSITION = (["AAAA", "CAAA"], "GAAA")
AMBIGUOUS_DIFFERENT_POSITIONS = (["AA", "CC"], "CA")


# ---- the inputs of the GPU tests (tests/test_gpu_barcodes.py), checked without a GPU by
# tests/test_barcode_model_cpu.py.  name -> (L, list [n_wl, L], reads [n * L]); `kind` says what the input can hold:
#   "all"    at least 8 reads of each of the four statuses
#   "full"   a full list: every read without N is exact, one N is ambiguous; no two-N reads are made, so there is
#            neither "none" nor "corrected"
#   "small"  L <= 2 or n_wl <= 2, where not every status can occur (one entry: nothing is ambiguous; L = 1: nothing is
#            further than one base from the list): whatever occurs
N_READS = (0, 1, 63, 64, 65, 10000)


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    cases = {}

    def add(name, kind, L, wl_pairs, n, seed, **kw):
        wl, pairs = wl_pairs
        rng = np.random.default_rng(seed)
        cases[name] = (kind, L, wl, listed_reads(rng, wl, n, pairs, **kw))

    for L in (1, 2, 15, 16, 17, 31, 32):
        rng = np.random.default_rng(100 + L)
        n_wl = {1: 3, 2: 12}.get(L, 5003)
        add("L%d" % L, "small" if L <= 2 else "all", L, random_list(rng, n_wl, L), 2000, 200 + L)
    for n_wl in (1, 2, 64):
        rng = np.random.default_rng(300 + n_wl)
        add("n_wl%d" % n_wl, "small" if n_wl <= 2 else "all", 16, random_list(rng, n_wl, 16), 1500, 400 + n_wl)
    add("clustered_low", "all", 16, clustered_list(16, "low"), 3000, 501)
    add("clustered_high", "all", 16, clustered_list(16, "high"), 3000, 502)
    add("clustered_high_L32", "all", 32, clustered_list(32, "high"), 3000, 503)
    add("full3", "full", 3, full_list(3), 1000, 504, two_n=0.0)
    rng = np.random.default_rng(600)
    add("reads10000", "all", 16, random_list(rng, 4999, 16), 10000, 601)
    return cases


@functools.lru_cache(maxsize=None)
def expected(name, max_mismatches):
    """the model's answer for a GPU input, computed once per process"""
    _, L, wl, reads = gpu_inputs()[name]
    return correct(reads, L, wl, max_mismatches)
