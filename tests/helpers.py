"""Shared helpers for the tests: seeded UMI bucket generators and an independent
brute-force model of the collapse (numpy, written from the algorithm's
definition -- not from the oracle's code)."""
import numpy as np

ALPHA = np.frombuffer(b"ACGT", dtype=np.uint8)


def hamming_matrix(umis):
    """Hamming distance over the 5-letter alphabet straight from the characters."""
    a = np.array([np.frombuffer(u.encode(), dtype=np.uint8) for u in umis])
    return (a[:, None, :] != a[None, :, :]).sum(-1)


def thr_f32(p, f):
    return int(np.float32(p) * np.float32(f + 1))


def brute_directional(umis, freq, k, p):
    """Survivors (input indices, output order) and root per input index.
    Definition: process UMIs in stable freq-descending order; a UMI still present
    becomes a root and removes everything reachable through edges u->v with
    dist(u,v)<=k and freq[v] <= thr(freq[u])."""
    n = len(umis)
    order = sorted(range(n), key=lambda i: (-freq[i], i))
    if n == 0:
        return [], []
    d = hamming_matrix(umis)
    thr = np.array([thr_f32(p, f) for f in freq])
    fr = np.array(freq)
    adj = (d <= k) & (fr[None, :] <= thr[:, None])
    np.fill_diagonal(adj, False)
    present = np.ones(n, bool)
    root_of = list(range(n))
    surv = []
    for r in order:
        if not present[r]:
            continue
        surv.append(r)
        present[r] = False
        frontier = [r]
        while frontier:
            nxt = []
            for u in frontier:
                vs = np.nonzero(adj[u] & present)[0]
                present[vs] = False
                for v in vs:
                    root_of[v] = r
                nxt.extend(vs.tolist())
            frontier = nxt
    return surv, root_of


def brute_adjacency(umis, freq, k, max_freq):
    n = len(umis)
    order = sorted(range(n), key=lambda i: (-freq[i], i))
    if n == 0:
        return [], []
    d = hamming_matrix(umis)
    fr = np.array(freq)
    present = np.ones(n, bool)
    root_of = list(range(n))
    surv = []
    for r in order:
        if not present[r]:
            continue
        surv.append(r)
        present[r] = False
        vs = np.nonzero((d[r] <= k) & (fr <= max_freq) & present)[0]
        present[vs] = False
        for v in vs:
            root_of[v] = r
    return surv, root_of


def random_bucket(rng, n_mol, L, err=0.05, mean_copies=3.0, n_frac=0.0):
    """Molecule model: n_mol true UMIs, geometric copy counts, per-base errors.
    Returns (umis in first-appearance order, freq)."""
    seen = {}
    for _ in range(n_mol):
        true = rng.choice(ALPHA, L)
        copies = int(rng.geometric(1.0 / mean_copies))
        for _ in range(copies):
            u = true.copy()
            mut = rng.random(L) < err
            for i in np.nonzero(mut)[0]:
                u[i] = rng.choice(ALPHA[ALPHA != u[i]])
            if n_frac:
                u[rng.random(L) < n_frac] = ord("N")
            s = u.tobytes().decode()
            seen[s] = seen.get(s, 0) + 1
    umis = list(seen.keys())
    return umis, [seen[u] for u in umis]


def clustered_bucket(rng, n_target, L, n_frac):
    """~n_target distinct UMIs: a few centres with many 1-2 error neighbours + random ones."""
    out = {}
    centres = rng.choice(ALPHA, (max(1, n_target // 40), L))
    while len(out) < n_target:
        if rng.random() < 0.7:
            u = centres[rng.integers(len(centres))].copy()
            for _ in range(int(rng.integers(0, 3))):
                u[rng.integers(L)] = rng.choice(ALPHA)
        else:
            u = rng.choice(ALPHA, L)
        if n_frac and rng.random() < n_frac:
            u[rng.integers(L)] = ord("N")
        s = u.tobytes()
        out[s] = out.get(s, 0) + int(rng.geometric(0.4))
        if len(out) >= 4 ** L - 1 and L < 6:
            break
    umis = list(out.keys())
    freq = np.array([out[u] for u in umis])
    order = np.lexsort((np.arange(len(umis)), -freq))
    return [umis[i].decode() for i in order], freq[order].tolist()


def canonical(umis, freq):
    """Stable freq-descending order (the rank order the batched ABI expects)."""
    order = sorted(range(len(umis)), key=lambda i: (-freq[i], i))
    return [umis[i] for i in order], [freq[i] for i in order], order


# ---- shipped library vs development build ---------------------------------------------------------
# The round-1 tile kernels and their options live in libumihip_dev.so only (make dev, -DUMIHIP_DEV).
# Run the legacy cross-checks with UMIHIP_LIB=<repo>/umi_collapse_rs_amd/libumihip_dev.so; under the
# shipped library they are skipped and option sets that name a legacy option are left out.
LEGACY_OPTS = {"prune", "bs_unit", "bs_sorted", "bs_tables", "two_phase", "bs_col_chunk", "bs_tab_min_run",
               "bs_transposed", "bs_tab_waves", "bitslice", "ovf_capacity"}


def is_dev_build():
    import os
    from umi_collapse_rs_amd import _lib
    return os.path.basename(_lib.LIB_PATH) == "libumihip_dev.so"


def usable(opts):
    """Can this option set be applied to the library under test?"""
    return is_dev_build() or not (set(opts) & LEGACY_OPTS)


def legacy_mark():
    import pytest
    return pytest.mark.skipif(not is_dev_build(), reason="round-1 tile kernels: development build only "
                                                          "(UMIHIP_LIB=.../libumihip_dev.so)")


def stage_model(pos, umis, score, merge):
    """deduplicate_sam.rs:148-176 + the canonical order, straight from the definition (a dict per
    position, plain Python: for a few 10^4 reads): positions by first appearance, a position's UMIs
    by freq descending then first appearance; per UMI its freq and the read that stands for it
    (merge 0: the first; 1: the highest score, the earlier on ties).  Returns (list of UMI strings,
    freq, rep, bucket_off)."""
    buckets = {}
    for i, (p, u) in enumerate(zip(pos, umis)):
        d = buckets.setdefault(int(p), {})
        e = d.get(u)
        sc = 0 if score is None else int(score[i])
        if e is None:
            d[u] = [1, i, sc]  # freq, rep, score of the rep
        else:
            e[0] += 1
            if merge and not (e[2] >= sc):
                e[1], e[2] = i, sc
    out_umis, freq, rep, off = [], [], [], [0]
    for p, d in buckets.items():  # (dicts keep insertion order: first appearance)
        items = sorted(d.items(), key=lambda kv: -kv[1][0])  # stable
        out_umis += [u for u, _ in items]
        freq += [e[0] for _, e in items]
        rep += [e[1] for _, e in items]
        off.append(len(out_umis))
    return out_umis, np.array(freq, np.int32), np.array(rep, np.uint64), np.array(off, np.uint64)


def grouped_stage_model(align, group, umis, score, umi_len, merge, gbits):
    """umi_stage_reads_grouped[_wide]: buckets = (align, group & mask) by first appearance, then the
    oracle's staging (stage_model above for UMIs of more than one key word)"""
    import oracle as orc
    gm = np.uint64((1 << gbits) - 1) if gbits < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    pairs = np.stack([align, group & gm if gbits else np.zeros_like(group)], axis=1)
    _, first, inv = np.unique(pairs, axis=0, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    bucket = rank[inv.reshape(-1)]
    if umi_len <= 21:
        return orc.stage_reads(bucket, umis, score, umi_len, merge=merge)
    u = [bytes(umis[i * umi_len:(i + 1) * umi_len]).decode() for i in range(len(align))]
    w_umis, freq, rep, off = stage_model(bucket, u, score, merge)
    keys, nmask = orc.encode_keys_wide(w_umis)
    return dict(keys=keys, nmask=nmask, freq=freq, rep=rep, bucket_off=off)


# ---- inputs where k is the limit that decides (tests of k > 3) -------------------------------------
# Random UMIs sit ~0.75 L substitutions apart: a random bucket has no pair anywhere near k = 6.  These
# buckets are built from centres with copies at planted distances k-1 .. k+2, their substitution sites
# chosen against the pigeonhole partition [j L / P, (j + 1) L / P), P = k + 1, that the segment index
# and the whole-read partition use.

def part_bounds(L, P):
    return [j * L // P for j in range(P + 1)]


def _planted_sites(rng, L, d, P, style, part_len):
    """d distinct substitution sites.  "last": one per part, parts 0, 1, ... first (d = k leaves only
    the last part equal: the tightest case of the pigeonhole; d = k + 1 leaves none); "first": parts
    P-1, P-2, ... (d = k leaves only part 0 equal); "rand": anywhere.  Parts are cut from the first
    part_len bases; sites beyond the parts' count are random."""
    d = min(d, L)
    if style == "rand" or P > part_len:
        return sorted(rng.choice(L, d, replace=False).tolist())
    b = part_bounds(part_len, P)
    order = list(range(P)) if style == "last" else list(range(P - 1, -1, -1))
    sites = []
    for j in order[:d]:
        lo, hi = b[j], b[j + 1]
        sites.append(int(rng.choice([lo, hi - 1, int(rng.integers(lo, hi))])))  # part edges too
    rest = [i for i in range(L) if i not in sites]
    sites += rng.choice(rest, d - len(sites), replace=False).tolist() if d > len(sites) else []
    return sorted(sites)


def planted_bucket(rng, n, L, k, n_frac=0.0, n_sites=(), part_len=None):
    """n distinct UMIs (fewer when 5^L runs out) in rank order with their freq: centres, and per
    centre copies at distance exactly k, k+1, k-1, k+2 (clipped to 1..L) in the styles of
    _planted_sites; with n_frac some copies carry an N at one of their substituted sites, at one of
    n_sites (the bases that straddle key words) when given.  Frequencies: centres from {1, 3, 5, 9, 20},
    copies from {1, 1, 2, 3, 5}, so that at p = 0.5 a centre-copy pair is symmetric (1, 1), one-way
    (5, 2) or no edge at all (3, 3)."""
    part_len = min(part_len or L, L)
    P = min(k, 4 * L) + 1  # (k beyond every distance: the parts no longer matter)
    out = {}
    tries = 0
    while len(out) < n and tries < 20 * n + 100:
        tries += 1
        c = rng.choice(ALPHA, L)
        # (the first centre and its first copy, at exactly k, are a one-way pair: a bucket of two entries
        # already has a removal that only a distance-k edge makes)
        out.setdefault(c.tobytes(), 9 if not out else int(rng.choice([1, 3, 5, 9, 20])))
        for d in (k, k + 1, k - 1, k + 2):
            if d < 1:
                continue
            for style in ("last", "first", "rand"):
                if len(out) >= n:
                    break
                u = c.copy()
                sites = _planted_sites(rng, L, d, P, style, part_len)
                for i in sites:
                    u[i] = rng.choice(ALPHA[ALPHA != c[i]])
                if n_frac and rng.random() < 12 * n_frac:  # (a copy, not a base: ~1 % of the bases of a 12-mer)
                    at = [i for i in n_sites if i < L]
                    i = int(rng.choice(at)) if at and rng.random() < 0.5 else int(rng.choice(sites))
                    if i not in sites:  # keep the planted distance: an N where a substitution was
                        u[sites[0]] = c[sites[0]]
                    u[i] = ord("N")
                out.setdefault(u.tobytes(), 1 if len(out) == 1 else int(rng.choice([1, 1, 2, 3, 5])))
    umis = [u.decode() for u in out]
    umis, freq, _ = canonical(umis, list(out.values()))
    return umis[:n], freq[:n]


def dist_blocks(keys, nm, rows=256):
    """The reference's distance (bitset.rs:77-91 per word, summed, halved) of every pair of one bucket,
    as (first row, int64 [rows, n]) blocks.  keys / nm: uint64 [n] or [n, w]."""
    keys = keys.reshape(len(keys), -1)
    nm = nm.reshape(len(nm), -1)
    for r0 in range(0, len(keys), rows):
        x = nm[r0:r0 + rows, None, :] ^ nm[None, :, :]
        v = np.bitwise_count(x | (keys[r0:r0 + rows, None, :] ^ keys[None, :, :])).astype(np.int64) \
            - np.bitwise_count(x).astype(np.int64) // 3
        yield r0, v.sum(-1) // 2


SIZE_CLASSES = ((2, 128), (129, 1024), (1025, 1 << 31))  # fused kernel / chunk kernel / deep


def limit_census(keys, nm, freq, off, k, p=0.5):
    """Per size class that the batch contains: pairs at distance exactly k and exactly k + 1, and of
    the former the symmetric / one-way / no-edge ones under the directional test.  dict class -> counts."""
    freq = np.asarray(freq, np.int64)
    out = {}
    for b in range(len(off) - 1):
        s, e = int(off[b]), int(off[b + 1])
        if e - s < 2:
            continue
        cls = next(c for c in SIZE_CLASSES if c[0] <= e - s <= c[1])
        c = out.setdefault(cls, dict(at_k=0, at_k1=0, sym=0, one_way=0, neither=0))
        f = freq[s:e]
        thr = np.array([thr_f32(p, int(x)) for x in f])
        for r0, d in dist_blocks(keys[s:e], nm[s:e]):
            upper = np.arange(e - s)[None, :] > (r0 + np.arange(len(d)))[:, None]
            at = (d == k) & upper
            c["at_k"] += int(at.sum())
            c["at_k1"] += int(((d == k + 1) & upper).sum())
            fwd = f[None, :] <= thr[r0:r0 + len(d), None]
            bwd = f[r0:r0 + len(d), None] <= thr[None, :]
            c["sym"] += int((at & fwd & bwd).sum())
            c["one_way"] += int((at & (fwd ^ bwd)).sum())
            c["neither"] += int((at & ~fwd & ~bwd).sum())
    return out


def assert_k_decides(census, umi_len, k, kept_k, kept_km1):
    """The two conditions a large-k case meets before the library is called: every size class has a
    pair at exactly k and one at exactly k + 1 (where the length allows such a distance at all), and
    the reference removes something through a distance-k edge (its result at k - 1 differs).  For
    k above the length the largest distance, umi_len, stands in for k."""
    kk = min(k, umi_len)
    assert census, "no bucket of two or more entries"
    for cls, c in census.items():
        assert c["at_k"] > 0, (cls, c)
        if kk + 1 <= umi_len:
            assert c["at_k1"] > 0, (cls, c)
    assert sum(c["sym"] for c in census.values()) and sum(c["one_way"] for c in census.values()) \
        and sum(c["neither"] for c in census.values()), census
    assert not np.array_equal(kept_k, kept_km1), "no removal goes through a distance-k edge"


# one-word cases of tests/test_gpu_large_k.py (checked on the CPU in tests/test_large_k_inputs_cpu.py)
ONE_WORD_BOUNDARY = [(21, 6), (21, 7), (20, 6), (18, 5), (17, 5), (15, 4), (14, 4), (12, 3), (11, 3)]
ONE_WORD_HUGE = [(L, k) for L in (6, 12, 21) for k in (L - 1, L, L + 1, 2 ** 30 - 1, 2 ** 30, 2 ** 31 - 1)]
ONE_WORD_SIZES = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1023, 1025, 3000]
# k >= L - 1 makes (nearly) every pair of a bucket an edge candidate: one bucket per kernel boundary there
ONE_WORD_SIZES_HUGE = [0, 1, 2, 63, 64, 65, 127, 128, 129, 511, 1025]


def seg_index_applies(umi_len, k):
    """The planner's rule (umihip_plan.hpp), restated: k + 1 parts, 8 at most, of 3 bases or more."""
    return k + 1 <= 8 and umi_len // (k + 1) >= 3


def one_word_batch(L, k, n_frac, seed=0):
    """The buckets of one one-word case: every size of ONE_WORD_SIZES in one call (of ONE_WORD_SIZES_HUGE
    where k >= L - 1; fewer entries where 4^L runs out)."""
    rng = np.random.default_rng(100000 + 1000 * L + min(k, 99) + seed)
    import oracle as orc
    keys, nm, fr, off = [], [], [], [0]
    for n in (ONE_WORD_SIZES_HUGE if k >= L - 1 else ONE_WORD_SIZES):
        n = min(n, 4 ** L // 3)
        umis, freq = planted_bucket(rng, n, L, min(k, L), n_frac) if n else ([], [])
        kk, mm = orc.encode_keys(umis)
        keys.append(kk); nm.append(mm); fr.extend(freq); off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


WIDE_CASES = [(L, k) for L in (22, 24, 43, 64, 85) for k in (4, 5, 6, 7, 8, L, 2 ** 31 - 1)]
WIDE_STRADDLE = (21, 42)


def wide_batch(L, k, n_frac=0.01, seed=0):
    """Buckets of one wide case: fused-range sizes, one for the chunk kernel, one deep (2,000 entries).  The parts are cut from the first word's 21 bases, where the segment
    index looks; N also at the straddling bases 21 and 42."""
    import oracle as orc
    rng = np.random.default_rng(200000 + 1000 * L + min(k, 99) + seed)
    keys, nm, fr, off = [], [], [], [0]
    for n in (2, 64, 128, 400, 2000):
        umis, freq = planted_bucket(rng, n, L, min(k, L), n_frac, WIDE_STRADDLE, part_len=21)
        kk, mm = orc.encode_keys_wide(umis)
        keys.append(kk); nm.append(mm); fr.extend(freq); off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


SEQ_CASES = sorted({(L, k) for L in (64, 100, 150, 256) for k in (4, 7, 8, 16, L, 400, 401, 2 ** 31 - 1)}
                   | {(150, 17), (150, 18), (256, 31), (256, 32)})
SEQ_STRADDLE = (21, 42, 85, 106, 149, 170, 213, 234)


def seq_partitioned(L, k):
    """umi_dedup_seqs cuts a bucket of 512 entries or more into k + 1 parts while a part has 8 bases
    (k clamped to 400 first)."""
    return L // (min(k, 400) + 1) >= 8


def seq_buckets(L, k, n_frac=0.01, seed=0, sizes=(2, 200, 600)):
    """[(seqs as bytes, freq)] of one whole-read case: a pair, a bucket below 512 entries (all pairs) and one above
    (partitioned where seq_partitioned)."""
    rng = np.random.default_rng(300000 + 1000 * L + min(k, 999) + seed)
    out = []
    for n in sizes:
        umis, freq = planted_bucket(rng, n, L, min(k, L), n_frac, SEQ_STRADDLE)
        out.append(([u.encode() for u in umis], freq))
    return out


def dense_clusters(rng, n_centres, copies, L, d_max):
    """Centres with many copies within d_max / 2 substitutions each (any two copies of a centre are within
    d_max): buckets whose edge lists run to a few 10^5 entries.  Rank order, freq."""
    out = {}
    for _ in range(n_centres):
        c = rng.choice(ALPHA, L)
        out.setdefault(c.tobytes(), int(rng.choice([3, 5, 9])))
        for _ in range(copies):
            u = c.copy()
            for i in rng.choice(L, int(rng.integers(1, d_max // 2 + 1)), replace=False):
                u[i] = rng.choice(ALPHA[ALPHA != c[i]])
            out.setdefault(u.tobytes(), int(rng.choice([1, 1, 2, 3])))
    umis, freq, _ = canonical([u.decode() for u in out], list(out.values()))
    return umis, freq


def equal_parts_of_pairs(seqs, pairs, P):
    """For every pair (i, j) of one bucket of equal-length reads: the set of parts [j L / P, (j + 1) L / P)
    on which the two reads agree exactly, as a frozenset."""
    L = len(seqs[0])
    arr = np.frombuffer(b"".join(seqs), np.uint8).reshape(len(seqs), L)
    b = part_bounds(L, P)
    out = []
    for i, j in pairs:
        ne = arr[i] != arr[j]
        out.append(frozenset(p for p in range(P) if not ne[b[p]:b[p + 1]].any()))
    return out


def assert_tight_pigeonhole(seqs, pairs, P):
    """A partitioned bucket holds a pair within k that agrees on the last part only and one that agrees on
    part 0 only: the two ends of the exactly-once masks (bits 0 and P - 1)."""
    eq = equal_parts_of_pairs(seqs, pairs, P)
    assert frozenset([P - 1]) in eq, "no pair within k equal in part %d only" % (P - 1)
    assert frozenset([0]) in eq, "no pair within k equal in part 0 only"


# ---- inputs for the pair lists themselves (tests/pair_list_model.py) --------------------------------
# The segment index bins an entry, in every part, by the part's leading bases (plan_segment of umihip_plan.hpp:
# as many as keep a sub-bucket around 32-64 entries, 2 at the least, the part's length at the most), and a
# pair is found by every part in whose bin its two entries meet.

def seg_bin_bases(n, L, k):
    """[(first base, bases that index the bins)] of the k + 1 parts of a bucket of n entries, restated."""
    P = k + 1
    cap = max(2, min(12, (int(n).bit_length() - 1 - 4) // 2))
    b = part_bounds(L, P)
    return [(b[j], min(b[j + 1] - b[j], cap)) for j in range(P)]


def seg_probe_entries(rng, L, k, part_len=None):
    """dict UMI -> freq of pairs that only one route through the segment index finds, and of pairs that
    several do.  Per part j a centre and a copy with one substitution at the first base of every other part:
    distance exactly k, equal on part j, in one bin nowhere else.  Then a centre and a copy that differ in
    the last base of the last part alone (one bin shared per part: every part finds the pair, the list wants
    it once) and, for k >= 2, one with a substitution at the first base of every part but the first two.
    Parts are cut from the first part_len bases.  Frequencies make the pairs symmetric, one-way and
    not permitted at all in turn (p = 0.5)."""
    part_len = min(part_len or L, L)
    P = k + 1
    b = part_bounds(part_len, P)
    fr = [(1, 1), (5, 2), (3, 3)]
    out = {}

    def put(c, sites, t):
        u = c.copy()
        for i in sites:
            u[i] = rng.choice(ALPHA[ALPHA != c[i]])
        out.setdefault(c.tobytes().decode(), fr[t % 3][0])
        out.setdefault(u.tobytes().decode(), fr[t % 3][1])

    t = 0
    for rep in range(3):  # (each kind of pair under each of the three freq relations)
        for j in range(P):
            put(rng.choice(ALPHA, L), [b[i] for i in range(P) if i != j], t + rep)
            t += 1
        put(rng.choice(ALPHA, L), [b[P] - 1], t + rep)
        t += 1
        if k >= 2:
            put(rng.choice(ALPHA, L), [b[i] for i in range(2, P)], t + rep)
            t += 1
    return out


def merged_bucket(*parts):
    """One bucket of several (umis, freq) lists or dicts: the first freq of a UMI holds; rank order."""
    out = {}
    for p in parts:
        for u, f in (p.items() if isinstance(p, dict) else zip(*p)):
            out.setdefault(u, int(f))
    umis, freq, _ = canonical(list(out), list(out.values()))
    return umis, freq
