"""Model of the collapse by Levenshtein distance (umi_dedup_batch_edit, --distance edit), independent of the
library: the distance by full dynamic programming on the characters, the collapse from its definition
(helpers.brute_directional / brute_adjacency with the distance matrix swapped), and the inputs of the GPU
tests -- UMIs that differ by a shift, which is what the Hamming distance misses."""
import numpy as np

from helpers import ALPHA, canonical, thr_f32

CODE_OF = {"A": 0, "T": 5, "C": 6, "G": 3, "N": 4}  # src/utils/read.rs:23-31
LETTER_OF = {v: k for k, v in CODE_OF.items()}


def levenshtein(a, b):
    """Substitution, insertion, deletion at cost 1 each; two letters match iff they are the same letter."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[-1]


def hamming(a, b):
    return sum(x != y for x, y in zip(a, b))


def edit_matrix(umis):
    """levenshtein() of every pair of equal-length UMIs: the same recurrence, one DP cell at a time for all
    pairs at once."""
    n = len(umis)
    if n == 0:
        return np.zeros((0, 0), np.int64)
    a = np.array([np.frombuffer(u.encode(), dtype=np.uint8) for u in umis])
    L = a.shape[1]
    prev = np.broadcast_to(np.arange(L + 1, dtype=np.int16), (n, n, L + 1)).copy()  # DP row 0: d(0, j) = j
    for i in range(1, L + 1):
        cur = np.empty_like(prev)
        cur[:, :, 0] = i
        for j in range(1, L + 1):
            cur[:, :, j] = np.minimum(np.minimum(prev[:, :, j] + 1, cur[:, :, j - 1] + 1),
                                      prev[:, :, j - 1] + (a[:, None, i - 1] != a[None, :, j - 1]))
        prev = cur
    return prev[:, :, L].astype(np.int64)


def hamming_matrix(umis):
    a = np.array([np.frombuffer(u.encode(), dtype=np.uint8) for u in umis])
    return (a[:, None, :] != a[None, :, :]).sum(-1)


def letter_counts(u):
    return [u.count(c) for c in "ACGT"]


def count_l1(a, b):
    """The shipped filter's quantity: L1 distance of the counts of A, C, G, T (N counts for nothing)."""
    return sum(abs(x - y) for x, y in zip(letter_counts(a), letter_counts(b)))


def myers_global(a, b):
    """The kernel's recurrence (umihip_edit.hip: edit_distance) in plain Python: Myers' bit vectors, Hyyro's
    formulation, global distance.  Bit i of a vector is letter i of a; 32-bit registers; score starts at
    len(a), Ph is shifted in as (Ph << 1) | 1, the score moves on bit len(a) - 1."""
    M = 0xFFFFFFFF
    L = len(a)
    assert L == len(b) and 1 <= L <= 21
    pv, mv, score = M, 0, L
    for cb in b:
        eq = 0
        for i, ca in enumerate(a):
            eq |= (ca == cb) << i
        # (the kernel's eq has garbage above bit L - 1 where the letter's code is 000: it never moves down)
        xv = eq | mv
        xh = ((((eq & pv) + pv) & M) ^ pv) | eq
        ph = (mv | ~(xh | pv)) & M
        mh = pv & xh
        score += ((ph >> (L - 1)) & 1) - ((mh >> (L - 1)) & 1)
        ph = ((ph << 1) | 1) & M
        mh = (mh << 1) & M
        pv = (mh | ~(xv | ph)) & M
        mv = ph & xv
    return score


def _collapse_directional(d, freq, k, p):
    n = len(freq)
    order = sorted(range(n), key=lambda i: (-freq[i], i))
    if n == 0:
        return [], []
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


def _collapse_adjacency(d, freq, k, max_freq):
    n = len(freq)
    order = sorted(range(n), key=lambda i: (-freq[i], i))
    if n == 0:
        return [], []
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


def brute_directional_edit(umis, freq, k, p, d=None):
    """helpers.brute_directional with d_E for the distance (d: the bucket's edit_matrix, if at hand)."""
    return _collapse_directional(edit_matrix(umis) if d is None else d, freq, k, p)


def brute_adjacency_edit(umis, freq, k, max_freq, d=None):
    return _collapse_adjacency(edit_matrix(umis) if d is None else d, freq, k, max_freq)


def model_batch(buckets, k, p=0.5, algo=0, adj_max_freq=0, mats=None):
    """kept u8 [N] / root u32 [N] of a batch of (umis, freq) buckets in rank order, global indices."""
    kept, root, at = [], [], 0
    for b, (umis, freq) in enumerate(buckets):
        d = mats[b] if mats is not None else None
        surv, root_of = (brute_directional_edit(umis, freq, k, p, d) if algo == 0
                         else brute_adjacency_edit(umis, freq, k, adj_max_freq, d))
        m = np.zeros(len(umis), np.uint8)
        m[surv] = 1
        kept.append(m)
        root.append(np.array(root_of, np.int64) + at)
        at += len(umis)
    if not kept:
        return np.zeros(0, np.uint8), np.zeros(0, np.uint32)
    return np.concatenate(kept), np.concatenate(root).astype(np.uint32)


def encode(umis):
    """Keys and N masks of the batched ABI (src/utils/mod.rs:63-83), straight from the code table."""
    keys = np.zeros(len(umis), np.uint64)
    nm = np.zeros(len(umis), np.uint64)
    for i, u in enumerate(umis):
        kk = mm = 0
        for b, ch in enumerate(u):
            kk |= CODE_OF[ch] << (3 * b)
            if ch == "N":
                mm |= 7 << (3 * b)
        keys[i], nm[i] = kk, mm
    return keys, nm


def decode(keys, umi_len):
    return ["".join(LETTER_OF[(int(k) >> (3 * b)) & 7] for b in range(umi_len)) for k in keys]


def pack(buckets):
    """(keys, nmask, freq, bucket_off) of a list of (umis, freq) buckets."""
    keys, nm, fr, off = [np.zeros(0, np.uint64)], [np.zeros(0, np.uint64)], [], [0]
    for umis, freq in buckets:
        kk, mm = encode(umis)
        keys.append(kk); nm.append(mm); fr.extend(freq); off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


# ---- inputs ---------------------------------------------------------------------------------------

def shifted_reads(rng, n_mol, L, mean_copies=4.0, sub=0.03, indel=0.25, n_frac=0.0):
    """Molecule model with synthesis errors, read by read: n_mol true UMIs, geometric copy counts; a copy
    has per-base substitutions (sub) and, with probability indel, one of the two shifts of a fixed-length
    window -- base i deleted and a random base appended, or a random base inserted at i and the last base
    dropped.  Returns the reads' UMIs as strings, in order."""
    out = []
    for _ in range(n_mol):
        true = rng.choice(ALPHA, L)
        for _ in range(int(rng.geometric(1.0 / mean_copies))):
            u = true.copy()
            for i in np.nonzero(rng.random(L) < sub)[0]:
                u[i] = rng.choice(ALPHA[ALPHA != u[i]])
            if rng.random() < indel:
                i = int(rng.integers(0, L))
                if rng.random() < 0.5:  # deletion: the rest moves up, the next base of the read comes in
                    u = np.concatenate([u[:i], u[i + 1:], rng.choice(ALPHA, 1)])
                else:                   # insertion: the rest moves down, the last base falls out
                    u = np.concatenate([u[:i], rng.choice(ALPHA, 1), u[i:L - 1]])
            if n_frac:
                u[rng.random(L) < n_frac] = ord("N")
            out.append(u.tobytes().decode())
    return out


def shifted_bucket(rng, n_mol, L, mean_copies=4.0, sub=0.03, indel=0.25, n_frac=0.0, n_max=None):
    """One position of shifted_reads in rank order: (umis, freq); at most n_max distinct UMIs, the first to
    appear (molecules with their copies, not the most frequent ones)."""
    seen = {}
    for s in shifted_reads(rng, n_mol, L, mean_copies, sub, indel, n_frac):
        seen[s] = seen.get(s, 0) + 1
    umis = list(seen)[:n_max]
    umis, freq, _ = canonical(umis, [seen[u] for u in umis])
    return umis, freq


def same_composition_bucket(L, n, seed=0):
    """n distinct arrangements of one multiset of letters (L // 2 times A, the rest C: 924 of them at
    L = 12): every pair has the same letter counts and passes the count filter.  Rank order, freq."""
    import itertools
    rng = np.random.default_rng(seed)
    every = ["".join("A" if i in at else "C" for i in range(L)) for at in
             (set(c) for c in itertools.combinations(range(L), L // 2))]
    assert n <= len(every)
    pick = sorted(rng.choice(len(every), n, replace=False).tolist())
    umis = [every[i] for i in pick]
    freq = [int(f) for f in rng.choice([1, 1, 2, 3, 5, 9, 20], n)]
    umis, freq, _ = canonical(umis, freq)
    return umis, freq


def shift_only_pairs(umis, k, d_e=None):
    """Pairs (i < j) with d_E <= k < d_H: what a Hamming run cannot see."""
    d_e = edit_matrix(umis) if d_e is None else d_e
    d_h = hamming_matrix(umis)
    return int((np.triu((d_e <= k) & (d_h > k), 1)).sum())


SIZES = (1, 2, 63, 64, 65, 129, 600)
_batches = {}


def batch(L, n_frac):
    """One call's buckets -- every size of SIZES (fewer entries where the alphabet runs out), empty buckets in
    between -- with their distance matrices, made once per (L, n_frac)."""
    key = (L, n_frac)
    if key not in _batches:
        rng = np.random.default_rng(7000 + 100 * L + int(1000 * n_frac))
        buckets = []
        for n in SIZES:
            buckets.append(shifted_bucket(rng, n, L, n_frac=n_frac, n_max=n))
            buckets.append(([], []))
        mats = [edit_matrix(u) for u, _ in buckets]
        _batches[key] = (buckets, mats, pack(buckets))
    return _batches[key]


# ---- inputs that put pairs at every distance (tests/test_gpu_edit_distances.py) ------------------------------

LETTERS = "ACGTN"
PAIR_FREQS = ((2, 1), (1, 1), (3, 3))
_pairs = {}


def _random_string(rng, L, letters=LETTERS):
    return "".join(letters[c] for c in rng.integers(0, len(letters), L))


def adversarial_pairs(L, seed=0):
    """Ordered pairs (a, b) of distinct strings of length L over ACGTN with every distance 1..L among them, made
    once per (L, seed) and without repeats.  A family whose members are not symmetric comes in both orders, (a, b)
    and (b, a): the kernel takes the first entry of a pair as Myers' pattern and the second as its text.
      substitutions  exactly d of them at d places, d = 1..L, two pairs each of four kinds: among A, C, G, T;
                     every one to N; every one from N; any letter to any other
      filter bound   A*L against C*d + A*(L-d) and against A*(L-d) + C*d: L1 of the letter counts is 2 d
      rotations      by s = 1..L-1, of a random string and of ("ACGT"*6)[:L]: d_E small, d_H large
      homopolymers   x*L against y*d + x*(L-d) and x*(L-d) + y*d for all 20 ordered letter pairs and d = 1..L
                     (x = A: code 000, whose match vector has garbage above bit L-1; N: no letter count)
      alternating    xyxy.. against yxyx.. for all 20 ordered letter pairs
      reverse        a string against its reverse
      random         unrelated strings"""
    if (L, seed) in _pairs:
        return _pairs[(L, seed)]
    rng = np.random.default_rng(4100 + 100 * seed + L)
    out, seen = [], set()

    def add(a, b, both=True):
        for p in ((a, b), (b, a)) if both else ((a, b),):
            if p[0] != p[1] and p not in seen:
                seen.add(p)
                out.append(p)

    for d in range(1, L + 1):
        for _ in range(2):
            at = rng.choice(L, d, replace=False)
            a = list(_random_string(rng, L, "ACGT"))        # among A, C, G, T
            b = a[:]
            for i in at:
                b[i] = str(rng.choice([c for c in "ACGT" if c != a[i]]))
            add("".join(a), "".join(b))
            a = list(_random_string(rng, L, "ACGT"))        # every one to N
            b = a[:]
            for i in at:
                b[i] = "N"
            add("".join(a), "".join(b))
            b = list(_random_string(rng, L, "ACGT"))        # every one from N
            a = b[:]
            for i in at:
                a[i] = "N"
            add("".join(a), "".join(b))
            a = list(_random_string(rng, L))                # any letter to any other
            b = a[:]
            for i in at:
                b[i] = str(rng.choice([c for c in LETTERS if c != a[i]]))
            add("".join(a), "".join(b))
    for d in range(1, L + 1):
        add("A" * L, "C" * d + "A" * (L - d))
        add("A" * L, "A" * (L - d) + "C" * d)
    for base in (_random_string(rng, L), ("ACGT" * 6)[:L]):
        for s in range(1, L):
            add(base, base[s:] + base[:s])
    for x in LETTERS:
        for y in LETTERS:
            if x == y:
                continue
            for d in range(1, L + 1):
                add(x * L, y * d + x * (L - d))
                add(x * L, x * (L - d) + y * d)
    for x in LETTERS:
        for y in LETTERS:
            if x != y:
                add(((x + y) * 11)[:L], ((y + x) * 11)[:L], both=False)   # (the other order is the pair (y, x))
    for _ in range(4):
        a = _random_string(rng, L)
        add(a, a[::-1])
    for _ in range(8):
        add(_random_string(rng, L), _random_string(rng, L))
    _pairs[(L, seed)] = out
    return out


def pair_buckets(pairs, freqs=PAIR_FREQS):
    """One bucket of two entries per pair, a first, packed: (keys, nmask, freq, bucket_off).  freqs go round:
    at p = 0.5 a directional call merges (2, 1) and (1, 1) iff d_E(a, b) <= k (thresholds 1 and 1 against
    frequencies 1 and 1) and never (3, 3) (threshold 2 < 3 both ways)."""
    return pack([([a, b], list(freqs[i % len(freqs)])) for i, (a, b) in enumerate(pairs)])


def distinct_strings(L):
    """The strings of adversarial_pairs(L), each once, in order of appearance."""
    seen = {}
    for a, b in adversarial_pairs(L):
        seen.setdefault(a)
        seen.setdefault(b)
    return list(seen)


def mixed_bucket(L, n, seed):
    """n distinct strings of adversarial_pairs(L) -- all of them put in an order of the seed's, the first n of
    that (fewer where there are fewer) -- with frequencies drawn from a short list, in rank order: (umis, freq).
    Every family is in it, so its pairs spread over all distances and its letter counts over the filter's range."""
    rng = np.random.default_rng(seed)
    every = distinct_strings(L)
    umis = [every[i] for i in rng.permutation(len(every))[:n]]
    freq = [int(f) for f in rng.choice([1, 1, 2, 3, 5, 9, 20], len(umis))]
    umis, freq, _ = canonical(umis, freq)
    return umis, freq


def all_strings_bucket(L):
    """All 5^L strings of length L <= 4 in one bucket, freq 1 each: every pair there is."""
    import itertools
    assert L <= 4
    umis = ["".join(t) for t in itertools.product(LETTERS, repeat=L)]
    return umis, [1] * len(umis)


def count_l1_matrix(umis):
    """count_l1 of every pair of a bucket."""
    if not umis:
        return np.zeros((0, 0), np.int64)
    a = np.array([np.frombuffer(u.encode(), dtype=np.uint8) for u in umis])
    cnt = np.stack([(a == ord(c)).sum(1) for c in "ACGT"], 1).astype(np.int64)
    return np.abs(cnt[:, None, :] - cnt[None, :, :]).sum(-1)


def filter_hits(umis, k, l1=None):
    """Pairs i < j of a bucket that pass the kernel's filter, count_l1 <= 2 min(k, L) (the call clamps k to the
    length): what umi_stats.n_candidates counts.  l1: the bucket's count_l1_matrix, if at hand."""
    if len(umis) < 2:
        return 0
    l1 = count_l1_matrix(umis) if l1 is None else l1
    return int(np.triu(l1 <= 2 * min(k, len(umis[0])), 1).sum())


def permitted_pairs(d, freq, k, p=0.5, algo=0, amf=0):
    """Pairs i < j within k that the algorithm permits in at least one direction (what umi_stats.n_edges counts;
    the rule of seq_reference in tests/test_gpu_large_k.py): directional (0) freq[j] <= thr(freq[i]) or the
    other way round, adjacency (1) freq[j] <= amf, cluster (2) every pair."""
    n = len(freq)
    if n < 2:
        return 0
    f = np.array(freq, np.int64)
    near = np.triu(np.asarray(d) <= k, 1)
    if algo == 0:
        thr = np.array([thr_f32(p, int(x)) for x in freq], np.int64)
        ok = (f[None, :] <= thr[:, None]) | (f[:, None] <= thr[None, :])
    elif algo == 1:
        ok = np.broadcast_to(f[None, :] <= amf, (n, n))
    else:
        ok = np.ones((n, n), bool)
    return int((near & ok).sum())


def tile_hits(l1, k, L):
    """Filter hits of every 64 x 64 tile of edit_pair_kernel's walk over one bucket: row tiles start at
    multiples of 64 from the bucket's start, the column tiles of a row tile start at its first row and step by
    64, and only pairs with row < column count.  {(row0, col0): hits}."""
    n = len(l1)
    hit = np.triu(np.asarray(l1) <= 2 * min(k, L), 1)
    return {(r0, c0): int(hit[r0:r0 + 64, c0:c0 + 64].sum()) for r0 in range(0, n, 64) for c0 in range(r0, n, 64)}


WHOLE_SIZES = (2, 63, 64, 65, 129, 330)
_whole = {}


def whole_batch(L):
    """One call's buckets for the sweep over every k: a mixed_bucket of every size of WHOLE_SIZES with an empty
    bucket after each; their distance and count_l1 matrices; the packed call.  Made once per L."""
    if L not in _whole:
        buckets = []
        for n in WHOLE_SIZES:
            buckets.append(mixed_bucket(L, n, seed=n))
            buckets.append(([], []))
        _whole[L] = (buckets, [edit_matrix(u) for u, _ in buckets], [count_l1_matrix(u) for u, _ in buckets], pack(buckets))
    return _whole[L]


def all_strings_batch(L):
    """all_strings_bucket(L) as a call of its own, in whole_batch's form."""
    key = ("all", L)
    if key not in _whole:
        buckets = [all_strings_bucket(L)]
        _whole[key] = (buckets, [edit_matrix(u) for u, _ in buckets], [count_l1_matrix(u) for u, _ in buckets], pack(buckets))
    return _whole[key]
