"""Independent CPU model of whole-read keys (fastq mode): to_bitset over any length, the reference's
per-word distance in numpy, a part-equality join that finds the pairs within k without the library,
the collapse from neighbour lists, and the fastq mode's staging and output from the definition in
the CLI's header comment.  Plain Python / numpy, written from the definitions."""
import numpy as np

CODE = {ord("A"): 0, ord("T"): 5, ord("C"): 6, ord("G"): 3, ord("N"): 4}


def words(L):
    return (3 * L + 63) // 64


def to_bitset(seq, n_words):
    """src/utils/mod.rs:63-83: base i at bits 3i..3i+2 of the word string (bit by bit)."""
    k = [0] * n_words
    m = [0] * n_words
    for i, c in enumerate(seq):
        v = CODE[c]
        for j in range(3):
            bit = 3 * i + j
            if (v >> j) & 1:
                k[bit >> 6] |= 1 << (bit & 63)
            if v == 4:
                m[bit >> 6] |= 1 << (bit & 63)
    return k, m


def encode(seqs, n_words):
    """to_bitset of reads of one length (any number of them), vectorised over the reads; reads of
    mixed lengths go one by one."""
    keys = np.zeros((len(seqs), n_words), dtype=np.uint64)
    nm = np.zeros((len(seqs), n_words), dtype=np.uint64)
    if len({len(s) for s in seqs}) > 1:
        for i, s in enumerate(seqs):
            k, m = to_bitset(s, n_words)
            keys[i] = np.array(k, dtype=np.uint64)
            nm[i] = np.array(m, dtype=np.uint64)
        return keys, nm
    if not seqs or not seqs[0]:
        return keys, nm
    L = len(seqs[0])
    lut = np.zeros(256, dtype=np.uint64)
    for c, v in CODE.items():
        lut[c] = v
    codes = lut[np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(len(seqs), L)]
    for i in range(L):
        for j in range(3):
            bit = 3 * i + j
            one = np.uint64(1) << np.uint64(bit & 63)
            keys[:, bit >> 6] |= np.where((codes[:, i] >> np.uint64(j)) & np.uint64(1), one, np.uint64(0))
            nm[:, bit >> 6] |= np.where(codes[:, i] == 4, one, np.uint64(0))
    return keys, nm


def dist_rows(keys, nm, a, b):
    """bitset.rs:77-91 per word, utils/mod.rs:25: distances of the pairs (a[i], b[i])."""
    x = nm[a] ^ nm[b]
    d = np.bitwise_count(x | (keys[a] ^ keys[b])).astype(np.int64) - np.bitwise_count(x).astype(np.int64) // 3
    return d.sum(axis=1) // 2


def pairs_brute(keys, nm, k):
    """All pairs i < j within k (one bucket)."""
    n = len(keys)
    out = []
    for i in range(n - 1):
        j = np.arange(i + 1, n)
        d = dist_rows(keys, nm, np.full(len(j), i), j)
        out.extend((i, int(jj)) for jj in j[d <= k])
    return out


def pairs_join(seqs, keys, nm, k):
    """Pairs within k of one bucket of equal-length reads, found by exact part joins: k + 1 parts of
    the bases (pigeonhole), pairs of equal parts grouped with numpy, each decided by the distance."""
    n = len(seqs)
    if n < 2:
        return []
    L = len(seqs[0])
    arr = np.frombuffer(b"".join(seqs), dtype=np.uint8).reshape(n, L) if L else np.zeros((n, 0), np.uint8)
    P = min(k + 1, max(L, 1))
    cand = set()
    for j in range(P):
        lo, hi = j * L // P, (j + 1) * L // P
        part = np.ascontiguousarray(arr[:, lo:hi]).view(np.dtype((np.void, max(hi - lo, 1)))).ravel() \
            if hi > lo else np.zeros(n, dtype="V1")
        _, inv = np.unique(part, return_inverse=True)
        order = np.argsort(inv, kind="stable")
        grp = inv[order]
        starts = np.flatnonzero(np.r_[True, grp[1:] != grp[:-1], True])
        for s, e in zip(starts[:-1], starts[1:]):
            if e - s < 2:
                continue
            members = np.sort(order[s:e])
            for i in range(len(members) - 1):  # row by row: a heavy bin stays small in memory
                a = np.full(len(members) - i - 1, members[i])
                b = members[i + 1:]
                d = dist_rows(keys, nm, a, b)
                cand.update((int(members[i]), int(y)) for y in b[d <= k])
    return sorted(cand)


def thr_f32(p, f):
    prod = np.float32(p) * np.float32(np.int32(np.uint32(f) + np.uint32(1)))
    if np.isnan(prod):
        return 0
    if np.isinf(prod) or abs(prod) >= 2 ** 31:
        return 2 ** 31 - 1 if prod > 0 else -2 ** 31
    return int(prod)


def collapse(n, pairs, freq, algo, k, p=0.5, adj_max_freq=0):
    """Directional (algo 0) / adjacency (1) over one bucket in rank order (entries 0..n-1), from its
    pairs within k: (kept bool[n], root int[n])."""
    nb = [[] for _ in range(n)]
    for a, b in pairs:
        nb[a].append(b)
        nb[b].append(a)
    present = np.ones(n, bool)
    root = np.arange(n)
    kept = np.zeros(n, bool)
    for r in range(n):
        if not present[r]:
            continue
        kept[r] = True
        present[r] = False
        if algo == 0:
            frontier = [r]
            while frontier:
                nxt = []
                for u in frontier:
                    t = thr_f32(p, freq[u])
                    for v in nb[u]:
                        if present[v] and freq[v] <= t:
                            present[v] = False
                            root[v] = r
                            nxt.append(v)
                frontier = nxt
        else:
            for v in nb[r]:
                if present[v] and freq[v] <= adj_max_freq:
                    present[v] = False
                    root[v] = r
    return kept, root


def stage(seqs, quals, merge):
    """fastq mode's staging: buckets by length (first appearance), entries by freq descending then
    first appearance; rep = first read (merge 0) or highest average quality, first on ties (1)."""
    buckets = {}
    for i, (s, q) in enumerate(zip(seqs, quals)):
        d = buckets.setdefault(len(s), {})
        sc = avg_qual(q) if merge else 0
        e = d.get(s)
        if e is None:
            d[s] = [1, i, sc]
        else:
            e[0] += 1
            if merge and not (e[2] >= sc):
                e[1], e[2] = i, sc
    ent, off, blen = [], [0], []
    for L, d in buckets.items():
        items = sorted(d.items(), key=lambda kv: -kv[1][0])
        ent += [(s, e[0], e[1]) for s, e in items]
        off.append(len(ent))
        blen.append(L)
    return ent, off, blen


def avg_qual(q):
    if len(q) == 0:
        return 0
    return int(np.float32(sum(c - 33 for c in q)) / np.float32(len(q)))


def dedup(ent, off, blen, k, algo=0, p=0.5, adj_max_freq=0, join=False):
    """kept / root (global entry indices) of every bucket."""
    n = len(ent)
    kept = np.zeros(n, bool)
    root = np.arange(n)
    for b in range(len(blen)):
        lo, hi = off[b], off[b + 1]
        seqs = [e[0] for e in ent[lo:hi]]
        keys, nm = encode(seqs, max(1, words(blen[b])))
        pairs = pairs_join(seqs, keys, nm, k) if join else pairs_brute(keys, nm, k)
        kb, rb = collapse(hi - lo, pairs, [e[1] for e in ent[lo:hi]], algo, k, p, adj_max_freq)
        kept[lo:hi] = kb
        root[lo:hi] = rb + lo
    return kept, root


def output(seqs, quals, names, ent, off, kept, root, trim=0, tag=False):
    """The CLI's output text (see its header comment)."""
    rec = lambda i, extra=b"": (b"@" + names[i] + extra + b"\n" + seqs[i][trim:] + b"\n+\n" + quals[i][trim:] + b"\n")
    rep_of = {e[2]: j for j, e in enumerate(ent)}
    if not tag:
        return b"".join(rec(i) for i in range(len(seqs)) if i in rep_of and kept[rep_of[i]])
    cid = {}
    for i in range(len(seqs)):
        if i in rep_of and kept[rep_of[i]]:
            cid[rep_of[i]] = len(cid)
    size = {}
    for j, e in enumerate(ent):
        size[int(root[j])] = size.get(int(root[j]), 0) + e[1]
    entry = {}
    for j, e in enumerate(ent):
        entry[e[0]] = j
    out = []
    for i in range(len(seqs)):
        j = entry[seqs[i]]
        r = int(root[j])
        extra = b" cluster_id=%d" % cid[r]
        if ent[r][2] == i:
            extra += b" cluster_size=%d" % size[r]
        if ent[j][2] == i:
            extra += b" same_umi=%d" % ent[j][1]
        out.append(rec(i, extra))
    return b"".join(out)
