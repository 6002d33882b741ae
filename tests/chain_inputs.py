"""Deterministic buckets whose permitted pairs form one long chain, with their answers in closed form.

The path.  hamming_path(L) starts at A*L; step t advances base t % L one letter along ACGT.  Between
nodes i < j of the 3 L + 1 nodes exactly the bases t % L, t in [i, j), differ: dist(i, j) =
min(j - i, L).  Every stride-th node kept (stride = k <= L / 2): consecutive nodes are exactly k apart
and all others 2 k or more, so at edit distance k the path is induced -- the only pairs within k are
the consecutive ones, and the depth of the chain is the number of nodes less one.

The ladders put a freq on every path position (entries are handed over in rank order: freq
descending, ties in any order):
  sym      all freq 1, p = 0.5: every pair is permitted both ways (union-find, the LDS unite);
  halving  2^(n-1), ..., 4, 2, 1 over at most 31 nodes, p = 0.5: every pair one-way, the top freq 2^30;
  step2    2n, 2n - 2, ..., 2, p = 1.0: every pair one-way at any length (thr(f) = f + 1 admits f - 2,
           and thr(f - 2) = f - 1 refuses f);
  comb     F, F, F - 2, F - 2, ..., p = 1.0: symmetric and one-way pairs alternate, sets of two chained
           by one-way pairs.
Directional: every entry is reached from rank 0, so only entry 0 is kept and every root is entry 0.
Adjacency with adj_max_freq = 1 on sym: the greedy root loop over the path's neighbours (forward
order: kept, removed, kept, ...); adj_max_freq = 0 removes nothing.

Plain Python / numpy; the only randomness is one seeded permutation."""
import numpy as np

LETTERS = "ACGT"
ORDERS = ("forward", "reverse", "zigzag", "perm")
LADDERS = ("sym", "halving", "step2", "comb")
HALVING_MAX = 31  # 2^30 is the largest power of two an int32 freq holds


def hamming_path(L, stride=1):
    """The nodes 0, stride, 2 stride, ... of the path over L bases, as strings."""
    adv = [0] * L
    nodes = ["A" * L]
    for t in range(3 * L):
        adv[t % L] += 1
        nodes.append("".join(LETTERS[a] for a in adv))
    return nodes[::stride]


def n_nodes(L, stride=1):
    return 3 * L // stride + 1


def order_positions(n, order, seed=0):
    """Path position of entry e (equal freqs: ties may stand in any order)."""
    if order == "forward":
        return list(range(n))
    if order == "reverse":
        return list(range(n - 1, -1, -1))
    if order == "zigzag":
        out = []
        lo, hi = 0, n - 1
        while lo <= hi:
            out.append(lo)
            if hi != lo:
                out.append(hi)
            lo, hi = lo + 1, hi - 1
        return out
    if order == "perm":
        return np.random.default_rng(77000 + 131 * n + seed).permutation(n).tolist()
    raise ValueError(order)


class Chain:
    """One bucket: umis / freq in entry (rank) order, pos[e] = path position of entry e, the call's
    percentage p, the claimed depth (hops from entry 0 to the farthest entry along permitted pairs)."""

    def __init__(self, name, umis, freq, pos, p, depth):
        self.name, self.umis, self.freq, self.pos, self.p, self.depth = name, umis, freq, pos, p, depth
        self.n = len(umis)

    def directional(self):
        """(kept, root) inside the bucket: everything falls to rank 0."""
        kept = np.zeros(self.n, np.uint8)
        kept[:1] = 1
        return kept, np.zeros(self.n, np.uint32)

    def adjacency(self, max_freq):
        """(kept, root) inside the bucket of the greedy root loop (adjacency.rs): entry r, if still
        present, is kept and removes its present path neighbours of freq <= max_freq."""
        at = {p: e for e, p in enumerate(self.pos)}
        present = [True] * self.n
        kept = np.zeros(self.n, np.uint8)
        root = np.arange(self.n, dtype=np.uint32)
        for r in range(self.n):
            if not present[r]:
                continue
            kept[r] = 1
            present[r] = False
            for q in (self.pos[r] - 1, self.pos[r] + 1):
                e = at.get(q)
                if e is not None and present[e] and self.freq[e] <= max_freq:
                    present[e] = False
                    root[e] = r
        return kept, root


def chain(ladder, L, stride=1, order="forward", n=None):
    """The bucket of one ladder over the path of L bases (its first n nodes)."""
    nodes = hamming_path(L, stride)
    if ladder == "halving":
        n = min(n or len(nodes), HALVING_MAX)
    nodes = nodes[:n] if n else nodes
    n = len(nodes)
    name = "%s/L%d/s%d/%s/n%d" % (ladder, L, stride, order, n)
    if ladder == "sym":
        pos = order_positions(n, order)
        return Chain(name, [nodes[q] for q in pos], [1] * n, pos, 0.5, max(pos[0], n - 1 - pos[0]))
    if order != "forward":
        raise ValueError("a ladder of distinct freqs has one rank order")
    pos = list(range(n))
    if ladder == "halving":
        return Chain(name, nodes, [1 << (n - 1 - i) for i in range(n)], pos, 0.5, n - 1)
    if ladder == "step2":
        return Chain(name, nodes, [2 * (n - i) for i in range(n)], pos, 1.0, n - 1)
    if ladder == "comb":
        top = 2 * ((n + 1) // 2)
        return Chain(name, nodes, [top - 2 * (i // 2) for i in range(n)], pos, 1.0, n - 1)
    raise ValueError(ladder)


def thr_f32(p, f):
    """directional.rs:100-102: (percentage * (freq + 1) as f32) as i32"""
    return int(np.float32(p) * np.float32(f + 1))


def distances(umis, rows=128):
    """Hamming distance of every pair, straight from the characters: int [n, n]."""
    a = np.array([np.frombuffer(u.encode(), dtype=np.uint8) for u in umis])
    out = np.zeros((len(a), len(a)), np.int64)
    for r0 in range(0, len(a), rows):
        out[r0:r0 + rows] = (a[r0:r0 + rows, None, :] != a[None, :, :]).sum(-1)
    return out


def permitted_pairs(umis, freq, k, p):
    """bool [n, n]: u -> v permitted, dist(u, v) <= k and freq[v] <= threshold(p, freq[u])."""
    d = distances(umis)
    thr = np.array([thr_f32(p, f) for f in freq])
    adj = (d <= k) & (np.array(freq)[None, :] <= thr[:, None])
    np.fill_diagonal(adj, False)
    return adj


def hops_from_rank0(adj):
    """Breadth-first hop count from entry 0 along permitted pairs (-1: not reached)."""
    n = len(adj)
    hop = [-1] * n
    hop[0] = 0
    frontier = [0]
    while frontier:
        nxt = []
        for u in frontier:
            for v in np.nonzero(adj[u])[0].tolist():
                if hop[v] < 0:
                    hop[v] = hop[u] + 1
                    nxt.append(v)
        frontier = nxt
    return hop


def assemble(buckets):
    """[(umis, freq)] -> (all umis, freq int32, bucket_off uint64)."""
    umis = [u for b in buckets for u in b[0]]
    freq = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    return umis, freq, off


def expected(buckets, chains, algo=0, adj_max_freq=0):
    """The closed-form kept / root of a call in global entry indices, and the mask of the entries it
    covers: buckets[i] is chains[i]'s where chains[i] is a Chain, any other bucket where it is None."""
    n = sum(len(b[0]) for b in buckets)
    kept, root, known = np.zeros(n, np.uint8), np.zeros(n, np.uint32), np.zeros(n, bool)
    lo = 0
    for b, c in zip(buckets, chains):
        hi = lo + len(b[0])
        if c is not None:
            if algo == 0:
                kb, rb = c.directional()
            elif adj_max_freq < 1:
                kb, rb = np.ones(c.n, np.uint8), np.arange(c.n, dtype=np.uint32)
            else:
                kb, rb = c.adjacency(adj_max_freq)
            kept[lo:hi], root[lo:hi], known[lo:hi] = kb, rb + lo, True
        lo = hi
    return kept, root, known
