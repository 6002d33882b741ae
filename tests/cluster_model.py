"""Connected components (UMI_ALGO_CLUSTER, `--algo cluster`), from the definition.

The graph of a bucket has its entries as nodes and an edge i ~ j iff dist(i, j) <= k, for whatever distance
the entry point measures.  kept[i] = 1 iff i is the smallest index of its connected component, root[i] is that
smallest index.  Entries come in rank order, so the smallest index of a component is the entry the root loop of
the algorithm reaches first.  Frequencies, percentage and adj_max_freq take no part.

This is the definition the library and the command-line program are tested against: the oracle has no such
mode.  Its directional mode at percentage = inf agrees while freq < 2^31 - 1 (freq + 1 wraps there, as in the
reference); tests/test_cluster_model_cpu.py shows both.

Plain Python / numpy."""
import numpy as np


def components(d, k):
    """root[i] = smallest index of i's connected component of the graph d <= k (d: a square distance matrix of
    any integer type; the diagonal is not looked at).  Union-find over the pairs, smaller index as the parent."""
    d = np.asarray(d)
    n = len(d)
    parent = list(range(n))

    def find(x):
        while parent[x] != x:
            parent[x] = parent[parent[x]]
            x = parent[x]
        return x
    if n:
        ii, jj = np.nonzero(np.triu(d <= k, 1))
        for i, j in zip(ii.tolist(), jj.tolist()):
            a, b = find(i), find(j)
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(n)], dtype=np.uint32)


def components_bfs(d, k):
    """The same by a second formulation: breadth-first search from every index not yet reached, in ascending
    order -- the root loop of the algorithm with every neighbour admitted."""
    d = np.asarray(d)
    n = len(d)
    root = np.full(n, -1, dtype=np.int64)
    near = d <= k
    for r in range(n):
        if root[r] >= 0:
            continue
        root[r] = r
        frontier = [r]
        while frontier:
            nxt = []
            for u in frontier:
                vs = np.nonzero(near[u] & (root < 0))[0]
                root[vs] = r
                nxt.extend(vs.tolist())
            frontier = nxt
    return root.astype(np.uint32)


def kept_of(root):
    return (np.asarray(root) == np.arange(len(root))).astype(np.uint8)


def batch(mats, off, k):
    """(kept, root) of a whole call: mats[b] is the distance matrix of bucket b, off the bucket table; roots are
    global entry indices."""
    n = int(off[-1])
    root = np.arange(n, dtype=np.uint32)
    for b, d in enumerate(mats):
        s = int(off[b])
        if len(d):
            root[s:s + len(d)] = components(d, k) + s
    return kept_of(root), root


def word_distance(keys, nm):
    """The reference's distance between keys of one or several words (bitset.rs:77-91 per word, summed, halved --
    what umi_dist, the _wide and the _seqs entry points measure), all pairs of one bucket."""
    keys = np.asarray(keys, np.uint64)
    if not len(keys):
        return np.zeros((0, 0), np.int64)
    keys = keys.reshape(len(keys), -1)
    nm = np.zeros_like(keys) if nm is None else np.asarray(nm, np.uint64).reshape(len(keys), -1)
    out = np.zeros((len(keys), len(keys)), np.int64)
    for r0 in range(0, len(keys), 256):
        x = nm[r0:r0 + 256, None, :] ^ nm[None, :, :]
        v = np.bitwise_count(x | (keys[r0:r0 + 256, None, :] ^ keys[None, :, :])).astype(np.int64) \
            - np.bitwise_count(x).astype(np.int64) // 3
        out[r0:r0 + 256] = v.sum(-1) // 2
    return out


def batch_of_keys(keys, nm, off, k):
    """(kept, root) of a call from its keys and N masks (nm may be None) under word_distance."""
    keys = np.asarray(keys)
    mats = [word_distance(keys[int(off[b]):int(off[b + 1])], None if nm is None else nm[int(off[b]):int(off[b + 1])])
            for b in range(len(off) - 1)]
    return batch(mats, off, k)


class PyNaive:
    """A DataStruct in plain Python with Naive's semantics (src/data/naive.rs:26-40) over any distance function:
    remove_near(umi, k, max_freq) removes and returns every present UMI within k whose freq is at most
    max_freq, and the query itself."""

    dist = None  # set by of()

    @classmethod
    def of(cls, dist):
        return type("PyNaiveOf", (cls,), dict(dist=staticmethod(dist)))

    @classmethod
    def new(cls, umi_freq, umi_length, max_edits):
        self = cls()
        self.freq = dict(umi_freq)
        self.present = dict.fromkeys(umi_freq, True)
        return self

    def contains(self, umi):
        return self.present.get(umi, False)

    def remove_near(self, umi, k, max_freq):
        out = set()
        for v, there in self.present.items():
            if there and (v == umi or (self.dist(umi, v) <= k and self.freq[v] <= max_freq)):
                out.add(v)
        for v in out:
            self.present[v] = False
        return out
