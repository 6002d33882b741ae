"""Model of the one-mismatch correction after Cell Ranger (umi_dedup_batch_cr, --algo cr), independent of the
library.  The rule is stated twice: as Cell Ranger's correct_umi loop -- substitute the four nucleotides at every
position and look the result up in the bucket's dict -- and as an arg-max over candidates; test_cr_model_cpu.py
holds the two against each other.  Then kept / root / target / n_edges of a packed batch, and the inputs of the
GPU tests.

Inside one bucket of distinct UMIs with counts:
  candidates  t is a candidate for s when the two differ at exactly one base p and t[p] is one of A C G T
  target      the maximum of {s} and its candidates under (count, then the string; 'A' < 'C' < 'G' < 'N' < 'T' is
              the order of the bytes)
  molecules   the distinct targets; kept[i] iff i is a target; root[i] = i where kept, else target(i)"""
import itertools

import numpy as np

import edit_model as em
from helpers import canonical

NUCS = "ACGT"
LETTERS = "ACGTN"


def targets_loop(umis, freq):
    """Cell Ranger's loop: {umi: its correction}."""
    counts = dict(zip(umis, freq))
    out = {}
    for s in umis:
        corrected, count = s, counts[s]
        for p in range(len(s)):
            for nuc in NUCS:
                if nuc == s[p]:
                    continue
                test = s[:p] + nuc + s[p + 1:]
                value = counts.get(test, 0)
                if value > count or (value == count and corrected < test):
                    corrected, count = test, value
        out[s] = corrected
    return out


def candidates(s, umis):
    return [t for t in umis if sum(a != b for a, b in zip(s, t)) == 1
            and next(b for a, b in zip(s, t) if a != b) in NUCS]


def targets_argmax(umis, freq):
    """The arg-max statement: {umi: max of itself and its candidates by (count, string)}."""
    counts = dict(zip(umis, freq))
    return {s: max([s] + candidates(s, umis), key=lambda t: (counts[t], t)) for s in umis}


def one_base_pairs(umis):
    """Unordered pairs of a bucket at exactly one mismatching base, admissible or not."""
    have = set(umis)
    n = 0
    for s in umis:
        for p in range(len(s)):
            for c in LETTERS:
                t = s[:p] + c + s[p + 1:]
                n += c != s[p] and t in have and s < t
    return n


def model_bucket(umis, freq):
    """(kept, root, target) of one bucket, local indices."""
    at = {u: i for i, u in enumerate(umis)}
    assert len(at) == len(umis), "UMIs of a bucket are distinct"
    tg = targets_loop(umis, freq)
    target = np.array([at[tg[u]] for u in umis], np.int64)
    kept = np.zeros(len(umis), np.uint8)
    kept[target] = 1
    root = np.where(kept == 1, np.arange(len(umis)), target)
    return kept, root, target


def model_batch(buckets):
    """kept u8 [N], root u32 [N], target u32 [N] (global indices) and n_edges of a list of (umis, freq) buckets."""
    kept, root, target, at, pairs = [np.zeros(0, np.uint8)], [np.zeros(0, np.int64)], [np.zeros(0, np.int64)], 0, 0
    for umis, freq in buckets:
        k, r, t = model_bucket(umis, freq)
        kept.append(k); root.append(r + at); target.append(t + at)
        pairs += one_base_pairs(umis)
        at += len(umis)
    return (np.concatenate(kept), np.concatenate(root).astype(np.uint32), np.concatenate(target).astype(np.uint32), pairs)


def root_contract_holds(kept, root):
    kept, root = np.asarray(kept), np.asarray(root).astype(np.int64)
    idx = np.arange(len(kept))
    return bool((root[kept == 1] == idx[kept == 1]).all() and (kept[root] == 1).all())


def chains(umis, freq):
    """a -> b -> c with a != b != c: what a transitive collapse would fold and this rule does not."""
    tg = targets_loop(umis, freq)
    return sum(1 for a in umis if tg[a] != a and tg[tg[a]] != tg[a])


# ---- inputs ---------------------------------------------------------------------------------------

pack = em.pack
SIZES = (1, 2, 3, 63, 64, 65, 129, 600)
LENGTHS = (1, 2, 6, 12, 16, 17, 21)
TIE_FREQS = [1, 1, 1, 2, 2, 3, 5]
_made = {}


def dense_bucket(rng, n, L, n_frac=0.0):
    """About n distinct UMIs (fewer where the alphabet runs out) in rank order: molecules with substitution errors
    at a rate that makes distance-1 pairs abound, no shifts."""
    n_mol = max(1, n // 2)
    while True:
        b = em.shifted_bucket(rng, n_mol, L, mean_copies=6.0, sub=min(0.5, 1.5 / L), indel=0.0, n_frac=n_frac, n_max=n)
        if len(b[0]) >= min(n, 4 ** L):
            return b
        n_mol += max(1, n_mol // 2)


def batch(L, n_frac):
    """One call: a dense_bucket of every size of SIZES with an empty bucket after each; (buckets, packed, model)."""
    key = ("batch", L, n_frac)
    if key not in _made:
        rng = np.random.default_rng(9000 + 100 * L + int(1000 * n_frac))
        buckets = []
        for n in SIZES:
            buckets.append(dense_bucket(rng, n, L, n_frac))
            buckets.append(([], []))
        _made[key] = (buckets, pack(buckets), model_batch(buckets))
    return _made[key]


def tiny_bucket(rng, n, L, n_frac=0.0):
    """n <= 3 distinct UMIs: one random string and single substitutions of it (of the first, or of the one before:
    chains), counts from a short list."""
    letters = LETTERS if n_frac else NUCS
    umis = ["".join(rng.choice(list(letters), L))]
    while len(umis) < n:
        s = umis[int(rng.integers(0, len(umis)))]
        p = int(rng.integers(0, L))
        t = s[:p] + str(rng.choice([c for c in letters if c != s[p]])) + s[p + 1:]
        if t not in umis:
            umis.append(t)
    freq = [int(f) for f in rng.choice(TIE_FREQS, n)]
    umis, freq, _ = canonical(umis, freq)
    return umis, freq


def tiny_runs(L=12, lead=0, seed=0):
    """Runs of one- to three-entry buckets whose boundaries fall on, before and after multiples of 64 entries: `lead`
    entries in a first bucket shift every boundary; then stretches that end exactly on a multiple (threes and a one),
    one short of it, and with a bucket across it; then random sizes."""
    key = ("tiny", L, lead, seed)
    if key not in _made:
        rng = np.random.default_rng(500 + 10 * seed + lead)
        sizes = [lead] if lead else []
        sizes += [3] * 21 + [1]                 # 64: a boundary on the multiple
        sizes += [3] * 22                       # 63 + 3: a bucket across it
        sizes += [2] * 31 + [1, 1]              # 62, 63, 64
        sizes += [0, 1, 0, 2, 3, 0]
        sizes += [int(x) for x in rng.integers(1, 4, 300)]
        buckets = [tiny_bucket(rng, n, L, 0.1 if seed % 2 else 0.0) if n else ([], []) for n in sizes]
        _made[key] = (buckets, pack(buckets), model_batch(buckets))
    return _made[key]


def all_strings(L, letters=LETTERS, seed=0):
    """Every string of length L over `letters` in one bucket, counts from a short list (ties everywhere): every entry
    has all of its neighbours present."""
    key = ("all", L, letters, seed)
    if key not in _made:
        rng = np.random.default_rng(70 + L + seed)
        umis = ["".join(t) for t in itertools.product(letters, repeat=L)]
        freq = [int(f) for f in rng.choice(TIE_FREQS, len(umis))]
        umis, freq, _ = canonical(umis, freq)
        buckets = [(umis, freq)]
        _made[key] = (buckets, pack(buckets), model_batch(buckets))
    return _made[key]


def sized(n, L=12, seed=0):
    """One dense bucket of n entries (the edges of "cr_small_max")."""
    key = ("sized", n, L, seed)
    if key not in _made:
        rng = np.random.default_rng(3000 + n + seed)
        b = dense_bucket(rng, n, L)
        assert len(b[0]) == n
        buckets = [b, ([], []), tiny_bucket(rng, 2, L)]
        _made[key] = (buckets, pack(buckets), model_batch(buckets))
    return _made[key]


def every_input():
    """(name, buckets, packed, model) of every input the GPU tests use."""
    for L in LENGTHS:
        for nf in (0.0, 0.05):
            yield ("batch %d %.2f" % (L, nf),) + batch(L, nf)
    for lead in (0, 1, 2, 3):
        for seed in (0, 1):
            yield ("tiny %d %d" % (lead, seed),) + tiny_runs(12, lead, seed)
    for L in (1, 2, 3, 4):
        yield ("all %d" % L,) + all_strings(L)
    yield ("all 6",) + all_strings(6, NUCS)
    for n in (127, 128, 129):
        yield ("sized %d" % n,) + sized(n)


# ---- the program: a tagged BAM whose (cell, gene) buckets hold neighbours, chains and ties ---------------------

def cr_bam(seed=11, n_cells=4, n_genes=3, L=10):
    """(header, records): a few hundred reads "r<i>_<UMI>" with UB (the UMI again), CB and GX.  Per (cell, gene) a
    few molecules a, each with a one-mismatch neighbour b and a neighbour c of b two mismatches from a, at read
    counts that make a chain a -> b -> c, ties, a plain correction, or a chain that ends in a tie; the reads of a
    (cell, gene) lie at several positions, in an order of the seed's."""
    import struct

    import bamio
    import tag_model
    rng = np.random.default_rng(seed)
    cells = ["".join(rng.choice(list(NUCS), 16)) + "-1" for _ in range(n_cells)]
    reads = []
    for c in cells:
        for g in range(n_genes):
            for _ in range(int(rng.integers(2, 5))):
                a = "".join(rng.choice(list(NUCS), L))
                p, q = (int(x) for x in rng.choice(L, 2, replace=False))
                b = a[:p] + str(rng.choice([x for x in NUCS if x != a[p]])) + a[p + 1:]
                cc = b[:q] + str(rng.choice([x for x in NUCS if x != b[q]])) + b[q + 1:]
                n_a, n_b, n_c = ((1, 2, 4), (2, 2, 2), (3, 1, 0), (1, 3, 3))[int(rng.integers(0, 4))]
                reads += [(c, g, a)] * n_a + [(c, g, b)] * n_b + [(c, g, cc)] * n_c
    items = []
    for i, r in enumerate(int(x) for x in rng.permutation(len(reads))):
        c, g, umi = reads[r]
        p0 = 1000 + 500 * g + 10 * int(rng.integers(0, 5))
        tags = tag_model.aux_fields_before(rng) + tag_model.aux_z("UB", umi) + tag_model.aux_z("CB", c)
        tags += tag_model.aux_z("GX", "GENE%02d" % g) + b"xxi" + struct.pack("<i", i)
        quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
        items.append((p0, i, bamio.make_record("r%d_%s" % (i, umi), 0, 0, p0, int(rng.integers(0, 61)), [("M", 50)], 50, quals,
                                               tags=tags)))
    items.sort(key=lambda t: (t[0], t[1]))
    return bamio.make_header([("chr1", 10_000_000)]), [t[2] for t in items]


def staged_buckets(st):
    """the (umis, freq) buckets of a staged dict (gene_model.stage, tag_model.stage)"""
    umis = em.decode(st["keys"], st["umi_len"])
    off = st["bucket_off"].astype(np.int64)
    return [(umis[off[b]:off[b + 1]], [int(f) for f in st["freq"][off[b]:off[b + 1]]]) for b in range(len(off) - 1)]


def dedup_staged(st, k=1, p=0.5, algo="cr"):
    """gene_model.expected_output's `dedup`: the kept mask of a staged dict under the rule"""
    return model_batch(staged_buckets(st))[0]
