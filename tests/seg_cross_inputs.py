"""Inputs for the cross path of the segment index (option seg_cross: the pairs between super-bins read off the
super-bins' rest-code maps) and a numpy model of what it must find.

A deep bucket of n entries at k = 1 is cut in two parts; part 0's bins are indexed by nb0 bases, and 4^g adjacent bins
-- they share bases g .. nb0 - 1 of the key -- are one super-bin.  The model takes an entry apart the way the kernels
do: its super-bin code (the shared bases) and its rest-code (every other base: the bases outside the bins below, the g
low bases on top).  A cross pair is two entries of equal rest-code in super-bins whose codes differ in one base; a pair
inside a super-bin is two entries of one super-bin whose rest-codes differ in one base.  Together they are all pairs at
distance 1 of a bucket without N, which neighbours() counts without either code.
Keys: 3 bits per base, base b at bit 3 b, the low two bits tell the four bases apart (A 0, T 1, C 2, G 3)."""
import numpy as np

import oracle as orc
from helpers import canonical

LETTERS = "ATCG"  # by 2-bit code


def bases_of(keys, L):
    """[n, L] 2-bit codes of the keys' bases"""
    k = np.asarray(keys, np.uint64)
    return np.stack([((k >> np.uint64(3 * b)) & np.uint64(3)).astype(np.int64) for b in range(L)], axis=1)


def shape_of(n, L, g=0, cap=5632, smin=1024):
    """(nb0, g) the planner gives a bucket of n entries at k = 1 (plan_segment and choose_super_bases of
    umihip_plan.hpp, restated); g = 0: no super-bins.  g > 0 in the call: that exponent or none."""
    nb0 = min(L // 2, max(2, min(12, (int(n).bit_length() - 1 - 4) // 2)))
    for gg in range(min(4, nb0), 0, -1):
        if g and gg != g:
            continue
        if L - nb0 + gg > 8:
            continue
        expect = n >> (2 * (nb0 - gg))
        if expect > cap // 4 * 3 or expect < smin:
            continue
        return nb0, gg
    return nb0, 0


def cross_planned(L, g, seg_cross=1, map_mb=8):
    """the planner's cross rule (choose_cross), restated for one segment"""
    return bool(seg_cross) and g > 0 and L <= 16 and 4 ** L // 8 <= map_mb << 20


def codes_of(keys, L, nb0, g):
    """(super-bin code, rest-code) of every entry"""
    v = bases_of(keys, L)
    sb = np.zeros(len(v), np.int64)
    for b in range(g, nb0):
        sb |= v[:, b] << (2 * (b - g))
    rest = np.zeros(len(v), np.int64)
    for b in range(nb0, L):
        rest |= v[:, b] << (2 * (b - nb0))
    for b in range(g):
        rest |= v[:, b] << (2 * (L - nb0 + b))
    return sb, rest


def _pairs_one_base_apart(same, differ, n_bases):
    """index pairs (i, j) of entries with equal `same` whose `differ` codes (n_bases bases) differ in exactly one
    base, each pair once; no two entries share both codes"""
    bits = 2 * n_bases
    full = (same << bits) | differ
    order = np.argsort(full, kind="stable")
    srt = full[order]
    out = []
    for b in range(n_bases):
        for d in (1, 2, 3):
            other = (same << bits) | (differ ^ (d << (2 * b)))
            at = np.searchsorted(srt, other)
            hit = (at < len(srt)) & (srt[np.minimum(at, len(srt) - 1)] == other) & (other > full)
            out.append(np.stack([np.nonzero(hit)[0], order[at[hit]]], axis=1))
    return np.concatenate(out) if out else np.zeros((0, 2), np.int64)


def cross_pairs(keys, L, nb0, g):
    """the cross pairs, [m, 2] entry indices"""
    sb, rest = codes_of(keys, L, nb0, g)
    return _pairs_one_base_apart(rest, sb, nb0 - g)


def inside_pairs(keys, L, nb0, g):
    """the pairs inside the super-bins"""
    sb, rest = codes_of(keys, L, nb0, g)
    return _pairs_one_base_apart(sb, rest, L - nb0 + g)


def neighbours(keys, L):
    """pairs at distance 1 of a bucket of distinct keys without N, counted from the bases alone"""
    v = bases_of(keys, L)
    code = np.zeros(len(v), np.int64)
    for b in range(L):
        code |= v[:, b] << (2 * b)
    assert len(np.unique(code)) == len(code)
    return len(_pairs_one_base_apart(np.zeros(len(v), np.int64), code, L))


def key_of(sb, rest, L, nb0, g):
    """the UMI with these two codes"""
    v = [0] * L
    for b in range(g, nb0):
        v[b] = (sb >> (2 * (b - g))) & 3
    for b in range(nb0, L):
        v[b] = (rest >> (2 * (b - nb0))) & 3
    for b in range(g):
        v[b] = (rest >> (2 * (L - nb0 + b))) & 3
    return "".join(LETTERS[c] for c in v)


def batch_of(umis, freq):
    """one bucket in rank order: (keys, nmask, freq, bucket_off)"""
    umis, freq, _ = canonical(list(umis), list(freq))
    keys, nm = orc.encode_keys(umis)
    return keys, nm, np.array(freq, np.int32), np.array([0, len(umis)], np.uint64)


def three_classes(n):
    """7 / 3 / 1 in thirds of the rank order: at p = 0.5 two of three pairs are one-way, one in nine symmetric"""
    return [7] * (n // 3) + [3] * (n // 3) + [1] * (n - 2 * (n // 3))


def random_umis(rng, n_raw, L):
    """distinct random UMIs, sorted"""
    raw = rng.integers(0, 4, (n_raw, L))
    return sorted({"".join(LETTERS[c] for c in r) for r in raw})


def _freqs(rng, n):
    return np.minimum(rng.geometric(0.5, n), 40).tolist()


# L = 10, ~20,000 entries: nb0 = 5, g = 3 -- 16 super-bins (two shared bases), rest-codes of 8 bases (2,048 words)
L10 = dict(L=10, nb0=5, g=3)


def background(rng, n_raw, shape, sbs, rest_min=0):
    """random entries of the super-bins sbs alone, their rest-codes at least rest_min"""
    L, nb0, g = shape["L"], shape["nb0"], shape["g"]
    out = set()
    sbs = list(sbs)
    for _ in range(n_raw):
        out.add(key_of(sbs[int(rng.integers(len(sbs)))], int(rng.integers(rest_min, 4 ** (L - nb0 + g))), L, nb0, g))
    return sorted(out)


def lone_entry_with_all_partners(seed=0, partners=None):
    """An entry alone in super-bin 5 (code: base 3 = T, base 4 = T) whose rest-code stands once in each of the six
    super-bins one base away (or in those of `partners`), alone there as well; the other nine super-bins hold the bulk
    of the bucket, none of that rest-code.  Returns (batch, shape, index pairs the lone entry must be found in)."""
    rng = np.random.default_rng(1200 + seed)
    L, nb0, g = L10["L"], L10["nb0"], L10["g"]
    s0, r0 = 5, 0x9C31
    near = [s0 ^ (d << (2 * b)) for b in range(2) for d in (1, 2, 3)]
    far = [s for s in range(16) if s != s0 and s not in near]
    bulk = [u for u in background(rng, 20000, L10, far) if codes_of(orc.encode_keys([u])[0], L, nb0, g)[1][0] != r0]
    planted = [key_of(s0, r0, L, nb0, g)] + [key_of(s, r0, L, nb0, g) for s in (near if partners is None else partners)]
    umis = bulk + planted
    order = rng.permutation(len(umis))
    umis = [umis[i] for i in order]
    return batch_of(umis, _freqs(rng, len(umis))), dict(L10), len(planted) - 1


def map_edges(seed=0):
    """Every super-bin random, and in super-bins 0, 1 (one base apart) and 4 (one base from 0) the rest-codes 0, 31,
    4^8 - 32 and 4^8 - 1: hits at bits 0 and 31 of the first and the last word of the map, the last ones ranked behind
    every other entry of their super-bins (ranks that cross every word)."""
    rng = np.random.default_rng(1210 + seed)
    L, nb0, g = L10["L"], L10["nb0"], L10["g"]
    umis = set(background(rng, 20000, L10, range(16)))
    for s in (0, 1, 4):
        for r in (0, 31, 4 ** 8 - 32, 4 ** 8 - 1):
            umis.add(key_of(s, r, L, nb0, g))
    umis = sorted(umis)
    rng.shuffle(umis)
    return batch_of(umis, _freqs(rng, len(umis))), dict(L10)


def queue_fill(m, seed=0):
    """Super-bins 2 and 3 hold the same m rest-codes 0 .. m - 1 (one 64-word chunk of the map: one wave's queue takes
    m hits from it) and nothing else; the bulk lies in the other super-bins with rest-codes from 2,048 on, so that no
    other hit falls into that chunk of those two maps."""
    rng = np.random.default_rng(1220 + seed)
    L, nb0, g = L10["L"], L10["nb0"], L10["g"]
    umis = set(background(rng, 20000, L10, [s for s in range(16) if s not in (2, 3)], rest_min=2048))
    for r in range(m):
        umis.add(key_of(2, r, L, nb0, g))
        umis.add(key_of(3, r, L, nb0, g))
    umis = sorted(umis)
    rng.shuffle(umis)
    return batch_of(umis, _freqs(rng, len(umis))), dict(L10)


def dense_one_way(seed=0):
    """L = 8, ~22,000 of the 65,536 keys, freqs of three classes: nb0 = 4, g = 2, 16 super-bins of ~1,400; a pair of
    neighbouring super-bins shares ~480 rest-codes and two in three pairs are one-way at p = 0.5 -- with one CU's
    16 blocks a block's one-way pairs pass the 512 of its private slot"""
    rng = np.random.default_rng(1230 + seed)
    umis = random_umis(rng, 26000, 8)
    rng.shuffle(umis)
    return batch_of(umis, three_classes(len(umis))), dict(L=8, nb0=4, g=2)


def uniform(n_raw, L, seed=0):
    """a random deep bucket"""
    rng = np.random.default_rng(1240 + seed)
    umis = random_umis(rng, n_raw, L)
    rng.shuffle(umis)
    return batch_of(umis, _freqs(rng, len(umis)))


def with_key_twice(batch, seed=0, copies=20):
    """the batch with `copies` of its freq-1 keys a second time (both copies freq 1: a symmetric pair at distance 0)"""
    rng = np.random.default_rng(1250 + seed)
    keys, nm, fr, off = batch
    again = rng.choice(np.nonzero(fr == 1)[0], copies, replace=False)
    k2 = np.concatenate([keys, keys[again]])
    f2 = np.concatenate([fr, np.ones(len(again), np.int32)])
    order = np.lexsort((np.arange(len(k2)), -f2))
    return k2[order], np.zeros_like(k2), f2[order], np.array([0, len(k2)], np.uint64)


def crowded_super_bin(seed=0, freq=None):
    """L = 10 with bases 3 and 4 = A for a sixth of the rows: super-bin 0 holds ~4,600 entries among fifteen of
    ~1,100 -- above a cap of 2,048 (tests/test_gpu_seg_super.py's mixed call)"""
    rng = np.random.default_rng(1260 + seed)
    raw = rng.integers(0, 4, (21600, 10))
    raw[18000:, 3:5] = 0
    umis = sorted({"".join(LETTERS[c] for c in r) for r in raw})
    rng.shuffle(umis)
    return batch_of(umis, _freqs(rng, len(umis)) if freq is None else freq(len(umis))), dict(L10)
