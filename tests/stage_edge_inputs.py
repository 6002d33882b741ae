"""Inputs that put read staging (umi_stage_reads*, umi_stage_seqs) on the edges of its own structure:
read counts, entry runs and positions that start, end or straddle at a wave (64), a round (256), a tile
(2,048) or a rank block (16,384); the limits of the no-sort order (1,024 entries a position, 16 entries a
position on average); order keys of exactly 32 and 33 bits; composed keys of exactly 64 and 65 bits;
garbage above the counted key bits; every letter at every base.  tests/test_stage_edge_inputs_cpu.py
proves on the CPU that each input has the property it is named for, tests/test_gpu_stage_edges.py runs
them on the device.

A generator returns a StageInput: (align, group or None, umi bytes, score or None, L, bits, merge), the
arguments of one staging call in file order; bits is align_key_bits, or (align_key_bits, group_key_bits)
where there is a group key.  The keys carry random garbage above the counted bits; reference() masks it
off on the host before the project's reference sees the keys, the library gets them as they are.

Layouts.  A layout lists the positions in ascending key order, each as the run lengths (freqs) of its
entries.  The library sorts reads by (position key, UMI, file index), and how UMIs sort among themselves
is its own business (packed five letters to seven bits, or word by word).  Two devices make the offset of
every run in that sorted order known all the same: layouts that aim at an offset use one UMI per position,
and positions of several entries give every entry the same run length.  Every layout comes in three file
orders -- sorted (the layout's own order), reversed, shuffled with a fixed seed -- which decide position
rank, first appearance and rep, and leave the sorted order's runs where they are.

The two host rules of umihip_stage_plan.hpp are restated here in plain Python (sort_plan, order_plan);
plan_table() prints the table tests/cpp/test_stage_plan.cpp checks the header against."""
from typing import NamedTuple, Optional

import numpy as np

LETTERS = np.frombuffer(b"ACGT", np.uint8)
LETTERS5 = np.frombuffer(b"ACGTN", np.uint8)
ORDERS = ("sorted", "reversed", "shuffled")
LOCAL_MAX = 1024
INT32_MIN, INT32_MAX = -2 ** 31, 2 ** 31 - 1
EXTREMES = (INT32_MIN, -1, 0, 1, INT32_MAX)
U64 = np.uint64


class StageInput(NamedTuple):
    align: np.ndarray
    group: Optional[np.ndarray]
    umi: np.ndarray
    score: Optional[np.ndarray]
    L: int
    bits: object
    merge: int


# ---- the two plan rules, restated ------------------------------------------------------------------

def bits_for(v):
    b = 1
    while b < 64 and (v >> b):
        b += 1
    return b


def pack5_bits(L):
    return 7 * (L // 3) + (3 if L % 3 == 1 else 5 if L % 3 == 2 else 0)


def sort_plan(W, L, abits, gbits):
    """How the reads are sorted: the group key folded into the alignment word where both fit 64 bits,
    else a second position word; one composed key where position word and packed UMI fit 64 bits."""
    combine = gbits > 0 and abits + gbits <= 64
    a = abits + gbits if combine else abits
    g = 0 if combine or gbits <= 0 else gbits
    p5 = pack5_bits(L if W == 1 else 1)
    return dict(combine=combine, align_bits=a, group_bits=g, second_word=g > 0, p5_bits=p5,
                one_key=W == 1 and g == 0 and a + p5 <= 64, composed_bits=a + p5)


def order_plan(n, E, B, fmax, pmax, force_wide=False):
    """How the entries are ordered: a wave per position (local) where no position has more than 1,024
    entries and E >= 16 B, with (fmax - freq, first read) in 32 bits where bits_for(n - 1) + bits_for(fmax)
    fit, else in 64; otherwise a sort by (position rank, fmax - freq), on 32-bit keys where they fit."""
    freq_bits, rank_bits = bits_for(fmax), bits_for(B - 1 if B else 0)
    order_bits = min(64, freq_bits + rank_bits)
    first_bits = bits_for(n - 1 if n else 0)
    wide = force_wide or first_bits + freq_bits > 32
    return dict(local=pmax <= LOCAL_MAX and E >= 16 * B, wide=wide, first_bits=32 if wide else first_bits,
                freq_bits=freq_bits, rank_bits=rank_bits, order_bits=order_bits, key64=order_bits > 32)


def order_plan_of(inp, ref):
    """order_plan of a call, from the reference's output"""
    sizes = np.diff(ref["bucket_off"].astype(np.int64))
    return order_plan(len(inp.align), len(ref["freq"]), len(sizes), int(ref["freq"].max()), int(sizes.max()))


# every (W, L, align bits, group bits) and (n, E, B, fmax, pmax) the GPU tests run at, and the neighbours of
# every threshold
COMPOSE_LENGTHS = (1, 2, 3, 4, 5, 11, 12, 13, 20, 21)


def compose_bits(L):
    p = pack5_bits(L)
    return (63 - p, 64 - p, 65 - p, 64)


def grouped_bits(L):
    """(align bits, group bits) with align + group + packed UMI = 64 and 65, align + group = 64 and 65, both
    keys whole, both one bit, and one bit beside a whole word"""
    p = pack5_bits(L)
    a = (64 - p) // 2
    return ((a, 64 - p - a), (a, 65 - p - a), (40, 24), (40, 25), (64, 64), (1, 1), (1, 64))


def plan_table():
    """Lines "S W L abits gbits -> combine align_bits group_bits second_word p5_bits one_key composed_bits"
    and "O n E B fmax pmax force -> local wide first_bits freq_bits rank_bits order_bits key64"."""
    sort_rows = set()
    for L in range(1, 22):
        p = pack5_bits(L)
        for ab in {1, 12, 36, 37, 62 - p, 63 - p, 64 - p, 65 - p, 66 - p, 63, 64}:
            if 1 <= ab <= 64:
                sort_rows.add((1, L, ab, 0))
        for ab, gb in grouped_bits(L) + ((20, 43), (20, 44), (20, 45), (63, 1), (64, 1), (32, 32), (32, 33), (12, 8)):
            for d in (-1, 0, 1):
                if 1 <= ab <= 64 and 0 <= gb + d <= 64:
                    sort_rows.add((1, L, ab, gb + d))
    for L in (22, 24, 42, 43, 63, 64, 65, 85):
        W = (3 * L + 63) // 64
        for ab, gb in ((1, 0), (20, 0), (60, 0), (61, 0), (62, 0), (64, 0), (40, 24), (40, 25), (64, 64), (1, 1), (1, 64)):
            sort_rows.add((W, L, ab, gb))
    order_rows = set()
    n17 = 1 << 17
    for n in (1, 2, 63, 64, 65, 2048, 16384, 16385, n17 - 1, n17, n17 + 1, 163839, 163840, 524800, (1 << 30) - 1):
        for fmax in (1, 2, 3, 1024, 32767, 32768, 32769, 65535, 65536, (1 << 30) - 1):
            if fmax <= n:
                order_rows.add((n, 1024 + 1, 1, fmax, 1024, 0))   # local, narrow or wide
                order_rows.add((n, 1024 + 1, 1, fmax, 1025, 0))   # one entry too many for a wave
                order_rows.add((n, 1024 + 1, 1, fmax, 1024, 1))   # the environment switch
    for B in (1, 2, 39, 40, 1 << 16, (1 << 16) + 1, n17 - 1, n17, n17 + 1):
        for fmax in (1, 32767, 32768, 65535, 65536):
            for E in (16 * B - 1, 16 * B, 16 * B + 1, B):
                for pmax in (1, 16, 1023, 1024, 1025):
                    order_rows.add((E + fmax - 1, E, B, fmax, pmax, 0))
    order_rows.add((0, 0, 0, 0, 0, 0))
    lines = []
    for r in sorted(sort_rows):
        p = sort_plan(*r)
        lines.append("S %d %d %d %d -> %d %d %d %d %d %d %d" % (r + (
            p["combine"], p["align_bits"], p["group_bits"], p["second_word"], p["p5_bits"], p["one_key"], p["composed_bits"])))
    for r in sorted(order_rows):
        p = order_plan(*r[:5], force_wide=bool(r[5]))
        lines.append("O %d %d %d %d %d %d -> %d %d %d %d %d %d %d" % (r + (
            p["local"], p["wide"], p["first_bits"], p["freq_bits"], p["rank_bits"], p["order_bits"], p["key64"])))
    return lines


# ---- from an input to what the reference says about it ----------------------------------------------

def key_bits(inp):
    return inp.bits if isinstance(inp.bits, tuple) else (inp.bits, 0)


def masked(key, bits):
    return key if bits >= 64 else key & U64((1 << bits) - 1)


def dense_ids(key):
    """ids numbered by first appearance"""
    _, first, inv = np.unique(key, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.uint32)


def reference(inp):
    """dict(keys, nmask, freq, rep, bucket_off) by the project's references, the keys masked here: the C
    restatement for one-word ungrouped calls, helpers.stage_model + the restated to_bitset for wide ones,
    helpers.grouped_stage_model for grouped ones."""
    import oracle as orc
    from helpers import grouped_stage_model, stage_model
    abits, gbits = key_bits(inp)
    a = masked(inp.align, abits)
    if inp.group is not None:
        return grouped_stage_model(a, inp.group, inp.umi, inp.score, inp.L, inp.merge, gbits)
    if inp.L <= 21:
        return orc.stage_reads(dense_ids(a), inp.umi, inp.score, inp.L, inp.merge)
    n = len(a)
    strings = [bytes(inp.umi[i * inp.L:(i + 1) * inp.L]).decode() for i in range(n)]
    umis, freq, rep, off = stage_model(dense_ids(a), strings, inp.score, inp.merge)
    keys, nmask = orc.encode_keys_wide(umis)
    return dict(keys=keys, nmask=nmask, freq=freq, rep=rep, bucket_off=off)


def merge_variants(inp):
    """merge 0 (any read), merge 1 with the scores, merge 1 without"""
    return (inp._replace(merge=0), inp._replace(merge=1), inp._replace(merge=1, score=None))


class SortedView(NamedTuple):
    perm: np.ndarray         # file index of every read in sorted order
    entry_start: np.ndarray  # sorted offsets at which an entry's run begins
    pos_start: np.ndarray    # ... at which a position begins


def sorted_view(inp):
    """The reads in (group, alignment, UMI, file index) order.  UMIs are compared as text here, which is not
    the library's order: the offsets hold for the library where a position has one entry, or entries of
    equal run length."""
    abits, gbits = key_bits(inp)
    n = len(inp.align)
    a = masked(inp.align, abits)
    g = masked(inp.group, gbits) if inp.group is not None and gbits else np.zeros(n, U64)
    u = inp.umi.reshape(n, inp.L)
    perm = np.lexsort([np.arange(n)] + [u[:, c] for c in range(inp.L - 1, -1, -1)] + [a, g])
    sa, sg, su = a[perm], g[perm], u[perm]
    new_pos = np.ones(n, bool)
    new_pos[1:] = (sa[1:] != sa[:-1]) | (sg[1:] != sg[:-1])
    new_ent = new_pos.copy()
    new_ent[1:] |= (su[1:] != su[:-1]).any(1)
    return SortedView(perm, np.nonzero(new_ent)[0], np.nonzero(new_pos)[0])


# ---- layouts -------------------------------------------------------------------------------------------

def umi_rows(idx, L):
    """UMI number idx in letters, base 0 the lowest digit"""
    return LETTERS[(np.asarray(idx, np.int64)[:, None] >> (2 * np.arange(L))) & 3]


def file_perm(n, order, seed=0):
    if order == "sorted":
        return np.arange(n)
    if order == "reversed":
        return np.arange(n)[::-1].copy()
    assert order == "shuffled"
    return np.random.default_rng(90000 + seed).permutation(n)


def from_layout(layout, order, bits="small", L=12, score="random", seed=0):
    """The reads of a layout (positions in ascending key order, each a list of run lengths) in a file order.
    bits: "small" = as many as number the positions (a composed sort key), or a count up to 64; position p
    of P has p in the top bits_for(P - 1) counted bits -- the highest counted bit is in use -- and a fixed
    scramble below; garbage above.  Entry j of position p has UMI number j + 7 p."""
    P = len(layout)
    sizes = np.array([len(p) for p in layout])
    runs = np.array([r for p in layout for r in p], np.int64)
    assert P and runs.min() >= 1 and sizes.max() <= 4 ** L
    pos_of_run = np.repeat(np.arange(P), sizes)
    j_of_run = np.arange(len(runs)) - np.repeat(np.cumsum(sizes) - sizes, sizes)
    run_of_read = np.repeat(np.arange(len(runs)), runs)
    n = len(run_of_read)
    pb = bits_for(P - 1)
    bits = pb if bits == "small" else bits
    assert pb <= bits <= 64
    shift = bits - pb
    p64 = np.arange(P, dtype=U64)
    key = (p64 << U64(shift)) | ((p64 * U64(0x9E3779B97F4A7C15)) & U64((1 << shift) - 1))
    rng = np.random.default_rng(1000 + seed)
    perm = file_perm(n, order, seed)
    align = key[pos_of_run[run_of_read]][perm]
    if bits < 64:
        align = align | (rng.integers(0, 1 << 63, n, dtype=U64) * U64(2) + rng.integers(0, 2, n, dtype=U64)) << U64(bits)
    umi = umi_rows(((j_of_run + 7 * pos_of_run) % 4 ** L)[run_of_read], L)[perm].reshape(-1)
    if isinstance(score, str):
        score = dict(random=lambda: rng.integers(0, 60, n), equal=lambda: np.full(n, 30),
                     extremes=lambda: rng.choice(np.array(EXTREMES, np.int64), n))[score]()
    return StageInput(align, None, umi, np.asarray(score).astype(np.int32), L, bits, 1)


def with_best_at(inp, offsets, base, best, view=None):
    """Scores: `best` at the reads at these offsets of the sorted order, `base` everywhere else"""
    score = np.full(len(inp.align), base, np.int64)
    score[(view or sorted_view(inp)).perm[list(offsets)]] = best
    return inp._replace(score=score.astype(np.int32))


# -- read counts
COUNTS = (1, 2, 63, 64, 65, 255, 256, 257, 511, 512, 2047, 2048, 2049, 4095, 4096, 4097, 16383, 16384, 16385)
ENDINGS = ("own_position", "new_entry", "same_entry")


def counts_layout(n, ending, deep=False):
    """n reads whose last sorted read is alone in a position of its own / a new entry of the last position
    (two entries of one read: whichever UMI sorts last) / one more read of the last entry.  Before it:
    positions of one UMI read 1, 2, 3, 5 times in turn, which go through the order sort; deep: positions of
    20 entries read once or twice each, the remainder as one run in front, which a wave each orders.  None
    where n is too small for the ending."""
    tail = dict(own_position=[[1]], new_entry=[[1, 1]], same_entry=[[2]])[ending]
    left = n - sum(map(sum, tail))
    if left < 0:
        return None
    body = []
    if deep:
        while left >= 20 * (1 + len(body) % 2):
            body.append([1 + len(body) % 2] * 20)
            left -= 20 * body[-1][0]
        if left:
            body.insert(0, [left])
    else:
        while left:
            body.append([min((1, 2, 3, 5)[len(body) % 4], left)])
            left -= body[-1][0]
    return body + tail


# -- entry runs over wave, round and tile boundaries
BOUNDARIES = (64, 256, 2048, 4096)


def boundary_layout(b, delta):
    """single reads, then two runs of m reads, the first ending and the second beginning at sorted offset
    b + delta, then ten single reads"""
    m = min(100, b // 2)
    return [[1]] * (b + delta - m) + [[m], [m]] + [[1]] * 10


LONG_RUN = [[1]] * 2040 + [[5000]] + [[1]] * 10   # offsets 2040 .. 7039: the tile 4096 .. 6143 has no head
TILE_RUN = [[1]] * 2048 + [[2048]] + [[1]] * 7    # exactly the second tile
# best scores inside LONG_RUN (sorted offsets): the run's first and last read, the last lane of a wave and the
# first of the next, equal best in two waves, in two tiles, on both sides of a tile edge
LONG_RUN_BEST = dict(first=(2040,), last=(7039,), wave_last_lane=(2047 + 640,), wave_first_lane=(2048 + 640,),
                     two_waves=(2100, 2164), two_tiles=(2041, 6500), tile_edge=(4095, 4096),
                     three=(7039, 3000, 5000))
SCORE_PAIRS = ((0, 1), (INT32_MIN, -1), (-1, 0), (1, INT32_MAX), (INT32_MIN, INT32_MAX), (INT32_MIN, INT32_MIN + 1))

# -- positions over tiles
POSITION_LAYOUTS = dict(
    three_tiles_of_single_reads=[[1]] * (3 * 2048),           # every pos_min slot; E < 16 B: the sort
    one_position_over_three_tiles=[[1] * 5000],               # reversed: its first read lies in its last tile
    many_heads_in_a_round=[[1] * 17] * 300,                   # fifteen position heads a round; E >= 16 B: a wave each
)

# -- the limits of the no-sort order
SIZES_IN_LDS = (1, 2, 3, 4, 5, 63, 64, 65, 127, 128, 129, 1021, 1022, 1023, 1024)


def varied(size, p):
    """run lengths 1 .. 4 that differ inside a position: freq order and first appearance both matter"""
    return [1 + (3 * j + p) % 4 for j in range(size)]


LOCAL_LAYOUTS = dict(
    largest_1023=[varied(1023, 0)] + [varied(16, p) for p in range(1, 9)],
    largest_1024=[varied(1024, 0)] + [varied(16, p) for p in range(1, 9)],
    largest_1025=[varied(1025, 0)] + [varied(16, p) for p in range(1, 9)],
    e_is_16b=[varied(16, p) for p in range(40)],
    e_is_16b_less_1=[varied(16, p) for p in range(39)] + [varied(15, 39)],
    lds_sizes=[varied(s, p) for p, s in enumerate(SIZES_IN_LDS)] + [varied(64, p) for p in range(15, 20)],
)
# one position of 1,024 entries, freq by first appearance in the file (from_first_appearance below)
FREQ_PATTERNS = dict(
    equal=[3] * 1024,
    falling=list(range(1024, 0, -1)),
    rising=list(range(1, 1025)),
    interleaved=[2 + 5 * (j % 2) for j in range(1024)],
)


def from_first_appearance(freqs, bits="small", L=12, seed=0):
    """One position whose entry j, in order of first appearance in the file, is read freqs[j] times: the
    first reads of all entries in that order, then every further read, shuffled."""
    E = len(freqs)
    first = np.arange(E)
    rest = np.repeat(np.arange(E), np.asarray(freqs) - 1)
    rng = np.random.default_rng(2000 + seed)
    ent = np.concatenate([first, rng.permutation(rest)])
    n = len(ent)
    bits = 1 if bits == "small" else bits
    align = np.full(n, 1, U64) << U64(bits - 1)
    if bits < 64:
        align = align | (rng.integers(0, 1 << 62, n, dtype=U64) << U64(bits))
    umi = umi_rows((ent * 2654435761) % 4 ** L, L).reshape(-1)  # (odd multiplier: distinct; no order in the keys)
    return StageInput(align, None, umi, rng.integers(0, 60, n).astype(np.int32), L, bits, 1)


# -- order-key widths
def width_layout(kind, fmax, positions=None):
    """local: 2^17 reads, one UMI read fmax times in a position of 1,024 entries, the rest single reads in
    positions of at most 1,024 -- bits_for(2^17 - 1) + bits_for(fmax) = 32 at fmax 32,767, 33 from 32,768,
    and fmax - 1 itself takes the 16th bit from 32,769.  sort: one UMI read fmax times and single-read
    positions, `positions` in all -- bits_for(fmax) + bits_for(positions - 1) bits of order key."""
    if kind == "local":
        left = (1 << 17) - fmax - 1023
        return [[fmax] + [1] * 1023] + [[1] * 1024] * (left // 1024) + ([[1] * (left % 1024)] if left % 1024 else [])
    return [[1]] * (positions // 2) + [[fmax]] + [[1]] * (positions - 1 - positions // 2)


WIDTH_CASES = dict(
    local_32767=("local", 32767, None), local_32768=("local", 32768, None), local_32769=("local", 32769, None),
    sort_32767=("sort", 32767, 1 << 17), sort_32768=("sort", 32768, 1 << 17),
    sort_65535=("sort", 65535, 1 << 16), sort_65535_one_more=("sort", 65535, (1 << 16) + 1),
)


# ---- inputs that are no layouts --------------------------------------------------------------------------

def random_umis(rng, count, L, n_frac=0.15):
    u = rng.choice(LETTERS, (count, L))
    u[rng.random((count, L)) < n_frac] = ord("N")
    return u


def composition(L, bits, seed=0, n=1200):
    """Key composition: bits = align bits, or (align bits, group bits).  Position keys come in pairs that
    differ only in the highest counted bit and only in bit 0 (of either key); every read has garbage of its
    own in every bit above the counted ones, so reads of one position differ there; a handful of UMIs over
    ACGTN per call, read a few times each."""
    rng = np.random.default_rng(3000 + 97 * L + seed)
    abits, gbits = bits if isinstance(bits, tuple) else (bits, 0)

    def values(b):
        top = 1 << (b - 1)
        r = [int(x) for x in rng.integers(0, 1 << 62, 1)]
        r = [(x << 2 | 2) & ((1 << b) - 1) for x in r]
        return sorted({v & ((1 << b) - 1) for x in [0] + r for v in (x, x ^ top, x ^ 1, x ^ top ^ 1)})

    def garbage(col, b):
        col = np.array(col, dtype=U64)
        if b < 64:
            col = col | ((rng.integers(0, 1 << 63, n, dtype=U64) * U64(2) + rng.integers(0, 2, n, dtype=U64)) << U64(b))
        return col
    av, gv = values(abits), values(gbits) if gbits else [0]
    pairs = [(a, g) for a in av for g in gv]
    pick = rng.integers(0, len(pairs), n)
    align = garbage([pairs[i][0] for i in pick], abits)
    group = garbage([pairs[i][1] for i in pick], gbits) if gbits else None
    pool = random_umis(rng, min(12, 5 ** L), L)
    umi = pool[rng.integers(0, len(pool), n)].reshape(-1)
    return StageInput(align, group, umi, rng.integers(0, 60, n).astype(np.int32), L,
                      (abits, gbits) if gbits else abits, 1)


def alphabet_umis(L, seed=0):
    """Every one of ACGTN at every base (the other bases random ACGT), and all 5^min(L, 3) fillings of the
    first three and of the last three bases: distinct UMIs, as rows of letters"""
    rng = np.random.default_rng(4000 + L + seed)
    rows = []
    for b in range(L):
        for c in LETTERS5:
            u = rng.choice(LETTERS, L)
            u[b] = c
            rows.append(u)
    m = min(L, 3)
    for f in range(5 ** m):
        fill = LETTERS5[[(f // 5 ** i) % 5 for i in range(m)]]
        for at in (0, L - m):
            u = rng.choice(LETTERS, L)
            u[at:at + m] = fill
            rows.append(u)
    return np.unique(np.array(rows), axis=0)


def alphabet(L, bits, seed=0):
    """alphabet_umis(L), each read 1 to 3 times in each of two positions, shuffled; the two position keys
    differ in the highest counted bit"""
    rng = np.random.default_rng(4100 + L + seed)
    u = alphabet_umis(L, seed)
    ent = np.concatenate([np.repeat(np.arange(len(u)), rng.integers(1, 4, len(u))) + p * len(u) for p in (0, 1)])
    ent = rng.permutation(ent)
    n = len(ent)
    align = (ent // len(u)).astype(U64) << U64(bits - 1)
    if bits > 1:
        align |= U64(1)
    if bits < 64:
        align = align | (rng.integers(0, 1 << 62, n, dtype=U64) << U64(bits))
    return StageInput(align, None, u[ent % len(u)].reshape(-1), rng.integers(0, 60, n).astype(np.int32), L, bits, 1)


WIDE_LENGTHS = (22, 42, 43, 63, 64, 65, 85)
WIDE_COUNTS = (255, 256, 257, 513)
WIDE_BASES = (20, 21, 40, 42, 60, 63, 64, 84)  # windows that cross a key word: 20, 40, 84 (encode), 21, 42, 63, 84 (N mask)


def wide(L, n, bits=(20, 0), seed=0):
    """UMIs of more than one key word with each of ACGTN at each of WIDE_BASES that L has (the other bases
    random ACGT), n reads of them over three positions (and, with group bits, two groups)"""
    rng = np.random.default_rng(5000 + 131 * L + n + seed)
    rows = []
    for b in WIDE_BASES:
        if b < L:
            for c in LETTERS5:
                u = rng.choice(LETTERS, L)
                u[b] = c
                rows.append(u)
    u = np.array(rows)
    abits, gbits = bits
    align = rng.integers(0, 3, n).astype(U64) << U64(abits - 2 if abits >= 2 else 0)
    group = None
    if abits < 64:
        align = align & U64((1 << abits) - 1) | (rng.integers(0, 1 << 62, n, dtype=U64) << U64(abits))
    if gbits:
        group = rng.integers(0, 2, n).astype(U64) << U64(gbits - 1)
        if gbits < 64:
            group = group | (rng.integers(0, 1 << 62, n, dtype=U64) << U64(gbits))
    umi = u[rng.integers(0, len(u), n)].reshape(-1)
    return StageInput(align, group, umi, rng.integers(0, 60, n).astype(np.int32), L, bits if gbits else abits, 1)


# -- whole reads (umi_stage_seqs): one length, four sequences that differ in base 0 alone
SEQ_TAIL = b"CATTAGGACCAGTTACGGATCCATGAACGTTGCAAGCT" * 2
SEQS_IN_ORDER = [c + SEQ_TAIL for c in (b"A", b"G", b"T", b"C")]  # codes 0 3 5 6: the order of the key words


def seq_reads(run_lengths, order, seed=0):
    """Reads of one length: SEQS_IN_ORDER[j] run_lengths[j] times, so that run j begins at sorted offset
    sum(run_lengths[:j]); qualities random.  Returns (seqs, quals) in file order."""
    rng = np.random.default_rng(6000 + seed)
    which = np.repeat(np.arange(len(run_lengths)), run_lengths)[file_perm(sum(run_lengths), order, seed)]
    seqs = [SEQS_IN_ORDER[j] for j in which]
    quals = [bytes(q) for q in rng.integers(33, 75, (len(seqs), len(seqs[0])), dtype=np.uint8)]
    return seqs, quals


# run lengths whose boundaries fall on 63 / 64 / 65 and 2,047 / 2,048 / 2,049, for n = 2,047, 2,048, 2,049 and beyond
SEQ_RUNS = {
    "n2047": (63, 1, 1, 1982), "n2048": (64, 1, 1983), "n2049": (65, 1983, 1),
    "cut2047": (2047, 1, 1, 70), "cut2048": (64, 1984, 70), "cut2049": (63, 1986, 130, 1),
}
