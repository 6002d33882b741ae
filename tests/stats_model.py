"""Test-side definition of umi_dedup_stats (csrc/umihip_stats.hip) and of the three files of --output-stats
(host/umicollapse_main.cpp), in plain Python and numpy, independent of the library.

Family sizes: count_pre[min(freq[i], bins - 1)] counts every entry; total[r] is the sum of freq over root[i] == r,
count_post[min(total[i], bins - 1)] counts every kept entry.

Distances: a UMI's letter at base b is the 3-bit code at bits [3b, 3b + 3) of its key read as one little-endian
integer (000 A, 110 C, 011 G, 101 T, 100 N); two letters differ iff their codes differ.  Pair distances are taken
pair by pair on the decoded letters.  A set of m UMIs gives nothing for m = 0, "single" for m = 1, else bin
ceil(S / P) with S the sum of the pair distances and P = m (m - 1) / 2, in Python integers.  Per non-empty bucket
[s, e) with m kept entries: pre all its entries, post the kept ones, pre-null the entries pick(i) for i in [s, e),
post-null pick(i) for i in [s, s + m).  pick() is taken straight from its formula.

The per-UMI table is built from a dict keyed by the key as an integer."""
import numpy as np

CODE_LETTER = {0: "A", 6: "C", 3: "G", 5: "T", 4: "N"}
LETTER_CODE = {v: k for k, v in CODE_LETTER.items()}
M64 = (1 << 64) - 1


def n_words_of(umi_len):
    return (3 * umi_len + 63) // 64


def key_int(keys, i, n_words):
    """entry i's key as one little-endian integer"""
    return sum(int(keys[i * n_words + w]) << (64 * w) for w in range(n_words))


def decode(keys, i, umi_len, n_words):
    v = key_int(keys, i, n_words)
    return "".join(CODE_LETTER[(v >> (3 * b)) & 7] for b in range(umi_len))


def encode(umis, umi_len):
    """UMI strings -> keys uint64 [len(umis) * n_words]"""
    nw = n_words_of(umi_len)
    out = np.zeros(len(umis) * nw, np.uint64)
    for i, u in enumerate(umis):
        assert len(u) == umi_len
        v = sum(LETTER_CODE[ch] << (3 * b) for b, ch in enumerate(u))
        for w in range(nw):
            out[i * nw + w] = (v >> (64 * w)) & M64
    return out


def pair_sum(umis):
    """S: the sum of the letter distances over all pairs, pair by pair (every UMI against all behind it at once)"""
    if len(umis) < 2:
        return 0
    a = np.frombuffer("".join(umis).encode(), np.uint8).reshape(len(umis), -1)
    return sum(int(np.count_nonzero(a[i + 1:] != a[i])) for i in range(len(umis) - 1))


def column_sum(umis):
    """the same by the column identity: per base C(m, 2) - sum over letters C(count, 2)"""
    m = len(umis)
    s = 0
    for b in range(len(umis[0]) if umis else 0):
        counts = {}
        for u in umis:
            counts[u[b]] = counts.get(u[b], 0) + 1
        s += m * (m - 1) // 2 - sum(c * (c - 1) // 2 for c in counts.values())
    return s


def bin_of(umis, umi_len):
    """the column of dist a set goes to, None for an empty set"""
    m = len(umis)
    if m == 0:
        return None
    if m == 1:
        return umi_len + 1
    p = m * (m - 1) // 2
    return (pair_sum(umis) + p - 1) // p


def pick(i, seed, cum):
    """an entry drawn with probability proportional to its reads; cum: the inclusive scan of freq as Python ints"""
    x = (seed + 0x9E3779B97F4A7C15 * (i + 1)) & M64
    x ^= x >> 30
    x = (x * 0xBF58476D1CE4E5B9) & M64
    x ^= x >> 27
    x = (x * 0x94D049BB133111EB) & M64
    x ^= x >> 31
    t = (x * cum[-1]) >> 64
    lo, hi = 0, len(cum) - 1
    while lo < hi:
        mid = (lo + hi) // 2
        if cum[mid] > t:
            hi = mid
        else:
            lo = mid + 1
    return lo


def stats_model(keys, freq, kept, root, bucket_off, umi_len, n_words=None, seed=0, hist_bins=65536, per_umi=True):
    """umi_dedup_stats: dict of count_pre, count_post, dist and (per_umi) the five arrays of the table"""
    nw = n_words or n_words_of(umi_len)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    freq = [int(f) for f in np.asarray(freq)]
    kept = [int(k) != 0 for k in np.asarray(kept)]
    root = [int(r) for r in np.asarray(root)]
    off = [int(o) for o in np.asarray(bucket_off)]
    n = off[-1] if off else 0
    count_pre, count_post = np.zeros(hist_bins, np.uint64), np.zeros(hist_bins, np.uint64)
    dist = np.zeros((4, umi_len + 2), np.uint64)
    total = [0] * n
    for i in range(n):
        total[root[i]] += freq[i]
        count_pre[min(freq[i], hist_bins - 1)] += 1
    for i in range(n):
        if kept[i]:
            count_post[min(total[i], hist_bins - 1)] += 1
    cum, c = [], 0
    for i in range(n):
        c += freq[i]
        cum.append(c)
    umis = [decode(keys, i, umi_len, nw) for i in range(n)]
    for b in range(len(off) - 1):
        s, e = off[b], off[b + 1]
        if s == e:
            continue
        m = sum(kept[s:e])
        drawn = [umis[pick(i, seed, cum)] for i in range(s, e)]
        sets = (umis[s:e], drawn, [umis[i] for i in range(s, e) if kept[i]], drawn[:m])
        for row, members in enumerate(sets):
            col = bin_of(members, umi_len)
            if col is not None:
                dist[row, col] += 1
    out = {"count_pre": count_pre, "count_post": count_post, "dist": dist}
    if per_umi:
        table = {}
        for i in range(n):
            r = table.setdefault(key_int(keys, i, nw), [i, 0, 0, 0, 0])
            r[1] += 1
            r[2] += freq[i]
            if kept[i]:
                r[3] += 1
                r[4] += total[i]
        rows = [table[k] for k in sorted(table)]
        for j, (name, ty) in enumerate((("umi_entry", np.uint32), ("times_pre", np.uint32), ("reads_pre", np.uint64),
                                        ("times_post", np.uint32), ("reads_post", np.uint64))):
            out[name] = np.array([r[j] for r in rows], ty)
    return out


# ---- the three files of --output-stats PREFIX
def per_position_text(count_pre, count_post):
    """PREFIX_per_umi_per_position.tsv: a row per count with a non-zero instance, ascending; the last bin, if it took
    anything, reads "<bins - 1>+" """
    lines = ["counts\tinstances_pre\tinstances_post"]
    bins = len(count_pre)
    for c in range(bins):
        if int(count_pre[c]) or int(count_post[c]):
            lines.append("%d%s\t%d\t%d" % (c, "+" if c == bins - 1 else "", int(count_pre[c]), int(count_post[c])))
    return "\n".join(lines) + "\n"


def edit_distance_text(dist, algo):
    """PREFIX_edit_distance.tsv: rows 0..umi_len, all of them, then Single_UMI; columns pre, pre-null, post, post-null"""
    lines = ["edit_distance\tunique\tunique_null\t%s\t%s_null" % (algo, algo)]
    umi_len = dist.shape[1] - 2
    for j in range(umi_len + 2):
        name = str(j) if j <= umi_len else "Single_UMI"
        lines.append("%s\t%d\t%d\t%d\t%d" % (name, int(dist[0, j]), int(dist[1, j]), int(dist[2, j]), int(dist[3, j])))
    return "\n".join(lines) + "\n"


def per_umi_text(res, keys, umi_len, n_words=None):
    """PREFIX_per_umi.tsv: the table's rows in the library's order, the UMI decoded from keys[umi_entry]"""
    nw = n_words or n_words_of(umi_len)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    lines = ["UMI\ttimes_observed_pre\ttotal_counts_pre\ttimes_observed_post\ttotal_counts_post"]
    for j in range(len(res["umi_entry"])):
        lines.append("%s\t%d\t%d\t%d\t%d" % (decode(keys, int(res["umi_entry"][j]), umi_len, nw), int(res["times_pre"][j]),
                                             int(res["reads_pre"][j]), int(res["times_post"][j]), int(res["reads_post"][j])))
    return "\n".join(lines) + "\n"


def program_hist_bins(freq, bucket_off):
    """what the program passes: min(2^22, 2 + the largest bucket's reads)"""
    freq, off = np.asarray(freq, np.int64), [int(o) for o in np.asarray(bucket_off)]
    most = max([int(freq[off[b]:off[b + 1]].sum()) for b in range(len(off) - 1)] + [0])
    return min(1 << 22, 2 + most)


def stats_files(keys, freq, kept, root, bucket_off, umi_len, algo, seed=0, n_words=None):
    """the three files' texts as the program writes them: (per_umi_per_position, edit_distance, per_umi)"""
    res = stats_model(keys, freq, kept, root, bucket_off, umi_len, n_words, seed, program_hist_bins(freq, bucket_off), True)
    return (per_position_text(res["count_pre"], res["count_post"]), edit_distance_text(res["dist"], algo),
            per_umi_text(res, keys, umi_len, n_words))
