"""Test-side model of umi_correct_barcodes_multi (include/umihip.h), twice, and the makers of the tests' inputs.

The rule (this build's definition, after STARsolo's 1MM_multi[_pseudocounts]).  Per call: n reads of L bases (ACGTN),
their qualities (L bytes each, Phred + 33, 33..126), the list, min_posterior_permille and pseudocount, both 0..1000.

 1. every read gets barcode_model.correct's verdict with max_mismatches 1; exact, corrected and none are final
    (a single candidate is accepted whatever its count);
 2. exact_reads[e] = the reads of this call that are exact with match e;
 3. an ambiguous read's candidates are the listed barcodes one substitution away (one N: those that agree
    everywhere else), each with its mismatched position p and the weight
        w_e = (exact_reads[e] + pseudocount) * T[min(qual[p] - 33, 40)],   T[q] = round(2^26 * 10^(-q / 10));
 4. W = sum of the weights, e* = the candidate of greatest weight, the smallest index on ties; where W > 0 and
    1000 * w_e* >= min_posterior_permille * W the read is resolved (status 4, match e*), otherwise it stays
    ambiguous (status 3, match -1);
 5. counts[5]: the reads per status.

correct_multi() is that with a dict of the listed strings and the substitutions written out;
correct_multi_bruteforce() takes all-pairs Hamming distances in numpy; both weigh in Python ints."""
import functools

import numpy as np

import barcode_model as bm

EXACT, CORRECTED, NONE, AMBIGUOUS, RESOLVED = 0, 1, 2, 3, 4

T = (67108864, 53306465, 42342831, 33634106, 26716520, 21221686, 16856984, 13389979, 10636038, 8448505, 6710886,
     5330647, 4234283, 3363411, 2671652, 2122169, 1685698, 1338998, 1063604, 844851, 671089, 533065,
     423428, 336341, 267165, 212217, 168570, 133900, 106360, 84485, 67109, 53306, 42343,
     33634, 26717, 21222, 16857, 13390, 10636, 8449, 6711)


def table_from_formula():
    """T from its formula; no entry lies near a half, so the rounding does not hang on the last bit of a float"""
    out = []
    for q in range(41):
        x = 2.0 ** 26 * 10.0 ** (-q / 10.0)
        assert abs((x % 1.0) - 0.5) > 1e-6, (q, x)
        out.append(int(round(x)))
    return tuple(out)


def decide(cands, exact_reads, qual_row, permille, pseudocount):
    """(status, match) of an ambiguous read from its candidates [(entry, position)]"""
    w = {e: (int(exact_reads[e]) + pseudocount) * T[min(int(qual_row[p]) - 33, 40)] for e, p in cands}
    W = sum(w.values())
    best = min(w, key=lambda e: (-w[e], e))
    if W > 0 and 1000 * w[best] >= permille * W:
        return RESOLVED, best
    return AMBIGUOUS, -1


def _result(match, status, exact_reads):
    match, status = np.asarray(match, np.int32), np.asarray(status, np.uint8)
    return {"match": match, "status": status, "counts": np.bincount(status, minlength=5).astype(np.uint64),
            "exact_reads": np.asarray(exact_reads, np.uint32)}


def _check(reads, quals, L, permille, pseudocount):
    u, q = bm.as_rows(reads, L), bm.as_rows(quals, L)
    assert u.shape == q.shape and 0 <= permille <= 1000 and 0 <= pseudocount <= 1000
    assert not len(q) or (q.min() >= 33 and q.max() <= 126)
    return u, q


def correct_multi(reads, quals, L, whitelist, permille=975, pseudocount=0):
    """dict(match, status, counts, exact_reads) as Context.correct_barcodes_multi returns it, from the definition"""
    u, q = _check(reads, quals, L, permille, pseudocount)
    wl = [bytes(r) for r in bm.as_rows(whitelist, L)]
    index = {w: i for i, w in enumerate(wl)}
    first = bm.correct(u.reshape(-1), L, whitelist, 1)
    match, status = first["match"].copy(), first["status"].copy()
    exact_reads = np.bincount(match[status == EXACT], minlength=len(wl))
    for i in np.flatnonzero(status == AMBIGUOUS):
        r = bytes(u[i])
        cands = []
        for p in ([r.index(b"N")] if b"N" in r else range(L)):
            for c in b"ACGT":
                v = r[:p] + bytes([c]) + r[p + 1:]
                if c != r[p] and v in index:
                    cands.append((index[v], p))
        assert len(cands) >= 2
        status[i], match[i] = decide(cands, exact_reads, q[i], permille, pseudocount)
    return _result(match, status, exact_reads)


def correct_multi_bruteforce(reads, quals, L, whitelist, permille=975, pseudocount=0):
    """the same from the Hamming distance of every read to every entry"""
    u, q = _check(reads, quals, L, permille, pseudocount)
    w = bm.as_rows(whitelist, L)
    n, n_wl = len(u), len(w)
    match, status = np.full(n, -1, np.int32), np.full(n, NONE, np.uint8)
    cands = {}
    chunk = max(1, (1 << 25) // (n_wl * L))
    for lo in range(0, n, chunk):
        diff = u[lo:lo + chunk, None, :] != w[None, :, :]
        d = diff.sum(axis=2)
        for j in range(len(d)):
            zero, one = np.flatnonzero(d[j] == 0), np.flatnonzero(d[j] == 1)
            if len(zero):
                status[lo + j], match[lo + j] = EXACT, zero[0]
            elif len(one) == 1:
                status[lo + j], match[lo + j] = CORRECTED, one[0]
            elif len(one) > 1:
                status[lo + j] = AMBIGUOUS
                cands[lo + j] = [(int(e), int(diff[j, e].argmax())) for e in one]
    exact_reads = np.bincount(match[status == EXACT], minlength=n_wl)
    for i, c in cands.items():
        status[i], match[i] = decide(c, exact_reads, q[i], permille, pseudocount)
    return _result(match, status, exact_reads)


# ---- inputs -----------------------------------------------------------------------------------------------
# Phred values a quality byte is drawn from: the table's ends, values across it, and two beyond the cap
QUALS = np.array([0, 2, 12, 20, 30, 37, 40, 41, 60, 93], np.uint8) + 33


def random_quals(rng, n, L):
    return QUALS[rng.integers(0, len(QUALS), n * L)]


def multi_reads(rng, wl, n, pairs, deep=0.25, **kw):
    """listed_reads, a fraction `deep` of them replaced by exact reads of a few pair members (so that candidates
    differ in their counts), and random qualities"""
    w = np.asarray(wl, np.uint8)
    L = w.shape[1]
    u = bm.listed_reads(rng, w, n, pairs, ambiguous=0.2, **kw).reshape(-1, L)
    if len(pairs):
        few = [pairs[int(k)][int(rng.integers(0, 2))] for k in rng.integers(0, len(pairs), 1 + len(pairs) // 3)]
        for i in np.flatnonzero(rng.random(n) < deep):
            u[i] = w[few[int(rng.integers(0, len(few)))]]
    return u.reshape(-1), random_quals(rng, n, L)


def two_pass_case(rng):
    """L = 32: 96 variants, two passes of 64 (positions 0..20 in the first, 22..31 in the second, 21 across both).
    Unlisted reads whose listed neighbours lie only in the first pass, only in the second, and in both."""
    L = 32
    groups = [(1, 7), (0, 20), (3, 9, 14), (22, 31), (25, 28), (23, 27, 30), (2, 26), (20, 22), (0, 31), (5, 12, 24, 29),
              (21, 4), (21, 30), (21, 10, 25)]
    wl, reads = [], []
    for g in groups:
        for _ in range(6):
            r = bm.ACGT[rng.integers(0, 4, L)]
            mine = []
            for p in g:
                v = r.copy()
                v[p] = bm.ACGT[(np.searchsorted(bm.ACGT, v[p]) + rng.integers(1, 4)) % 4]
                mine.append(len(wl))
                wl.append(v)
            reads.append(r)
            for e in mine:  # exact reads of the neighbours, in different numbers
                reads += [wl[e]] * int(rng.integers(0, 4))
    wl = np.array(wl, np.uint8)
    assert len(set(map(bytes, wl))) == len(wl)
    order = rng.permutation(len(reads))
    u = np.array(reads, np.uint8)[order]
    return wl, u.reshape(-1), random_quals(rng, len(u), L)


def one_n_full_case(rng, n=1000):
    """full_list(3), every read with one N: four candidates, all listed, one quality for all bytes -- the counts
    alone decide.  Exact reads fall on few barcodes, so that some N reads have one heavy candidate."""
    wl, _ = bm.full_list(3)
    u = wl[rng.integers(0, 64, n)].copy()
    heavy = rng.random(n) < 0.93
    u[heavy] = wl[rng.choice([5, 17, 40], int(heavy.sum()))]
    with_n = np.flatnonzero(rng.random(n) < 0.3)
    u[with_n, rng.integers(0, 3, len(with_n))] = ord("N")
    return wl, u.reshape(-1), np.full(n * 3, 33 + 30, np.uint8)


def hot_case(rng, n=10000, hot=8000):
    """one barcode carries `hot` of n exact reads: the histogram's hot address"""
    wl, pairs = bm.random_list(rng, 64, 16)
    u, q = multi_reads(rng, wl, n, pairs)
    u = u.reshape(n, 16)
    u[rng.permutation(n)[:hot]] = wl[pairs[0][0]]
    return wl, u.reshape(-1), q


def no_exact_case(rng, n=600):
    """no read is exact: every count is 0"""
    wl, pairs = bm.random_list(rng, 64, 16)
    u, q = multi_reads(rng, wl, n, pairs, deep=0.0)
    u = u.reshape(n, 16)
    listed = set(map(bytes, wl))
    u = u[[bytes(r) not in listed for r in u]]
    return wl, u.reshape(-1), q[:u.size]


N_READS = (0, 1, 63, 64, 65, 10000)


# name -> (kind, L, list [n_wl, L], reads [n * L], quals [n * L]); kind "all": at least 8 reads of each of the five
# statuses under the default parameters (tests/test_barcode_multi_model_cpu.py checks it); "some": whatever occurs
@functools.lru_cache(maxsize=None)
def gpu_inputs():
    cases = {}

    def add(name, kind, L, wl_pairs, n, seed):
        wl, pairs = wl_pairs
        cases[name] = (kind, L, wl) + multi_reads(np.random.default_rng(seed), wl, n, pairs)

    for L in (2, 16, 17, 32):
        rng = np.random.default_rng(1100 + L)
        add("L%d" % L, "some" if L == 2 else "all", L, bm.random_list(rng, 12 if L == 2 else 5003, L), 2000, 1200 + L)
    for n_wl in (2, 64):
        rng = np.random.default_rng(1300 + n_wl)
        add("n_wl%d" % n_wl, "some" if n_wl == 2 else "all", 16, bm.random_list(rng, n_wl, 16), 1500, 1400 + n_wl)
    # (clustered lists hold every variant of six bases: few reads have two neighbours without being listed)
    add("clustered_low", "some", 16, bm.clustered_list(16, "low"), 3000, 1501)
    add("clustered_high", "some", 16, bm.clustered_list(16, "high"), 3000, 1502)
    add("reads10000", "all", 16, bm.random_list(np.random.default_rng(1600), 4999, 16), 10000, 1601)
    cases["two_pass_L32"] = ("some", 32) + two_pass_case(np.random.default_rng(1700))
    cases["full3_one_n"] = ("some", 3) + one_n_full_case(np.random.default_rng(1701))
    cases["hot"] = ("some", 16) + hot_case(np.random.default_rng(1702))
    cases["no_exact"] = ("some", 16) + no_exact_case(np.random.default_rng(1703))
    return cases


@functools.lru_cache(maxsize=None)
def expected(name, permille=975, pseudocount=0):
    """the model's answer for a GPU input, computed once per process"""
    _, L, wl, reads, quals = gpu_inputs()[name]
    return correct_multi(reads, quals, L, wl, permille, pseudocount)


# ---- hand-made cases: (list, reads, qualities as Phred values per base, permille, pseudocount, status and match of
# the last read).  The reads before the last are exact and give the candidates their counts.
def _q(*phred):
    return bytes(33 + p for p in phred)


def hand_cases():
    wl = ["AAAA", "CAAA", "AACA"]
    cases = {}
    # candidates 0 and 1 through position 0 (one quality): 39 against 1, 1000 * 39 == 975 * 40 exactly -> accepted
    cases["threshold_met"] = (wl, ["AAAA"] * 39 + ["CAAA"] + ["GAAA"], 975, 0, RESOLVED, 0)
    # 38 against 1: 1000 * 38 = 38000 < 975 * 39 = 38025 -> ambiguous
    cases["threshold_missed"] = (wl, ["AAAA"] * 38 + ["CAAA"] + ["GAAA"], 975, 0, AMBIGUOUS, -1)
    # permille 999: 999 against 1 meets it exactly (999000 = 999 * 1000); 998 against 1 is one unit below
    # (998000 = 999 * 999 - 1, in units of the shared T[q])
    cases["threshold_999_met"] = (wl, ["AAAA"] * 999 + ["CAAA"] + ["GAAA"], 999, 0, RESOLVED, 0)
    cases["threshold_999_one_below"] = (wl, ["AAAA"] * 998 + ["CAAA"] + ["GAAA"], 999, 0, AMBIGUOUS, -1)
    cases["equal_weights_500"] = (wl, ["AAAA"] * 3 + ["CAAA"] * 3 + ["GAAA"], 500, 0, RESOLVED, 0)
    cases["equal_weights_0"] = (wl, ["AAAA"] * 3 + ["CAAA"] * 3 + ["GAAA"], 0, 0, RESOLVED, 0)
    cases["equal_weights_501"] = (wl, ["AAAA"] * 3 + ["CAAA"] * 3 + ["GAAA"], 501, 0, AMBIGUOUS, -1)
    cases["permille_1000_sole_weight"] = (wl, ["CAAA"] * 2 + ["GAAA"], 1000, 0, RESOLVED, 1)
    cases["permille_1000_shared"] = (wl, ["AAAA"] * 500 + ["CAAA"] + ["GAAA"], 1000, 0, AMBIGUOUS, -1)
    cases["permille_0_no_weight"] = (wl, ["GAAA"], 0, 0, AMBIGUOUS, -1)   # W = 0
    cases["pseudocount_1_no_exact"] = (wl, ["GAAA"], 500, 1, RESOLVED, 0)  # equal weights again
    cases["pseudocount_0_no_exact"] = (wl, ["GAAA"], 500, 0, AMBIGUOUS, -1)
    return {k: (v[0], v[1], None) + v[2:] for k, v in cases.items()}


def hand_quality_cases():
    """the read CACA has CAAA (entry 1) through position 2 and AACA (entry 2) through position 0, one exact read
    each: the qualities at positions 0 and 2 decide.  (list, reads, quals, permille, pseudocount, status, match)"""
    wl = ["AAAA", "CAAA", "AACA"]
    reads = ["CAAA", "AACA", "CACA"]  # one exact read each; CACA: CAAA (entry 1) at p = 2, AACA (entry 2) at p = 0
    cases = {}
    for name, q0, q2 in (("cap_40", 40, 0), ("cap_93", 93, 0)):
        # w_1 = T[q2] = 2^26, w_2 = T[40] = 6711 both times: entry 1 wins
        cases[name] = (wl, reads, [_q(9, 9, 9, 9)] * 2 + [_q(q0, 9, q2, 9)], 975, 0, RESOLVED, 1)
    cases["quality_byte_33_both"] = (wl, reads, [_q(0, 0, 0, 0)] * 3, 500, 0, RESOLVED, 1)  # equal: smaller index
    cases["quality_byte_33_one"] = (wl, reads, [_q(9, 9, 9, 9)] * 2 + [_q(0, 9, 20, 9)], 975, 0, RESOLVED, 2)
    cases["quality_near"] = (wl, reads, [_q(9, 9, 9, 9)] * 2 + [_q(20, 9, 30, 9)], 975, 0, AMBIGUOUS, -1)
    return cases
