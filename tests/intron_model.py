"""Test-side definition of umi_assign_genes_introns / --gene-introns (include/umihip.h has the same rule), in plain
Python over tests/annotation_model.py, and the makers of the tests' inputs.

Blocks of a read, exon lines, admissible strands and the set E of genes that hit a read are annotation_model's
(umi_assign_genes'), unchanged.  New:
  Gene body: group the taken lines of a gene by (reference, strand as written: +, - or .).  Each group gives one
    body, [min start, max end) over the group's lines.  The minimum and maximum may come from different lines.  A gene
    with lines on two references, or on + and ., has one body per group.  No gene or transcript lines are needed.
  B: the genes with a body on the read's reference, on an admissible strand (same rule as exons, and a . body is
    always admissible), that shares at least one base with one of the read's blocks.  E is a subset of B.
  exon-first (STARsolo's GeneFull_ExonOverIntron, stated with this project's overlap-of-one rule):
    |E| = 1: assigned to that gene, tier exon.  |E| >= 2: several.  |E| = 0 and |B| = 1: assigned, tier intron.
    |E| = 0 and |B| = 0: none.  |E| = 0 and |B| >= 2: several.
  all (plain GeneFull on derived bodies):
    |B| = 1: assigned, tier exon if E is not empty, else intron.  |B| = 0: none.  |B| >= 2: several.
  off: umi_assign_genes's result, every assigned read tier exon.
The minimum overlap is 1 throughout: a block that starts in an exon and runs into the intron is tier exon.
The tier of a read that is not assigned is 0."""
import functools
import struct

import numpy as np

import annotation_model as am
import bamio

ASSIGNED, NONE, SEVERAL = am.ASSIGNED, am.NONE, am.SEVERAL
TIER_EXON, TIER_INTRON = 0, 1
OFF, EXON_FIRST, ALL = 0, 1, 2
INTRONS = {"off": OFF, "exon-first": EXON_FIRST, "all": ALL}
GENE_BODY_TOP_CAP = 512   # sampled segment ends of a body table in LDS, at most (csrc/umihip_internal.h)
TOP = 2 ** 31 - 1         # the largest end a line can have


def bodies(exons):
    """the bodies of the lines, as lines (ref, start, end, strand, gene), in the order their groups first appear"""
    span = {}
    for ref, s, e, strand, g in exons:
        lo, hi = span.get((g, ref, strand), (s, e))
        span[(g, ref, strand)] = (min(lo, s), max(hi, e))
    return [(ref, lo, hi, strand, g) for (g, ref, strand), (lo, hi) in span.items()]


def hits(lines, ref, pos, reverse, cigar, mode):
    """the genes with a line on ref, on an admissible strand, that shares a base with a block of the read"""
    out = set()
    for s, e in am.blocks(pos, cigar):
        for xr, xs, xe, xstrand, g in lines:
            if xr == ref and am.admissible(xstrand, reverse, mode) and xs < e and s < xe:
                out.add(g)
    return out


def verdict(E, B, introns):
    """(status, gene, tier) from the two sets, the rule word for word"""
    one = lambda s: next(iter(s))
    if introns == OFF:
        return (ASSIGNED, one(E), TIER_EXON) if len(E) == 1 else (NONE, -1, 0) if not E else (SEVERAL, -1, 0)
    if introns == EXON_FIRST:
        if len(E) == 1:
            return ASSIGNED, one(E), TIER_EXON
        if len(E) >= 2:
            return SEVERAL, -1, 0
        if len(B) == 1:
            return ASSIGNED, one(B), TIER_INTRON
        return (NONE, -1, 0) if not B else (SEVERAL, -1, 0)
    assert introns == ALL
    if len(B) == 1:
        return ASSIGNED, one(B), TIER_EXON if E else TIER_INTRON
    return (NONE, -1, 0) if not B else (SEVERAL, -1, 0)


def assign(exons, ref, pos, reverse, cigar, mode, introns):
    """(status, gene, tier) of one read, line by line"""
    return verdict(hits(exons, ref, pos, reverse, cigar, mode), hits(bodies(exons), ref, pos, reverse, cigar, mode), introns)


def hit_sets(lines, reads, mode):
    """hits() of every read, the lines of a read's reference and admissible strands held in arrays"""
    by = {}
    for xr, xs, xe, xstrand, g in lines:
        for rev in (0, 1):
            if am.admissible(xstrand, rev, mode):
                by.setdefault((xr, rev), []).append((xs, xe, g))
    by = {k: np.array(v, np.int64) for k, v in by.items()}
    out = []
    for ref, pos, rev, cigar in reads:
        x = by.get((ref, 1 if rev else 0))
        hit = set()
        if x is not None:
            for s, e in am.blocks(pos, cigar):
                hit.update(x[(x[:, 0] < e) & (s < x[:, 1]), 2].tolist())
        out.append(hit)
    return out


def assign_all(exons, reads, mode, introns):
    """dict(gene int32, status uint8, tier uint8, counts uint64 [4]: by exon, by intron, none, several)"""
    E, B = hit_sets(exons, reads, mode), hit_sets(bodies(exons), reads, mode)
    gene, status, tier = np.full(len(reads), -1, np.int32), np.zeros(len(reads), np.uint8), np.zeros(len(reads), np.uint8)
    for i in range(len(reads)):
        status[i], gene[i], tier[i] = verdict(E[i], B[i], introns)
    return {"gene": gene, "status": status, "tier": tier, "counts": counts_of(status, tier)}


def counts_of(status, tier):
    status, tier = np.asarray(status), np.asarray(tier)
    return np.array([((status == ASSIGNED) & (tier == TIER_EXON)).sum(), ((status == ASSIGNED) & (tier == TIER_INTRON)).sum(),
                     (status == NONE).sum(), (status == SEVERAL).sum()], np.uint64)


@functools.lru_cache(maxsize=None)
def fuzz_expected(mode, introns):
    return assign_all(am.fuzz_annotation(), am.fuzz_reads(), mode, introns)


def fuzz_classes(mode):
    """the reads of the fuzz input by what the two rules make of them: tier intron (under exon-first), rescued by
    exon-first (several under all, assigned under exon-first), several under both, none (under both: B is empty)"""
    first, full = fuzz_expected(mode, EXON_FIRST), fuzz_expected(mode, ALL)
    return {"intron": int(((first["status"] == ASSIGNED) & (first["tier"] == TIER_INTRON)).sum()),
            "rescued": int(((first["status"] == ASSIGNED) & (full["status"] == SEVERAL)).sum()),
            "several": int(((first["status"] == SEVERAL) & (full["status"] == SEVERAL)).sum()),
            "none": int(((first["status"] == NONE) & (full["status"] == NONE)).sum())}


# ---- the hand-written cases -----------------------------------------------------------------------------

def M(pos, length=20, ref=0, rev=False):
    return (ref, pos, rev, (("M", length),))


# reference 0: gene 1 nested in gene 0's intron, same strand.  1: gene 3 nested in gene 2's intron, opposite strands.
# 2: genes 4 and 5 with overlapping exons.  3: genes 6 and 7 side by side.  4: gene 8, its body's ends from different
# lines (the line with the largest end comes first, the one with the smallest start last); gene 9 on + and on '.'.
# 5: gene 9 again.  6: gene 10 at coordinate 0, gene 11 at the top coordinate.  7, 9: no lines (8: gene 12, one exon)
HAND_EXONS = (
    (0, 100, 200, "+", 0), (0, 800, 900, "+", 0), (0, 400, 450, "+", 1), (0, 500, 550, "+", 1),
    (1, 100, 200, "+", 2), (1, 800, 900, "+", 2), (1, 400, 450, "-", 3), (1, 500, 550, "-", 3),
    (2, 100, 200, "+", 4), (2, 150, 250, "+", 5), (2, 300, 350, "+", 5),
    (3, 100, 150, "+", 6), (3, 300, 350, "+", 6), (3, 500, 550, "+", 7), (3, 700, 750, "+", 7),
    (4, 250, 300, "-", 8), (4, 180, 200, "-", 8), (4, 100, 150, "-", 8),
    (4, 1000, 1050, "+", 9), (4, 1200, 1250, "+", 9), (4, 1500, 1550, ".", 9), (4, 1700, 1750, ".", 9),
    (5, 100, 150, "+", 9), (5, 300, 350, "+", 9),
    (6, 0, 10, "+", 10), (6, 50, 60, "+", 10), (6, TOP - 100, TOP - 90, "+", 11), (6, TOP - 10, TOP, "+", 11),
    (8, 100, 200, "+", 12),
)
HAND_N_GENES = 13


def hand_reads():
    """[(what, read)]; every case on both strands, so that every strand mode meets it"""
    cases = [
        ("inner exon", M(410)), ("inner intron", M(460)), ("outer intron clear of the inner body", M(250)),
        ("outer exon", M(120)), ("exon end into the intron", M(190)), ("intron into the exon start", M(790)),
        ("inner body's last base", M(549, 1)), ("behind the inner body", M(550, 1)),
        ("opposite: inner exon", M(410, ref=1)), ("opposite: inner intron", M(460, ref=1)), ("opposite: outer intron", M(250, ref=1)),
        ("exons of two genes", M(160, ref=2)), ("exon of one, body of both", M(110, ref=2)), ("intron of 5 alone", M(260, ref=2)),
        ("two exons of gene 0, N over gene 1's body", (0, 180, False, (("M", 20), ("N", 600), ("M", 20)))),
        ("the same with a deletion", (0, 180, False, (("M", 20), ("D", 600), ("M", 20)))),
        ("gene 6's intron and gene 7's", (3, 200, False, (("M", 20), ("N", 380), ("M", 20)))),
        ("gene 6's intron and between the genes", (3, 200, False, (("M", 20), ("N", 180), ("M", 20)))),
        ("gene 6's intron and gene 7's exon", (3, 200, False, (("M", 20), ("N", 280), ("M", 20)))),
        ("before the body", M(99, 1, ref=4)), ("the body's first base", M(100, 1, ref=4)),
        ("the body's last base", M(299, 1, ref=4)), ("behind the body", M(300, 1, ref=4)),
        ("in the body's first intron", M(160, 5, ref=4)), ("in its second", M(220, 5, ref=4)),
        ("gene 9 on +", M(1100, ref=4)), ("gene 9 on .", M(1600, ref=4)), ("between gene 9's bodies", M(1300, ref=4)),
        ("across both of gene 9's bodies", M(1240, 300, ref=4)), ("gene 9 on the other reference", M(200, ref=5)),
        ("gene 9's coordinates of reference 4 on 5", M(1100, ref=5)),
        ("no words", (0, 410, False, ())), ("no block", (0, 410, False, (("S", 5), ("I", 3), ("H", 2), ("P", 1)))),
        ("an N alone", (0, 410, False, (("N", 30),))), ("an empty M", (0, 410, False, (("M", 0),))),
        ("coordinate 0", M(0, 1, ref=6)), ("an intron near 0", M(20, 1, ref=6)), ("gene 10's last base", M(59, 1, ref=6)),
        ("behind gene 10", M(60, 1, ref=6)), ("an intron near the top", M(TOP - 50, 1, ref=6)),
        ("the top base", M(TOP - 1, 1, ref=6)), ("beyond the top", M(TOP - 1, 5, ref=6)), ("at 2^31 - 1", M(TOP, 3, ref=6)),
        ("before gene 11", M(TOP - 101, 1, ref=6)), ("gene 11's first base", M(TOP - 100, 1, ref=6)),
        ("from 0 to the top", (6, 5, False, (("M", 1), ("N", 2 ** 28 - 1)) + (("N", 2 ** 28 - 1),) * 7 + (("M", 5),))),
        ("a reference without lines", M(150, ref=7)), ("another", M(150, ref=9)), ("a reference far away", M(150, ref=TOP)),
        ("one exon, no intron", M(150, ref=8)), ("beside it", M(210, ref=8)),
    ]
    out = []
    for what, (ref, pos, _, cigar) in cases:
        out += [(what + ", +", (ref, pos, False, cigar)), (what + ", -", (ref, pos, True, cigar))]
    return out


# ---- the combs: tables of a given number of segments ----------------------------------------------------

@functools.lru_cache(maxsize=None)
def body_comb(n):
    """n two-exon genes on '+', every gene distinct and apart from the next: n segments in the '+' body table, 2 n in
    the '+' exon table"""
    return tuple(x for i in range(n) for x in ((0, 30 * i, 30 * i + 5, "+", i), (0, 30 * i + 15, 30 * i + 20, "+", i)))


@functools.lru_cache(maxsize=None)
def body_comb_reads(n, seed=9, reads=2000):
    """reads in the exons, in the gaps between a gene's exons and between the genes, some spliced, a tenth reversed"""
    rng = np.random.default_rng(seed + n)
    out = []
    for _ in range(reads):
        pos = max(0, int(rng.integers(0, 30 * n + 30)) - 10)
        cigar = [("M", int(rng.integers(1, 9)))]
        if rng.random() < 0.3:
            cigar += [("N", int(rng.integers(1, 40))), ("M", int(rng.integers(1, 9)))]
        out.append((0, pos, bool(rng.random() < 0.1), tuple(cigar)))
    # the two ends of the table, and of each chunk of the sampled top where there is one
    for i in (0, 1, n - 2, n - 1, GENE_BODY_TOP_CAP - 1, GENE_BODY_TOP_CAP, GENE_BODY_TOP_CAP + 1, 2 * GENE_BODY_TOP_CAP):
        if 0 <= i < n:
            out += [(0, 30 * i + d, False, (("M", 1),)) for d in (-1, 0, 4, 5, 10, 14, 15, 19, 20) if 30 * i + d >= 0]
    return tuple(out)


# ---- a BAM for the program ------------------------------------------------------------------------------

def with_gene_tags(recs, exons, gene_ids, mode, introns):
    """annotation_model.with_gene_tags under --gene-introns: the model's verdict of every record in GX"""
    import tag_model
    body_lines = bodies(exons)
    out, tiers = [], []
    for rec in recs:
        r = bamio.parse_record(rec)
        rev = bool(r["flag"] & 0x10)
        st, g, tier = verdict(hits(exons, r["tid"], r["pos"], rev, r["cigar"], mode),
                              hits(body_lines, r["tid"], r["pos"], rev, r["cigar"], mode), introns)
        tag = b"" if st == NONE else tag_model.aux_z("GX", gene_ids[g] if st == ASSIGNED else "a;b")
        body = rec[4:] + tag
        out.append(struct.pack("<i", len(body)) + body)
        tiers.append((st, tier, bool(r["flag"] & 0x4) or r["tid"] < 0))
    return out, tiers
