"""Test-side definition of umi_assign_genes_transcripts / --gene-rule transcript (include/umihip.h has the same rule),
in plain Python over tests/annotation_model.py, whose blocks() and admissible() it takes unchanged, and the makers of
the tests' inputs.

The rule (STARsolo's Gene, Cell Ranger's transcriptome-compatible reads):
  Exons: (ref, start, end, strand, gene, transcript), half-open, 0-based, transcript in 0..n_transcripts - 1.  All
    exons of one transcript share ref, strand and gene (else the call refuses).  A transcript's exons are taken in
    ascending order whatever order they come in; those that overlap or abut are united: x_1 < x_2 < ... < x_n,
    disjoint, at least one base between neighbours.
  Blocks: annotation_model.blocks()'s, b_1 .. b_m: M = X D extend a block, N closes it (a zero-length N too: two
    abutting blocks), I S H P consume nothing, empty blocks are left out.
  Fit: a read fits transcript t when t is on the read's reference and on an admissible strand (annotation_model.
    admissible(); a '.' transcript always), m >= 1, and there is a j such that b_i lies inside x_{j+i-1} for every i,
    and for every i < m: end(b_i) == end(x_{j+i-1}) and start(b_{i+1}) == start(x_{j+i}).  A read with more blocks
    than t has exons from j on does not fit t.
  Verdict: G = the genes with a transcript the read fits.  One gene: ASSIGNED with its index; none: NONE, -1; two or
    more: SEVERAL, -1.  G is a subset of annotation_model's E."""
import bisect
import functools

import numpy as np

import annotation_model as am
from annotation_model import ASSIGNED, NONE, SEVERAL, FORWARD, REVERSE, UNSTRANDED, MODES, blocks, admissible  # noqa: F401

N_GENES = 40


def transcripts_of(exons):
    """{transcript: (ref, strand, gene, [(start, end)] united and ascending)}; ValueError where a transcript's exons
    differ in ref, strand or gene"""
    raw = {}
    for ref, s, e, strand, g, t in exons:
        head = raw.setdefault(t, ((ref, strand, g), []))
        if head[0] != (ref, strand, g):
            raise ValueError("transcript %d lies on two references, strands or genes" % t)
        head[1].append((s, e))
    out = {}
    for t, ((ref, strand, g), xs) in raw.items():
        united = []
        for s, e in sorted(xs):
            if united and s <= united[-1][1]:
                united[-1] = (united[-1][0], max(united[-1][1], e))
            else:
                united.append((s, e))
        out[t] = (ref, strand, g, united)
    return out


def fits(xs, bl):
    """does the read with blocks bl fit the united exons xs"""
    if not bl:
        return False
    starts = [x[0] for x in xs]
    j = bisect.bisect_right(starts, bl[0][0]) - 1  # the one exon that can hold b_1: united exons are disjoint
    if j < 0 or j + len(bl) > len(xs):
        return False
    for i, (s, e) in enumerate(bl):
        xs_, xe_ = xs[j + i]
        if not (xs_ <= s and e <= xe_):
            return False
        if i + 1 < len(bl) and e != xe_:
            return False
        if i > 0 and s != xs_:
            return False
    return True


def fitting(trs, ref, pos, reverse, cigar, mode):
    """the transcripts (ids, ascending) that the read fits; trs: transcripts_of()'s"""
    bl = blocks(pos, cigar)
    return [t for t in sorted(trs) if trs[t][0] == ref and admissible(trs[t][1], reverse, mode) and fits(trs[t][3], bl)]


def verdict(genes):
    genes = set(genes)
    if not genes:
        return NONE, -1
    return (ASSIGNED, genes.pop()) if len(genes) == 1 else (SEVERAL, -1)


def assign(exons, ref, pos, reverse, cigar, mode):
    """(status, gene) of one read"""
    trs = transcripts_of(exons)
    return verdict(trs[t][2] for t in fitting(trs, ref, pos, reverse, cigar, mode))


def assign_all(exons, reads, mode):
    """dict(gene int32, status uint8, counts uint64 [3]) over reads [(ref, pos, reverse, cigar)]: the same rule, the
    transcripts of a read's reference and admissible strands held in arrays and tried where their span holds the read's"""
    trs = transcripts_of(exons)
    by = {}
    for t in sorted(trs):
        ref, strand, g, xs = trs[t]
        for rev in (0, 1):
            if admissible(strand, rev, mode):
                by.setdefault((ref, rev), []).append((g, xs))
    span = {k: (np.array([xs[0][0] for _, xs in v], np.int64), np.array([xs[-1][1] for _, xs in v], np.int64)) for k, v in by.items()}
    gene, status = np.full(len(reads), -1, np.int32), np.zeros(len(reads), np.uint8)
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        bl = blocks(pos, cigar)
        k = (ref, 1 if rev else 0)
        near = np.flatnonzero((span[k][0] <= bl[0][0]) & (bl[-1][1] <= span[k][1])) if bl and k in by else ()
        st, g = verdict(by[k][j][0] for j in near if fits(by[k][j][1], bl))
        status[i], gene[i] = st, g
    return {"gene": gene, "status": status, "counts": np.bincount(status, minlength=3).astype(np.uint64)}


def overlap_exons(exons):
    """the same lines without their transcripts: annotation_model's exons"""
    return [e[:5] for e in exons]


def n_transcripts_of(exons):
    return 1 + max([e[5] for e in exons], default=-1)


# ---- GTF ------------------------------------------------------------------------------------------------

def transcript_ids(exons, gene_ids):
    """an id per transcript: T<gene id>.<k>, k counting the gene's transcripts in order of their number"""
    seen, out = {}, {}
    for t in sorted({e[5] for e in exons}):
        g = next(e[4] for e in exons if e[5] == t)
        seen[g] = seen.get(g, 0) + 1
        out[t] = "T%s.%d" % (gene_ids[g], seen[g])
    return out


def gtf_lines(exons, ref_names, gene_ids, tr_ids=None, attribute="transcript_id", extra=()):
    """one line per exon with gene_id and the transcript's id under `attribute`"""
    tr_ids = transcript_ids(exons, gene_ids) if tr_ids is None else tr_ids
    out = ["#!genome-build synthetic", ""]
    for ref, s, e, strand, g, t in exons:
        attrs = 'gene_id "%s"; %s "%s";' % (gene_ids[g], attribute, tr_ids[t])
        out.append("\t".join([ref_names[ref], "synthetic", "exon", str(s + 1), str(e), ".", strand, ".", attrs]))
    return out + list(extra)


# ---- the fuzz inputs ------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def fuzz_annotation(seed=17, n_genes=N_GENES):
    """3 references of 9,000 bases, 40 genes in pairs on one reference, 2 to 5 transcripts a gene that share exons: exons
    skipped, alternative ends, retained introns, an exon given as two overlapping or abutting lines, minus-strand
    transcripts listed descending, some transcripts on '.'.  The odd gene of most pairs lies over the even one, on its
    strand: some of its exons contain the other's, some overlap them in part."""
    rng = np.random.default_rng(seed)
    exons, t, base = [], 0, None
    for g in range(n_genes):
        ref = (g // 2) % am.N_REFS
        if g % 2 == 1 and rng.random() < 0.75:  # a partner over the even gene
            strand, gene_exons = base[0], []
            for s, e in base[1]:
                u = rng.random()
                if u < 0.3:
                    gene_exons.append((s, e))
                elif u < 0.5:
                    gene_exons.append((max(0, s - int(rng.integers(1, 20))), e + int(rng.integers(1, 20))))
                elif u < 0.8:
                    d = int(rng.integers(8, 30))
                    gene_exons.append((s + d, e + d + int(rng.integers(0, 12))))
            if len(gene_exons) < 2:
                gene_exons = [(s + 5, e + 5) for s, e in base[1][:2]]
        else:
            strand = "+-"[int(rng.integers(0, 2))]
            at, gene_exons = int(rng.integers(0, am.REF_LEN - 2800)), []
            for _ in range(int(rng.integers(5, 11))):
                length = int(rng.integers(40, 260))
                gene_exons.append((at, at + length))
                at += length + int(rng.integers(30, 300))
        gene_exons = sorted(set(gene_exons))
        if g % 2 == 0:
            base = (strand, gene_exons)
        for k in range(int(rng.integers(2, 6))):
            st = "." if rng.random() < 0.06 else strand
            keep = [x for x in gene_exons if k == 0 or rng.random() < 0.75]
            if len(keep) < 2:
                keep = gene_exons[:2]
            lines = []
            i = 0
            while i < len(keep):
                s, e = keep[i]
                u = rng.random()
                if u < 0.08 and i + 1 < len(keep):  # a retained intron: one exon from this one's start to the next one's end
                    e = keep[i + 1][1]
                    i += 1
                elif u < 0.16:  # an alternative end
                    e += 25
                if rng.random() < 0.1 and e - s > 20:  # one exon as two lines, overlapping or abutting
                    cut = s + (e - s) // 2
                    lines += [(s, cut + (5 if rng.random() < 0.5 else 0)), (cut, e)]
                else:
                    lines.append((s, e))
                i += 1
            if st == "-":
                lines.reverse()
            elif rng.random() < 0.1:
                lines = [lines[j] for j in rng.permutation(len(lines))]
            exons += [(ref, s, e, st, g, t) for s, e in lines]
            t += 1
    return tuple(exons)


def read_from_transcript(rng, xs, pos0, length):
    """(pos, cigar) of a read of `length` transcript bases from offset pos0 of the spliced transcript, dressed with
    clips, insertions, deletions inside an exon, = and X"""
    pieces, left, off = [], length, pos0
    for k, (s, e) in enumerate(xs):
        n = e - s
        if off >= n:
            off -= n
            continue
        take = min(left, n - off)
        pieces.append((s + off, take))
        left -= take
        off = 0
        if not left:
            break
    cigar = []
    if rng.random() < 0.1:
        cigar.append(("H", int(rng.integers(1, 6))))
    if rng.random() < 0.25:
        cigar.append(("S", int(rng.integers(1, 9))))
    for k, (s, n) in enumerate(pieces):
        if k:
            cigar.append(("N", s - (pieces[k - 1][0] + pieces[k - 1][1])))
        u = rng.random()
        if u < 0.12 and n >= 6:
            a = int(rng.integers(1, n - 1))
            cigar += [("M", a), ("I", int(rng.integers(1, 4))), ("M", n - a)]
        elif u < 0.24 and n >= 8:
            a, d = int(rng.integers(1, n - 4)), int(rng.integers(1, 3))
            cigar += [("M", a), ("D", d), ("=", n - a - d)]
        elif u < 0.3 and n >= 4:
            cigar += [("=", n - 2), ("X", 1), ("P", 1), ("M", 1)]
        else:
            cigar.append(("M", n))
    if rng.random() < 0.25:
        cigar.append(("S", int(rng.integers(1, 9))))
    return pieces[0][0], cigar


@functools.lru_cache(maxsize=None)
def fuzz_reads(seed=23, n=5000):
    """5,000 reads: 60 % cut from a transcript of the fuzz annotation (a quarter of them then moved by a base, or with an
    N a base longer or shorter, or run on beyond their exon), mostly on their transcript's strand; the rest
    annotation_model's random reads"""
    rng = np.random.default_rng(seed)
    trs = transcripts_of(fuzz_annotation())
    ids = sorted(trs)
    reads = []
    for _ in range(n):
        if rng.random() >= 0.6:
            reads.append((int(rng.integers(0, am.N_REFS)), int(rng.integers(0, am.REF_LEN)), bool(rng.random() < 0.4),
                          am.random_cigar(rng, rng.random() < 0.33)))
            continue
        ref, strand, _, xs = trs[ids[int(rng.integers(0, len(ids)))]]
        total = sum(e - s for s, e in xs)
        length = min(total, int(rng.integers(25, 400 if rng.random() < 0.35 else 120)))
        pos, cigar = read_from_transcript(rng, xs, int(rng.integers(0, total - length + 1)), length)
        u = rng.random()
        if u < 0.08:
            pos += int(rng.choice([-1, 1]))
        elif u < 0.16:
            at = [i for i, c in enumerate(cigar) if c[0] == "N"]
            if at:
                i = at[int(rng.integers(0, len(at)))]
                cigar[i] = ("N", max(0, cigar[i][1] + int(rng.choice([-1, 1]))))
        elif u < 0.25:
            cigar.insert(len(cigar) - (1 if cigar[-1][0] == "S" else 0), ("M", int(rng.integers(1, 200))))
        rev = (strand == "-") if strand != "." else bool(rng.random() < 0.5)
        if rng.random() < 0.4:
            rev = not rev
        reads.append((ref, pos, rev, cigar))
    return tuple((r, p, v, tuple(c)) for r, p, v, c in reads)


@functools.lru_cache(maxsize=None)
def fuzz_expected(mode):
    return assign_all(fuzz_annotation(), fuzz_reads(), mode)


@functools.lru_cache(maxsize=None)
def comb_annotation(n):
    """n distinct exons in the '+' table: transcripts of two exons each, 50 genes in turn (an odd n: the last
    transcript has one)"""
    return tuple((0, 10 * i, 10 * i + 5, "+", (i // 2) % 50, i // 2) for i in range(n))


@functools.lru_cache(maxsize=None)
def comb_reads(n, seed=5, reads=3000):
    rng = np.random.default_rng(seed + n)
    out = []
    for _ in range(reads):
        i = int(rng.integers(0, n))
        u = rng.random()
        if u < 0.3 and i % 2 == 0 and i + 1 < n:  # the transcript's junction, sometimes a base off
            a, d = int(rng.integers(1, 6)), int(rng.integers(-1, 2)) if rng.random() < 0.3 else 0
            out.append((0, 10 * i + 5 - a, bool(rng.random() < 0.1), (("M", a), ("N", 5 + d), ("M", int(rng.integers(1, 6))))))
        else:
            pos = max(0, 10 * i + int(rng.integers(-2, 6)))
            out.append((0, pos, bool(rng.random() < 0.1), (("M", int(rng.integers(1, 7))),)))
    for i in (0, 1, n - 2, n - 1, am.GENE_TOP_CAP - 1, am.GENE_TOP_CAP, am.GENE_TOP_CAP + 1):
        if 0 <= i < n:
            out += [(0, 10 * i + d, False, (("M", 1),)) for d in (-1, 0, 4, 5) if 10 * i + d >= 0]
    return tuple(out)


def with_gene_tags(recs, exons, gene_ids, mode):
    """the records with their model-assigned genes in GX, as annotation_model.with_gene_tags writes them"""
    import struct

    import bamio
    import tag_model
    trs = transcripts_of(exons)
    out = []
    for rec in recs:
        r = bamio.parse_record(rec)
        st, g = verdict(trs[t][2] for t in fitting(trs, r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], mode))
        tag = b"" if st == NONE else tag_model.aux_z("GX", gene_ids[g] if st == ASSIGNED else "a;b")
        body = rec[4:] + tag
        out.append(struct.pack("<i", len(body)) + body)
    return out
