"""Test-side definition of umi_assign_genes / --gene-annotation (include/umihip.h has the same rule), in plain
Python over tests/bamio.py, a GTF writer, and the makers of the tests' inputs.

The rule (featureCounts -t exon -g gene_id -s 0|1|2 with its defaults: minimum overlap 1, no -O, single-end):
  Blocks of a read: start at the record's pos (0-based) and walk the CIGAR.  M, =, X and D extend the current
    block on the reference; N closes the block and skips its length; I, S, H and P consume nothing.  Blocks are
    half-open [s, e); a read with no reference-consuming operation has no block (an empty block shares no base).
  Exons: (ref, start, end, strand, gene), half-open, 0-based, strand '+', '-' or '.'.
  Hits: gene g hits a read when one of its exons is on the read's reference, on an admissible strand, and shares
    at least one base with one of the read's blocks.
  Admissible strand: the read's strand is '-' when flag 0x10 is set, else '+'.  forward: the exon's strand equals
    the read's; reverse: it is the opposite; unstranded: any.  A '.' exon is admissible under all three.
  Result: exactly one gene hits: ASSIGNED with its index; none: NONE, -1; two or more: SEVERAL, -1."""
import functools
import gzip
import struct

import numpy as np

import bamio

ASSIGNED, NONE, SEVERAL = 0, 1, 2
FORWARD, REVERSE, UNSTRANDED = 0, 1, 2
MODES = {"forward": FORWARD, "reverse": REVERSE, "unstranded": UNSTRANDED}
OPS = bamio.CIGAR_OPS  # "MIDNSHP=X"
# the library's constants the tests place their sizes by (csrc/umihip_internal.h)
GENE_THREADS = 1024       # lanes of a block, a read each
GENE_BLOCKS_PER_CU = 2    # the grid's cap: this many blocks per CU, a stride beyond
GENE_TOP_CAP = 4096       # sampled segment ends of a table in LDS, at most: the stride doubles beyond


def blocks(pos, cigar):
    """the read's blocks [(s, e)]; cigar a list of (op letter, length)"""
    out, s, e = [], pos, pos
    for op, n in cigar:
        if op in "M=XD":
            e += n
        elif op == "N":
            if e > s:
                out.append((s, e))
            s = e = e + n
        else:
            assert op in "ISHP", op
    if e > s:
        out.append((s, e))
    return out


def admissible(exon_strand, reverse, mode):
    if exon_strand == "." or mode == UNSTRANDED:
        return True
    read_strand = "-" if reverse else "+"
    return (exon_strand == read_strand) == (mode == FORWARD)


def assign(exons, ref, pos, reverse, cigar, mode):
    """(status, gene) of one read, exon by exon"""
    hit = set()
    for s, e in blocks(pos, cigar):
        for xr, xs, xe, xstrand, g in exons:
            if xr == ref and admissible(xstrand, reverse, mode) and xs < e and s < xe:
                hit.add(g)
    if not hit:
        return NONE, -1
    return (ASSIGNED, hit.pop()) if len(hit) == 1 else (SEVERAL, -1)


def assign_all(exons, reads, mode):
    """dict(gene int32, status uint8, counts uint64 [3]) over reads [(ref, pos, reverse, cigar)]: the same rule, the
    exons of a read's reference and admissible strands held in arrays"""
    by = {}
    for xr, xs, xe, xstrand, g in exons:
        for rev in (0, 1):
            if admissible(xstrand, rev, mode):
                by.setdefault((xr, rev), []).append((xs, xe, g))
    by = {k: np.array(v, np.int64) for k, v in by.items()}
    gene, status = np.full(len(reads), -1, np.int32), np.zeros(len(reads), np.uint8)
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        x = by.get((ref, 1 if rev else 0))
        hit = set()
        if x is not None:
            for s, e in blocks(pos, cigar):
                hit.update(x[(x[:, 0] < e) & (s < x[:, 1]), 2].tolist())
        status[i] = NONE if not hit else ASSIGNED if len(hit) == 1 else SEVERAL
        if len(hit) == 1:
            gene[i] = hit.pop()
    return {"gene": gene, "status": status, "counts": np.bincount(status, minlength=3).astype(np.uint64)}


def cigar_words(cigar):
    return [n << 4 | OPS.index(op) for op, n in cigar]


def pack_reads(reads):
    """the call's five read arrays: ref, pos (int32), reverse (uint8), cigar (uint32), cigar_off (uint64)"""
    words, off = [], [0]
    for _, _, _, cigar in reads:
        words += cigar_words(cigar)
        off.append(len(words))
    return (np.array([r[0] for r in reads], np.int32), np.array([r[1] for r in reads], np.int32),
            np.array([1 if r[2] else 0 for r in reads], np.uint8), np.array(words, np.uint32), np.array(off, np.uint64))


def n_genes_of(exons):
    return 1 + max([g for *_, g in exons], default=-1)


# ---- GTF ------------------------------------------------------------------------------------------------

def gtf_lines(exons, ref_names, gene_ids, feature="exon", attribute="gene_id", gene_names=None, extra=()):
    """one line per exon (columns 4 and 5 are 1-based inclusive), a header comment, an empty line, and `extra` lines"""
    out = ["#!genome-build synthetic", ""]
    for ref, s, e, strand, g in exons:
        attrs = 'transcript_id "T%s.1"; %s "%s";' % (gene_ids[g], attribute, gene_ids[g])
        if gene_names is not None and gene_names[g] is not None:
            attrs += ' gene_name "%s";' % gene_names[g]
        out.append("\t".join([ref_names[ref], "synthetic", feature, str(s + 1), str(e), ".", strand, ".", attrs]))
    return out + list(extra)


def write_gtf(path, lines, gz=False):
    data = ("\n".join(lines) + "\n").encode()
    with (gzip.open(path, "wb") if gz else open(path, "wb")) as f:
        f.write(data)
    return str(path)


# ---- the fuzz inputs ------------------------------------------------------------------------------------

REF_LEN = 9000
N_REFS = 3


@functools.lru_cache(maxsize=None)
def fuzz_annotation(seed=7, n_genes=40):
    """3 references, about 40 genes and 300 exons: genes overlap on both strands, some exons are '.', and gene 0
    repeats an exon.  A tuple of (ref, start, end, strand, gene)."""
    rng = np.random.default_rng(seed)
    exons = []
    for g in range(n_genes):
        ref, strand = g % N_REFS, "+-"[int(rng.integers(0, 2))]
        at = int(rng.integers(0, REF_LEN - 2500))
        for _ in range(int(rng.integers(5, 11))):
            length = int(rng.integers(40, 260))
            st = "." if rng.random() < 0.06 else strand
            exons.append((ref, at, at + length, st, g))
            if rng.random() < 0.15:  # a second transcript's line: an overlapping exon of the same gene
                exons.append((ref, at + length // 3, at + length + 25, st, g))
            at += length + int(rng.integers(30, 320))
    first = next(e for e in exons if e[4] == 0)
    exons.append(first)
    return tuple(exons)


def random_cigar(rng, spliced):
    """a CIGAR over all nine operations; `spliced`: with at least one N"""
    c = []
    if rng.random() < 0.1:
        c.append(("H", int(rng.integers(1, 6))))
    if rng.random() < 0.25:
        c.append(("S", int(rng.integers(1, 9))))
    pieces = int(rng.integers(1, 4)) + (1 if spliced else 0)
    for p in range(pieces):
        c.append(("M=X"[int(rng.choice(3, p=[0.8, 0.1, 0.1]))], int(rng.integers(5, 45))))
        u = rng.random()
        if u < 0.15:
            c += [("I", int(rng.integers(1, 4))), ("M", int(rng.integers(3, 20)))]
        elif u < 0.3:
            c += [("D", int(rng.integers(1, 5))), ("M", int(rng.integers(3, 20)))]
        elif u < 0.35:
            c += [("P", 1), ("M", int(rng.integers(3, 20)))]
        if p + 1 < pieces:
            if spliced and (p == 0 or rng.random() < 0.5):
                c.append(("N", int(rng.integers(30, 500))))
            else:
                c.append(("D", 1))
    if rng.random() < 0.25:
        c.append(("S", int(rng.integers(1, 9))))
    if rng.random() < 0.1:
        c.append(("H", int(rng.integers(1, 6))))
    return c


@functools.lru_cache(maxsize=None)
def fuzz_reads(seed=11, n=5000):
    """5,000 reads over the fuzz annotation's references, a third spliced, 40 % on the reverse strand"""
    rng = np.random.default_rng(seed)
    reads = []
    for _ in range(n):
        reads.append((int(rng.integers(0, N_REFS)), int(rng.integers(0, REF_LEN)), bool(rng.random() < 0.4),
                      random_cigar(rng, rng.random() < 0.33)))
    return tuple((r, p, v, tuple(c)) for r, p, v, c in reads)


@functools.lru_cache(maxsize=None)
def fuzz_expected(mode):
    return assign_all(fuzz_annotation(), fuzz_reads(), mode)


@functools.lru_cache(maxsize=None)
def comb_annotation(n):
    """n exons that give n segments in the '+' table (none in the '-' table): apart, one gene each of 50 in turn"""
    return tuple((0, 10 * i, 10 * i + 5, "+", i % 50) for i in range(n))


@functools.lru_cache(maxsize=None)
def comb_reads(n, seed=5, reads=3000):
    rng = np.random.default_rng(seed + n)
    out = []
    for _ in range(reads):
        pos = int(rng.integers(0, 10 * n + 20)) - 10
        if pos < 0:
            pos = 0
        u = rng.random()
        cigar = [("M", int(rng.integers(1, 12)))]
        if u < 0.3:
            cigar += [("N", int(rng.integers(1, 40))), ("M", int(rng.integers(1, 12)))]
        out.append((0, pos, bool(rng.random() < 0.1), tuple(cigar)))
    # the two ends of the table, and of each chunk of the sampled top where there is one
    for i in (0, 1, n - 2, n - 1, GENE_TOP_CAP - 1, GENE_TOP_CAP, GENE_TOP_CAP + 1):
        if 0 <= i < n:
            out += [(0, 10 * i + d, False, (("M", 1),)) for d in (-1, 0, 4, 5)if 10 * i + d >= 0]
    return tuple(out)


# ---- a BAM for the program ------------------------------------------------------------------------------

def annotation_bam(seed, exons, ref_names, n_reads=1500, n_cells=6, umi_len=10, pool=3):
    """(header, records without a gene tag, cell barcodes): a coordinate-ordered BAM over the annotation's references
    whose reads carry UB, CB and CR like gene_model.gene_bam's, with spliced reads and reads on both strands; the
    UMIs of a (cell, 200-base window) come from a small pool, so that molecules repeat"""
    import gene_model
    import tag_model
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    while True:
        cells = ["".join(letters[x] for x in rng.integers(0, 4, 16)) for _ in range(n_cells)]
        if all(gene_model.hamming(a, b) >= 4 for i, a in enumerate(cells) for b in cells[:i]):
            break
    pools, items = {}, []
    for i in range(n_reads):
        ref, pos = int(rng.integers(0, len(ref_names))), int(rng.integers(0, REF_LEN))
        c = int(rng.integers(0, n_cells))
        key = (c, ref, pos // 200)
        if key not in pools:
            pools[key] = ["".join(letters[x] for x in rng.integers(0, 4, umi_len)) for _ in range(pool)]
        umi = pools[key][int(rng.integers(0, pool))]
        if rng.random() < 0.05:
            at = int(rng.integers(0, umi_len))
            umi = umi[:at] + letters[(letters.index(umi[at]) + 1) % 4] + umi[at + 1:]
        raw = cells[c]
        if rng.random() < 0.15:
            at = int(rng.integers(0, 16))
            raw = raw[:at] + letters[(letters.index(raw[at]) + 1) % 4] + raw[at + 1:]
        cigar = random_cigar(rng, rng.random() < 0.3)
        flag = (0x10 if rng.random() < 0.4 else 0) | (0x4 if rng.random() < 0.02 else 0)
        tags = tag_model.aux_fields_before(rng)
        if rng.random() >= 0.02:
            tags += tag_model.aux_z("UB", umi)
        if rng.random() >= 0.02:
            tags += tag_model.aux_z("CB", cells[c] + "-1") + tag_model.aux_z("CR", raw)
        tags += b"xxi" + struct.pack("<i", i)
        seq_len = sum(n for op, n in cigar if op in "MIS=X")
        quals = rng.integers(20, 41, seq_len).astype(np.uint8).tobytes()
        items.append((ref, pos, i, bamio.make_record("r%d" % i, flag, ref, pos, int(rng.integers(0, 61)), cigar, seq_len,
                                                     quals, tags=tags)))
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    return bamio.make_header([(n, REF_LEN + 4000) for n in ref_names]), [t[3] for t in items], cells


def with_gene_tags(recs, exons, gene_ids, mode):
    """the records with their model-assigned genes in GX: the gene's id where one hits, 'a;b' where several do (the
    program looks at no more than the separator), no tag where none does"""
    import tag_model
    out = []
    for rec in recs:
        r = bamio.parse_record(rec)
        st, g = assign(exons, r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], mode)
        tag = b"" if st == NONE else tag_model.aux_z("GX", gene_ids[g] if st == ASSIGNED else "a;b")
        body = rec[4:] + tag
        out.append(struct.pack("<i", len(body)) + body)
    return out
