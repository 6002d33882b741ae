"""Test-side definition of umi_assign_genes_classes, umi_velocity_matrix and --velocity (include/umihip.h has the same
rule), in plain Python over tests/annotation_model.py, tests/intron_model.py and tests/gene_model.py, and the makers
of the tests' inputs.

A gene-level rule in exact integers.  It is NOT velocyto's or STARsolo's transcript-model rule: the project keeps no
transcript models.  A read's blocks, exons, admissible strands, E, B, status, gene and tier are intron_model's
(umi_assign_genes_introns'), unchanged.  New, for an assigned read with gene g:
  Blocks are cut to [0, 2^31) and the empty ones left out: b1 .. bm.  A gap is the stretch between one block's end
    and the next one's start (what N operations skipped).
  cover of an interval [s, e): the number of its positions that lie in an exon of g on the read's reference and on an
    admissible strand.  It is computed from g's own lines, whatever other genes lie there.
  INTRONIC (4): tier intron.  Tier exon: SPANNING (3) where the blocks' summed cover is less than their summed length
    (the read leaves the exons into an intron or past the gene's end); otherwise JUNCTION (2) where m >= 2 and some gap
    has cover < its length (the read skips an intron); otherwise EXONIC (1).  NONE (0) where the read is not assigned.
Molecules: a molecule is a kept entry r (kept[r] != 0); its reads are the reads i with read_entry[i] != UNSTAGED and
  root[read_entry[i]] == r.  s: one of them is JUNCTION; u: one is SPANNING or INTRONIC.  s and not u: spliced.  u and
  not s: unspliced.  Otherwise (both kinds, or EXONIC reads alone, or no read): ambiguous.  An entry with kept == 0
  counts nowhere.  The three layers are laid out as gene_model.count_model lays out its molecules."""
import functools

import numpy as np

import annotation_model as am
import intron_model as im

NONE, EXONIC, JUNCTION, SPANNING, INTRONIC = 0, 1, 2, 3, 4
CLASS_NAMES = ("none", "exonic", "junction", "exon-intron", "intronic")
UNSTAGED = 0xFFFFFFFF
LIMIT = 2 ** 31
SPLICED, UNSPLICED, AMBIGUOUS = 0, 1, 2


def clip(s, e):
    return max(s, 0), min(e, LIMIT)


def read_blocks(pos, cigar):
    """the read's blocks cut to [0, 2^31), the empty ones left out"""
    return [(s, e) for s, e in (clip(s, e) for s, e in am.blocks(pos, cigar)) if e > s]


def gaps(blocks):
    return [(a[1], b[0]) for a, b in zip(blocks, blocks[1:])]


def cover_of(intervals, s, e):
    """the positions of [s, e) that lie in one of the intervals (half-open, in any order, overlapping or not)"""
    s, e = clip(s, e)
    total, at = 0, s
    for a, b in sorted(intervals):
        a, b = max(a, at), min(b, e)
        if b > a:
            total += b - a
            at = b
    return total


def own_exons(exons, g, ref, reverse, mode):
    return [(xs, xe) for xr, xs, xe, xstrand, xg in exons if xg == g and xr == ref and am.admissible(xstrand, reverse, mode)]


def cover(exons, g, ref, reverse, mode, s, e):
    return cover_of(own_exons(exons, g, ref, reverse, mode), s, e)


def class_of(own, tier, pos, cigar):
    """the class of an assigned read from its gene's admissible exons on its reference"""
    if tier == im.TIER_INTRON:
        return INTRONIC
    bl = read_blocks(pos, cigar)
    if sum(cover_of(own, s, e) for s, e in bl) < sum(e - s for s, e in bl):
        return SPANNING
    if len(bl) >= 2 and any(cover_of(own, s, e) < e - s for s, e in gaps(bl)):
        return JUNCTION
    return EXONIC


def classify(exons, ref, pos, reverse, cigar, mode, introns):
    """(status, gene, tier, class) of one read, line by line"""
    st, g, tier = im.assign(exons, ref, pos, reverse, cigar, mode, introns)
    if st != im.ASSIGNED:
        return st, g, tier, NONE
    return st, g, tier, class_of(own_exons(exons, g, ref, reverse, mode), tier, pos, cigar)


def class_counts_of(cls):
    return np.bincount(np.asarray(cls, np.int64), minlength=5).astype(np.uint64)


def classify_all(exons, reads, mode, introns):
    """intron_model.assign_all's dict, and cls uint8 and class_counts uint64 [5] beside it; the lines of a (gene,
    reference, read strand) are gathered once"""
    out = im.assign_all(exons, reads, mode, introns)
    by = {}
    for xr, xs, xe, xstrand, g in exons:
        for rev in (0, 1):
            if am.admissible(xstrand, rev, mode):
                by.setdefault((g, xr, rev), []).append((xs, xe))
    cls = np.zeros(len(reads), np.uint8)
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        if out["status"][i] == im.ASSIGNED:
            cls[i] = class_of(by.get((int(out["gene"][i]), ref, 1 if rev else 0), []), int(out["tier"][i]), pos, cigar)
    out["cls"], out["class_counts"] = cls, class_counts_of(cls)
    return out


# ---- molecules ------------------------------------------------------------------------------------------

def evidence(read_entry, read_class, root, n):
    """per entry: bit 0 a JUNCTION read, bit 1 a SPANNING or INTRONIC read, among the reads of the molecule it roots"""
    ev = np.zeros(n, np.uint8)
    for e, c in zip(np.asarray(read_entry).tolist(), np.asarray(read_class).tolist()):
        if e == UNSTAGED:
            continue
        assert 0 <= e < n and 0 <= c <= 4
        if c == JUNCTION:
            ev[root[e]] |= 1
        elif c in (SPANNING, INTRONIC):
            ev[root[e]] |= 2
    return ev


def molecule_layers(read_entry, read_class, kept, root):
    """int8 [N]: SPLICED, UNSPLICED or AMBIGUOUS for every kept entry, -1 for the others"""
    kept, root = np.asarray(kept), np.asarray(root).astype(np.int64)
    ev = evidence(read_entry, read_class, root, len(kept))
    layer = np.where(ev == 1, SPLICED, np.where(ev == 2, UNSPLICED, AMBIGUOUS)).astype(np.int8)
    layer[kept == 0] = -1
    return layer


def layer_of_classes(classes):
    """the layer of a molecule with reads of these classes"""
    s, u = JUNCTION in classes, SPANNING in classes or INTRONIC in classes
    return SPLICED if s and not u else UNSPLICED if u and not s else AMBIGUOUS


def velocity_model(read_entry, read_class, kept, root, off, row, col):
    """umi_velocity_matrix in dictionaries: (out_row, out_col, spliced, unspliced, ambiguous), uint32, over the distinct
    (col, row) of the non-empty buckets, sorted by col, then row -- gene_model.count_model's layout"""
    layer = molecule_layers(read_entry, read_class, kept, root)
    off = np.asarray(off).astype(np.int64)
    cells = {}
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if lo == hi:
            continue
        c = cells.setdefault((int(col[b]), int(row[b])), [0, 0, 0])
        for k in range(3):
            c[k] += int((layer[lo:hi] == k).sum())
    order = sorted(cells)
    return (np.array([r for _, r in order], np.uint32), np.array([c for c, _ in order], np.uint32)) + tuple(
        np.array([cells[p][k] for p in order], np.uint32) for k in range(3))


# ---- the hand-written cases (the issue's table): reference 0, strand +, forward, G0 and G1 ----------------

HAND_EXONS = ((0, 100, 200, "+", 0), (0, 300, 400, "+", 0), (0, 1000, 1100, "+", 1))
HAND_READS = (
    (150, (("M", 50),), EXONIC), (180, (("M", 40),), SPANNING), (180, (("M", 20), ("N", 100), ("M", 20)), JUNCTION),
    (220, (("M", 50),), INTRONIC), (110, (("M", 10), ("N", 5), ("M", 10)), EXONIC), (380, (("M", 40),), SPANNING),
    (150, (("M", 20), ("D", 2), ("M", 20)), EXONIC), (190, (("M", 20), ("N", 90), ("M", 20)), SPANNING),
    (500, (("M", 50),), NONE),
)
# {classes of a molecule's reads: its layer}
HAND_MOLECULES = (((EXONIC, JUNCTION), SPLICED), ((EXONIC,), AMBIGUOUS), ((JUNCTION, SPANNING), AMBIGUOUS),
                  ((INTRONIC,), UNSPLICED), ((EXONIC, INTRONIC), UNSPLICED))


# ---- the fuzz inputs of the classes ---------------------------------------------------------------------

N_REFS = 3
FUZZ_GENES = 200


@functools.lru_cache(maxsize=None)
def fuzz_genes(seed=23):
    """(lines, primary exons per gene, strand per gene, ref per gene): about 200 genes in about 1,000 lines on 3
    references.  A gene has 3 to 6 exons; some of its lines overlap (a second transcript's longer exon), some are '.'.
    Genes overlap their neighbours on either strand now and then; every eighth gene lies nested in an intron of the
    gene before it, and every sixteenth is one exon that fills such an intron exactly, so that the exon table has no
    uncovered base between two of the outer gene's exons."""
    rng = np.random.default_rng(seed)
    lines, prim, strands, refs = [], [], [], []
    cursor = [0] * N_REFS
    for g in range(FUZZ_GENES):
        ref = g % N_REFS
        strand = "+-"[int(rng.integers(0, 2))]
        host = g - N_REFS  # the gene before it on this reference
        mine = []
        if g % 8 == 7 and host >= 0 and len(prim[host]) >= 2:
            j = int(np.argmax([b[0] - a[1] for a, b in zip(prim[host], prim[host][1:])]))
            lo, hi = prim[host][j][1], prim[host][j + 1][0]
            if g % 16 == 15:
                mine, strand = [(lo, hi)], strands[host]
            else:
                w = (hi - lo) // 5
                mine = [(lo + w, lo + 2 * w), (lo + 3 * w, lo + 4 * w)]
                if rng.random() < 0.5:
                    strand = strands[host]
        else:
            at = cursor[ref] + int(rng.integers(-250, 700))
            at = max(at, 0)
            for _ in range(int(rng.integers(3, 7))):
                length = int(rng.integers(60, 250))
                mine.append((at, at + length))
                at += length + int(rng.integers(80, 400) if rng.random() < 0.8 else rng.integers(500, 900))
            cursor[ref] = at
        for s, e in mine:
            st = "." if rng.random() < 0.05 else strand
            lines.append((ref, s, e, st, g))
            if len(mine) > 2 and rng.random() < 0.15:
                lines.append((ref, s + (e - s) // 3, e + 25, st, g))
        prim.append(mine)
        strands.append(strand)
        refs.append(ref)
    return tuple(lines), tuple(tuple(p) for p in prim), tuple(strands), tuple(refs)


def fuzz_annotation():
    return fuzz_genes()[0]


def decorate(rng, length):
    """CIGAR operations that consume exactly `length` reference bases and skip nothing"""
    u = rng.random()
    if length < 6 or u < 0.5:
        return [("M=X"[int(rng.choice(3, p=[0.8, 0.1, 0.1]))], length)]
    a = int(rng.integers(1, length - 3))
    if u < 0.65:
        return [("M", a), ("I", int(rng.integers(1, 4))), ("M", length - a)]
    if u < 0.8:
        d = int(rng.integers(1, min(4, length - a - 1) + 1))
        return [("=", a), ("D", d), ("X", length - a - d)]
    if u < 0.9:
        return [("M", a), ("P", 1), ("M", length - a)]
    return [("M", a), ("N", 0), ("M", length - a)]  # (an N that skips nothing: two blocks, an empty gap)


def with_ends(rng, core):
    front = ([("H", int(rng.integers(1, 6)))] if rng.random() < 0.1 else []) + ([("S", int(rng.integers(1, 9)))] if rng.random() < 0.2 else [])
    back = ([("S", int(rng.integers(1, 9)))] if rng.random() < 0.2 else []) + ([("H", int(rng.integers(1, 6)))] if rng.random() < 0.1 else [])
    return tuple(front + core + back)


@functools.lru_cache(maxsize=None)
def fuzz_reads(seed=29, n=5000):
    """5,000 reads: three quarters aimed at a gene -- inside an exon, across an exon's edge, over one or two introns
    from exon to exon, inside an intron, over a covered gap -- a fifth of them on the gene's other strand, and a
    quarter anywhere, with annotation_model's random CIGARs.  Every CIGAR operation occurs."""
    _, prim, strands, refs = fuzz_genes()
    rng = np.random.default_rng(seed)
    reads = []
    while len(reads) < n:
        if rng.random() < 0.25:
            span = 1 + max(e for p in prim for _, e in p)
            reads.append((int(rng.integers(0, N_REFS)), int(rng.integers(0, span)), bool(rng.random() < 0.5),
                          tuple(am.random_cigar(rng, rng.random() < 0.33))))
            continue
        g = int(rng.integers(0, FUZZ_GENES))
        ex = prim[g]
        rev = (strands[g] == "-") != bool(rng.random() < 0.2)
        kind = int(rng.integers(0, 5))
        i = int(rng.integers(0, len(ex)))
        s, e = ex[i]
        if kind == 0:  # inside an exon
            length = int(rng.integers(10, min(60, e - s) + 1))
            pos, core = int(rng.integers(s, e - length + 1)), decorate(rng, length)
        elif kind == 1:  # across an exon's edge, either one
            a, k = int(rng.integers(1, 30)), int(rng.integers(1, 30))
            pos, core = (e - a, decorate(rng, a + k)) if rng.random() < 0.5 else (max(0, s - k), decorate(rng, a + min(k, s)))
        elif kind == 2 and len(ex) >= 2:  # from exon to exon
            i = min(i, len(ex) - 2)
            hops = 2 if i + 2 < len(ex) and rng.random() < 0.25 else 1
            a = int(rng.integers(5, min(40, ex[i][1] - ex[i][0]) + 1))
            pos, core = ex[i][1] - a, decorate(rng, a)
            for h in range(1, hops + 1):
                nxt = ex[i + h]
                b = nxt[1] - nxt[0] if h < hops else int(rng.integers(5, min(40, nxt[1] - nxt[0]) + 1))
                core += [("N", nxt[0] - ex[i + h - 1][1])] + decorate(rng, b)
        elif kind == 3 and len(ex) >= 2:  # inside an intron
            i = min(i, len(ex) - 2)
            lo, hi = ex[i][1], ex[i + 1][0]
            if hi - lo < 12:
                continue
            length = int(rng.integers(5, min(50, hi - lo) + 1))
            pos, core = int(rng.integers(lo, hi - length + 1)), decorate(rng, length)
        else:  # over a gap that lies in the exon
            if e - s < 30:
                continue
            pos = int(rng.integers(s, e - 29))
            core = [("M", 10), ("N", int(rng.integers(1, 10))), ("M", 10)]
        reads.append((refs[g], pos, rev, with_ends(rng, core)))
    return tuple(reads)


@functools.lru_cache(maxsize=None)
def fuzz_expected(mode, introns):
    return classify_all(fuzz_annotation(), fuzz_reads(), mode, introns)


# ---- the inputs of the matrix ---------------------------------------------------------------------------

def make_molecules(seed, sizes, n_rows, n_cols, reads_per_entry=3, removed=0.3, filtered=0.1, unstaged=0.1, far_roots=False):
    """dict(read_entry, read_class, kept, root, off, row, col) over buckets of the given sizes.  In a bucket, about
    `removed` of the entries hang on another entry of it (far_roots: on its first entry, however far away), and about
    `filtered` of the roots are themselves not kept (what the multi-gene filter leaves).  Every molecule draws a
    profile -- junctions, introns, both, or plain exons -- and its reads their classes from it; the reads come in
    shuffled order, about `unstaged` more of them unstaged."""
    rng = np.random.default_rng(seed)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    root = np.arange(n, dtype=np.uint32)
    kept = np.ones(n, np.uint8)
    for b, size in enumerate(sizes):
        lo = int(off[b])
        if size < 2:
            continue
        hang = np.flatnonzero(rng.random(size) < removed)
        hang = hang[hang != 0]  # (the first entry is a root)
        roots = np.setdiff1d(np.arange(size), hang)
        root[lo + hang] = lo if far_roots else lo + rng.choice(roots, len(hang))
        kept[lo + hang] = 0
    own = np.flatnonzero(root == np.arange(n))
    kept[own[rng.random(len(own)) < filtered]] = 0
    profiles = np.array([(EXONIC, JUNCTION), (EXONIC, INTRONIC, SPANNING), (JUNCTION, SPANNING, INTRONIC, EXONIC), (EXONIC, EXONIC)], object)
    profile_of = rng.choice(4, n, p=[0.3, 0.3, 0.2, 0.2])
    entries = np.repeat(np.arange(n, dtype=np.uint32), rng.integers(1, 2 * reads_per_entry, n))
    cls = np.array([profiles[profile_of[root[e]]][int(rng.integers(0, len(profiles[profile_of[root[e]]])))] for e in entries], np.uint8)
    extra = int(len(entries) * unstaged)
    entries = np.concatenate([entries, np.full(extra, UNSTAGED, np.uint32)])
    cls = np.concatenate([cls, rng.integers(0, 5, extra).astype(np.uint8)])
    order = rng.permutation(len(entries))
    return dict(read_entry=entries[order], read_class=cls[order], kept=kept, root=root, off=off,
                row=rng.integers(0, n_rows, len(sizes)).astype(np.uint32), col=rng.integers(0, n_cols, len(sizes)).astype(np.uint32))


@functools.lru_cache(maxsize=None)
def fuzz_molecules(seed=41):
    """about 3,000 buckets of 0 to 40 entries and a few deep ones, 50 genes, 30 cells"""
    rng = np.random.default_rng(seed)
    sizes = [int(x) for x in rng.choice([0, 1, 1, 2, 3, 5, 8, 32, 33, 40], 3000)] + [257, 700, 33, 0, 1]
    return make_molecules(seed, sizes, 50, 30)


# ---- a BAM for the program, and what --velocity writes for it --------------------------------------------

REF_NAMES = ["chrA", "chrB", "chrC"]
GENE_IDS = ["ENSG%05d" % (7 * g + 3) for g in range(FUZZ_GENES)]


def velocity_bam(seed=3, genes=24, n_cells=4, umi_len=10, pool=3):
    """(header, records without a gene tag, cell barcodes): a coordinate-ordered BAM of a few hundred of the fuzz reads
    -- those the first `genes` genes take under forward / exon-first, and some that no gene or several take -- with UB,
    CB and CR like annotation_model.annotation_bam's.  The UMIs of a (cell, gene) come from a small pool, a tenth of them
    from a pool of the whole cell, so that molecules have several reads and a cell shows a UMI under two genes."""
    import bamio
    import gene_model
    import struct
    import tag_model
    exp = fuzz_expected(am.FORWARD, im.EXON_FIRST)
    reads = fuzz_reads()
    take = [i for i in range(len(reads)) if exp["status"][i] == im.ASSIGNED and exp["gene"][i] < genes]
    take += list(np.flatnonzero(exp["status"] == im.NONE)[:40]) + list(np.flatnonzero(exp["status"] == im.SEVERAL)[:30])
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    draw = lambda n: "".join(letters[x] for x in rng.integers(0, 4, n))
    while True:
        cells = [draw(16) for _ in range(n_cells)]
        if all(gene_model.hamming(a, b) >= 4 for i, a in enumerate(cells) for b in cells[:i]):
            break
    pools, items = {}, []
    for n, i in enumerate(take):
        ref, pos, rev, cigar = reads[int(i)]
        c = int(rng.integers(0, n_cells))
        key = (c, -1) if rng.random() < 0.1 else (c, int(exp["gene"][i]))
        if key not in pools:
            pools[key] = [draw(umi_len) for _ in range(pool)]
        umi = pools[key][int(rng.integers(0, pool))]
        if rng.random() < 0.04:
            at = int(rng.integers(0, umi_len))
            umi = umi[:at] + letters[(letters.index(umi[at]) + 1) % 4] + umi[at + 1:]
        flag = (0x10 if rev else 0) | (0x4 if rng.random() < 0.02 else 0)
        tags = tag_model.aux_fields_before(rng)
        if rng.random() >= 0.02:
            tags += tag_model.aux_z("UB", umi)
        if rng.random() >= 0.02:
            tags += tag_model.aux_z("CB", cells[c] + "-1") + tag_model.aux_z("CR", cells[c])
        tags += b"xxi" + struct.pack("<i", n)
        seq_len = sum(k for op, k in cigar if op in "MIS=X")
        quals = rng.integers(20, 41, seq_len).astype(np.uint8).tobytes()
        items.append((ref, pos, n, bamio.make_record("r%d" % n, flag, ref, pos, int(rng.integers(0, 61)), list(cigar), seq_len, quals, tags=tags)))
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    top = 1 + max(e for _, _, e, _, _ in fuzz_annotation())
    return bamio.make_header([(name, top + 4000) for name in REF_NAMES]), [t[3] for t in items], cells


def layer_files(genes, cells, n_rows, n_cols, triplets):
    """the five files of a velocity directory; triplets = (row, col, spliced, unspliced, ambiguous) in the call's order"""
    import gene_model
    row, col = triplets[0], triplets[1]
    out = {f: gene_model.matrix_files(genes, cells, n_rows, n_cols, (row[:0], col[:0], row[:0], row[:0]))[f] for f in ("features.tsv", "barcodes.tsv")}
    for name, v in zip(("spliced.mtx", "unspliced.mtx", "ambiguous.mtx"), triplets[2:]):
        some = v != 0
        out[name] = gene_model.matrix_files(genes, cells, n_rows, n_cols, (row[some], col[some], v[some], v[some]))["matrix.mtx"]
    return out


def expected_cli(recs, mode, introns, k=1, p=0.5, algo="dir", dedup=None, multigene=False):
    """what umicollapse --per-cell --per-gene --gene-annotation --gene-introns --count-matrix --velocity makes of the
    records: dict(files: DIR/velocity's five (features.tsv by gene id), triplets, class_counts over the mapped records,
    layers (the molecules by layer), molecules, st, mask)"""
    import bamio
    import gene_model
    import multigene_model as mm
    import tag_model
    exons = fuzz_annotation()
    cls = np.zeros(len(recs), np.uint8)
    for i, rec in enumerate(recs):
        r = bamio.parse_record(rec)
        if not (r["flag"] & 0x4) and r["tid"] >= 0:
            cls[i] = classify(exons, r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], mode, introns)[3]
    tagged, _ = im.with_gene_tags(recs, exons, GENE_IDS, mode, introns)
    st = gene_model.stage(tagged, per_cell=True)
    kept, root = mm.collapse(st, k, p, algo, dedup)
    mask = kept
    if multigene:
        mask = mm.filter_model(st["keys"], st["freq"], kept, root, st["bucket_off"], st["bucket_cell"], st["umi_len"])[0]
    # every staged read's entry: the entry of its (cell, gene) bucket that holds its UMI
    off = st["bucket_off"].astype(np.int64)
    entry = {}
    for b in range(len(off) - 1):
        for e in range(int(off[b]), int(off[b + 1])):
            aux = tag_model.parse_aux(tagged[int(st["rep"][e])])
            entry[(aux["CB"][1], aux["GX"][1], aux["UB"][1])] = e
    read_entry = np.full(len(recs), UNSTAGED, np.uint32)
    for i, rec in enumerate(tagged):
        aux = tag_model.parse_aux(rec)
        if bamio.parse_record(rec)["flag"] & 0x4 or "UB" not in aux or "CB" not in aux:
            continue
        if gene_model.gene_class(aux["GX"][1] if "GX" in aux else None) == "one":
            read_entry[i] = entry[(aux["CB"][1], aux["GX"][1], aux["UB"][1])]
    trip = velocity_model(read_entry, cls, mask, root, st["bucket_off"], st["bucket_gene"], st["bucket_cell"])
    assert int((read_entry != UNSTAGED).sum()) == int(st["freq"].sum())
    return dict(files=layer_files(st["genes"], st["cells"], len(st["genes"]), len(st["cells"]), trip), triplets=trip,
                class_counts=class_counts_of(cls), layers=[int(v.sum()) for v in trip[2:]], molecules=int(np.count_nonzero(mask)),
                st=st, mask=mask)
