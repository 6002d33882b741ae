"""Test-side definition of umi_assign_genes_transcripts_classes / --transcript-introns (include/umihip.h has the same
rule), in plain Python over tests/transcript_model.py, tests/intron_model.py and tests/velocity_model.py, and the
makers of the tests' inputs.

Stated after Cell Ranger 7's counting with introns and velocyto / STARsolo Velocyto, not claimed equal to them: there
is no intron validation and no per-model logic across a molecule's reads.  All of it is exact integers.

  Exons come with their transcripts: (ref, start, end, strand, gene, transcript), as transcript_model takes them.
  Blocks, admissible strands, fit and G (the genes with a transcript the read fits) are transcript_model's, unchanged.
    m is the number of non-empty blocks.
  Bodies and B (the genes whose admissible body on the read's reference shares a base with a block) are intron_model's,
    unchanged, derived from the same lines without their transcripts.  E is annotation_model's.  G <= E <= B.
  Gene, status, tier:
    exon-first: |G| = 1: assigned to it, tier transcript (0).  |G| >= 2: several.  |G| = 0 and |B| = 1: assigned, tier
      body (1).  |G| = 0 and |B| = 0: none.  |G| = 0 and |B| >= 2: several.
    all: |B| = 1: assigned to it, tier transcript where G is not empty, else body.  |B| = 0: none.  |B| >= 2: several.
    off: transcript_model's gene and status, every assigned read tier transcript.
  Class of an assigned read with gene g:
    tier transcript: JUNCTION where m >= 2, else EXONIC (every gap of a fitting read is an intron of a transcript it
      fits).
    tier body: the blocks are cut to [0, 2^31) as in velocity_model.read_blocks; c is the summed cover of the blocks by
      g's admissible exon lines on the reference.  c == 0: INTRONIC.  0 < c < the summed length: SPANNING.  c == the
      summed length: velocity_model.class_of's verdict on the gaps -- JUNCTION where a gap is not covered whole by g's
      own exons, else EXONIC.
    not assigned: NONE.
  Molecules are velocity_model's (umi_velocity_matrix), unchanged."""
import functools
import struct

import numpy as np

import annotation_model as am
import intron_model as im
import transcript_model as tm
import velocity_model as vm

ASSIGNED, NONE, SEVERAL = am.ASSIGNED, am.NONE, am.SEVERAL
TIER_TRANSCRIPT, TIER_BODY = 0, 1
OFF, EXON_FIRST, ALL = im.OFF, im.EXON_FIRST, im.ALL
INTRONS = im.INTRONS
C_NONE, EXONIC, JUNCTION, SPANNING, INTRONIC = vm.NONE, vm.EXONIC, vm.JUNCTION, vm.SPANNING, vm.INTRONIC


def verdict(G, B, introns):
    """(status, gene, tier) from the two sets, the rule word for word"""
    one = lambda s: next(iter(s))
    if introns == OFF:
        return (ASSIGNED, one(G), TIER_TRANSCRIPT) if len(G) == 1 else (NONE, -1, 0) if not G else (SEVERAL, -1, 0)
    if introns == EXON_FIRST:
        if len(G) == 1:
            return ASSIGNED, one(G), TIER_TRANSCRIPT
        if len(G) >= 2:
            return SEVERAL, -1, 0
        if len(B) == 1:
            return ASSIGNED, one(B), TIER_BODY
        return (NONE, -1, 0) if not B else (SEVERAL, -1, 0)
    assert introns == ALL
    if len(B) == 1:
        return ASSIGNED, one(B), TIER_TRANSCRIPT if G else TIER_BODY
    return (NONE, -1, 0) if not B else (SEVERAL, -1, 0)


def class_of(own, tier, pos, cigar):
    """the class of an assigned read; own: its gene's admissible exon lines on its reference"""
    if tier == TIER_TRANSCRIPT:
        return JUNCTION if len(am.blocks(pos, cigar)) >= 2 else EXONIC
    bl = vm.read_blocks(pos, cigar)
    c, length = sum(vm.cover_of(own, s, e) for s, e in bl), sum(e - s for s, e in bl)
    if c == 0:
        return INTRONIC
    if c < length:
        return SPANNING
    return vm.class_of(own, im.TIER_EXON, pos, cigar)  # (the blocks are covered whole: its verdict is the gaps')


def sets_of(exons, ref, pos, reverse, cigar, mode):
    """(G, E, B) of one read, line by line"""
    trs = tm.transcripts_of(exons)
    lines = tm.overlap_exons(exons)
    G = {trs[t][2] for t in tm.fitting(trs, ref, pos, reverse, cigar, mode)}
    return G, im.hits(lines, ref, pos, reverse, cigar, mode), im.hits(im.bodies(lines), ref, pos, reverse, cigar, mode)


def classify(exons, ref, pos, reverse, cigar, mode, introns):
    """(status, gene, tier, class) of one read, line by line"""
    G, _, B = sets_of(exons, ref, pos, reverse, cigar, mode)
    st, g, tier = verdict(G, B, introns)
    if st != ASSIGNED:
        return st, g, tier, C_NONE
    return st, g, tier, class_of(vm.own_exons(tm.overlap_exons(exons), g, ref, reverse, mode), tier, pos, cigar)


def counts_of(status, tier):
    return im.counts_of(status, tier)


def classify_all(exons, reads, mode, introns):
    """dict(gene int32, status uint8, tier uint8, cls uint8, counts uint64 [4]: by a transcript, by a body, none,
    several; class_counts uint64 [5]).  G's verdict is transcript_model.assign_all's: |G| is 1, 0 or more by its status"""
    exons, reads = list(exons), list(reads)
    lines = tm.overlap_exons(exons)
    fit = tm.assign_all(exons, reads, mode)
    B = im.hit_sets(im.bodies(lines), reads, mode) if introns != OFF else [set()] * len(reads)
    by = {}
    for xr, xs, xe, xstrand, g in lines:
        for rev in (0, 1):
            if am.admissible(xstrand, rev, mode):
                by.setdefault((g, xr, rev), []).append((xs, xe))
    n = len(reads)
    gene, status, tier, cls = np.full(n, -1, np.int32), np.zeros(n, np.uint8), np.zeros(n, np.uint8), np.zeros(n, np.uint8)
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        fs = int(fit["status"][i])
        G = {int(fit["gene"][i])} if fs == ASSIGNED else set() if fs == NONE else {-1, -2}  # (several: any two stand in)
        status[i], gene[i], tier[i] = verdict(G, B[i], introns)
        if status[i] == ASSIGNED:
            cls[i] = class_of(by.get((int(gene[i]), ref, 1 if rev else 0), []), int(tier[i]), pos, cigar)
    return {"gene": gene, "status": status, "tier": tier, "cls": cls, "counts": counts_of(status, tier),
            "class_counts": vm.class_counts_of(cls)}


# ---- the hand table (the issue's): reference 0, all lines '+', forward --------------------------------------

def _tr(gene, transcript, xs):
    return [(0, s, e, "+", gene, transcript) for s, e in xs]


HAND_EXONS = tuple(_tr(0, 0, [(100, 200), (300, 400), (500, 600)]) + _tr(0, 1, [(100, 200), (300, 600)])  # T1 retains an intron
                   + _tr(1, 2, [(220, 240), (260, 280)])                                                  # nested in G0's first intron
                   + _tr(2, 3, [(1000, 1100), (1200, 1300)]))
HAND_N_GENES, HAND_N_TRANSCRIPTS = 3, 4
T, B_ = TIER_TRANSCRIPT, TIER_BODY
_M, _N = (lambda n: ("M", n)), (lambda n: ("N", n))
# (pos, cigar, reverse, exon-first: (status, gene, tier, class), all: the same where it differs, else None)
HAND_READS = (
    (150, (_M(50),), False, (ASSIGNED, 0, T, EXONIC), None),
    (180, (_M(20), _N(100), _M(20)), False, (ASSIGNED, 0, T, JUNCTION), None),
    (380, (_M(20), _N(100), _M(20)), False, (ASSIGNED, 0, T, JUNCTION), None),  # the gene-level rule: EXONIC
    (420, (_M(50),), False, (ASSIGNED, 0, T, EXONIC), None),                    # fits T1 only
    (180, (_M(40),), False, (ASSIGNED, 0, B_, SPANNING), None),
    (190, (_M(40),), False, (SEVERAL, -1, 0, C_NONE), None),
    (205, (_M(10),), False, (ASSIGNED, 0, B_, INTRONIC), None),
    (225, (_M(10),), False, (ASSIGNED, 1, T, EXONIC), (SEVERAL, -1, 0, C_NONE)),
    (180, (_M(20), _N(101), _M(20)), False, (ASSIGNED, 0, B_, JUNCTION), None),
    (150, (_M(20), _N(0), _M(20)), False, (ASSIGNED, 0, B_, EXONIC), None),
    (110, (_M(10), _N(5), _M(10)), False, (ASSIGNED, 0, B_, EXONIC), None),
    (1080, (_M(20), _N(100), _M(20)), False, (ASSIGNED, 2, T, JUNCTION), None),
    (700, (_M(50),), False, (NONE, -1, 0, C_NONE), None),
    (150, (_M(50),), True, (NONE, -1, 0, C_NONE), None),                        # a read on the reverse strand
    (590, (_M(20),), False, (ASSIGNED, 0, B_, SPANNING), None),
    (180, (_M(20), _N(100), _M(100), _N(100), _M(20)), False, (ASSIGNED, 0, T, JUNCTION), None),
    (580, (_M(20), _N(100), _M(20)), False, (ASSIGNED, 0, B_, SPANNING), None),  # more blocks than T0 / T1 have exons left
)
HAND_GENE_LEVEL_DIFFERS = 2  # the read (index) that velocity_model calls EXONIC under exon-first


def hand_reads():
    return [(0, pos, rev, cigar) for pos, cigar, rev, _, _ in HAND_READS]


def hand_expected(introns):
    """[(status, gene, tier, class)] of the hand table's reads under exon-first or all"""
    assert introns in (EXON_FIRST, ALL)
    return [first if introns == EXON_FIRST or full is None else full for _, _, _, first, full in HAND_READS]


# ---- the fuzz inputs ------------------------------------------------------------------------------------

def fuzz_annotation():
    return tm.fuzz_annotation()


N_GENES = tm.N_GENES


@functools.lru_cache(maxsize=None)
def extra_reads(seed=61, n=600):
    """reads that transcript_model's read maker rarely draws, cut from the fuzz annotation's transcripts: two blocks
    inside one exon (an N within the exon, or of no length), and a splice over an exon the transcript has (an isoform
    the annotation may lack), mostly on the transcript's strand"""
    rng = np.random.default_rng(seed)
    trs = tm.transcripts_of(tm.fuzz_annotation())
    ids = sorted(trs)
    # most of them where one gene's span alone holds the blocks: there a read without a fit has one body, whatever the strand
    span = {}
    for ref, _, g, xs in trs.values():
        lo, hi = span.get(g, (ref, xs[0][0], xs[-1][1]))[1:]
        span[g] = (ref, min(lo, xs[0][0]), max(hi, xs[-1][1]))
    depth = np.zeros((am.N_REFS, am.REF_LEN + 4000), np.int32)
    for ref, lo, hi in span.values():
        depth[ref, lo:hi] += 1
    out = []
    while len(out) < n:
        ref, strand, _, xs = trs[ids[int(rng.integers(0, len(ids)))]]
        rev = (strand == "-") if strand != "." else bool(rng.random() < 0.5)
        if rng.random() < 0.4:  # (the other strand: what "reverse" assigns)
            rev = not rev
        if rng.random() < 0.4:
            s, e = xs[int(rng.integers(0, len(xs)))]
            if e - s < 30:
                continue
            a, b = int(rng.integers(3, 12)), int(rng.integers(3, 12))
            gap = 0 if rng.random() < 0.3 else int(rng.integers(1, e - s - a - b))
            pos = int(rng.integers(s, e - a - b - gap + 1))
        elif len(xs) >= 3:
            i = int(rng.integers(0, len(xs) - 2))
            a, b = int(rng.integers(3, min(30, xs[i][1] - xs[i][0]) + 1)), int(rng.integers(3, min(30, xs[i + 2][1] - xs[i + 2][0]) + 1))
            pos, gap = xs[i][1] - a, xs[i + 2][0] - xs[i][1]
        else:
            continue
        alone = depth[ref, pos:pos + a].max() == 1 and depth[ref, pos + a + gap:pos + a + gap + b].max() == 1
        if alone or rng.random() < 0.1:
            out.append((ref, pos, rev, (("M", a), ("N", gap), ("M", b))))
    return tuple(out)


@functools.lru_cache(maxsize=None)
def fuzz_reads():
    """transcript_model's 5,000 reads and extra_reads() behind them"""
    return tm.fuzz_reads() + extra_reads()


@functools.lru_cache(maxsize=None)
def fuzz_expected(mode, introns):
    return classify_all(tm.fuzz_annotation(), fuzz_reads(), mode, introns)


# ---- the combs ------------------------------------------------------------------------------------------

@functools.lru_cache(maxsize=None)
def body_comb(n):
    """n genes of one two-exon transcript each, apart from one another: n segments in the '+' body table"""
    return tuple(e + (e[4],) for e in im.body_comb(n))


def body_comb_reads(n):
    """intron_model's: reads in the exons, in the introns and on their edges, some spliced"""
    return im.body_comb_reads(n)


# ---- a BAM for the program ------------------------------------------------------------------------------

REF_NAMES = ["chrA", "chrB", "chrC"]
GENE_IDS = ["ENSG%05d" % (7 * g + 3) for g in range(tm.N_GENES)]


def cli_bam(seed=3, n_reads=600, n_cells=4, umi_len=10, pool=3):
    """(header, records without a gene tag, cell barcodes): a coordinate-ordered BAM of a few hundred of the fuzz reads
    -- every read of fuzz_reads() that a body assigns under forward / exon-first or that is not EXONIC, and others up to
    n_reads -- with UB, CB and CR, built as velocity_model.velocity_bam builds its BAM"""
    import bamio
    import gene_model
    import tag_model
    exp = fuzz_expected(am.FORWARD, EXON_FIRST)
    reads = fuzz_reads()
    rng = np.random.default_rng(seed)
    want = np.flatnonzero((exp["tier"] == TIER_BODY) | (exp["cls"] >= JUNCTION))
    take = sorted(set(rng.choice(want, min(len(want), n_reads * 2 // 3), replace=False).tolist())
                  | set(rng.choice(len(reads), n_reads // 3, replace=False).tolist()))
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
    return bamio.make_header([(name, am.REF_LEN + 4000) for name in REF_NAMES]), [t[3] for t in items], cells


def record_verdicts(recs, exons, mode, introns):
    """[(status, gene, tier, class, mapped)] of the records, line by line"""
    import bamio
    out = []
    for rec in recs:
        r = bamio.parse_record(rec)
        mapped = not (r["flag"] & 0x4) and r["tid"] >= 0
        out.append(classify(exons, r["tid"], r["pos"], bool(r["flag"] & 0x10), r["cigar"], mode, introns) + (mapped,))
    return out


def with_gene_tags(recs, exons, gene_ids, mode, introns):
    """the records with the model's verdicts in GX, as intron_model.with_gene_tags writes them, and the verdicts"""
    import tag_model
    verdicts = record_verdicts(recs, exons, mode, introns)
    out = []
    for rec, (st, g, _, _, _) in zip(recs, verdicts):
        tag = b"" if st == NONE else tag_model.aux_z("GX", gene_ids[g] if st == ASSIGNED else "a;b")
        body = rec[4:] + tag
        out.append(struct.pack("<i", len(body)) + body)
    return out, verdicts


def expected_cli(recs, mode, introns, k=1, p=0.5, algo="dir", multigene=False):
    """what umicollapse --per-cell --per-gene --gene-annotation --gene-rule transcript --transcript-introns --count-matrix
    --velocity makes of the records, as velocity_model.expected_cli tells it for the gene-level rule: dict(files:
    DIR/velocity's five, triplets, class_counts over the mapped records, layers, molecules, counts: the mapped records by
    a transcript, by a body, none, several)"""
    import bamio
    import gene_model
    import multigene_model as mm
    import tag_model
    tagged, verdicts = with_gene_tags(recs, list(tm.fuzz_annotation()), GENE_IDS, mode, introns)
    mapped = np.array([v[4] for v in verdicts], bool)
    cls = np.where(mapped, np.array([v[3] for v in verdicts], np.uint8), 0).astype(np.uint8)
    status, tier = np.array([v[0] for v in verdicts], np.uint8)[mapped], np.array([v[2] for v in verdicts], np.uint8)[mapped]
    st = gene_model.stage(tagged, per_cell=True)
    kept, root = mm.collapse(st, k, p, algo, None)
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
    read_entry = np.full(len(recs), vm.UNSTAGED, np.uint32)
    for i, rec in enumerate(tagged):
        aux = tag_model.parse_aux(rec)
        if bamio.parse_record(rec)["flag"] & 0x4 or "UB" not in aux or "CB" not in aux:
            continue
        if gene_model.gene_class(aux["GX"][1] if "GX" in aux else None) == "one":
            read_entry[i] = entry[(aux["CB"][1], aux["GX"][1], aux["UB"][1])]
    trip = vm.velocity_model(read_entry, cls, mask, root, st["bucket_off"], st["bucket_gene"], st["bucket_cell"])
    assert int((read_entry != vm.UNSTAGED).sum()) == int(st["freq"].sum())
    return dict(files=vm.layer_files(st["genes"], st["cells"], len(st["genes"]), len(st["cells"]), trip), triplets=trip,
                class_counts=vm.class_counts_of(cls), layers=[int(v.sum()) for v in trip[2:]], molecules=int(np.count_nonzero(mask)),
                counts=counts_of(status, tier), tagged=tagged, verdicts=verdicts)
