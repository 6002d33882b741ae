"""The rule of umi_junction_matrix and --junction-matrix in plain Python and numpy: the junctions of a read, the junction
table, the (column, junction) triplets, the four counts, the filtered renumbering and the files of DIR/junctions.
include/umihip.h states the same in words; this file is what the tests hold the library and the program to."""
import numpy as np

UNSTAGED = 0xFFFFFFFF
POS_MAX = 2**31 - 1
OPS = "MIDNSHP=X"


class BadOp(ValueError):
    pass


def cigar_words(text_or_pairs):
    """BAM's words (len << 4 | op) of "10M5N3M" or of [(10, 'M'), (5, 3), ...]."""
    if isinstance(text_or_pairs, str):
        pairs, num = [], ""
        for ch in text_or_pairs:
            if ch.isdigit():
                num += ch
            else:
                pairs.append((int(num), ch))
                num = ""
        text_or_pairs = pairs
    return [(int(n) << 4) | (OPS.index(op) if isinstance(op, str) else int(op)) for n, op in text_or_pairs]


def read_blocks(pos, words):
    """The non-empty blocks [s, e) of a read: umi_assign_genes_transcripts' blocks."""
    blocks, s, e = [], int(pos), int(pos)
    for w in words:
        op, n = int(w) & 15, int(w) >> 4
        if op > 8:
            raise BadOp(op)
        if op in (0, 2, 7, 8):
            e += n
        elif op == 3:
            if e > s:
                blocks.append((s, e))
            s = e = e + n
    if e > s:
        blocks.append((s, e))
    return blocks


def read_junctions(pos, words):
    """The junctions (start, end) = [e, s) of a read, in ascending order: between consecutive non-empty blocks, where
    0 <= e < s <= 2^31 - 1."""
    b = read_blocks(pos, words)
    out = []
    for (_, e), (s, _) in zip(b, b[1:]):
        if 0 <= e < s <= POS_MAX:
            out.append((e, s))
    return out


def entry_columns(bucket_off, col):
    n = int(bucket_off[-1]) if len(bucket_off) else 0
    out = np.zeros(n, np.int64)
    for b in range(len(bucket_off) - 1):
        out[int(bucket_off[b]):int(bucket_off[b + 1])] = int(col[b])
    return out


def junction_matrix(read_ref, read_pos, cigar, cigar_off, read_entry, kept, root, bucket_off, col):
    """((jn_ref, jn_start, jn_end) int32, (out_jn, out_col, molecules uint32, reads uint64), counts uint64 [4])."""
    ecol = entry_columns(bucket_off, col)
    occ = []  # (ref, start, end, molecule, column)
    spliced = 0
    for i in range(len(read_ref)):
        e = int(read_entry[i])
        if e == UNSTAGED:
            continue
        r = int(root[e])
        if not kept[r]:
            continue
        js = read_junctions(int(read_pos[i]), cigar[int(cigar_off[i]):int(cigar_off[i + 1])])
        spliced += bool(js)
        occ += [(int(read_ref[i]), a, b, r, int(ecol[r])) for a, b in js]
    table = sorted({o[:3] for o in occ})
    number = {j: k for k, j in enumerate(table)}
    pairs = {}
    for ref, a, b, r, c in occ:
        mols, reads = pairs.setdefault((c, number[(ref, a, b)]), (set(), [0]))
        mols.add(r)
        reads[0] += 1
    keys = sorted(pairs)
    jn = tuple(np.array([t[k] for t in table], np.int32) for k in range(3))
    trip = (np.array([k[1] for k in keys], np.uint32), np.array([k[0] for k in keys], np.uint32),
            np.array([len(pairs[k][0]) for k in keys], np.uint32), np.array([pairs[k][1][0] for k in keys], np.uint64))
    return jn, trip, np.array([spliced, len(occ), len(table), len(keys)], np.uint64)


def filter_columns(jn, trip, called):
    """The called cells' part: `called` the raw column numbers in ascending order.  Columns are renumbered in that order,
    junctions without a triplet left are dropped and the rest renumbered in table order."""
    new_col = {int(c): k for k, c in enumerate(called)}
    keep = np.array([int(c) in new_col for c in trip[1]], bool)
    used = sorted({int(j) for j in trip[0][keep]})
    new_jn = {j: k for k, j in enumerate(used)}
    fjn = tuple(a[used] if len(used) else a[:0] for a in jn)
    ftrip = (np.array([new_jn[int(j)] for j in trip[0][keep]], np.uint32),
             np.array([new_col[int(c)] for c in trip[1][keep]], np.uint32), trip[2][keep], trip[3][keep])
    return fjn, ftrip


def features_tsv(jn, ref_names):
    """<reference name>\\t<start + 1>\\t<end>: the intron's first and last base, 1-based."""
    return "".join("%s\t%d\t%d\n" % (ref_names[int(r)], int(a) + 1, int(b)) for r, a, b in zip(*jn)).encode()


def matrix_mtx(header, n_rows, n_cols, rows, cols, values):
    """A matrix in the raw matrix.mtx's layout: `header` its lines in front of the size line; `row col value` lines,
    1-based, in the order given (column, then row)."""
    out = [header, "%d %d %d\n" % (n_rows, n_cols, len(rows))]
    out += ["%d %d %d\n" % (int(r) + 1, int(c) + 1, int(v)) for r, c, v in zip(rows, cols, values)]
    return "".join(out).encode()


# ---- inputs for the tests -------------------------------------------------------------------------------------

def make_pool(rng, n_refs=3, per_ref=40):
    """per reference a sorted list of disjoint introns (start, end) with exons of 20 to 200 bases between them"""
    pool = []
    for _ in range(n_refs):
        at, introns = int(rng.integers(50, 500)), []
        for _ in range(per_ref):
            at += int(rng.integers(20, 200))
            n = int(rng.integers(1, 3000))
            introns.append((at, at + n))
            at += n
        pool.append(introns)
    return pool


def spliced_read(rng, introns, j, k, plain=False):
    """(pos, words) of a read over introns j .. j + k - 1 of one reference, its M stretches decorated with S, H, I, D,
    = and X (plain: M and N alone); k == 0: a read without a junction"""
    a, b = int(rng.integers(1, 20)), int(rng.integers(1, 20))
    if k == 0:
        return int(rng.integers(0, 5000)), cigar_words([(a + b, "M")])
    pos, pairs = introns[j][0] - a, []

    def exon(n):
        kind = 0 if plain or n < 3 else int(rng.integers(0, 5))
        x = int(rng.integers(1, n)) if n > 1 else 1
        if kind == 1:
            return [(x, "M"), (2, "I"), (n - x, "M")]
        if kind == 2 and n - x > 1:
            return [(x, "="), (1, "D"), (n - x - 1, "X")]
        if kind == 3:
            return [(x, "M"), (0, "P"), (n - x, "M")]
        return [(n, "M")]
    pairs += exon(a)
    for t in range(k):
        s, e = introns[j + t]
        if not plain and e - s > 1 and rng.random() < 0.2:  # (several N with nothing of the reference between them)
            x = int(rng.integers(1, e - s))
            pairs += [(x, "N"), (3, "I"), (e - s - x, "N")]
        else:
            pairs.append((e - s, "N"))
        pairs += exon(introns[j + t + 1][0] - e if t + 1 < k else b)
    if not plain and rng.random() < 0.3:
        pairs = [(2, "H"), (4, "S")] + pairs + [(3, "S")]
    return pos, cigar_words(pairs)


def make_reads(rng, pool, counts, plain=False):
    """read_ref, read_pos, cigar, cigar_off of reads with the given numbers of junctions each"""
    ref, pos, words, off = [], [], [], [0]
    for k in counts:
        r = int(rng.integers(0, len(pool)))
        k = min(int(k), len(pool[r]))
        p, w = spliced_read(rng, pool[r], int(rng.integers(0, len(pool[r]) - k + 1)), k, plain)
        ref.append(r), pos.append(p)
        words += w
        off.append(len(words))
    return (np.array(ref, np.int32), np.array(pos, np.int32), np.array(words, np.uint32), np.array(off, np.uint64))


def counted_reads(m):
    """the reads that count: staged, under a kept root"""
    e = m["read_entry"]
    staged = e != UNSTAGED
    out = np.zeros(len(e), bool)
    out[staged] = m["kept"][m["root"][e[staged]]] != 0
    return out


def make_inputs(seed, sizes, n_cols, total=None, choices=(0, 0, 1, 1, 2, 3), **molecules):
    """velocity_model.make_molecules' buckets and reads, every read with a CIGAR over a small pool of introns.  total:
    the junction occurrences of the counted reads, exactly (None: as drawn)."""
    import velocity_model as vm
    m = vm.make_molecules(seed, sizes, 1, n_cols, **molecules)
    del m["read_class"], m["row"]
    rng = np.random.default_rng(seed + 1000)
    counts = rng.choice(np.array(choices), len(m["read_entry"]))
    if total is not None:
        idx = np.flatnonzero(counted_reads(m))
        left = int(total)
        for i in idx:
            counts[i] = min(int(counts[i]), left)
            left -= int(counts[i])
        assert left == 0, "too few counted reads for %d occurrences" % total
    m["read_ref"], m["read_pos"], m["cigar"], m["cigar_off"] = make_reads(rng, make_pool(rng), counts)
    return m


def model_of(m):
    return junction_matrix(m["read_ref"], m["read_pos"], m["cigar"], m["cigar_off"], m["read_entry"], m["kept"], m["root"], m["off"],
                           m["col"])


# ---- what the program writes ------------------------------------------------------------------------------------

MTX_HEADER = "%%MatrixMarket matrix coordinate integer general\n"


def directory_files(jn, trip, n_cols, ref_names):
    """features.tsv, matrix.mtx and reads.mtx of a junction directory (barcodes.tsv is its parent's, byte for byte)"""
    return {"features.tsv": features_tsv(jn, ref_names),
            "matrix.mtx": matrix_mtx(MTX_HEADER, len(jn[0]), n_cols, trip[0], trip[1], trip[2]),
            "reads.mtx": matrix_mtx(MTX_HEADER, len(jn[0]), n_cols, trip[0], trip[1], trip[3])}


def tagged_records(recs):
    """velocity_model.velocity_bam()'s records with the GX tags of the forward, exon-first assignment"""
    import annotation_model as am
    import intron_model as im
    import velocity_model as vm
    return im.with_gene_tags(recs, vm.fuzz_annotation(), vm.GENE_IDS, am.FORWARD, im.EXON_FIRST)[0]


def expected_cli(tagged, ref_names, per_cell=True, cell_min_molecules=None, multigene=False):
    """what umicollapse [--per-cell] --per-gene --count-matrix --junction-matrix makes of records that carry their GX tags
    (or get the same genes from --gene-annotation): dict(files: DIR/junctions' without barcodes.tsv, filtered: DIR/junctions/
    filtered's or None, counts, jn, trip, called).  A read is a record, in file order."""
    import bamio
    import gene_model
    import multigene_model as mm
    import tag_model
    st = gene_model.stage(tagged, per_cell=per_cell)
    kept, root = mm.collapse(st, 1, 0.5, "dir", None)
    mask = kept
    if multigene:
        mask = mm.filter_model(st["keys"], st["freq"], kept, root, st["bucket_off"], st["bucket_cell"], st["umi_len"])[0]
    off = st["bucket_off"].astype(np.int64)
    entry = {}
    for b in range(len(off) - 1):
        for e in range(int(off[b]), int(off[b + 1])):
            aux = tag_model.parse_aux(tagged[int(st["rep"][e])])
            entry[(aux["CB"][1] if per_cell else None, aux["GX"][1], aux["UB"][1])] = e
    read_entry = np.full(len(tagged), UNSTAGED, np.uint32)
    ref, pos, words, woff = [], [], [], [0]
    for i, rec in enumerate(tagged):
        aux = tag_model.parse_aux(rec)
        r = bamio.parse_record(rec)
        ref.append(r["tid"]), pos.append(r["pos"])
        words += cigar_words([(n, op) for op, n in r["cigar"]])  # (bamio has (op, length))
        woff.append(len(words))
        if r["flag"] & 0x4 or "UB" not in aux or (per_cell and "CB" not in aux):
            continue
        if gene_model.gene_class(aux["GX"][1] if "GX" in aux else None) == "one":
            read_entry[i] = entry[(aux["CB"][1] if per_cell else None, aux["GX"][1], aux["UB"][1])]
    assert int((read_entry != UNSTAGED).sum()) == int(st["freq"].sum())
    n_cols = len(st["cells"]) if per_cell else 1
    col = st["bucket_cell"] if per_cell else np.zeros(len(off) - 1, np.uint32)
    jn, trip, counts = junction_matrix(np.array(ref, np.int32), np.array(pos, np.int32), np.array(words, np.uint32),
                                       np.array(woff, np.uint64), read_entry, mask, root, st["bucket_off"], col)
    out = dict(files=directory_files(jn, trip, n_cols, ref_names), filtered=None, counts=counts, jn=jn, trip=trip, called=None, st=st,
               mask=mask)
    if cell_min_molecules is not None:
        per_col = np.zeros(n_cols, np.int64)
        np.add.at(per_col, np.repeat(np.asarray(col).astype(np.int64), np.diff(off)), (np.asarray(mask) != 0).astype(np.int64))
        out["called"] = np.flatnonzero(per_col >= cell_min_molecules)
        fjn, ftrip = filter_columns(jn, trip, out["called"])
        out["filtered"] = directory_files(fjn, ftrip, len(out["called"]), ref_names)
    return out
