"""Test-side definition of umi_saturation_curve and --saturation-curve (include/umihip.h has the same rule), in plain
Python, a second restatement in plain loops over reads, the hash's known answers, and the makers of the tests' inputs.

Nested read subsampling in exact integers.  The collapse is the full-depth one: kept[] and root[] are taken as they
are, nothing is collapsed again per depth (what Cell Ranger does from its molecule table).
  Hash of read i (its index in read_entry), mod 2^64: z = seed + (i + 1) * 0x9E3779B97F4A7C15;
    z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9; z = (z ^ z >> 27) * 0x94D049BB133111EB; z ^= z >> 31; h = z >> 32.
  Level of a read: lev = (h * L) >> 32, in 0..L-1.  A read is in depth j, the sample of (j + 1) / L of the reads, when
    lev <= j.  Depth L-1 holds every read.
  Molecules: a molecule is an entry r with kept[r] != 0; its reads are the reads i with read_entry[i] != UNSTAGED and
    root[read_entry[i]] == r; its level is the smallest level of its reads; it is absent at every depth if it has none.
    A counted read is a read whose root is kept; reads under a root with kept == 0 count nowhere.  A molecule belongs
    to the bucket that holds r.
  Pairs: a distinct (col, row) among the non-empty buckets (several buckets may share one, as in
    gene_model.count_model); its level is the smallest level of the molecules of its buckets.
  Selected columns: with cell_mask those with cell_mask[c] != 0, whether they hold a molecule or not; without, the
    columns with a molecule at full depth.  n_sel is their number.
  curve[L][8], row j = depth j, everything cumulative (lev <= j): reads (counted reads), molecules, pairs, cells
    (selected columns with a molecule), molecules_in_cells, pairs_in_cells (those in selected columns),
    median_molecules (over all n_sel selected columns, those with none as 0, the lower median -- element
    floor((n_sel - 1) / 2) in ascending order, as in cells_model -- of a column's molecules; 0 for n_sel = 0),
    median_genes (the same for a column's pairs)."""
import functools

import numpy as np

import velocity_model as vm

UNSTAGED = vm.UNSTAGED
COLUMNS = ("reads", "molecules", "pairs", "cells", "molecules_in_cells", "pairs_in_cells", "median_molecules", "median_genes")
M64 = (1 << 64) - 1
# (seed, i) -> h, level at L = 10
KNOWN = (((0, 0), 0xe220a839, 8), ((0, 1), 0x6e789e6a, 4), ((0, 2), 0x06c45d18, 0), ((7, 0), 0x63cbe1e4, 3),
         ((M64, 12345), 0x33aea165, 2), ((0, 2 ** 32 - 1), 0xbeeb67ea, 7))
KNOWN_PER_LEVEL = [9828, 10105, 10208, 9927, 10017, 10085, 10014, 9943, 9795, 10078]  # seed 0, i < 100,000, L = 10


def read_hash(seed, i):
    z = (seed + (i + 1) * 0x9E3779B97F4A7C15) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z >> 32


def read_level(seed, i, n_levels):
    return (read_hash(seed, i) * n_levels) >> 32


def levels(seed, n_reads, n_levels):
    """read_level of reads 0 .. n_reads-1, int64, in numpy's wrapping 64-bit arithmetic"""
    with np.errstate(over="ignore"):
        z = np.uint64(seed) + (np.arange(n_reads, dtype=np.uint64) + np.uint64(1)) * np.uint64(0x9E3779B97F4A7C15)
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        z ^= z >> np.uint64(31)
        return (((z >> np.uint64(32)) * np.uint64(n_levels)) >> np.uint64(32)).astype(np.int64)


def lower_median(values):
    values = sorted(values)
    return values[(len(values) - 1) // 2] if values else 0


def saturation_model(read_entry, kept, root, off, row, col, n_cols, n_levels=10, seed=0, cell_mask=None):
    """umi_saturation_curve: uint64 [n_levels, 8]"""
    L = n_levels
    read_entry, kept = np.asarray(read_entry), np.asarray(kept)
    root, off = np.asarray(root).astype(np.int64), np.asarray(off).astype(np.int64)
    n = len(kept)
    lev = levels(seed, len(read_entry), L)
    staged = np.flatnonzero(read_entry != UNSTAGED)
    assert (read_entry[staged] < n).all()
    r = root[read_entry[staged].astype(np.int64)]
    assert ((r >= 0) & (r < n)).all()
    counted = kept[r] != 0
    mol_level = np.full(n, L, np.int64)  # L: no read
    np.minimum.at(mol_level, r[counted], lev[staged][counted])
    reads = np.bincount(lev[staged][counted], minlength=L)
    molecules = np.zeros(L, np.int64)
    pair_level, col_molecules = {}, {}  # (col, row) -> level; col -> molecules per level
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if lo == hi:
            continue
        c, key = int(col[b]), (int(col[b]), int(row[b]))
        pair_level.setdefault(key, L)
        for e in range(lo, hi):
            if kept[e] and mol_level[e] < L:
                molecules[mol_level[e]] += 1
                pair_level[key] = min(pair_level[key], int(mol_level[e]))
                col_molecules.setdefault(c, np.zeros(L, np.int64))[mol_level[e]] += 1
    pairs = np.zeros(L, np.int64)
    col_pairs = {}
    for (c, _), l in pair_level.items():
        if l < L:
            pairs[l] += 1
            col_pairs.setdefault(c, np.zeros(L, np.int64))[l] += 1
    selected = sorted(col_molecules) if cell_mask is None else [int(c) for c in np.flatnonzero(np.asarray(cell_mask))]
    none = np.zeros(L, np.int64)
    sel_m = [np.cumsum(col_molecules.get(c, none)) for c in selected]
    sel_p = [np.cumsum(col_pairs.get(c, none)) for c in selected]
    curve = np.zeros((L, 8), np.uint64)
    for j in range(L):
        curve[j, 0], curve[j, 1], curve[j, 2] = reads[:j + 1].sum(), molecules[:j + 1].sum(), pairs[:j + 1].sum()
        curve[j, 3] = sum(1 for m in sel_m if m[j])
        curve[j, 4], curve[j, 5] = sum(int(m[j]) for m in sel_m), sum(int(p[j]) for p in sel_p)
        curve[j, 6], curve[j, 7] = lower_median([int(m[j]) for m in sel_m]), lower_median([int(p[j]) for p in sel_p])
    return curve


def saturation_restated(read_entry, kept, root, off, row, col, n_cols, n_levels=10, seed=0, cell_mask=None):
    """the same, depth by depth: the reads of the depth are walked, and what they reach is counted in sets"""
    off = [int(x) for x in off]
    bucket_of = {}
    for b in range(len(off) - 1):
        for e in range(off[b], off[b + 1]):
            bucket_of[e] = b
    full = None
    rows = []
    for j in list(range(n_levels))[::-1]:  # (full depth first: it says which columns are selected without a mask)
        n_reads, mols = 0, set()
        for i, e in enumerate(read_entry):
            e = int(e)
            if e == UNSTAGED or read_level(seed, i, n_levels) > j:
                continue
            r = int(root[e])
            if kept[r]:
                n_reads += 1
                mols.add(r)
        pairs = {(int(col[bucket_of[r]]), int(row[bucket_of[r]])) for r in mols}
        if full is None:
            full = sorted({int(col[bucket_of[r]]) for r in mols})
        selected = full if cell_mask is None else [c for c in range(n_cols) if cell_mask[c]]
        per_m = {c: 0 for c in selected}
        per_p = {c: 0 for c in selected}
        for r in mols:
            c = int(col[bucket_of[r]])
            if c in per_m:
                per_m[c] += 1
        for c, _ in pairs:
            if c in per_p:
                per_p[c] += 1
        rows.append([n_reads, len(mols), len(pairs), sum(1 for v in per_m.values() if v), sum(per_m.values()), sum(per_p.values()),
                     lower_median(per_m.values()), lower_median(per_p.values())])
    return np.array(rows[::-1], np.uint64).reshape(n_levels, 8)


# ---- the file of --saturation-curve -----------------------------------------------------------------------

HEADER = "depth\treads\tmolecules\tsaturation\tpairs\tcells\tmolecules_in_cells\tpairs_in_cells\tmedian_molecules\tmedian_genes\n"


def saturation_text(reads, molecules):
    """floor(10000 (reads - molecules) / reads) as 0.dddd, in integers; 0.0000 for no reads"""
    v = 10000 * (reads - molecules) // reads if reads else 0
    return "%d.%04d" % (v // 10000, v % 10000)


def curve_file(curve):
    L = len(curve)
    lines = [HEADER]
    for j in range(L):
        c = [int(x) for x in curve[j]]
        lines.append("\t".join(["%d/%d" % (j + 1, L), str(c[0]), str(c[1]), saturation_text(c[0], c[1])] + [str(x) for x in c[2:]]) + "\n")
    return "".join(lines).encode()


# ---- the inputs ---------------------------------------------------------------------------------------------

def make(seed, sizes, n_rows, n_cols, readless=0.0, **kw):
    """velocity_model.make_molecules' dict without the classes; about `readless` of the entries lose their reads
    (they become unstaged), so that there are molecules without any read"""
    m = dict(vm.make_molecules(seed, sizes, n_rows, n_cols, **kw))
    del m["read_class"]
    if readless:
        rng = np.random.default_rng(seed + 1000)
        gone = rng.random(len(m["kept"])) < readless
        entry = m["read_entry"].copy()
        staged = entry != UNSTAGED
        entry[staged & gone[np.where(staged, entry, 0)]] = UNSTAGED
        m["read_entry"] = entry
    return m


@functools.lru_cache(maxsize=None)
def fuzz(readless=0.1):
    """velocity_model.fuzz_molecules()'s buckets, a tenth of the entries without any read"""
    m = dict(vm.fuzz_molecules())
    del m["read_class"]
    rng = np.random.default_rng(77)
    gone = rng.random(len(m["kept"])) < readless
    entry = m["read_entry"].copy()
    staged = entry != UNSTAGED
    entry[staged & gone[np.where(staged, entry, 0)]] = UNSTAGED
    m["read_entry"] = entry
    return m


def model_of(m, n_cols, n_levels=10, seed=0, cell_mask=None):
    return saturation_model(m["read_entry"], m["kept"], m["root"], m["off"], m["row"], m["col"], n_cols, n_levels, seed, cell_mask)


def expected_cli(recs, n_levels=10, seed=0, per_cell=True, cell_min_molecules=None, multigene=False):
    """what umicollapse [--per-cell] --per-gene --gene-annotation (forward, exon-first) --count-matrix --saturation-curve
    makes of velocity_model.velocity_bam()'s records: dict(file, curve, molecules, reads).  read_entry is by record
    number, as velocity_model.expected_cli builds it."""
    import annotation_model as am
    import bamio
    import gene_model
    import intron_model as im
    import multigene_model as mm
    import tag_model
    exons = vm.fuzz_annotation()
    tagged, _ = im.with_gene_tags(recs, exons, vm.GENE_IDS, am.FORWARD, im.EXON_FIRST)
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
    read_entry = np.full(len(recs), UNSTAGED, np.uint32)
    for i, rec in enumerate(tagged):
        aux = tag_model.parse_aux(rec)
        if bamio.parse_record(rec)["flag"] & 0x4 or "UB" not in aux or (per_cell and "CB" not in aux):
            continue
        if gene_model.gene_class(aux["GX"][1] if "GX" in aux else None) == "one":
            read_entry[i] = entry[(aux["CB"][1] if per_cell else None, aux["GX"][1], aux["UB"][1])]
    assert int((read_entry != UNSTAGED).sum()) == int(st["freq"].sum())
    n_cols = len(st["cells"])
    cell_mask = None
    if cell_min_molecules is not None:
        per_col = np.zeros(n_cols, np.int64)
        np.add.at(per_col, np.repeat(st["bucket_cell"].astype(np.int64), np.diff(off)), (np.asarray(mask) != 0).astype(np.int64))
        cell_mask = (per_col >= cell_min_molecules).astype(np.uint8)
    curve = saturation_model(read_entry, mask, root, st["bucket_off"], st["bucket_gene"], st["bucket_cell"], n_cols, n_levels, seed,
                             cell_mask)
    r = np.asarray(root).astype(np.int64)[read_entry[read_entry != UNSTAGED].astype(np.int64)]
    return dict(file=curve_file(curve), curve=curve, molecules=int(np.count_nonzero(mask)),
                reads=int(np.count_nonzero(np.asarray(mask)[r])), st=st, mask=mask, cell_mask=cell_mask)
