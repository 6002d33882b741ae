"""Test-side definition of umi_call_cells (csrc/umihip_cells.hip) and of --cell-filter (host/umicollapse_main.cpp), in
plain numpy, independent of the library.

Input: triplets (row, col, molecules, reads) sorted by col, then row, every (col, row) once.  Per column c: T[c] the
sum of molecules, R[c] the sum of reads, G[c] its triplets with molecules > 0.  The candidates are the n columns with
T[c] >= 1, S their totals in descending order.  A rule yields one threshold t; column c is called iff T[c] >= 1 and
T[c] >= t, a tie at the threshold whole.
  CR22: i = min(n - 1, floor(N * (1000 - P) / 1000)), m = S[i], t = max(1, floor((2 m + R) / (2 R)))
  TOP : t = S[min(n - 1, N - 1)]
  MIN : t = max(1, min_molecules)
  n == 0: t = 0, nothing is called.
Medians are lower medians: element floor((k - 1) / 2) of the k called values in ascending order, 0 for k = 0.

call_model states it; the generators below give the inputs the tests name; cells_bam is a small --per-cell --per-gene
BAM whose cells differ in depth by a factor of thirty, files_model the program's added files from its raw ones."""
import struct
from collections import namedtuple

import numpy as np

import bamio
import gene_model as gm
import tag_model

CR22, TOP, MIN = 0, 1, 2
NOT_CALLED = 0xFFFFFFFF
COUNTS = ("candidates", "called", "threshold", "knee", "molecules_in_cells", "reads_in_cells", "molecules", "reads",
          "median_molecules", "median_genes")
M64 = (1 << 64) - 1

Case = namedtuple("Case", "row col molecules reads n_rows n_cols")


def threshold(totals_desc, rule, expect_cells=3000, percentile_permille=990, max_min_ratio=10, min_molecules=1):
    """(t, m) for the candidates' totals in descending order (Python ints)"""
    n = len(totals_desc)
    if n == 0:
        return 0, 0
    if rule == CR22:
        m = int(totals_desc[min(n - 1, expect_cells * (1000 - percentile_permille) // 1000)])
        return max(1, (2 * m + max_min_ratio) // (2 * max_min_ratio)), m
    if rule == TOP:
        return int(totals_desc[min(n - 1, expect_cells - 1)]), 0
    assert rule == MIN
    return max(1, min_molecules), 0


def lower_median(values):
    a = sorted(int(v) for v in values)
    return a[(len(a) - 1) // 2] if a else 0


def call_model(case, rule, expect_cells=3000, percentile_permille=990, max_min_ratio=10, min_molecules=1):
    """(dict of the per-column arrays, the filtered triplets (row, col, molecules, reads), dict of COUNTS)"""
    row, col = np.asarray(case.row, np.uint32), np.asarray(case.col, np.uint32)
    mol, reads = np.asarray(case.molecules, np.uint32), np.asarray(case.reads, np.uint64)
    n_cols = case.n_cols
    c64 = col.astype(np.int64)
    T, R = np.zeros(n_cols, np.uint64), np.zeros(n_cols, np.uint64)
    G = np.zeros(n_cols, np.uint32)
    np.add.at(T, c64, mol.astype(np.uint64))
    np.add.at(R, c64, reads)
    np.add.at(G, c64, (mol != 0).astype(np.uint32))
    cand = T[T >= 1]
    desc = np.sort(cand)[::-1]
    t, m = threshold([int(x) for x in desc], rule, expect_cells, percentile_permille, max_min_ratio, min_molecules)
    called = (T >= 1) & (T >= np.uint64(min(t, M64)))
    new_col = np.full(n_cols, NOT_CALLED, np.uint32)
    new_col[called] = np.arange(int(called.sum()), dtype=np.uint32)
    keep = called[c64] & (mol != 0) if len(col) else np.zeros(0, bool)
    counts = [len(cand), int(called.sum()), t, m, sum(int(x) for x in T[called]) & M64, sum(int(x) for x in R[called]) & M64,
              sum(int(x) for x in T) & M64, sum(int(x) for x in R) & M64, lower_median(T[called]), lower_median(G[called])]
    per = {"cell_molecules": T, "cell_reads": R, "cell_genes": G, "called": called.astype(np.uint8), "new_col": new_col}
    return per, (row[keep], new_col[c64[keep]], mol[keep], reads[keep]), dict(zip(COUNTS, counts))


# ---- inputs

def from_pairs(pairs, molecules, reads, n_rows, n_cols):
    """a Case from (col, row) pairs in any order: sorted, the values following their pairs"""
    order = sorted(range(len(pairs)), key=lambda i: pairs[i])
    return Case(np.array([pairs[i][1] for i in order], np.uint32), np.array([pairs[i][0] for i in order], np.uint32),
                np.asarray(molecules, np.uint32)[order] if len(order) else np.zeros(0, np.uint32),
                np.asarray(reads, np.uint64)[order] if len(order) else np.zeros(0, np.uint64), n_rows, n_cols)


def values(rng, nnz, zero_share=0.15, top=6):
    """small molecule counts (ties between columns are the rule, not the exception), a share of them 0; reads at or
    above the molecules, never 0"""
    mol = rng.integers(1, top, nnz).astype(np.uint32)
    mol[rng.random(nnz) < zero_share] = 0
    return mol, (mol.astype(np.uint64) + rng.integers(1, 50, nnz).astype(np.uint64))


def random_case(seed, nnz, n_rows=97, n_cols=None):
    """exactly nnz triplets at distinct random places of an n_rows x n_cols matrix, geometric column depths"""
    rng = np.random.default_rng(seed)
    if n_cols is None:
        n_cols = max(1, (3 * nnz) // n_rows + 3)
    assert nnz <= n_rows * n_cols
    weight = rng.random(n_cols) ** 6 + 1e-3
    weight[rng.random(n_cols) < 0.2] = 0  # (gaps: columns without a triplet)
    weight[0] += 1e-6
    cells = set()
    while len(cells) < nnz:
        want = nnz - len(cells)
        c = rng.choice(n_cols, size=2 * want + 8, p=weight / weight.sum())
        r = rng.integers(0, n_rows, len(c))
        for pair in zip(c.tolist(), r.tolist()):
            if len(cells) < nnz:
                cells.add(pair)
        weight += 1e-4  # (a full column cannot stall the draw)
    mol, reads = values(rng, nnz)
    return from_pairs(sorted(cells), mol, reads, n_rows, n_cols)


def runs_case(seed, runs, gap_every=3, empty_tail=5):
    """columns of the given numbers of triplets, in that order; every gap_every-th column id is skipped and the last
    empty_tail columns hold nothing"""
    rng = np.random.default_rng(seed)
    n_rows = max(runs) + 7
    pairs, c = [], 0
    for k, length in enumerate(runs):
        if gap_every and k % gap_every == gap_every - 1:
            c += 1 + k % 2
        rows = np.sort(rng.choice(n_rows, size=length, replace=False))
        pairs += [(c, int(r)) for r in rows]
        c += 1
    mol, reads = values(rng, len(pairs))
    return Case(np.array([p[1] for p in pairs], np.uint32), np.array([p[0] for p in pairs], np.uint32), mol, reads, n_rows,
                c + empty_tail)


def one_column(seed, nnz):
    rng = np.random.default_rng(seed)
    mol, reads = values(rng, nnz)
    return Case(np.arange(nnz, dtype=np.uint32), np.zeros(nnz, np.uint32), mol, reads, max(nnz, 1), 1)


def one_each(seed, nnz):
    """every column one triplet"""
    rng = np.random.default_rng(seed)
    mol, reads = values(rng, nnz)
    return Case(rng.integers(0, 11, nnz).astype(np.uint32), np.arange(nnz, dtype=np.uint32), mol, reads, 11, max(nnz, 1))


def big_case():
    """column 1: three rows of 0xFFFFFFFF molecules (a total above 2^32) and reads near 2^40; column 3: triplets that
    are all 0 molecules (reads, no candidate); columns 0, 2, 4: small; column 5 empty"""
    big = 0xFFFFFFFF
    pairs = [(0, 1), (0, 2), (1, 0), (1, 3), (1, 4), (2, 2), (3, 0), (3, 1), (4, 4)]
    mol = [3, 0, big, big, big, 7, 0, 0, 3]
    reads = [5, 2, (1 << 40) - 3, (1 << 40) - 1, 1 << 39, 9, 4, 6, 3]
    return from_pairs(pairs, mol, reads, 5, 6)


def totals_case(totals, n_rows=3):
    """columns of the given totals, one triplet each (total 0: a triplet of 0 molecules)"""
    n = len(totals)
    return Case(np.arange(n, dtype=np.uint32) % n_rows, np.arange(n, dtype=np.uint32), np.array(totals, np.uint32),
                np.array(totals, np.uint64) + np.uint64(1), n_rows, n)


TIED_TOTALS = (50, 40, 40, 40, 12, 4, 4, 4, 1)
# a rule of each kind whose threshold (40, 4, 40) three columns of tied_case hold exactly
TIED_RULES = (dict(rule=TOP, expect_cells=2), dict(rule=CR22, expect_cells=2, percentile_permille=0, max_min_ratio=10),
              dict(rule=MIN, min_molecules=40))


def tied_case(seed, totals=TIED_TOTALS, n_rows=40):
    """columns of the given totals in random order, each split over several triplets, triplets of 0 molecules among
    them"""
    rng = np.random.default_rng(seed)
    pairs, mol = [], []
    for c, total in enumerate(rng.permutation(totals).tolist()):
        parts = int(rng.integers(1, min(total, 6) + 1))
        cuts = np.sort(rng.choice(np.arange(1, total), size=parts - 1, replace=False)) if parts > 1 else np.zeros(0, np.int64)
        values_c = np.diff(np.concatenate([[0], cuts, [total]])).tolist() + [0] * int(rng.integers(0, 3))
        rows = np.sort(rng.choice(n_rows, size=len(values_c), replace=False))
        pairs += [(c, int(r)) for r in rows]
        mol += [values_c[i] for i in rng.permutation(len(values_c))]
    reads = np.array(mol, np.uint64) + rng.integers(1, 9, len(mol)).astype(np.uint64)
    return from_pairs(pairs, mol, reads, n_rows, len(totals))


# ---- the program's side

DEPTHS = (30, 30, 24, 24, 20, 6, 6, 3, 2, 1)  # molecules per cell of cells_bam
# the rules the CLI tests run: flags and the model's parameters
CLI_RULES = {
    "cr2.2": (["--cell-filter", "cr2.2", "--expect-cells", "4", "--cell-filter-percentile", "0.5", "--cell-filter-ratio", "4"],
              dict(rule=CR22, expect_cells=4, percentile_permille=500, max_min_ratio=4)),
    "top-cells": (["--cell-filter", "top-cells", "--expect-cells", "3"], dict(rule=TOP, expect_cells=3)),
    "min-molecules": (["--cell-filter", "min-molecules", "--cell-min-molecules", "5"], dict(rule=MIN, min_molecules=5)),
}


def cells_bam(seed, umi_len=10, n_genes=9, depths=DEPTHS):
    """(header, records, barcodes): reads with UB, CB ("<16 bases>-1"), CR (the 16 bases) and GX.  Cell c holds
    depths[c] molecules -- UMIs at least 3 substitutions apart, so that no collapse joins two -- of 1 to 3 reads each,
    over random genes; one UMI of the deepest cell lies under two genes with different reads (--umi-filtering
    multi-gene removes a molecule there)."""
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    draw = lambda L: "".join(letters[x] for x in rng.integers(0, 4, L))
    cells = []
    while len(cells) < len(depths):
        b = draw(16)
        if all(gm.hamming(b, v) >= 4 for v in cells):
            cells.append(b)
    umis = []
    while len(umis) < sum(depths):
        u = draw(umi_len)
        if all(gm.hamming(u, v) >= 3 for v in umis):
            umis.append(u)
    reads, at = [], 0  # (cell, gene, UMI, count)
    for c, depth in enumerate(depths):
        for _ in range(depth):
            reads.append((c, int(rng.integers(0, n_genes)), umis[at], int(rng.integers(1, 4))))
            at += 1
    c0, g0, u0, _ = reads[0]
    reads[0] = (c0, g0, u0, 3)
    reads.append((c0, (g0 + 1) % n_genes, u0, 1))  # (the same UMI under a second gene of cell 0: one read against three)
    items, i = [], 0
    for c, g, u, count in reads:
        for _ in range(count):
            pos = 1000 + 10 * int(rng.integers(0, 200))
            tags = tag_model.aux_z("UB", u) + tag_model.aux_z("CB", cells[c] + "-1") + tag_model.aux_z("CR", cells[c])
            tags += tag_model.aux_z("GX", "GENE%02d" % g) + b"xxi" + struct.pack("<i", i)
            quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
            items.append((pos, i, bamio.make_record("r%d" % i, 0, 0, pos, int(rng.integers(0, 61)), [("M", 50)], 50, quals, tags=tags)))
            i += 1
    items.sort(key=lambda t: (t[0], t[1]))
    return bamio.make_header([("chr1", 10_000_000)]), [t[2] for t in items], cells


def case_of_files(files):
    """the triplets of a --count-matrix directory's matrix.mtx and reads.mtx as a Case, and its barcodes"""
    out = []
    for name in ("matrix.mtx", "reads.mtx"):
        lines = files[name].decode().splitlines()
        n_rows, n_cols, nnz = (int(x) for x in lines[1].split())
        out.append([tuple(int(x) for x in l.split()) for l in lines[2:]])
        assert len(out[-1]) == nnz
    assert [t[:2] for t in out[0]] == [t[:2] for t in out[1]]
    case = Case(np.array([t[0] - 1 for t in out[0]], np.uint32), np.array([t[1] - 1 for t in out[0]], np.uint32),
                np.array([t[2] for t in out[0]], np.uint32), np.array([t[2] for t in out[1]], np.uint64), n_rows, n_cols)
    return case, files["barcodes.tsv"].splitlines()


def files_model(files, **rule):
    """what --cell-filter adds to a --count-matrix directory with these four files: ({path below DIR: bytes}, counts)"""
    case, cells = case_of_files(files)
    per, trip, counts = call_model(case, **rule)
    called = [c for c in range(case.n_cols) if per["called"][c]]
    sub = gm.matrix_files([], [cells[c] for c in called], case.n_rows, len(called), trip)
    table = b"barcode\treads\tmolecules\tgenes\tcalled\n" + b"".join(
        b"%s\t%d\t%d\t%d\t%d\n" % (cells[c], int(per["cell_reads"][c]), int(per["cell_molecules"][c]), int(per["cell_genes"][c]),
                                  int(per["called"][c])) for c in range(case.n_cols) if per["cell_molecules"][c] >= 1)
    out = {"filtered/features.tsv": files["features.tsv"], "filtered/barcodes.tsv": sub["barcodes.tsv"],
           "filtered/matrix.mtx": sub["matrix.mtx"], "filtered/reads.mtx": sub["reads.mtx"], "cells.tsv": table}
    return out, counts
