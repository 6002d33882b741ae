"""Inputs that send every grid-stride kernel of the analysis calls round its loop more than once, for
tests/test_gpu_grid_trips.py; tests/test_grid_trip_inputs_cpu.py proves on the CPU, with the models alone, that each one
has the property it is named for.

Every call since the collapse sizes a kernel's grid as min(blocks the input needs, n_cus * c) and lets a block stride
over the rest.  On a whole device a second trip starts only beyond half a million items, which no plain-Python model
gets through in a test's time; with the option "grid_cus" at 1 the same code runs from a few thousand items on.  The
inputs are sized for that: counts of the form 2 T + 64 a + b with 0 < b < 64 against the capacity T of one trip -- two
full trips and a partial third whose last wave is itself partial.

Nothing here is a new model: the references are tests/*_model.py as they are, the inputs come from their generators
and from the generators of the per-feature GPU test files."""
import functools

import numpy as np

import annotation_model as am
import barcode_model as bm
import barcode_multi_model as bmm
import cells_model as clm
import consensus_model as cm
import gene_model as gm
import intron_model as im
import seq_model as sm
import velocity_model as vm
import whitelist_model as wm

GRIDS = (1, 3)  # "grid_cus": one CU, and a stride that is no power of two

# What one trip of a kernel's grid takes with "grid_cus" at 1: name -> (items, what an item is, the launch line in
# umi_collapse_rs_amd/csrc that caps the grid).  A block has 256 threads (4 waves) unless said otherwise.
CAPACITY = {
    "stats_entry":      (2048, "entries: 8 blocks", "umihip_stats.hip:674"),
    "stats_post":       (2048, "entries: 8 blocks", "umihip_stats.hip:722"),
    "stats_lane":       (2048, "non-empty buckets: 8 blocks", "umihip_stats.hip:706"),
    "stats_wave":       (2048, "non-empty buckets: 8 blocks", "umihip_stats.hip:710"),
    "stats_deep":       (32, "pieces of deep buckets: 8 blocks, a wave each", "umihip_stats.hip:714"),
    "barcode_build":    (2048, "list entries: 8 blocks", "umihip_barcode.hip:497"),
    "barcode_check":    (2048, "reads: 8 blocks", "umihip_barcode.hip:500"),
    "barcode_lookup":   (2048, "reads: 8 blocks", "umihip_barcode.hip:538"),
    "barcode_resolve":  (32, "queued reads: 8 blocks, a wave each", "umihip_barcode.hip:562"),
    "correct_check":    (2048, "reads: 8 blocks", "umihip_correct.hip:233"),
    "correct":          (4096, "reads: 8 blocks of CORR_CHUNK = 512", "umihip_correct.hip:256"),
    "cells_keys":       (2048, "columns: 8 blocks", "umihip_cells.hip:349"),
    "cells_call":       (2048, "columns: 8 blocks", "umihip_cells.hip:349"),
    "count_reduce":     (2048, "non-empty buckets: 8 blocks", "umihip_count.hip:265"),
    "velocity_reduce":  (2048, "non-empty buckets: 8 blocks", "umihip_velocity.hip:314"),
    "velocity_scatter": (4096, "reads: 16 blocks", "umihip_velocity.hip:292"),
    "mg_entry":         (2048, "entries: 8 blocks", "umihip_multigene.hip:386"),
    "mg_write":         (2048, "entries: 8 blocks", "umihip_multigene.hip:420"),
    "gene_assign":      (2048, "reads: 2 blocks of 1,024", "umihip_genes.hip:171"),
    "gene_introns":     (2048, "reads: 2 blocks of 1,024", "umihip_gene_introns.hip:196"),
    "gene_classes":     (2048, "reads: 2 blocks of 1,024", "umihip_gene_classes.hip:240"),
    "cons_vote":        (2048, "entries a tile: GW = 32 waves, 64 entries each", "umihip_consensus.hip:537"),
    "cons_deep":        (32, "GW: chunks of one deep cluster a round", "umihip_consensus.hip:541"),
    "cons_deep_call":   (32, "GW: deep clusters", "umihip_consensus.hip:542"),
    "consb_vote":       (512, "clusters a tile: GW = 8 waves (2 blocks), 64 clusters each", "umihip_consensus_bam.hip:555"),
    "consb_deep":       (8, "GW: pieces of one deep cluster a round", "umihip_consensus_bam.hip:559"),
    "consb_deep_call":  (8, "GW: deep clusters", "umihip_consensus_bam.hip:560"),
    "seq_pair":         (16, "one-wave blocks, persistent: a block deals itself tiles", "umihip_seq_api.cpp:133"),
}
T = 2048
CORR_TILE, CONS_CHUNK, CONSB_CHUNK, CONS_GW, CONSB_GW = 1024, 128, 128, 32, 8  # umihip_internal.h, umihip_consensus*.hip


def cap(name):
    return CAPACITY[name][0]


def trips(n, per_trip):
    """(full trips, whole waves of the last trip, lanes of its last wave)"""
    full, rest = divmod(int(n), per_trip)
    return full, rest // 64, rest % 64


def two_trips_and_a_partial_wave(n, per_trip):
    full, _, b = trips(n, per_trip)
    return full >= 2 and 0 < b < 64


# ---- umi_correct_umis ---------------------------------------------------------------------------------------------------

CORR_READS = 2 * 4096 + 513
CORR_LISTS = {"one_tile": CORR_TILE, "tile_and_one": CORR_TILE + 1, "two_tiles_and_three": 2 * CORR_TILE + 3}
CORR_LENGTHS = (12, 20)  # one and two 32-bit words a packed UMI
CORR_BAD = ((8500, 3, ord("x")), (8200, 0, ord("n")), (8200, 7, 0))  # (read, base, byte): both reads in the third trip


@functools.lru_cache(maxsize=None)
def correct_case(L, name):
    """(list uint8 [n_wl * L], reads uint8 [CORR_READS * L]); the list's last entry -- alone in its tile, or nearly, in the
    longer lists -- is read in every trip, the last read of all included"""
    rng = np.random.default_rng(4000 + 100 * L + CORR_LISTS[name])
    wl = wm.random_list(rng, CORR_LISTS[name], L)
    reads = wm.noisy_reads(rng, wl, L, CORR_READS).reshape(-1, L).copy()
    for r in (7, 4096 + 7, 2 * 4096 + 7, CORR_READS - 1):
        reads[r] = wl.reshape(-1, L)[-1]
    return wl, reads.reshape(-1)


@functools.lru_cache(maxsize=None)
def correct_expected(L, name):
    wl, reads = correct_case(L, name)
    return wm.correct(reads, L, wl, 1, 1)


def correct_bad_reads(L, name):
    bad = correct_case(L, name)[1].copy()
    for r, b, ch in CORR_BAD:
        bad[r * L + b] = ch
    return bad


# ---- umi_correct_barcodes / _multi --------------------------------------------------------------------------------------

BC_LENGTHS = (16, 17)  # the tag is the key itself / the hash's high half
BC_LIST = 2 * T + 77
BC_READS = 2 * T + 65
BC_DUP = (2 * T - 1096, 5)  # entry 3000 is entry 5 again: found by barcode_dup_kernel's second trip
BC_BAD = ((2 * T + 54, 3, ord("x")), (2 * T + 24, 0, ord("n")))  # (read, base, byte): both reads in the third trip
BC_BAD_QUAL = (2 * T + 34, 2, 10)                               # ... and a quality byte outside 33..126 there


def n_count(rows):
    return (rows == ord("N")).sum(axis=1)


@functools.lru_cache(maxsize=None)
def barcode_case(L):
    """(list [n_wl, L], reads uint8 [n * L], qualities uint8 [n * L]).  Every third wave of 64 reads, and the one
    whole wave of the last trip, holds listed barcodes and two-N reads only (nothing of it goes to the wave's queue);
    the others hold every kind; the last read, alone in its wave, is ambiguous."""
    rng = np.random.default_rng(1600 + L)
    wl, pairs = bm.random_list(rng, BC_LIST, L)
    reads, quals = bmm.multi_reads(rng, wl, BC_READS, pairs)
    u = reads.reshape(-1, L).copy()
    for w in list(range(0, 2 * T // 64, 3)) + [2 * T // 64]:
        for i in range(64 * w, 64 * w + 64):
            u[i] = wl[int(rng.integers(0, len(wl)))]
            if i % 5 == 0:
                u[i, rng.choice(L, size=2, replace=False)] = ord("N")
    st = bm.correct(u.reshape(-1), L, wl, 1)["status"]
    u[-1] = u[np.flatnonzero(st == bm.AMBIGUOUS)[0]]
    return wl, np.ascontiguousarray(u.reshape(-1)), quals


@functools.lru_cache(maxsize=None)
def barcode_expected(L, mm):
    wl, reads, _ = barcode_case(L)
    return bm.correct(reads, L, wl, mm)


@functools.lru_cache(maxsize=None)
def barcode_multi_expected(L):
    wl, reads, quals = barcode_case(L)
    return bmm.correct_multi(reads, quals, L, wl)


def barcode_dup_list(L):
    dup = barcode_case(L)[0].copy()
    dup[BC_DUP[0]] = dup[BC_DUP[1]]
    return dup


def barcode_bad_reads(L):
    bad = barcode_case(L)[1].copy()
    for r, b, ch in BC_BAD:
        bad[r * L + b] = ch
    return bad


def barcode_bad_quals(L):
    bad = barcode_case(L)[2].copy()
    r, b, ch = BC_BAD_QUAL
    bad[r * L + b] = ch
    return bad


def goes_to_the_queue(L):
    """bool per read: what barcode_lookup_kernel queues under max_mismatches 1 -- not listed, one N at the most"""
    wl, reads, _ = barcode_case(L)
    return (barcode_expected(L, 1)["status"] != bm.EXACT) & (n_count(reads.reshape(-1, L)) <= 1)


# ---- umi_count_matrix and umi_velocity_matrix ---------------------------------------------------------------------------

MATRIX_BUCKETS = 2 * T + 300
MATRIX_ROWS, MATRIX_COLS = 500, 40


def matrix_sizes(seed):
    """MATRIX_BUCKETS non-empty buckets, mostly of 1 to 4 entries, every 37th of 33 to 90 (a wave's: more than 32), an
    empty one behind every seventh and at both ends"""
    rng = np.random.default_rng(seed)
    sizes = [0]
    for j in range(MATRIX_BUCKETS):
        sizes.append(int(rng.integers(33, 91)) if j % 37 == 5 else int(rng.integers(1, 5)))
        if j % 7 == 6:
            sizes.append(0)
    return sizes + [0]


@functools.lru_cache(maxsize=None)
def count_case():
    """(kept, freq, off, row, col, n_rows, n_cols) as tests/test_gpu_count_matrix.py has them"""
    from test_gpu_count_matrix import entries
    rng = np.random.default_rng(71)
    sizes = matrix_sizes(70)
    kept, freq, off = entries(rng, sizes)
    row = rng.integers(0, MATRIX_ROWS, len(sizes)).astype(np.uint32)
    col = rng.integers(0, MATRIX_COLS, len(sizes)).astype(np.uint32)
    return kept, freq, off, row, col, MATRIX_ROWS, MATRIX_COLS


@functools.lru_cache(maxsize=None)
def count_expected():
    return gm.count_model(*count_case()[:5])


@functools.lru_cache(maxsize=None)
def velocity_case():
    return vm.make_molecules(72, matrix_sizes(73), MATRIX_ROWS, MATRIX_COLS)


@functools.lru_cache(maxsize=None)
def velocity_expected():
    m = velocity_case()
    return vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])


def non_empty_sizes(off):
    d = np.diff(np.asarray(off).astype(np.int64))
    return d[d > 0]


# ---- umi_filter_multigene -----------------------------------------------------------------------------------------------

MG_ENTRIES = 2 * T + 200
MG_LENGTHS = (12, 22)  # a one-word key composed with the group, and a wide one


@functools.lru_cache(maxsize=None)
def multigene_case(L):
    """a tests/test_gpu_multigene.py Case: small buckets over few UMIs and five cells, so that (cell, UMI) runs of
    several molecules lie everywhere"""
    from test_gpu_multigene import pool_case
    rng = np.random.default_rng(900 + L)
    sizes = []
    while sum(sizes) < MG_ENTRIES:
        sizes.append(min(int(rng.choice([0, 1, 1, 2, 3, 6])), MG_ENTRIES - sum(sizes)))
    return pool_case(901 + L, sizes, L, 5, pool=400)


# ---- umi_call_cells -----------------------------------------------------------------------------------------------------

CELLS_COLS = 2 * T + 100


@functools.lru_cache(maxsize=None)
def cells_cases():
    """"one_each": a triplet a column; "runs": columns of one to five triplets, every third column id skipped or two of
    them (empty columns all along), six empty ones at the end"""
    rng = np.random.default_rng(55)
    runs = [int(x) for x in rng.integers(1, 6, 2794)]
    return {"one_each": clm.one_each(57, CELLS_COLS), "runs": clm.runs_case(56, runs, empty_tail=6)}


def cells_rules(name):
    from test_gpu_call_cells import rules_for
    return rules_for(cells_cases()[name])


@functools.lru_cache(maxsize=None)
def cells_expected(name, k):
    return clm.call_model(cells_cases()[name], **cells_rules(name)[k])


# ---- umi_assign_genes, _introns, _classes -------------------------------------------------------------------------------

GENE_READS = 2 * T + 100
GENE_TOPS = ((1, 1), (1, 0), (0, 0))  # ("gene_top", "gene_body_top")
N_GENES, N_GENES_CLASSES = 40, vm.FUZZ_GENES


def gene_reads():
    return am.fuzz_reads(n=GENE_READS)


def class_reads():
    return vm.fuzz_reads(n=GENE_READS)


@functools.lru_cache(maxsize=None)
def genes_expected(mode):
    return am.assign_all(am.fuzz_annotation(), gene_reads(), mode)


@functools.lru_cache(maxsize=None)
def introns_expected(mode, introns):
    return im.assign_all(am.fuzz_annotation(), gene_reads(), mode, introns)


@functools.lru_cache(maxsize=None)
def classes_expected(mode, introns):
    return vm.classify_all(vm.fuzz_annotation(), class_reads(), mode, introns)


# ---- umi_dedup_stats ----------------------------------------------------------------------------------------------------

STATS_BUCKETS = 2 * T + 300
STATS_LENGTHS = (12, 43)
STATS_B_SPLIT = 64
STATS_B_DEEP = 3 * 1024 + 5


def stats_a_sizes():
    """STATS_BUCKETS non-empty buckets of 1 to 3 entries; bucket j is a wave's (9 to 70 entries) where j % 40 == 7,
    but in no block of 256 buckets whose number is 3 mod 4: those blocks queue nothing in their round.  Empty buckets
    behind every fifth and at both ends."""
    rng = np.random.default_rng(31)
    sizes = [0, 0]
    for j in range(STATS_BUCKETS):
        wave = j % 40 == 7 and (j // 256) % 4 != 3
        sizes.append(int(rng.integers(9, 71)) if wave else int(rng.integers(1, 4)))
        if j % 5 == 4:
            sizes.append(0)
    return sizes + [0]


@functools.lru_cache(maxsize=None)
def stats_case_a(L):
    """(keys, freq, kept, root, off, L) as tests/test_gpu_stats.py has them, kept[] / root[] from its forest()"""
    from test_gpu_stats import made_case
    return made_case(3100 + L, stats_a_sizes(), L)


def stats_b_sizes():
    """under "stats_split" 64: 63 deep buckets of 64 to 200 entries (a piece each) and one of 3 x 1,024 + 5 (four
    pieces): 67 pieces, three trips of the deep kernels; lane's and wave's buckets between them"""
    rng = np.random.default_rng(32)
    sizes = []
    for j in range(63):
        sizes += [int(rng.integers(64, 201)), int(rng.integers(1, 9)), 0, int(rng.integers(9, 64))]
        if j == 40:
            sizes.append(STATS_B_DEEP)
    return sizes


@functools.lru_cache(maxsize=None)
def stats_case_b():
    from test_gpu_stats import made_case
    return made_case(3200, stats_b_sizes(), 12)


@functools.lru_cache(maxsize=None)
def stats_expected(name, L=12, per_umi=True):
    import stats_model as stm
    keys, freq, kept, root, off, L = stats_case_a(L) if name == "a" else stats_case_b()
    return stm.stats_model(keys, freq, kept, root, off, L, seed=5, hist_bins=65536, per_umi=per_umi)


# ---- umi_consensus_seqs -------------------------------------------------------------------------------------------------

CONS_SPLIT = 4  # "cons_split" of the deep cases: a cluster of four reads or more is a deep one
CONS_DEEP_CLUSTERS = 2 * CONS_GW + 11
CONS_DEEP_READS = 2 * CONS_GW * CONS_CHUNK + 130
CONS_CLOSE_BASE, CONS_CLOSE_MARGIN = 3, 7  # the deepest cluster's vote at this base is decided by this much
ACGT = np.frombuffer(b"ACGT", np.uint8)


def _cons_reads(rng, mol, copies, err):
    """`copies` reads of one molecule: the first one exact, the others with substitutions and N at rate err"""
    reads = np.tile(mol, (copies, 1))
    hit = rng.random(reads.shape) < err
    hit[0] = False
    reads[hit] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(hit.sum()))
    return [r.tobytes() for r in reads]


def _cons_finish(rng, seqs, mol_of, L, close_vote=None):
    """shuffle the reads, stage them by the model, and hang every entry on its molecule's entry.  close_vote: a
    molecule whose reads say A or C at base CONS_CLOSE_BASE; their qualities there are set so that A wins by
    CONS_CLOSE_MARGIN over all of them together -- leave any reads out and the called quality, or the base, changes"""
    order = rng.permutation(len(seqs))
    seqs = [seqs[i] for i in order]
    quals = [rng.integers(33, 90, L, dtype=np.uint8).tobytes() for _ in seqs]
    if close_vote is not None:
        mine = [i for i, s in enumerate(seqs) if mol_of[s] == close_vote]
        q = {i: 33 + 20 + i % 21 for i in mine}
        sign = lambda i: 1 if seqs[i][CONS_CLOSE_BASE] == ord("A") else -1
        d = sum(sign(i) * (q[i] - 33) for i in mine) - CONS_CLOSE_MARGIN
        for i in mine:  # (a step of one towards the margin per read, as far as it takes)
            if d == 0:
                break
            step = -1 if d * sign(i) > 0 else 1
            q[i] += step
            d += step * sign(i)
        assert d == 0
        for i in mine:
            quals[i] = quals[i][:CONS_CLOSE_BASE] + bytes([q[i]]) + quals[i][CONS_CLOSE_BASE + 1:]
    ent, off, blen = sm.stage(seqs, quals, 1)
    at = {e[0]: j for j, e in enumerate(ent)}
    root = np.array([at[mol_of[e[0]]] for e in ent], np.uint32)
    kept = (root == np.arange(len(ent))).astype(np.uint8)
    staged = dict(freq=np.array([e[1] for e in ent], np.int32), entry_of_read=np.array(cm.entry_of_reads(seqs, ent), np.uint32),
                  bucket_off=np.array(off, np.uint64), bucket_len=np.array(blen, np.int32))
    return seqs, quals, staged, kept, root


@functools.lru_cache(maxsize=None)
def cons_entries_case(n_entries, L=24):
    """exactly n_entries entries: molecules of 1 to 4 reads with errors, an entry per distinct read, each under its
    molecule's entry (about a third of the entries are kept).  (seqs, quals, staged, kept, root)"""
    rng = np.random.default_rng(8000 + n_entries)
    seqs, mol_of = [], {}
    while len(mol_of) < n_entries:
        mol = rng.choice(ACGT, L)
        if mol.tobytes() in mol_of:
            continue
        copies = min(int(rng.integers(1, 5)), n_entries - len(mol_of))
        reads = _cons_reads(rng, mol, copies, 0.12)
        if any(mol_of.get(r, mol.tobytes()) != mol.tobytes() for r in reads):
            continue
        for r in reads:
            mol_of[r] = mol.tobytes()
        seqs += reads
    return _cons_finish(rng, seqs, mol_of, L)


@functools.lru_cache(maxsize=None)
def cons_deep_case(L=20):
    """under "cons_split" 4: CONS_DEEP_CLUSTERS clusters of four reads or more -- one of CONS_DEEP_READS -- among 150 of
    one to three"""
    rng = np.random.default_rng(8100)
    counts = [int(rng.integers(4, 10)) for _ in range(CONS_DEEP_CLUSTERS - 1)] + [int(rng.integers(1, 4)) for _ in range(150)]
    counts = [counts[i] for i in rng.permutation(len(counts))]
    counts.insert(100, CONS_DEEP_READS)
    seqs, mol_of, big = [], {}, None
    for copies in counts:
        while True:
            mol = rng.choice(ACGT, L)
            reads = _cons_reads(rng, mol, copies, 0.03)
            if copies == CONS_DEEP_READS:  # every other read of the deepest cluster says C where the molecule says A
                mol[CONS_CLOSE_BASE] = ord("A")
                reads = [r[:CONS_CLOSE_BASE] + (b"A", b"C")[i & 1] + r[CONS_CLOSE_BASE + 1:] for i, r in enumerate(reads)]
                big = mol.tobytes()
            if all(mol_of.get(r, mol.tobytes()) == mol.tobytes() for r in reads):
                break
        for r in reads:
            mol_of[r] = mol.tobytes()
        seqs += reads
    return _cons_finish(rng, seqs, mol_of, L, close_vote=big)


@functools.lru_cache(maxsize=None)
def cons_expected(name):
    seqs, quals, staged, kept, root = cons_deep_case() if name == "deep" else cons_entries_case(name)
    return cm.clusters(seqs, quals, staged["entry_of_read"], kept, root)


CONS_ENTRIES = (700, 2 * T + 70)


# ---- umi_consensus_bam --------------------------------------------------------------------------------------------------

CONSB_CLUSTERS = (300, 1100)
CONSB_DEEP_CLUSTERS = 2 * CONSB_GW + 4
CONSB_DEEP_VOTERS = 2 * CONSB_GW * CONSB_CHUNK + 130


def _consb_case(seed, depths, L=36):
    """a tests/test_gpu_consensus_bam.py Case: cluster c has depths[c] voters; a ninth as many reads vote nowhere"""
    from test_gpu_consensus_bam import Case, family
    from umi_collapse_rs_amd._lib import UMI_NO_CLUSTER
    rng = np.random.default_rng(seed)
    reads = []
    for c, depth in enumerate(depths):
        reads += [(s, q, L, c) for s, q in family(rng, L, depth, err=0.03, odd_codes=0.02)] if depth else []
    for _ in range(len(reads) // 9):
        s, q = family(rng, L, 1)[0]
        reads.append((s, q, L, UMI_NO_CLUSTER))
    order = rng.permutation(len(reads))
    return Case([reads[i] for i in order], [L] * len(depths))


@functools.lru_cache(maxsize=None)
def consb_clusters_case(n_clusters):
    rng = np.random.default_rng(8200 + n_clusters)
    depths = [0 if c % 97 == 5 else int(rng.integers(1, 4)) for c in range(n_clusters)]
    return _consb_case(8300 + n_clusters, depths)


@functools.lru_cache(maxsize=None)
def consb_deep_case():
    """under "cons_split" 4: CONSB_DEEP_CLUSTERS clusters of four voters or more -- one of CONSB_DEEP_VOTERS -- among 100
    of none to three"""
    rng = np.random.default_rng(8400)
    depths = [int(rng.integers(4, 10)) for _ in range(CONSB_DEEP_CLUSTERS - 1)] + [int(rng.integers(0, 4)) for _ in range(100)]
    depths = [depths[i] for i in rng.permutation(len(depths))]
    depths.insert(60, CONSB_DEEP_VOTERS)
    return _consb_case(8401, depths)


@functools.lru_cache(maxsize=None)
def consb_expected(name):
    return (consb_deep_case() if name == "deep" else consb_clusters_case(name)).want()
