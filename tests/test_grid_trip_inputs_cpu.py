"""The inputs of tests/grid_trip_inputs.py, checked on the CPU before a kernel sees them: with the models alone, each
one gives its kernels two full trips and a partial third whose last wave is partial when "grid_cus" is 1 (counts of
the form 2 T + 64 a + b, 0 < b < 64, against the capacities of grid_trip_inputs.CAPACITY), and has the further
property it is named for -- waves that queue and waves that do not in every trip, wave buckets in every round, a
duplicate beyond the first trip, a bad byte in the third, deep clusters enough to wrap the deep kernels' rounds."""
import numpy as np
import pytest

import annotation_model as am
import barcode_model as bm
import grid_trip_inputs as gi
import intron_model as im
import velocity_model as vm

T = gi.T


def chunks(a, size):
    return [a[i:i + size] for i in range(0, len(a), size)]


def test_the_capacity_table():
    assert gi.trips(2 * T + 65, T) == (2, 1, 1) and gi.trips(2 * T, T) == (2, 0, 0)
    assert gi.two_trips_and_a_partial_wave(2 * T + 65, T) and not gi.two_trips_and_a_partial_wave(2 * T + 64, T)
    assert not gi.two_trips_and_a_partial_wave(T + 65, T)
    for name, (items, what, source) in gi.CAPACITY.items():
        assert items in (8, 16, 32, 512, 2048, 4096) and ":" in source and what, name
    # eight 256-thread blocks a CU everywhere but: the gene kernels (two of 1,024), velocity's scatter (16), the BAM
    # consensus (two blocks: GW = 8 waves), the whole-read pair kernel (16 one-wave blocks)
    assert gi.cap("correct") == 8 * 512 and gi.cap("velocity_scatter") == 16 * 256 and gi.cap("gene_assign") == 2 * 1024
    assert gi.cap("cons_vote") == 64 * gi.CONS_GW and gi.cap("consb_vote") == 64 * gi.CONSB_GW
    assert gi.cap("cons_deep") == gi.CONS_GW == 8 * 4 and gi.cap("consb_deep") == gi.CONSB_GW == 2 * 4
    assert am.GENE_THREADS * am.GENE_BLOCKS_PER_CU == gi.cap("gene_classes")


# ---- umi_correct_umis

@pytest.mark.parametrize("name", list(gi.CORR_LISTS))
@pytest.mark.parametrize("L", gi.CORR_LENGTHS)
def test_correct_umis_inputs(L, name):
    wl, reads = gi.correct_case(L, name)
    n, n_wl = len(reads) // L, len(wl) // L
    assert n == gi.CORR_READS and gi.trips(n, gi.cap("correct")) == (2, 8, 1)
    assert gi.two_trips_and_a_partial_wave(n, gi.cap("correct_check"))
    assert (L + 15) // 16 == {12: 1, 20: 2}[L]
    tiles = -(-n_wl // gi.CORR_TILE)
    assert tiles == {"one_tile": 1, "tile_and_one": 2, "two_tiles_and_three": 3}[name]
    assert n_wl % gi.CORR_TILE == {"one_tile": 0, "tile_and_one": 1, "two_tiles_and_three": 3}[name]
    exp = gi.correct_expected(L, name)
    for trip in chunks(np.arange(n), gi.cap("correct")):  # every verdict in every trip, matches in every tile of the list
        m = exp["match"][trip]
        exact, corrected = (m >= 0) & (exp["best"][trip] == 0), (m >= 0) & (exp["best"][trip] > 0)
        assert exact.any() and corrected.any() and (m < 0).any()
        assert {int(x) // gi.CORR_TILE for x in m[m >= 0]} == set(range(tiles))
    if name != "one_tile":  # the list's last entry, alone in its tile or nearly, is somebody's match in the last trip
        assert (exp["match"][2 * gi.cap("correct"):] >= (tiles - 1) * gi.CORR_TILE).any()
    bad = gi.correct_bad_reads(L, name)
    rows = np.flatnonzero(~np.isin(bad.reshape(-1, L), np.frombuffer(b"ACGTN", np.uint8)).all(axis=1))
    assert rows.tolist() == [8200, 8500] and rows.min() >= 2 * gi.cap("correct")
    assert rows.min() // gi.cap("correct_check") == 4  # (the check kernel's fifth trip)


# ---- umi_correct_barcodes / _multi

@pytest.mark.parametrize("L", gi.BC_LENGTHS)
def test_barcode_inputs(L):
    wl, reads, quals = gi.barcode_case(L)
    n = len(reads) // L
    assert len(wl) == gi.BC_LIST and gi.two_trips_and_a_partial_wave(len(wl), gi.cap("barcode_build"))
    assert n == gi.BC_READS and gi.trips(n, gi.cap("barcode_lookup")) == (2, 1, 1) and len(quals) == len(reads)
    assert len(set(map(bytes, wl))) == len(wl)
    one, zero = gi.barcode_expected(L, 1), gi.barcode_expected(L, 0)
    rows, queued = reads.reshape(-1, L), gi.goes_to_the_queue(L)
    ns = gi.n_count(rows)
    for trip in chunks(np.arange(n), gi.cap("barcode_lookup")):
        waves = [queued[w].any() for w in chunks(trip, 64)]
        assert any(waves) and not all(waves)  # waves that queue reads and waves that queue none
        st, k = one["status"][trip], ns[trip]
        if len(trip) == gi.cap("barcode_lookup"):  # every kind of read: listed, one substitution or one N away, two N, ambiguous, unlisted
            assert (st == bm.EXACT).any() and ((st == bm.CORRECTED) & (k == 0)).any() and ((st == bm.CORRECTED) & (k == 1)).any()
            assert (k == 2).any() and (st == bm.AMBIGUOUS).any() and ((st == bm.NONE) & (k == 0)).any()
            assert (zero["status"][trip] == bm.NONE).sum() > (st == bm.NONE).sum()
    assert len(trip) == 65 and waves == [False, True]  # the last trip: a quiet wave, then one read that is queued
    assert one["status"][-1] == bm.AMBIGUOUS
    # the duplicate lies beyond the list's first trip, its twin inside it
    dup = gi.barcode_dup_list(L)
    later, first = gi.BC_DUP
    assert later >= gi.cap("barcode_build") > first and bytes(dup[later]) == bytes(dup[first])
    assert len(set(map(bytes, dup))) == len(dup) - 1
    # the bad bytes lie in the third trip of the check kernels, the smaller of the two bad reads behind the larger in the list
    assert [r for r, _, _ in gi.BC_BAD] == [2 * T + 54, 2 * T + 24] and 2 * T < gi.BC_BAD_QUAL[0] < n
    rows_bad = gi.barcode_bad_reads(L).reshape(-1, L)
    assert np.flatnonzero(~np.isin(rows_bad, np.frombuffer(b"ACGTN", np.uint8)).all(axis=1)).tolist() == [2 * T + 24, 2 * T + 54]
    q_bad = gi.barcode_bad_quals(L).reshape(-1, L)
    assert np.flatnonzero(((q_bad < 33) | (q_bad > 126)).any(axis=1)).tolist() == [gi.BC_BAD_QUAL[0]]
    # the second pass: three trips of the resolve kernel and more, ambiguous reads of the first pass in every trip of it
    multi = gi.barcode_multi_expected(L)
    amb = np.flatnonzero(one["status"] == bm.AMBIGUOUS)
    assert len(amb) >= 70 > 2 * gi.cap("barcode_resolve") and amb[-1] == n - 1
    assert all(len(np.intersect1d(amb, trip)) for trip in chunks(np.arange(n), gi.cap("barcode_lookup")))
    assert all(int(c) > 0 for c in multi["counts"]) and multi["counts"][4] + multi["counts"][3] == len(amb)
    assert (multi["exact_reads"][gi.cap("barcode_build"):] > 0).any() and int(multi["exact_reads"].sum()) == int(multi["counts"][0])


# ---- umi_count_matrix and umi_velocity_matrix

def rounds_hold_a_waves_bucket(off, small):
    sizes = gi.non_empty_sizes(off)
    assert len(sizes) == gi.MATRIX_BUCKETS and gi.trips(len(sizes), T) == (2, 4, 44)
    for block in chunks(sizes, 256):  # every round of every block: several buckets for the queue, most for the lanes
        assert (block > small).sum() >= (2 if len(block) == 256 else 1) and (block <= small).sum() > (block > small).sum()
    d = np.diff(np.asarray(off).astype(np.int64))
    assert d[0] == 0 and d[-1] == 0 and (d == 0).sum() > 600  # empty buckets at both ends and in between


def test_count_matrix_input():
    kept, freq, off, row, col, n_rows, n_cols = gi.count_case()
    rounds_hold_a_waves_bucket(off, 32)
    r, c, m, rd = gi.count_expected()
    assert 1000 < len(r) < gi.MATRIX_BUCKETS  # pairs shared between buckets, many of them
    assert int(rd.sum()) == int(freq.astype(np.int64).sum())


def test_velocity_matrix_input():
    m = gi.velocity_case()
    rounds_hold_a_waves_bucket(m["off"], 32)
    n_reads = len(m["read_entry"])
    assert n_reads > 2 * gi.cap("velocity_scatter") + 65 and gi.two_trips_and_a_partial_wave(n_reads, gi.cap("velocity_scatter"))
    got = gi.velocity_expected()
    assert min(int(got[k].sum()) for k in (2, 3, 4)) > 500
    staged = m["read_entry"] != vm.UNSTAGED
    for trip in chunks(np.arange(n_reads), gi.cap("velocity_scatter")):  # evidence of both kinds, and reads without an entry
        c = m["read_class"][trip][staged[trip]]
        assert (c == vm.JUNCTION).any() and np.isin(c, (vm.SPANNING, vm.INTRONIC)).any() and not staged[trip].all()


# ---- umi_filter_multigene

@pytest.mark.parametrize("L", gi.MG_LENGTHS)
def test_multigene_input(L):
    case = gi.multigene_case(L)
    n = len(case.freq)
    assert n == gi.MG_ENTRIES and gi.trips(n, gi.cap("mg_entry")) == (2, 3, 8)
    assert case.nw == {12: 1, 22: 2}[L]
    kept_out, freq_out, counts = case.expected()
    assert counts["runs"] > 100 and counts["removed"] > 100
    molecule = case.kept != 0
    for trip in chunks(np.arange(n), gi.cap("mg_entry")):  # in every trip: molecules removed, molecules that survive, others
        assert (molecule[trip] & (kept_out[trip] == 0)).any() and kept_out[trip].any() and not molecule[trip].all()
        assert (freq_out[trip] != case.freq[trip]).any()


# ---- umi_call_cells

def test_call_cells_inputs():
    cases = gi.cells_cases()
    for name, case in cases.items():
        assert case.n_cols == gi.CELLS_COLS and gi.trips(case.n_cols, gi.cap("cells_call")) == (2, 1, 36)
        rules = gi.cells_rules(name)
        assert len(rules) >= 9
        called, everywhere = set(), 0
        for k in range(len(rules)):
            per, trip, counts = gi.cells_expected(name, k)
            called.add(counts["called"])
            everywhere += all(0 < int(c.sum()) < len(c) for c in chunks(per["called"], gi.cap("cells_call")))
        assert len(called) >= 4 and everywhere >= 3  # rules that draw different lines; cells and others in every trip
    per = gi.cells_expected("one_each", 0)[0]
    assert (np.bincount(cases["one_each"].col, minlength=gi.CELLS_COLS) == 1).all()
    per = gi.cells_expected("runs", 0)[0]
    empty = per["cell_genes"] == 0
    assert all(e.any() for e in chunks(np.bincount(cases["runs"].col, minlength=gi.CELLS_COLS) == 0, 256))  # empty columns everywhere
    assert empty.sum() > 1000 and np.bincount(cases["runs"].col).max() == 5


# ---- umi_assign_genes, _introns, _classes

def test_gene_inputs():
    assert len(gi.gene_reads()) == len(gi.class_reads()) == gi.GENE_READS
    assert gi.trips(gi.GENE_READS, gi.cap("gene_assign")) == (2, 1, 36)
    assert am.n_genes_of(am.fuzz_annotation()) == gi.N_GENES and am.n_genes_of(vm.fuzz_annotation()) <= gi.N_GENES_CLASSES
    for trip in chunks(np.arange(gi.GENE_READS), gi.cap("gene_assign")):
        if len(trip) < 500:
            continue
        st = gi.genes_expected(am.FORWARD)["status"][trip]
        assert set(st.tolist()) == {am.ASSIGNED, am.NONE, am.SEVERAL}
        for introns in (im.EXON_FIRST, im.ALL):
            e = gi.introns_expected(am.FORWARD, introns)
            assert set(e["tier"][trip].tolist()) == {0, im.TIER_EXON, im.TIER_INTRON}
            c = gi.classes_expected(am.FORWARD, introns)
            assert set(c["cls"][trip].tolist()) == {0, 1, 2, 3, 4}
    # the last, partial trip still holds a read with a gene under every call
    tail = slice(2 * gi.cap("gene_assign"), None)
    assert (gi.genes_expected(am.FORWARD)["gene"][tail] >= 0).any()
    assert (gi.introns_expected(am.FORWARD, im.ALL)["tier"][tail] == im.TIER_INTRON).any()
    assert (gi.classes_expected(am.FORWARD, im.EXON_FIRST)["cls"][tail] > 0).any()


# ---- umi_dedup_stats

@pytest.mark.parametrize("L", gi.STATS_LENGTHS)
def test_stats_case_a(L):
    keys, freq, kept, root, off, L = gi.stats_case_a(L)
    sizes = gi.non_empty_sizes(off)
    assert len(sizes) == gi.STATS_BUCKETS and gi.trips(len(sizes), gi.cap("stats_wave")) == (2, 4, 44)
    assert len(freq) > 2 * T and gi.two_trips_and_a_partial_wave(len(freq), gi.cap("stats_entry"))
    assert sizes.max() <= 70 < 4096  # nothing is a deep bucket at the default split
    wave = sizes > 8
    assert set(sizes[~wave].tolist()) == {1, 2, 3} and sizes[wave].min() >= 9 and 80 < wave.sum() < 120
    for trip in chunks(wave, gi.cap("stats_wave")):  # a round of the grid: eight blocks of 256 buckets (fewer in the last)
        blocks = [int(b.sum()) for b in chunks(trip, 256)]
        assert sum(blocks) >= 4 and max(blocks) >= 2 and (min(blocks) == 0 or len(trip) < gi.cap("stats_wave"))
    assert [int(b.sum()) for b in chunks(wave, 256)][-2:] == [6, 1]  # ... and both blocks of the last round queue
    d = np.diff(off.astype(np.int64))
    assert (d == 0).sum() > 800 and d[0] == 0 and d[-1] == 0
    # kept[] / root[] are a forest inside the buckets: roots kept, in their own bucket; some entries removed in every trip
    assert (kept[root] != 0).all() and (np.searchsorted(off, root, side="right") == np.searchsorted(off, np.arange(len(root)), side="right")).all()
    assert all((k == 0).any() and (k != 0).any() for k in chunks(kept, gi.cap("stats_post")))
    exp = gi.stats_expected("a", L)
    assert exp["dist"].sum(axis=1).tolist() == [gi.STATS_BUCKETS] * 4 and len(exp["umi_entry"]) > 1000


def test_stats_case_b():
    keys, freq, kept, root, off, L = gi.stats_case_b()
    sizes = gi.non_empty_sizes(off)
    deep = sizes[sizes >= gi.STATS_B_SPLIT]
    assert len(deep) == 64 and deep.max() == gi.STATS_B_DEEP == 3 * 1024 + 5 and sorted(deep)[-2] <= 200
    pieces = int((-(-deep // 1024)).sum())
    assert pieces == 67 and gi.trips(pieces * 64, gi.cap("stats_deep") * 64)[:2] == (2, 3)  # a wave a piece: three trips
    assert ((sizes > 8) & (sizes < gi.STATS_B_SPLIT)).sum() >= 60 and (sizes <= 8).sum() >= 60
    assert gi.stats_expected("b")["dist"].sum(axis=1).tolist() == [len(sizes)] * 4


# ---- umi_consensus_seqs

@pytest.mark.parametrize("n_entries", gi.CONS_ENTRIES)
def test_consensus_entry_counts(n_entries):
    seqs, quals, staged, kept, root = gi.cons_entries_case(n_entries)
    assert len(kept) == n_entries == len(staged["freq"]) and int(staged["freq"].sum()) == len(seqs)
    lanes = -(-n_entries // gi.CONS_GW)
    if n_entries == 700:  # one tile: lanes 0..21 of a wave hold entries, the last of them in some waves only
        assert lanes == 22 and n_entries % gi.CONS_GW != 0
    else:  # three trips of the tile loop, the last of them two lanes deep in some waves, three in the others
        assert gi.trips(n_entries, gi.cap("cons_vote")) == (2, 1, 6)
    assert (kept[root] != 0).all() and 0.2 < kept.mean() < 0.6
    # every wave of a tile has several kept entries in its lanes and gaps between them: the loop over its set bits
    # turns several times; the few lanes of the last tile hold kept entries too, beyond lane 0
    el = np.arange(n_entries)
    tile, lane, gw = el // gi.cap("cons_vote"), (el // gi.CONS_GW) % 64, el % gi.CONS_GW
    for t in range(tile.max() + 1):
        for w in range(gi.CONS_GW):
            mine = kept[(tile == t) & (gw == w)]
            assert len(mine) < 20 or (mine.sum() >= 3 and not mine.all())
        assert kept[(tile == t) & (lane > 0)].any()
    want = gi.cons_expected(n_entries)
    assert len(want) == int(kept.sum()) and max(m for *_, m in want) >= 4
    assert sum(1 for r, s, q, m in want if m > 1 and s != seqs[0]) > 100


def test_consensus_deep_clusters():
    seqs, quals, staged, kept, root = gi.cons_deep_case()
    want = gi.cons_expected("deep")
    sizes = np.array([m for *_, m in want])
    deep = sizes[sizes >= gi.CONS_SPLIT]
    assert len(deep) == gi.CONS_DEEP_CLUSTERS >= 70 and gi.trips(len(deep) * 64, gi.CONS_GW * 64)[:2] == (2, 11)
    assert len(deep) > 64  # the deep kernel's lanes look at a second batch of 64
    assert deep.max() == gi.CONS_DEEP_READS and -(-int(deep.max()) // gi.CONS_CHUNK) == 2 * gi.CONS_GW + 2  # three rounds of chunks
    assert sorted(deep)[-2] < gi.CONS_CHUNK and (sizes < gi.CONS_SPLIT).sum() == 150
    assert len(seqs) // gi.CONS_SPLIT + 1 >= len(deep)  # (the call's deep_cap)
    # the deepest cluster's vote at one base is close: A over C by a margin that any read left out would move
    r, s, q, m = max(want, key=lambda w: w[3])
    at = gi.CONS_CLOSE_BASE
    votes = [(seqs[i][at], quals[i][at]) for i, e in enumerate(staged["entry_of_read"]) if root[e] == r]
    assert sorted({b for b, _ in votes}) == [ord("A"), ord("C")] and len(votes) == gi.CONS_DEEP_READS
    margin = sum((x - 33) * (1 if b == ord("A") else -1) for b, x in votes)
    assert margin == gi.CONS_CLOSE_MARGIN and (s[at], q[at]) == (ord("A"), 33 + margin)
    assert min(x for _, x in votes) - 33 > 2 * margin  # (no single read's weight is as small as the margin)


# ---- umi_consensus_bam

@pytest.mark.parametrize("n_clusters", gi.CONSB_CLUSTERS)
def test_consensus_bam_cluster_counts(n_clusters):
    case = gi.consb_clusters_case(n_clusters)
    assert len(case.clen) == n_clusters
    if n_clusters == 300:
        assert -(-n_clusters // gi.CONSB_GW) == 38  # lanes 0..37 of a wave hold clusters
    else:
        assert gi.trips(n_clusters, gi.cap("consb_vote")) == (2, 1, 12)
    want = gi.consb_expected(n_clusters)
    depth = np.array([d for *_, d, e in want])
    assert (depth == 0).sum() >= n_clusters // 100 and depth.max() == 3 and sum(1 for *_, e in want if e > 0) > n_clusters // 10
    assert (case.cluster == 0xFFFFFFFF).sum() > n_clusters // 10


def test_consensus_bam_deep_clusters():
    case = gi.consb_deep_case()
    depth = np.bincount(case.cluster[case.cluster != 0xFFFFFFFF], minlength=len(case.clen))
    deep = depth[depth >= gi.CONS_SPLIT]
    assert len(deep) == gi.CONSB_DEEP_CLUSTERS >= 20 and gi.trips(len(deep) * 64, gi.CONSB_GW * 64)[:2] == (2, 4)
    assert deep.max() == gi.CONSB_DEEP_VOTERS and -(-int(deep.max()) // gi.CONSB_CHUNK) == 2 * gi.CONSB_GW + 2
    assert sorted(deep)[-2] < gi.CONSB_CHUNK and (depth < gi.CONS_SPLIT).sum() == 100
    assert len(case.lens) // gi.CONS_SPLIT + 1 >= len(deep)
    want = gi.consb_expected("deep")
    assert max(d for *_, d, e in want) == gi.CONSB_DEEP_VOTERS
