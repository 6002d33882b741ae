"""The staging edge inputs of tests/stage_edge_inputs.py, checked on the CPU before a kernel sees them: with
the oracle / the models alone, each named input has the property it is named for (a run starts at b - 1, b,
b + 1; the largest position has exactly 1,024 entries; E = 16 B - 1; fmax = 32,768 beside an entry of freq 1;
two positions differ only in the highest counted bit; ...), and the plain-Python statement of the two host
rules sends it down the path it is meant for."""
import numpy as np
import pytest

import seq_model as sm
import stage_edge_inputs as si


def plan(inp, ref=None):
    return si.order_plan_of(inp, ref or si.reference(inp))


def test_the_rules_at_their_thresholds():
    assert [si.pack5_bits(L) for L in (1, 2, 3, 12, 20, 21)] == [3, 5, 7, 28, 47, 49]
    assert si.sort_plan(1, 12, 36, 0)["one_key"] and not si.sort_plan(1, 12, 37, 0)["one_key"]
    assert si.sort_plan(1, 12, 36, 0)["composed_bits"] == 64
    assert si.sort_plan(1, 12, 20, 16)["one_key"] and not si.sort_plan(1, 12, 20, 17)["one_key"]
    assert si.sort_plan(1, 12, 20, 44)["combine"] and si.sort_plan(1, 12, 20, 45)["second_word"]
    assert not si.sort_plan(2, 24, 1, 0)["one_key"]
    n = 1 << 17  # 2^17 reads and one UMI read 32,768 times: the wide order key, far below 2^24 reads
    assert not si.order_plan(n, 99000, 97, 32767, 1024)["wide"] and si.order_plan(n, 99000, 97, 32768, 1024)["wide"]
    assert si.order_plan(n, 99000, 97, 3, 1024, force_wide=True)["wide"]
    assert si.order_plan(n, 16 * 97, 97, 3, 1024)["local"] and not si.order_plan(n, 16 * 97 - 1, 97, 3, 1024)["local"]
    assert not si.order_plan(n, 99000, 97, 3, 1025)["local"]
    assert len(si.plan_table()) > 1000


@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("n", si.COUNTS)
def test_read_counts_and_their_last_read(n, order):
    for ending in si.ENDINGS:
        for deep in (False, True):
            layout = si.counts_layout(n, ending, deep)
            if layout is None:
                assert n == 1 and ending != "own_position"
                continue
            inp = si.from_layout(layout, order)
            sv = si.sorted_view(inp)
            assert len(inp.align) == n == len(sv.perm)
            if ending == "own_position":
                assert sv.pos_start[-1] == n - 1
            elif ending == "new_entry":
                assert sv.entry_start[-1] == n - 1 and sv.pos_start[-1] == n - 2
            else:
                assert sv.entry_start[-1] == n - 2 and sv.pos_start[-1] == n - 2
            if order == "shuffled" and n in (2049, 16384):
                p = plan(inp)
                assert p["local"] == deep and not p["wide"] and not p["key64"]


@pytest.mark.parametrize("b", si.BOUNDARIES)
def test_runs_begin_and_end_beside_the_boundaries(b):
    m = min(100, b // 2)
    for delta in (-1, 0, 1):
        for order in si.ORDERS:
            inp = si.from_layout(si.boundary_layout(b, delta), order)
            sv = si.sorted_view(inp)
            starts = sv.entry_start.tolist()
            at = starts.index(b + delta)
            assert starts[at - 1] == b + delta - m and starts[at + 1] == b + delta + m  # one run ends, one begins there
            ref = si.reference(inp)
            assert sorted(ref["freq"].tolist())[-2:] == [m, m] and not plan(inp, ref)["local"]


def test_the_long_run_and_where_its_best_scores_lie():
    for layout, start, length in ((si.LONG_RUN, 2040, 5000), (si.TILE_RUN, 2048, 2048)):
        for order in si.ORDERS:
            sv = si.sorted_view(si.from_layout(layout, order))
            starts = sv.entry_start.tolist()
            assert start in starts and starts[starts.index(start) + 1] == start + length
            if layout is si.LONG_RUN:  # the tile 4,096 .. 6,143 has no head at all
                assert not any(4096 <= s < 6144 for s in starts)
                assert not any(4096 <= s < 6144 for s in sv.pos_start.tolist())
            else:  # the run is exactly the second tile
                assert [s for s in starts if 2048 <= s < 4096] == [2048] and 4096 in starts
    best = si.LONG_RUN_BEST
    assert all(2040 <= x <= 7039 for v in best.values() for x in v)
    assert best["wave_last_lane"][0] % 64 == 63 and best["wave_first_lane"][0] % 64 == 0
    a, b = best["two_waves"]
    assert a // 64 != b // 64 and a // 2048 == b // 2048
    a, b = best["two_tiles"]
    assert a // 2048 != b // 2048
    assert best["tile_edge"] == (4095, 4096)
    inp = si.from_layout(si.LONG_RUN, "shuffled")
    sv = si.sorted_view(inp)
    for name, at in best.items():  # the earliest of the equal best reads stands for the run
        for base, top in si.SCORE_PAIRS:
            ref = si.reference(si.with_best_at(inp, at, base, top))
            assert ref["rep"][ref["freq"] == 5000][0] == sv.perm[min(at)], name
    assert set(si.from_layout(si.LONG_RUN, "sorted", score="extremes").score.tolist()) == set(si.EXTREMES)


def test_positions_over_tiles():
    for name, layout in si.POSITION_LAYOUTS.items():
        for order in si.ORDERS:
            inp = si.from_layout(layout, order)
            sv, ref = si.sorted_view(inp), si.reference(inp)
            p = plan(inp, ref)
            if name == "three_tiles_of_single_reads":
                assert sv.pos_start.tolist() == list(range(6144)) and not p["local"]
            elif name == "one_position_over_three_tiles":
                assert sv.pos_start.tolist() == [0] and len(sv.entry_start) == 5000 and not p["local"]
                if order == "reversed":  # the position's first read in the file is its last in sorted order
                    assert int(np.argmin(sv.perm)) >= 4096
            else:
                assert len(sv.pos_start) == 300 and len(sv.entry_start) == 5100 and p["local"]
                assert min(np.bincount(sv.pos_start // 256)[:-1]) >= 15  # many position heads in every round


def test_the_limits_of_the_no_sort_order():
    want = dict(largest_1023=(1023, True), largest_1024=(1024, True), largest_1025=(1025, False),
                e_is_16b=(16, True), e_is_16b_less_1=(16, False), lds_sizes=(1024, True))
    for name, layout in si.LOCAL_LAYOUTS.items():
        inp = si.from_layout(layout, "shuffled")
        ref = si.reference(inp)
        sizes = np.diff(ref["bucket_off"].astype(np.int64))
        E, B = len(ref["freq"]), len(sizes)
        assert (int(sizes.max()), plan(inp, ref)["local"]) == want[name], name
        assert sorted(sizes.tolist()) == sorted(len(p) for p in layout)
        if name.startswith("largest"):
            assert sizes.min() >= 16 and E >= 16 * B
        if name == "e_is_16b":
            assert E == 16 * B
        if name == "e_is_16b_less_1":
            assert E == 16 * B - 1
        if name == "lds_sizes":
            assert set(si.SIZES_IN_LDS) <= set(sizes.tolist()) and E >= 16 * B
        assert len(set(ref["freq"].tolist())) == 4  # freq differs inside the positions


@pytest.mark.parametrize("name", list(si.FREQ_PATTERNS))
def test_freq_patterns_by_first_appearance(name):
    freqs = si.FREQ_PATTERNS[name]
    inp = si.from_first_appearance(freqs)
    ref = si.reference(inp._replace(merge=0))
    assert ref["bucket_off"].tolist() == [0, 1024]
    by_first = np.argsort(ref["rep"])  # merge 0: rep is the first read
    assert ref["freq"][by_first].tolist() == freqs and ref["rep"][by_first].tolist() == list(range(1024))
    p = plan(inp, ref)
    assert p["local"] and not p["wide"]


@pytest.mark.parametrize("name", list(si.WIDTH_CASES))
def test_order_key_widths(name):
    kind, fmax, positions = si.WIDTH_CASES[name]
    inp = si.from_layout(si.width_layout(kind, fmax, positions), "shuffled")
    assert len(inp.align) <= 165000
    ref = si.reference(inp)
    p = plan(inp, ref)
    assert ref["freq"].max() == fmax and ref["freq"].min() == 1  # fmax - freq takes its largest value
    if kind == "local":
        assert len(inp.align) == 1 << 17 and p["local"] and np.diff(ref["bucket_off"].astype(np.int64)).max() == 1024
        assert p["wide"] == (fmax >= 32768)
        assert 17 + p["freq_bits"] == (32 if fmax == 32767 else 33)
        if fmax == 32767:  # all 32 bits of the narrow key in use
            assert ((fmax - 1) << p["first_bits"] | (len(inp.align) - 1)).bit_length() == 32
        if fmax == 32769:  # ... and here the freq field itself would not fit beside 17 bits of read index
            assert (fmax - 1).bit_length() == 16
    else:
        B = len(ref["bucket_off"]) - 1
        assert B == positions and not p["local"]
        assert p["order_bits"] == dict(sort_32767=32, sort_32768=33, sort_65535=32, sort_65535_one_more=33)[name]
        assert p["key64"] == (p["order_bits"] == 33)
        if p["key64"]:  # positions on both sides of rank 2^16
            assert B > 1 << 16


@pytest.mark.parametrize("L", si.COMPOSE_LENGTHS)
def test_key_composition_inputs(L):
    p5 = si.pack5_bits(L)
    for bits, one_key in zip(si.compose_bits(L), (True, True, False, False)):
        sp = si.sort_plan(1, L, bits, 0)
        assert sp["one_key"] == one_key and sp["composed_bits"] == bits + p5
        _check_composition(si.composition(L, bits), bits, 0)
    plans = [si.sort_plan(1, L, a, g) for a, g in si.grouped_bits(L)]
    assert [(p["combine"], p["one_key"]) for p in plans[:4]] == [(True, True), (True, False), (True, False), (False, False)]
    assert plans[0]["composed_bits"] == 64 and plans[2]["align_bits"] == 64 and plans[3]["second_word"]
    assert plans[4]["second_word"] and plans[5]["combine"] and plans[6]["second_word"]
    for a, g in si.grouped_bits(L):
        _check_composition(si.composition(L, (a, g)), a, g)


def _check_composition(inp, abits, gbits):
    for key, bits in ((inp.align, abits), (inp.group, gbits)):
        if not bits:
            assert key is None
            continue
        vals = set(si.masked(key, bits).tolist())
        top = 1 << (bits - 1)
        assert any(v ^ top in vals for v in vals)  # a pair that differs only in the highest counted bit
        assert any(v ^ 1 in vals for v in vals)    # ... only in bit 0
        if bits < 64:  # one position, different garbage above the counted bits -- in every such bit
            m = si.masked(key, bits)
            same = key[m == m[0]]
            assert len(set(same.tolist())) > 1
            assert np.bitwise_or.reduce(key) >> np.uint64(bits) == (1 << (64 - bits)) - 1
            assert np.bitwise_and.reduce(key) >> np.uint64(bits) == 0
    ref = si.reference(inp)
    assert ref["freq"].max() > 1 and len(ref["bucket_off"]) - 1 >= 4


@pytest.mark.parametrize("L", range(1, 22))
def test_alphabet_inputs(L):
    u = si.alphabet_umis(L)
    assert len(np.unique(u, axis=0)) == len(u)
    for b in range(L):
        assert set(u[:, b].tolist()) == set(b"ACGTN")
    m = min(L, 3)
    for at in (0, L - m):
        assert len(np.unique(u[:, at:at + m], axis=0)) == 5 ** m
    for bits in (1, 64):
        inp = si.alphabet(L, bits)
        ref = si.reference(inp)
        assert ref["bucket_off"].tolist() == [0, len(u), 2 * len(u)] and set(ref["freq"].tolist()) == {1, 2, 3}
        assert si.sort_plan(1, L, bits, 0)["one_key"] == (bits == 1)


@pytest.mark.parametrize("L", si.WIDE_LENGTHS)
def test_wide_inputs(L):
    inp = si.wide(L, 513)
    u = inp.umi.reshape(-1, L)
    for b in si.WIDE_BASES:
        if b < L:
            assert set(u[:, b].tolist()) == set(b"ACGTN"), b
    assert max(b for b in si.WIDE_BASES if b < L) >= 20
    ref = si.reference(inp)
    assert ref["keys"].shape[1] == (3 * L + 63) // 64 == ref["nmask"].shape[1]
    assert all(ref["nmask"][:, w].any() for w in range(ref["keys"].shape[1]) if any(64 * w <= 3 * b < 64 * (w + 1) for b in si.WIDE_BASES if b < L))
    whole = si.wide(L, 257, (64, 0))  # a whole-word alignment key, its highest bit in use
    assert whole.bits == 64 and whole.group is None and int(whole.align.max()) >> 63 == 1
    assert len(si.reference(whole)["bucket_off"]) - 1 == 3
    g = si.wide(L, 257, bits=(40, 25))
    assert si.sort_plan((3 * L + 63) // 64, L, 40, 25)["second_word"] and len(si.reference(g)["bucket_off"]) - 1 == 6


def test_whole_read_runs():
    keys, _ = sm.encode(si.SEQS_IN_ORDER, sm.words(len(si.SEQS_IN_ORDER[0])))
    as_int = [sum(int(w) << (64 * i) for i, w in enumerate(k)) for k in keys]
    assert as_int == sorted(as_int) and len(set(as_int)) == 4  # the order the runs are laid out in
    cuts = set()
    for name, runs in si.SEQ_RUNS.items():
        cuts |= set(np.cumsum(runs).tolist())
        for order in si.ORDERS:
            seqs, quals = si.seq_reads(runs, order)
            assert len(seqs) == sum(runs) == len(quals)
            assert [seqs.count(s) for s in si.SEQS_IN_ORDER[:len(runs)]] == list(runs)
    assert {63, 64, 65, 2047, 2048, 2049} <= cuts
    assert {sum(si.SEQ_RUNS[k]) for k in ("n2047", "n2048", "n2049")} == {2047, 2048, 2049}
