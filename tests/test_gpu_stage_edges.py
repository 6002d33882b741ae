"""Read staging on the device at the edges of its own structure (the inputs of tests/stage_edge_inputs.py,
proven on the CPU in tests/test_stage_edge_inputs_cpu.py): read counts, entry runs and positions on and beside
the wave, round, tile and rank-block sizes; the limits of the no-sort order; order keys of 32 and 33 bits
without the environment switch; composed keys of 64 and 65 bits; garbage above the counted key bits; every
letter at every base; every bad byte; UMIs of several key words through the byte-wise encode; the extent of
what the device forms write; whole reads.  Every comparison is bit for bit against the project's references
(stage_edge_inputs.reference: the keys masked on the host; the library gets them as they are)."""
import numpy as np
import pytest

import seq_model as sm
import stage_edge_inputs as si

pytestmark = pytest.mark.gpu

FIELDS = ("bucket_off", "keys", "nmask", "freq", "rep")


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def call(ctx, inp):
    abits, gbits = si.key_bits(inp)
    if inp.group is not None:
        f = ctx.stage_reads_grouped_wide if inp.L > 21 else ctx.stage_reads_grouped
        return f(inp.align, inp.group, inp.umi, inp.score, inp.L, merge=inp.merge, align_key_bits=abits,
                 group_key_bits=gbits)
    f = ctx.stage_reads_wide if inp.L > 21 else ctx.stage_reads
    return f(inp.align, inp.umi, inp.score, inp.L, merge=inp.merge, align_key_bits=abits)


def same(got, want, what):
    for f in FIELDS:
        a, b = np.asarray(got[f]), np.asarray(want[f])
        assert a.shape == b.shape, (what, f, a.shape, b.shape)
        bad = np.nonzero((a.astype(np.uint64) != b.astype(np.uint64)).reshape(len(a), -1).any(1))[0]
        assert len(bad) == 0, (what, f, len(bad), bad[:5].tolist(), a[bad[:3]].tolist(), b[bad[:3]].tolist())


def check(ctx, inp, what, merges=True):
    for v in (si.merge_variants(inp) if merges else (inp,)):
        same(call(ctx, v), si.reference(v), (what, "bits", inp.bits, "merge", v.merge, "scores", v.score is not None))


def check_layout(ctx, layout, what, **kw):
    """a layout in its three file orders, on a composed key (as few key bits as number the positions) and on
    whole 64-bit keys (a sort per word), with merge 0, merge 1 and merge 1 without scores"""
    for order in si.ORDERS:
        for bits in ("small", 64):
            check(ctx, si.from_layout(layout, order, bits, **kw), (what, order))


# ---- read counts ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("n", si.COUNTS)
def test_read_counts(ctx, n):
    for ending in si.ENDINGS:
        for deep in (False, True):
            layout = si.counts_layout(n, ending, deep)
            if layout is not None and not (deep and layout == si.counts_layout(n, ending)):
                check_layout(ctx, layout, (n, ending, "deep" if deep else "flat"))


# ---- entry runs over wave, round and tile boundaries ------------------------------------------------------

@pytest.mark.parametrize("b", si.BOUNDARIES)
def test_entry_runs_beside_the_boundaries(ctx, b):
    m = min(100, b // 2)
    for delta in (-1, 0, 1):
        layout = si.boundary_layout(b, delta)
        check_layout(ctx, layout, (b, delta))
        at = b + delta
        for order in si.ORDERS:
            for bits in ("small", 64):
                for score in ("equal", "extremes"):
                    check(ctx, si.from_layout(layout, order, bits, score=score), (b, delta, order, score), merges=False)
                inp = si.from_layout(layout, order, bits)
                view = si.sorted_view(inp)
                for i, (base, best) in enumerate(si.SCORE_PAIRS):  # the best score at the runs' first, then last reads
                    where = (at - m, at) if i % 2 == 0 else (at - 1, at + m - 1)
                    check(ctx, si.with_best_at(inp, where, base, best, view), (b, delta, order, where, base, best), merges=False)


@pytest.mark.parametrize("order", si.ORDERS)
def test_a_run_over_three_tiles_and_its_best_scores(ctx, order):
    for bits in ("small", 64):
        inp = si.from_layout(si.LONG_RUN, order, bits)
        check(ctx, inp, ("long run", order))
        for score in ("equal", "extremes"):
            check(ctx, si.from_layout(si.LONG_RUN, order, bits, score=score), ("long run", order, score), merges=False)
        view = si.sorted_view(inp)
        for name, at in si.LONG_RUN_BEST.items():
            for base, best in si.SCORE_PAIRS:
                v = si.with_best_at(inp, at, base, best, view)
                got = call(ctx, v)
                same(got, si.reference(v), ("long run", order, bits, name, base, best))
                assert got["rep"][got["freq"] == 5000][0] == view.perm[min(at)]  # the earliest of the equal best
        for score in ("random", "equal"):
            check(ctx, si.from_layout(si.TILE_RUN, order, bits, score=score), ("tile run", order, score))


# ---- positions over tiles -----------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(si.POSITION_LAYOUTS))
def test_positions_over_tiles(ctx, name):
    check_layout(ctx, si.POSITION_LAYOUTS[name], name)


# ---- the limits of the no-sort order --------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(si.LOCAL_LAYOUTS))
def test_no_sort_limits(ctx, name):
    check_layout(ctx, si.LOCAL_LAYOUTS[name], name)


@pytest.mark.parametrize("name", list(si.FREQ_PATTERNS))
def test_freq_patterns_in_a_position_of_1024_entries(ctx, name):
    for bits in ("small", 64):
        check(ctx, si.from_first_appearance(si.FREQ_PATTERNS[name], bits), (name, bits))


# ---- order-key widths (no environment switch: the rule itself picks the kernel) ---------------------------------

@pytest.mark.parametrize("order", si.ORDERS)
@pytest.mark.parametrize("name", list(si.WIDTH_CASES))
def test_order_key_widths(ctx, name, order):
    kind, fmax, positions = si.WIDTH_CASES[name]
    layout = si.width_layout(kind, fmax, positions)
    for bits in ("small", 64):
        check(ctx, si.from_layout(layout, order, bits), (name, order))


# ---- key composition ------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", si.COMPOSE_LENGTHS)
def test_key_composition(ctx, L):
    for bits in si.compose_bits(L):
        check(ctx, si.composition(L, bits), ("composition", L, bits))
    for bits in si.grouped_bits(L):
        check(ctx, si.composition(L, bits), ("grouped composition", L, bits))


@pytest.mark.parametrize("bits", [(40, 24), (40, 25)])
def test_grouped_wide_key_composition(ctx, bits):
    check(ctx, si.composition(24, bits), ("grouped wide", bits))


# ---- alphabet and packing -------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", range(1, 22))
def test_alphabet_and_packing(ctx, L):
    import oracle as orc
    u = si.alphabet_umis(L)
    keys, nm = orc.encode_keys([bytes(r).decode() for r in u])  # every UMI of the set, in both positions
    for bits in (1, 64):  # the composed key (pack5 / unpack5) and a sort per word
        for v in si.merge_variants(si.alphabet(L, bits)):
            what = ("alphabet", L, bits, "merge", v.merge, "scores", v.score is not None)
            got = call(ctx, v)
            same(got, si.reference(v), what)
            for b in (0, 1):
                s, e = int(got["bucket_off"][b]), int(got["bucket_off"][b + 1])
                assert sorted(zip(got["keys"][s:e].tolist(), got["nmask"][s:e].tolist())) == \
                    sorted(zip(keys.tolist(), nm.tolist())), what


# ---- bad bytes ------------------------------------------------------------------------------------------------

BAD_L, BAD_N = 12, 300  # a whole chunk of 256 reads and a partial one
BAD_PLACES = (0, 1, 2, 3, 299 * 12, 299 * 12 + 6, 300 * 12 - 1, 100 * 12 + 5, 255 * 12 + 11, 256 * 12, 17 * 12 + 2, 298 * 12 + 3)
BAD_BYTES = [v for v in range(256) if v not in b"ACGTN"]


def bad_byte_reads():
    rng = np.random.default_rng(11)
    umi = si.random_umis(rng, BAD_N, BAD_L, 0.05).reshape(-1)
    align = rng.integers(0, 20, BAD_N).astype(np.uint64)
    return si.StageInput(align, None, umi, rng.integers(0, 60, BAD_N).astype(np.int32), BAD_L, 5, 1)


def test_every_bad_byte_host_form(ctx):
    from umi_collapse_rs_amd import UmiHipError
    from umi_collapse_rs_amd._lib import UMI_ERR_CHAR
    assert len(BAD_BYTES) == 251
    inp = bad_byte_reads()
    for i, v in enumerate(BAD_BYTES):
        text = inp.umi.copy()
        text[BAD_PLACES[i % len(BAD_PLACES)]] = v
        with pytest.raises(UmiHipError) as e:
            call(ctx, inp._replace(umi=text))
        assert e.value.code == UMI_ERR_CHAR, (v, e.value)
    same(call(ctx, inp), si.reference(inp), "the good call after 251 refused ones")


def test_every_bad_byte_device_form_off_the_word_boundary(ctx):
    from umi_collapse_rs_amd import UmiHipError
    from umi_collapse_rs_amd._lib import UMI_ERR_CHAR
    inp = bad_byte_reads()
    dev = DeviceCall(inp, shift=1)
    good = dev.raw.cpu()
    for i, v in enumerate(BAD_BYTES):
        text = good.clone()
        text[1 + BAD_PLACES[i % len(BAD_PLACES)]] = v
        dev.raw.copy_(text)  # (one upload a call)
        with pytest.raises(UmiHipError) as e:
            dev.run(ctx)
        assert e.value.code == UMI_ERR_CHAR, (v, e.value)
    dev.raw.copy_(good)
    same(dev.run(ctx), si.reference(inp), "the good call after 251 refused ones")


# ---- the device forms: text off the word boundary, the extent of the writes -----------------------------------

GUARD = 64
SENT64, SENT32 = -0x5A5A5A5A5A5A5A5B, -0x5A5A5A5B


class DeviceCall:
    """One device-form call: inputs on the device, the UMI text `shift` bytes off a 4-byte boundary; outputs at
    their documented capacity (n_reads entries, n_reads + 1 offsets) plus GUARD elements of a sentinel, which
    run() finds intact."""

    def __init__(self, inp, shift=0, wide=None):
        import torch
        self.inp, self.shift = inp, shift
        self.wide = inp.L > 21 if wide is None else wide
        self.n, self.w = len(inp.align), (3 * inp.L + 63) // 64
        dev = torch.device("cuda", 0)
        up = lambda a, ty: torch.from_numpy(np.ascontiguousarray(a).view(ty).copy()).to(dev)
        self.align = up(inp.align, np.int64)
        self.group = up(inp.group, np.int64) if inp.group is not None else None
        self.score = up(inp.score, np.int32) if inp.score is not None else None
        self.raw = torch.zeros(len(inp.umi) + 8, dtype=torch.uint8, device=dev)
        self.raw[shift:shift + len(inp.umi)] = up(inp.umi, np.uint8)
        n, w = self.n, self.w
        self.cap = dict(keys=n * w, nmask=n * w, rep=n, freq=n, bucket_off=n + 1)
        self.out = {f: torch.full((c + GUARD,), SENT32 if f == "freq" else SENT64,
                                  dtype=torch.int32 if f == "freq" else torch.int64, device=dev)
                    for f, c in self.cap.items()}

    def run(self, ctx, nmask=True):
        import torch
        inp, o = self.inp, {f: t.data_ptr() for f, t in self.out.items()}
        abits, gbits = si.key_bits(inp)
        torch.cuda.synchronize()
        stream = torch.cuda.current_stream().cuda_stream
        umi = self.raw.data_ptr() + self.shift
        score = self.score.data_ptr() if self.score is not None else 0
        group = self.group.data_ptr() if self.group is not None else 0
        tail = (o["keys"], o["nmask"] if nmask else 0, o["freq"], o["rep"], o["bucket_off"])
        if self.wide:  # (0 group bits: the plain wide device call)
            ne, nb = ctx.stage_reads_grouped_wide_device(self.align.data_ptr(), group, umi, score, self.n, inp.L, *tail,
                                                         merge=inp.merge, align_key_bits=abits, group_key_bits=gbits, stream=stream)
        elif inp.group is not None:
            ne, nb = ctx.stage_reads_grouped_device(self.align.data_ptr(), group, umi, score, self.n, inp.L, *tail,
                                                    merge=inp.merge, align_key_bits=abits, group_key_bits=gbits, stream=stream)
        else:
            ne, nb = ctx.stage_reads_device(self.align.data_ptr(), umi, score, self.n, inp.L, *tail, merge=inp.merge,
                                            align_key_bits=abits, stream=stream)
        torch.cuda.synchronize()
        host = {f: t.cpu().numpy() for f, t in self.out.items()}
        for f, c in self.cap.items():
            assert (host[f][c:] == (SENT32 if f == "freq" else SENT64)).all(), ("written behind the capacity", f)
        if not nmask:
            assert (host["nmask"] == SENT64).all()
        assert ne <= self.n and nb <= ne and int(host["bucket_off"][nb]) == ne
        w = self.w
        shape = (ne, w) if self.wide else (ne,)
        return dict(keys=host["keys"][:ne * w].view(np.uint64).reshape(shape),
                    nmask=host["nmask"][:ne * w].view(np.uint64).reshape(shape), freq=host["freq"][:ne],
                    rep=host["rep"][:ne].view(np.uint64), bucket_off=host["bucket_off"][:nb + 1].view(np.uint64))


@pytest.mark.parametrize("L", si.WIDE_LENGTHS)
def test_wide_umis_through_the_byte_wise_encode(ctx, L):
    for n in si.WIDE_COUNTS:
        for abits in (20, 64):  # a small alignment key and a whole word
            for v in si.merge_variants(si.wide(L, n, (abits, 0))):
                want = si.reference(v)
                for shift in range(4):
                    same(DeviceCall(v, shift).run(ctx), want, ("wide", L, n, abits, shift, v.merge, v.score is not None))
    for bits in ((40, 24), (40, 25), (64, 64)):  # grouped: one position word, two
        for v in si.merge_variants(si.wide(L, 257, bits)):
            want = si.reference(v)
            same(DeviceCall(v, 3).run(ctx), want, ("grouped wide", L, bits, v.merge, v.score is not None))
            same(call(ctx, v), want, ("grouped wide, host form", L, bits, v.merge, v.score is not None))


def extent_inputs():
    yield "one read", si.from_layout([[1]], "sorted")
    yield "one wave", si.from_layout(si.counts_layout(64, "own_position"), "shuffled")
    yield "one tile", si.from_layout(si.counts_layout(2048, "new_entry"), "shuffled", 64)
    yield "a tile and a read", si.from_layout(si.counts_layout(2049, "same_entry"), "reversed")
    yield "all single reads: E = B = n", si.from_layout([[1]] * 4097, "shuffled")
    yield "one position of single reads: E = n", si.from_layout([[1] * 4097], "shuffled")
    yield "a wave per position", si.from_layout(si.LOCAL_LAYOUTS["e_is_16b"], "shuffled")
    yield "1,024 entries in LDS", si.from_layout(si.LOCAL_LAYOUTS["largest_1024"], "shuffled", 64)
    yield "grouped, one word", si.composition(12, (40, 24))
    yield "grouped, two words", si.composition(12, (40, 25))
    yield "one-word UMIs through the wide call", si.composition(21, 15)
    yield "wide", si.wide(43, 513)


def test_extent_of_the_device_forms_writes(ctx):
    for what, inp in extent_inputs():
        for v in si.merge_variants(inp):
            for shift in (0, 2):
                wide = True if what.startswith("one-word UMIs through") else None
                dev = DeviceCall(v, shift, wide)
                got = dev.run(ctx)
                if wide and inp.L <= 21:
                    got["keys"], got["nmask"] = got["keys"][:, 0], got["nmask"][:, 0]
                same(got, si.reference(v), (what, shift, v.merge))
        got = DeviceCall(inp, 1).run(ctx, nmask=False)  # nmask may be NULL: nothing written there
        want = si.reference(inp)
        assert np.array_equal(got["freq"], want["freq"]) and np.array_equal(got["rep"], want["rep"]), what


# ---- whole reads ------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", list(si.SEQ_RUNS))
def test_whole_reads_at_the_boundaries(ctx, name):
    for order in si.ORDERS:
        seqs, quals = si.seq_reads(si.SEQ_RUNS[name], order)
        for merge in (0, 1):
            got = ctx.stage_seqs(seqs, quals, merge=merge)
            ent, off, blen = sm.stage(seqs, quals, merge)
            keys, nm = sm.encode([e[0] for e in ent], sm.words(len(seqs[0])))
            what = (name, order, merge)
            assert list(got["bucket_len"]) == blen and list(got["bucket_off"]) == off, what
            assert np.array_equal(got["freq"], np.array([e[1] for e in ent], np.int32)), what
            assert np.array_equal(got["rep"], np.array([e[2] for e in ent], np.uint64)), what
            assert np.array_equal(got["keys"], keys) and np.array_equal(got["nmask"], nm), what
            entry = {e[0]: j for j, e in enumerate(ent)}
            assert np.array_equal(got["entry_of_read"], np.array([entry[s] for s in seqs], np.uint32)), what
