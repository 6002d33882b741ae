"""umi_filter_multigene / umi_filter_multigene_device on the GPU against tests/multigene_model.py: kept_out, freq_out
and the three counts by exact equality, on both call forms.  The shapes walk csrc/umihip_multigene.hip: entry counts
on and beside a wave's 64, a block's 256, the scan's tile of 2,048 and the radix sort's round and tile of 256 and
4,096 entries (csrc/umihip_radix.hip); runs that begin and end on those edges; one run that holds everything; keys
of one to four words, composed into one sort key or sorted word by word; totals beyond 32 bits."""
import ctypes as C

import numpy as np
import pytest

import multigene_model as mm
import stats_model as sm

pytestmark = pytest.mark.gpu
WAVE, BLOCK, SCAN_TILE, SORT_ROUND, SORT_TILE = 64, 256, 2048, 256, 4096
GUARD = 67  # bytes (kept_out) and elements (freq_out) on both sides of the outputs


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


class Case:
    def __init__(self, keys, freq, kept, root, off, group, n_groups, L):
        self.keys = np.ascontiguousarray(keys, np.uint64).reshape(-1)
        self.freq = np.ascontiguousarray(freq, np.int32)
        self.kept = np.ascontiguousarray(kept, np.uint8)
        self.root = np.ascontiguousarray(root, np.uint32)
        self.off = np.ascontiguousarray(off, np.uint64)
        self.group = np.ascontiguousarray(group, np.uint32)
        self.n_groups, self.L, self.nw = int(n_groups), L, sm.n_words_of(L)
        self._exp = None

    def expected(self):  # (computed once)
        if self._exp is None:
            self._exp = mm.filter_model(self.keys, self.freq, self.kept, self.root, self.off, self.group, self.L)
        return self._exp


def host_call(c, case, want_freq=True):
    return c.filter_multigene(case.keys, case.freq, case.kept, case.root, case.off, case.group, case.n_groups, case.L,
                              n_words=case.nw, want_freq=want_freq)


def device_call(c, case, want_freq=True, stream=None):
    """the _device form on tensors of its own: kept[] and kept_out one byte off alignment, guards around both outputs"""
    import torch
    n = len(case.freq)
    t_kept = torch.zeros(n + 1, dtype=torch.uint8, device="cuda:0")
    t_kept[1:] = dev(case.kept)
    t_keys, t_freq, t_root = dev(case.keys.view(np.int64)), dev(case.freq), dev(case.root.view(np.int32))
    t_group = dev(case.group.view(np.int32))
    k_out = torch.full((n + 2 * GUARD,), 0x5A, dtype=torch.uint8, device="cuda:0")
    f_out = torch.full((n + 2 * GUARD,), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    counts = c.filter_multigene_device(t_keys.data_ptr(), t_freq.data_ptr(), t_kept.data_ptr() + 1, t_root.data_ptr(), case.off,
                                       t_group.data_ptr(), case.n_groups, case.L, k_out.data_ptr() + GUARD,
                                       d_freq_out=f_out.data_ptr() + 4 * GUARD if want_freq else 0, n_words=case.nw,
                                       stream=stream.cuda_stream if stream is not None else 0)
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    k, f = k_out.cpu().numpy(), f_out.cpu().numpy()
    assert (k[:GUARD] == 0x5A).all() and (k[GUARD + n:] == 0x5A).all(), "kept_out written outside [0, N)"
    assert (f[:GUARD] == 0x5A5A5A5A).all() and (f[GUARD + n:] == 0x5A5A5A5A).all(), "freq_out written outside [0, N)"
    if not want_freq:
        assert (f == 0x5A5A5A5A).all()
    return k[GUARD:GUARD + n], (f[GUARD:GUARD + n] if want_freq else None), counts


def same(got, exp, want_freq=True):
    (gk, gf, gc), (ek, ef, ec) = got, exp
    assert gc == ec, (gc, ec)
    assert gk.dtype == np.uint8 and gk.shape == ek.shape
    bad = np.flatnonzero(gk != ek)
    assert not len(bad), ("kept_out", bad[:10].tolist(), gk[bad[:10]], ek[bad[:10]])
    if want_freq:
        assert gf.dtype == np.int32 and gf.shape == ef.shape
        bad = np.flatnonzero(gf != ef)
        assert not len(bad), ("freq_out", bad[:10].tolist(), gf[bad[:10]], ef[bad[:10]])
    else:
        assert gf is None


def check(c, case, forms=("host", "device"), want_freq=True, stream=None):
    exp = case.expected()
    if "host" in forms:
        same(host_call(c, case, want_freq), exp, want_freq)
    if "device" in forms:
        same(device_call(c, case, want_freq, stream), exp, want_freq)
    return exp


# ---- cases

def umi_of(v, L):
    """a UMI without N from an integer, base 0 the least significant digit"""
    return "".join("ACGT"[(v >> (2 * b)) & 3] for b in range(L))


def singles(umis, freq, group, n_groups, L, order=None):
    """one-entry buckets, every entry a molecule; order: a permutation of the buckets"""
    n = len(umis)
    idx = np.arange(n) if order is None else np.asarray(order)
    keys = sm.encode(list(umis), L).reshape(n, -1)[idx]
    return Case(keys, np.asarray(freq)[idx], np.ones(n, np.uint8), np.arange(n), np.arange(n + 1), np.asarray(group)[idx], n_groups, L)


def runs_case(seed, lengths, L=12, shuffle=True, max_freq=3):
    """runs of the given lengths in the sorted order: run j is group j's, all its molecules hold one UMI"""
    rng = np.random.default_rng(seed)
    group = np.repeat(np.arange(len(lengths)), lengths)
    n = len(group)
    umis = [umi_of(int(g) * 7919 + 5, L) for g in group]
    freq = rng.integers(1, max_freq + 1, n)
    return singles(umis, freq, group, len(lengths), L, rng.permutation(n) if shuffle else None)


def forest(rng, sizes):
    """hand-made kept[] / root[]: per bucket some entries kept (values other than 1 among them), the others under one
    of them"""
    kept, root, base = [], [], 0
    for b, size in enumerate(sizes):
        if size:
            how = ("all", "one", "some")[b % 3]
            k = np.ones(size, bool) if how == "all" else np.zeros(size, bool) if how == "one" else rng.random(size) < 0.5
            k[int(rng.integers(0, size))] = True
            idx = np.flatnonzero(k)
            kept += [int(rng.integers(1, 256)) if x else 0 for x in k]
            root += [base + (i if k[i] else int(idx[rng.integers(0, len(idx))])) for i in range(size)]
        base += size
    return np.array(kept, np.uint8), np.array(root, np.uint32)


def garbage_above(rng, keys, L):
    """random bits from 3 L up in every key's last word"""
    nw = sm.n_words_of(L)
    top = 3 * L - 64 * (nw - 1)
    if top < 64:
        k = keys.reshape(-1, nw)
        k[:, nw - 1] |= rng.integers(0, 2 ** 63, len(k), dtype=np.uint64) << np.uint64(top)
    return keys


def pool_case(seed, sizes, L, n_groups, pool=None, n_frac=0.2, max_freq=4, garbage=True):
    """random buckets over a small pool of UMIs (N letters among them; some differ in the first base only, some in
    the last only), hand-made forests, random groups with n_groups - 1 among them"""
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    pool = pool or max(3, n // 3)
    base = ["".join("ACGTN"[x] if rng.random() < n_frac else "ACGT"[x % 4] for x in rng.integers(0, 5, L)) for _ in range(pool)]
    swap = lambda ch: "ACGTN"[("ACGTN".index(ch) + 1) % 5]
    base += [swap(u[0]) + u[1:] for u in base[:pool // 3]] + [u[:-1] + swap(u[-1]) for u in base[:pool // 3]]
    umis = [base[int(rng.integers(0, len(base)))] for _ in range(n)]
    keys = sm.encode(umis, L)
    if garbage:
        keys = garbage_above(rng, keys, L)
    kept, root = forest(rng, sizes)
    # (many groups: a few ids far apart, so that buckets still share one)
    group = rng.integers(0, n_groups, len(sizes)) if n_groups <= 16 else rng.choice([0, n_groups // 2, n_groups - 1], len(sizes))
    group[np.flatnonzero(np.asarray(sizes) > 0)[-1]] = n_groups - 1
    off = np.concatenate([[0], np.cumsum(sizes)])
    return Case(keys, rng.integers(1, max_freq + 1, n), kept, root, off, group, n_groups, L)


# ---- the structure's edges

COUNTS = [1, 2, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1, SORT_TILE - 1,
          SORT_TILE, SORT_TILE + 1, 2 * SORT_TILE + 1]


@pytest.mark.parametrize("n", COUNTS)
def test_molecule_counts_on_and_beside_the_edges(ctx, n):
    """n molecules in one-entry buckets over few UMIs and cells: runs of every small length"""
    rng = np.random.default_rng(n)
    umis = [umi_of(int(v) * 104729, 12) for v in rng.integers(0, max(1, n // 3), n)]
    case = singles(umis, rng.integers(1, 4, n), rng.integers(0, 3, n), 3, 12)
    exp = check(ctx, case)
    assert n < 8 or (exp[2]["runs"] > 0 and 0 < exp[2]["removed"] < n)


@pytest.mark.parametrize("shuffle", [True, False])
def test_runs_that_begin_and_end_on_a_waves_and_a_blocks_edge(ctx, shuffle):
    lengths = [WAVE, 1, WAVE - 1, 2 * WAVE, 2, WAVE - 2, 3 * WAVE, BLOCK, BLOCK - 1, 1, 3, WAVE - 3, 2 * BLOCK + WAVE, 1, 1, 2, WAVE - 4,
               SORT_TILE - 27 * WAVE, SORT_TILE, 5]
    starts = np.concatenate([[0], np.cumsum(lengths)])
    assert {0, WAVE, 2 * WAVE, BLOCK, 2 * BLOCK, 3 * BLOCK, 4 * BLOCK, SORT_TILE, 2 * SORT_TILE} <= set(starts.tolist())
    exp = check(ctx, runs_case(7, lengths, shuffle=shuffle))
    assert exp[2]["runs"] == sum(1 for x in lengths if x > 1)
    # the same runs with one strict winner each: every run keeps exactly one molecule
    case = runs_case(8, lengths, shuffle=shuffle)
    first = {}
    for i, g in enumerate(case.group):
        first.setdefault(int(g), i)
    case.freq[list(first.values())] = 9
    exp = check(ctx, case)
    assert int(exp[0].sum()) == len(lengths)


LONG = 20000


@pytest.mark.parametrize("winner", [None, 0, LONG - 1, WAVE - 1, WAVE, BLOCK * 30], ids=lambda w: "tied" if w is None else "winner at %d" % w)
def test_one_run_holds_every_molecule(ctx, winner):
    """20,000 one-entry buckets of one cell share a UMI (the sort is stable: the winner's place in the run is its entry)"""
    freq = np.full(LONG, 2)
    if winner is not None:
        freq[winner] = 3
    case = singles(["ACGTTGCAACGT"] * LONG, freq, np.zeros(LONG, int), 1, 12)
    exp = check(ctx, case)
    assert exp[2]["runs"] == 1
    if winner is None:
        assert exp[2] == {"runs": 1, "removed": LONG, "removed_reads": 2 * LONG} and not exp[0].any()
    else:
        assert np.flatnonzero(exp[0]).tolist() == [winner] and exp[2]["removed_reads"] == 2 * (LONG - 1)


def test_two_and_three_runs_with_the_tie_at_the_top_and_below(ctx):
    totals = [(3, 1), (1, 3), (2, 2), (5, 3, 3), (3, 5, 3), (3, 3, 5), (4, 4, 1), (1, 4, 4), (4, 1, 4), (2, 2, 2), (7,)]
    umis, freq, group = [], [], []
    for j, t in enumerate(totals):
        umis += [umi_of(j * 31 + 1, 12)] * len(t)
        freq += list(t)
        group += [j % 2] * len(t)
    exp = check(ctx, singles(umis, freq, group, 2, 12, np.random.default_rng(3).permutation(len(umis))))
    assert exp[2] == {"runs": 10, "removed": 2 + 2 + 3 * 2 + 3 * 3 + 3, "removed_reads": sum(sum(t) for t in totals[:-1]) - 2 * 3 - 3 * 5}


# ---- keys

@pytest.mark.parametrize("L,n_groups", [(1, 3), (12, 1), (12, 1000), (12, 2 ** 27), (12, 2 ** 27 + 1), (21, 1), (21, 2), (21, 70000), (22, 9),
                                        (42, 9), (43, 2 ** 32 - 1), (64, 3), (85, 9)])
def test_key_widths_and_group_counts(ctx, L, n_groups):
    """one word composed with the group into a single sort key (up to 64 bits with the molecule bit: 12 bases with
    2^27 groups, 21 bases with one) and beyond; the bases that straddle words; garbage above the UMI; N letters"""
    sizes = [0, 3, 1, 0, 0, 7, 2, 40, 1, 1, 1, 70, 5, 0, 130, 2, 1, 0]
    case = pool_case(L * 1000 + n_groups % 997, sizes, L, n_groups, pool=4 if L == 1 else None)
    assert int(case.group.max()) == n_groups - 1
    exp = check(ctx, case)
    assert exp[2]["runs"] > 0 and exp[2]["removed"] > 0


@pytest.mark.parametrize("L", [12, 22, 43, 85])
def test_keys_that_differ_in_one_word_only(ctx, L):
    """UMIs that agree but for the first base, and but for the last: one run each, never joined; N equals N and
    differs from every base; the same UMI in two groups is two runs"""
    mid = "ACGT" * 22
    umis = []
    for first in "ACGTN":
        for last in "ACGTN":
            umis += [first + mid[:L - 2] + last] * 2  # (two molecules each: every UMI is a 2-run in its group)
    n = len(umis)
    freq = np.arange(n) % 2 + 1  # (the second of a pair wins)
    rng = np.random.default_rng(L)
    case = singles(umis + umis, np.concatenate([freq, freq]), [0] * n + [1] * n, 2, L, rng.permutation(2 * n))
    garbage_above(rng, case.keys, L)
    exp = check(ctx, case)
    assert exp[2] == {"runs": 50, "removed": 50, "removed_reads": 50}


# ---- totals

def test_totals_beyond_32_bits(ctx):
    big = 2 ** 31 - 1
    u = [umi_of(v, 12) for v in (11, 22, 33, 44)]
    #        bucket 0: a cluster of three          bucket 1      bucket 2 / 3: bit 0       bucket 4 / 5: tie above 2^32
    umis = [u[0], u[3], u[3],                      u[0],         u[1], u[1],               u[2], u[3], u[3], u[2], u[3], u[3]]
    freq = [big, big, big,                         big - 2,      6, 7,                     big, big, big, big, big, big]
    kept = [1, 0, 0,                               1,            1, 1,                     1, 0, 0, 1, 0, 0]
    root = [0, 0, 0,                               3,            4, 5,                     6, 6, 6, 9, 9, 9]
    off = [0, 3, 4, 5, 6, 9, 12]
    case = Case(sm.encode(umis, 12), freq, kept, root, off, [0] * 6, 1, 12)
    exp = check(ctx, case)
    # 3 * big and big - 2 agree in their low 32 bits: the cluster wins only by bit 32
    assert (3 * big) & 0xFFFFFFFF == big - 2
    assert exp[0].tolist() == [1, 0, 0, 0, 0, 1, 0, 0, 0, 0, 0, 0]
    assert exp[2] == {"runs": 3, "removed": 4, "removed_reads": big - 2 + 6 + 6 * big}
    assert exp[1].tolist() == [big, big, big, 0, 0, 7, 0, 0, 0, 0, 0, 0]


# ---- the contract

def test_empty_buckets_between_full_ones(ctx):
    sizes = [0, 0, 2, 0, 1, 0, 0, 5, 70, 0, 1, 1, 0, 0]
    case = pool_case(5, sizes, 12, 4, pool=3)
    case.group[[0, 1, 3, 5]] = 4000  # (the groups of empty buckets are not looked at)
    exp = check(ctx, case)
    assert exp[2]["runs"] > 0


def test_no_buckets_and_all_buckets_empty(ctx):
    z = np.zeros(0)
    for off, group in (([0], []), ([0, 0, 0, 0], [9, 9, 9])):
        case = Case(z, z, z, z, off, group, 0, 7)
        got = host_call(ctx, case)
        assert len(got[0]) == 0 and got[2] == {"runs": 0, "removed": 0, "removed_reads": 0}
        counts = ctx.filter_multigene_device(0, 0, 0, 0, case.off, 0, 0, 7, 0)
        assert counts == {"runs": 0, "removed": 0, "removed_reads": 0}


def test_without_freq_out(ctx):
    check(ctx, pool_case(6, [3, 0, 9, 70, 1, 1, 2], 12, 3), want_freq=False)


def test_host_form_writes_its_outputs_only(ctx):
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    case = pool_case(6, [3, 0, 9, 70, 1, 1, 2], 12, 3)
    n = len(case.freq)
    k = np.full(n + 2 * GUARD, 0x5A, np.uint8)
    f = np.full(n + 2 * GUARD, 0x5A5A5A5A, np.int32)
    counts = np.zeros(3, np.uint64)
    p = _lib.ptr
    rc = umi.load().umi_filter_multigene(ctx._h, p(case.keys, C.c_uint64), case.nw, case.L, p(case.freq, C.c_int32), p(case.kept, C.c_uint8),
                                         p(case.root, C.c_uint32), p(case.off, C.c_uint64), len(case.off) - 1, p(case.group, C.c_uint32),
                                         case.n_groups, p(k[GUARD:], C.c_uint8), p(f[GUARD:], C.c_int32), p(counts, C.c_uint64))
    assert rc == 0
    exp = case.expected()
    assert (k[GUARD:GUARD + n] == exp[0]).all() and (f[GUARD:GUARD + n] == exp[1]).all()
    assert (k[:GUARD] == 0x5A).all() and (k[GUARD + n:] == 0x5A).all() and (f[:GUARD] == 0x5A5A5A5A).all() and (f[GUARD + n:] == 0x5A5A5A5A).all()
    assert counts.tolist() == [exp[2]["runs"], exp[2]["removed"], exp[2]["removed_reads"]]


def test_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    check(ctx, pool_case(9, [3, 0, 9, 70, 1, 1, 2, 300], 22, 5), forms=("device",), stream=s)


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        check(c, pool_case(9, [3, 0, 9, 70, 1, 1, 2, 300], 12, 5))
    finally:
        c.close()


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the filter lets it end first, its result is still handed out,
    and right, afterwards -- and is what the filter of that very call takes as input"""
    import torch
    import oracle as orc
    from umi_collapse_rs_amd import synth
    pos, bases = synth.molecule_reads(seed=31, n_positions=300, reads_per_position=25, umi_len=12, err=0.02)
    st = synth.stage(pos, synth.bases_to_keys(bases))
    keys, freq, off = (np.ascontiguousarray(st["keys"], np.uint64), np.ascontiguousarray(st["freq"], np.int32),
                       np.ascontiguousarray(st["bucket_off"], np.uint64))
    okept, oroot, _ = orc.dedup_batch(keys, None, freq, off, 12, 1)
    t_keys, t_freq = dev(keys.view(np.int64)), dev(freq)
    t_kept = torch.zeros(len(keys), dtype=torch.uint8, device="cuda:0")
    t_root = torch.zeros(len(keys), dtype=torch.int32, device="cuda:0")
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_freq.data_ptr(), off, 12, t_kept.data_ptr(), t_root.data_ptr(),
                                 k=1, stream=s.cuda_stream)
    check(ctx, pool_case(9, [3, 0, 9, 70, 1, 1, 2, 300], 12, 5))
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum())
    group = np.arange(len(off) - 1) % 3
    exp = check(ctx, Case(keys, freq, okept, oroot, off, group, 3, 12))
    assert exp[2]["removed"] + int(exp[0].sum()) == stats["n_kept"]


def fails(code, call):
    import umi_collapse_rs_amd as umi
    with pytest.raises(umi.UmiHipError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def good_case():
    case = pool_case(61, [3, 0, 12, 70], 12, 4)
    case.kept[15:], case.root[15:] = 1, np.arange(15, 85)  # (the last bucket: everything kept, whatever the forest drew)
    return case


def changed(case, **kw):
    c = Case(case.keys, case.freq, case.kept.copy(), case.root.copy(), case.off.copy(), case.group.copy(), case.n_groups, case.L)
    for name, value in kw.items():
        setattr(c, name, value)
    return c


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_errors(ctx, form):
    from umi_collapse_rs_amd import _lib
    good = good_case()
    check(ctx, good, forms=(form,))
    call = host_call if form == "host" else device_call
    refused = lambda case: fails(_lib.UMI_ERR_ARG, lambda: call(ctx, case))
    # counted on the device
    c = changed(good)
    c.root[20], c.kept[20] = 0, 0  # an entry of the last bucket under one of the first
    assert "root" in refused(c)
    c = changed(good)
    c.kept[20], c.kept[21] = 0, 0
    c.root[20], c.root[21] = 15, 20  # entry 21 under entry 20, which was not kept
    assert "root" in refused(c)
    c = changed(good)
    c.root[16] = 17  # a kept entry under another
    assert "root" in refused(c)
    c = changed(good)
    c.root[16] = 2 ** 32 - 1  # far outside every array
    assert "root" in refused(c)
    c = changed(good)
    c.group[2] = 4  # n_groups
    assert "group" in refused(c)
    c = changed(good)
    c.group[1] = 4  # (an empty bucket's group is not looked at)
    check(ctx, c, forms=(form,))
    # found on the host
    c = changed(good)
    c.off[1], c.off[2] = 5, 3
    assert "monotone" in refused(c)
    c = changed(good)
    c.off[0] = 1
    assert "bucket_off[0]" in refused(c)
    assert "umi_len" in refused(changed(good, L=0))
    n = len(good.freq)
    assert "umi_len" in refused(changed(good, L=86, nw=4, keys=np.zeros(4 * n, np.uint64)))
    assert "n_words" in refused(changed(good, nw=2, keys=np.zeros(2 * n, np.uint64)))
    assert "groups" in refused(changed(good, n_groups=0))
    check(ctx, good, forms=(form,))  # (and the context still works)


def test_nulls_aliases_and_sizes_are_refused_before_anything_is_read(ctx):
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    L = umi.load()
    fake = [C.c_void_p(4096 * (i + 1)) for i in range(7)]
    off = np.array([0, 5], np.uint64)
    counts = np.zeros(3, np.uint64)
    pc, po = _lib.ptr(counts, C.c_uint64), _lib.ptr(off, C.c_uint64)

    def call(args, off_p=po, nb=1, counts_p=pc, n_words=1, umi_len=12):
        keys, freq, kept, root, group, kout, fout = args
        return L.umi_filter_multigene_device(ctx._h, keys, n_words, umi_len, freq, kept, root, off_p, nb, group, 3, kout, fout, counts_p, None)
    assert call(fake, counts_p=None) == _lib.UMI_ERR_ARG and "counts" in L.umi_last_error().decode()
    for hole in range(6):  # (freq_out alone may be NULL)
        args = list(fake)
        args[hole] = None
        assert call(args) == _lib.UMI_ERR_ARG and "NULL" in L.umi_last_error().decode(), hole
    assert call(fake, off_p=None) == _lib.UMI_ERR_ARG and "bucket_off" in L.umi_last_error().decode()
    alias = list(fake)
    alias[5] = fake[2]  # kept_out == kept
    assert call(alias) == _lib.UMI_ERR_ARG and "its own input" in L.umi_last_error().decode()
    alias = list(fake)
    alias[6] = fake[1]  # freq_out == freq
    assert call(alias) == _lib.UMI_ERR_ARG and "its own input" in L.umi_last_error().decode()
    big = np.array([0, 2 ** 30], np.uint64)
    assert call(fake, off_p=_lib.ptr(big, C.c_uint64)) == _lib.UMI_ERR_ARG and "30-bit" in L.umi_last_error().decode()
    assert call(fake, nb=2 ** 30) == _lib.UMI_ERR_ARG and "30-bit" in L.umi_last_error().decode()
    assert L.umi_filter_multigene_device(None, *fake[:1], 1, 12, *fake[1:4], po, 1, fake[4], 3, fake[5], fake[6], pc, None) == _lib.UMI_ERR_ARG
    assert "ctx" in L.umi_last_error().decode()


# ---- what the library's own collapse leaves

@pytest.mark.parametrize("algo", [0, 1, 2], ids=["directional", "adjacency", "cluster"])
def test_fuzz_on_the_collapses_own_arrays(ctx, algo):
    """buckets of 1 to 40 entries over a pool small enough that about a third of the molecules share their UMI with
    another of their cell; kept[] / root[] from a real dedup_batch call"""
    shared = runs = 0
    for seed in range(17):
        rng = np.random.default_rng(1000 * algo + seed)
        nb, L = int(rng.integers(1, 60)), 12
        n_groups = int(rng.integers(1, 6))
        pool = [umi_of(int(v), L) for v in rng.integers(0, 4 ** L, max(64, nb * 24))]
        umis, freq, sizes = [], [], []
        for _ in range(nb):
            size = int(rng.integers(1, 41))
            mine = {}
            for u in rng.choice(len(pool), size, replace=False):
                mine[pool[int(u)]] = int(rng.integers(1, 9))
            centre = list(mine)[0]  # (neighbours of one of them, so that the collapse has something to remove)
            for at in rng.integers(0, L, size // 3):
                v = centre[:at] + "ACGT"[("ACGT".index(centre[at]) + 1) % 4] + centre[at + 1:]
                mine.setdefault(v, 1)
            order = sorted(mine, key=lambda t: -mine[t])  # rank order: freq descending, stable
            umis += order
            freq += [mine[t] for t in order]
            sizes.append(len(order))
        off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        keys = sm.encode(umis, L)
        kept, root, _ = ctx.dedup_batch(keys, None, np.array(freq, np.int32), off, L, k=1, algo=algo, adj_max_freq=2)
        case = Case(keys, freq, kept, root, off, rng.integers(0, n_groups, nb), n_groups, L)
        exp = check(ctx, case, forms=("host",) if seed % 2 else ("device",))
        assert exp[2]["removed"] + int(exp[0].sum()) == int(np.count_nonzero(kept))
        shared += exp[2]["removed"] + exp[2]["runs"]
        runs += int(np.count_nonzero(kept))
    assert 0.15 < shared / runs < 0.6, (shared, runs)
