"""umi_dedup_stats / umi_dedup_stats_device on the GPU against tests/stats_model.py: the three tables and the per-UMI
table by exact equality, on both call forms.  The shapes walk every path of csrc/umihip_stats.hip: buckets on both
sides of the 8-entry bound between a lane's and a wave's, of the 64 entries a wave takes at a time, of "stats_split"
(set to 256, and at its default 4096) and of the 1024 entries of a deep bucket's piece; keys of one to four words with
the two bases that straddle words; family sizes on both sides of the 2048 bins a block counts in LDS and above the
last bin; kept[] / root[] from the oracle's three algorithms and from hand-made forests."""
import numpy as np
import pytest

import cluster_model
import oracle as orc
import stats_model as sm

pytestmark = pytest.mark.gpu
TABLE = ("umi_entry", "times_pre", "reads_pre", "times_post", "reads_post")
LANE_MAX, HIST_LDS, PIECE, SPLIT = 8, 2048, 1024, 4096  # the bounds csrc/umihip_internal.h chooses


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).copy()).to("cuda:0")


def device_call(c, case, seed, hist_bins, per_umi, stream=None):
    """the _device form on tensors of its own: kept[] one byte off alignment, the outputs pre-filled with a pattern"""
    import torch
    keys, freq, kept, root, off, L = case
    n, nw = len(freq), sm.n_words_of(L)
    t_kept = torch.zeros(n + 1, dtype=torch.uint8, device="cuda:0")
    t_kept[1:] = dev(np.asarray(kept, np.uint8))
    t_keys, t_freq, t_root = dev(np.asarray(keys, np.uint64).view(np.int64)), dev(np.asarray(freq, np.int32)), \
        dev(np.asarray(root, np.uint32).view(np.int32))
    fill64 = lambda m: torch.full((max(m, 1),), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device="cuda:0")
    fill32 = lambda m: torch.full((max(m, 1),), 0x5A5A5A5A, dtype=torch.int32, device="cuda:0")
    pre, post, dist = fill64(hist_bins), fill64(hist_bins), fill64(4 * (L + 2))
    tab = dict(d_umi_entry=fill32(n), d_times_pre=fill32(n), d_reads_pre=fill64(n), d_times_post=fill32(n), d_reads_post=fill64(n))
    torch.cuda.synchronize()
    rows = c.dedup_stats_device(t_keys.data_ptr(), t_freq.data_ptr(), t_kept.data_ptr() + 1, t_root.data_ptr(), off, L,
                                pre.data_ptr(), post.data_ptr(), dist.data_ptr(), n_words=nw, seed=seed, hist_bins=hist_bins,
                                stream=stream.cuda_stream if stream is not None else 0,
                                **({k: v.data_ptr() for k, v in tab.items()} if per_umi else {}))
    if stream is not None:
        stream.synchronize()
    torch.cuda.synchronize()
    out = {"count_pre": pre.cpu().numpy().view(np.uint64), "count_post": post.cpu().numpy().view(np.uint64),
           "dist": dist.cpu().numpy().view(np.uint64).reshape(4, L + 2)}
    if per_umi:
        for name in TABLE:
            a = tab["d_" + name].cpu().numpy()
            out[name] = a.view(np.uint32 if a.dtype == np.int32 else np.uint64)[:rows]
    else:
        assert rows == 0
    return out


def same(got, exp):
    assert set(got) == set(exp), (sorted(got), sorted(exp))
    for name in exp:
        a, b = got[name], exp[name]
        assert a.dtype == b.dtype and a.shape == b.shape, (name, a.dtype, b.dtype, a.shape, b.shape)
        bad = np.argwhere(a != b)
        assert not len(bad), (name, bad[:10].tolist(), a[a != b][:10], b[a != b][:10])


_model = {}


def check(c, case, seed=0, hist_bins=65536, per_umi=True, forms=("host", "device"), stream=None, name=None):
    keys, freq, kept, root, off, L = case
    ident = (name, seed, hist_bins, per_umi)
    if name is None or ident not in _model:  # (a named case's reference is computed once)
        _model[ident] = sm.stats_model(keys, freq, kept, root, off, L, seed=seed, hist_bins=hist_bins, per_umi=per_umi)
    exp = _model[ident]
    if "host" in forms:
        same(c.dedup_stats(keys, freq, kept, root, off, L, n_words=sm.n_words_of(L), seed=seed, hist_bins=hist_bins,
                           per_umi=per_umi), exp)
    if "device" in forms:
        same(device_call(c, case, seed, hist_bins, per_umi, stream), exp)
    return exp


def random_umis(rng, n, L, n_frac, pool):
    """n UMIs around `pool` centres, so that pairs at small distances and equal UMIs occur"""
    centres = rng.integers(0, 4, (max(1, pool), L))
    out = []
    for _ in range(n):
        u = centres[int(rng.integers(0, len(centres)))].copy()
        for at in rng.integers(0, L, int(rng.integers(0, 3))):
            u[at] = rng.integers(0, 4)
        text = "".join("ACGT"[x] for x in u)
        if n_frac and rng.random() < n_frac:
            at = int(rng.integers(0, L))
            text = text[:at] + "N" + text[at + 1:]
        out.append(text)
    return out


def forest(rng, sizes, mode="random"):
    """hand-made kept[] / root[]: per bucket some entries kept (at least one; values other than 1 among them), the
    others under one of them.  Buckets in turn: everything kept, a single entry kept, a random share."""
    kept, root, base = [], [], 0
    for b, size in enumerate(sizes):
        if size:
            how = mode if mode != "random" else ("all", "one", "some")[b % 3]
            k = np.ones(size, bool) if how == "all" else np.zeros(size, bool) if how == "one" else rng.random(size) < 0.4
            k[int(rng.integers(0, size))] = True
            idx = np.flatnonzero(k)
            kept += [int(rng.integers(1, 256)) if x else 0 for x in k]
            root += [base + (i if k[i] else int(idx[rng.integers(0, len(idx))])) for i in range(size)]
        base += size
    return np.array(kept, np.uint8), np.array(root, np.uint32)


def made_case(seed, sizes, L, n_frac=0.05, mode="random", max_freq=30):
    rng = np.random.default_rng(seed)
    n = int(sum(sizes))
    umis = random_umis(rng, n, L, n_frac, pool=max(2, n // 6))
    freq = rng.integers(1, max_freq, n).astype(np.int32)
    kept, root = forest(rng, sizes, mode)
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    return sm.encode(umis, L), freq, kept, root, off, L


def oracle_case(seed, sizes, L, algo, k=1, n_frac=0.03):
    """seeded buckets in rank order, kept[] / root[] the oracle's (adjacency removes entries of up to two reads)"""
    rng = np.random.default_rng(seed)
    umis, freq = [], []
    real = []
    for size in sizes:
        seen = {}
        for u in random_umis(rng, size * 3, L, n_frac, pool=max(1, size // 4)):
            if len(seen) < size or u in seen:
                seen[u] = seen.get(u, 0) + int(rng.integers(1, 5))
        order = sorted(seen, key=lambda t: -seen[t])
        umis += order
        freq += [seen[t] for t in order]
        real.append(len(order))
    off = np.concatenate([[0], np.cumsum(real)]).astype(np.uint64)
    freq = np.array(freq, np.int32)
    keys, nm = orc.encode_keys(umis) if L <= 21 else orc.encode_keys_wide(umis)
    if algo == 2:  # (connected components: tests/cluster_model.py defines them, the oracle has no such mode)
        kept, root = cluster_model.batch_of_keys(keys, nm, off.astype(np.int64), k)
    elif L <= 21:
        kept, root, _ = orc.dedup_batch(keys, nm, freq, off, L, k, algo=algo, adj_max_freq=2)
    else:
        kept, root, _ = orc.dedup_batch_wide(keys, nm, freq, off, L, k, algo=algo, adj_max_freq=2)
    keys = np.ascontiguousarray(keys).reshape(-1)
    assert (keys == sm.encode(umis, L)).all()
    return keys, freq, kept, root, off, L


SIZES = [0, 0, 1, 2, 3, LANE_MAX, LANE_MAX + 1, 0, 63, 64, 65, 129, 1, 0]


@pytest.mark.parametrize("L", [1, 8, 12, 21, 22, 42, 43, 64, 85])
def test_bucket_sizes_and_key_widths(ctx, L):
    """empty buckets between the others and at both ends; buckets where everything is kept and where one entry is"""
    sizes = SIZES + ([600, 0] if L in (12, 43, 85) else [0])
    case = made_case(L, sizes, L)
    assert case[4][1] == 0 and case[4][-1] == case[4][-2]
    exp = check(ctx, case, seed=L)
    non_empty = sum(1 for s in sizes if s)
    assert exp["dist"].sum(axis=1).tolist() == [non_empty] * 4 and int(exp["dist"][2, L + 1]) >= 4


def test_without_n(ctx):
    check(ctx, made_case(77, SIZES, 12, n_frac=0.0), seed=1)


@pytest.mark.parametrize("algo", [0, 1, 2], ids=["directional", "adjacency", "cluster"])
@pytest.mark.parametrize("L", [12, 22])
def test_the_oracles_collapse(ctx, algo, L):
    case = oracle_case(5 + algo, [0, 1, 2, 3, 7, 9, 40, 0, 70, 130, 300], L, algo)
    exp = check(ctx, case, seed=9)
    assert 0 < int(exp["count_post"].sum()) < len(case[1])  # something was removed
    assert int(exp["reads_post"].sum()) == int(case[1].astype(np.int64).sum())


@pytest.mark.parametrize("split", [256, None], ids=["split 256", "default split"])
def test_a_deep_bucket_and_the_sizes_around_the_split(split):
    """one bucket of 1,500 entries, and buckets on both sides of the split and of a piece's 1,024 entries: counted by
    the whole grid with "stats_split" 256, by one wave each at its default"""
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        if split:
            c.set_option("stats_split", split)
        sizes = [1500, 0, 255, 256, 257, 3, PIECE - 1, PIECE, PIECE + 1, 2 * PIECE + 1, 70]
        check(c, made_case(21, sizes, 10), seed=3, name="deep")
    finally:
        c.close()


def test_sizes_around_the_default_split(ctx):
    check(ctx, made_case(22, [SPLIT - 1, 5, SPLIT, SPLIT + 1], 8, n_frac=0.01), seed=4)


@pytest.mark.parametrize("split", [256, None], ids=["split 256", "default split"])
def test_one_root_for_1500_entries(split):
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        if split:
            c.set_option("stats_split", split)
        exp = check(c, made_case(23, [2, 1500, 9], 12, mode="one"), seed=5, name="one root")
        assert int(exp["count_post"].sum()) == 3
    finally:
        c.close()


def test_options_range(ctx):
    from umi_collapse_rs_amd import _lib
    for bad in (63, 2 ** 30 + 1, 0, -1):
        fails(_lib.UMI_ERR_ARG, lambda: ctx.set_option("stats_split", bad))
    ctx.set_option("stats_split", 2 ** 30)
    ctx.set_option("stats_split", SPLIT)


@pytest.mark.parametrize("hist_bins", [2, 3, 4096, 65536])
def test_family_sizes_around_the_lds_bound_and_the_last_bin(ctx, hist_bins):
    """freq and totals on both sides of the 2,048 bins counted in LDS; totals above hist_bins - 1"""
    rng = np.random.default_rng(31)
    sizes = [4, 0, 12, 70, 3]
    keys, freq, kept, root, off, L = made_case(31, sizes, 9)
    freq[:] = rng.choice([1, 2, 3, HIST_LDS - 1, HIST_LDS, HIST_LDS + 1, 4095, 4096, 5000], len(freq))
    freq[0:4] = [HIST_LDS - 3, 1, 1, 1]
    kept[0:4], root[0:4] = [1, 0, 0, 0], [0, 0, 0, 0]  # a total of exactly HIST_LDS
    exp = check(ctx, (keys, freq, kept, root, off, L), seed=6, hist_bins=hist_bins)
    assert int(exp["count_post"][min(HIST_LDS, hist_bins - 1)]) >= 1
    reached = hist_bins <= 4096  # (no family is as large as 65,535)
    assert (int(exp["count_pre"][hist_bins - 1]) > 0) == reached and (int(exp["count_post"][hist_bins - 1]) > 0) == reached
    assert int(exp["count_pre"][0]) == int(exp["count_post"][0]) == 0


@pytest.mark.parametrize("seed", [0, 2 ** 64 - 1])
def test_seeds_and_reads_beyond_32_bits(ctx, seed):
    keys, freq, kept, root, off, L = made_case(41, [3, 9, 0, 70, 2], 12, max_freq=6)
    freq[[1, 20]] = 2 ** 31 - 1
    freq[5] = 2 ** 30
    freq[40] = 2 ** 31 - 1
    assert int(freq.astype(np.int64).sum()) > 2 ** 32
    exp = check(ctx, (keys, freq, kept, root, off, L), seed=seed, name="big reads")
    other = sm.stats_model(keys, freq, kept, root, off, L, seed=seed ^ 1, per_umi=False)
    assert (exp["dist"][0] == other["dist"][0]).all() and (exp["dist"][2] == other["dist"][2]).all()


def test_the_null_depends_on_the_seed():
    case = made_case(42, [30] * 40, 12)
    a = sm.stats_model(*case, seed=0, per_umi=False)["dist"]
    b = sm.stats_model(*case, seed=1, per_umi=False)["dist"]
    assert (a[1] != b[1]).any() and (a[0] == b[0]).all()


@pytest.mark.parametrize("per_umi", [True, False])
def test_per_umi_table_on_and_off(ctx, per_umi):
    exp = check(ctx, made_case(51, SIZES + [300], 12), seed=7, per_umi=per_umi, name="on and off")
    assert ("umi_entry" in exp) == per_umi


def test_one_umi_in_every_bucket_and_all_umis_distinct(ctx):
    rng = np.random.default_rng(52)
    sizes = [5, 1, 70, 0, 9, 300, 2]
    keys, freq, kept, root, off, L = made_case(52, sizes, 12, n_frac=0.0)
    common = sm.encode(["ACGTTGCAACGT"], 12)[0]
    for b in range(len(sizes)):
        if sizes[b]:
            keys[int(off[b]) + int(rng.integers(0, sizes[b]))] = common
    exp = check(ctx, (keys, freq, kept, root, off, L), seed=8)
    row = [j for j, e in enumerate(exp["umi_entry"]) if keys[int(e)] == common]
    assert len(row) == 1 and int(exp["times_pre"][row[0]]) >= 6
    # all distinct: 1,000 keys of two words, in random order
    L = 30
    perm = rng.permutation(1000)
    umis = ["".join("ACGT"[(int(v) >> (2 * b)) & 3] for b in range(L)) for v in perm * 7919]
    assert len(set(umis)) == 1000
    kept, root = forest(rng, [400, 600])
    exp = check(ctx, (sm.encode(umis, L), rng.integers(1, 9, 1000).astype(np.int32), kept, root, np.array([0, 400, 1000], np.uint64), L))
    assert len(exp["umi_entry"]) == 1000 and (exp["times_pre"] == 1).all()


@pytest.mark.parametrize("L", [22, 43, 85])
def test_keys_that_differ_only_in_the_last_word(ctx, L):
    """at 22 and 43 bases only the straddling base reaches the last word, with two bits and with one: A / C / N and
    A / N agree in the bits before it"""
    rng = np.random.default_rng(L)
    nw = sm.n_words_of(L)
    s = 64 * (nw - 1) // 3  # the base that holds the last word's first bit
    head = "".join("ACGT"[x] for x in rng.integers(0, 4, s))
    cand = [head + "A" * (L - s)] + [head + "".join("ACGTN"[x] for x in rng.integers(0, 5, L - s)) for _ in range(400)]
    keys = sm.encode(cand, L).reshape(-1, nw)
    umis = [u for u, k in zip(cand, keys) if (k[:nw - 1] == keys[0, :nw - 1]).all()][:200]
    n = len(umis)
    keys = sm.encode(umis, L)
    distinct = len(set(keys[nw - 1::nw].tolist()))
    assert n > 50 and all(len(set(keys[w::nw].tolist())) == 1 for w in range(nw - 1)) and distinct == {22: 3, 43: 2}.get(L, distinct) > 1
    kept, root = forest(rng, [3, n - 3])
    exp = check(ctx, (keys, rng.integers(1, 9, n).astype(np.int32), kept, root, np.array([0, 3, n], np.uint64), L), seed=2)
    assert len(exp["umi_entry"]) == distinct


def test_on_a_stream(ctx):
    import torch
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.default_stream())
    check(ctx, made_case(51, SIZES + [300], 12), seed=7, forms=("device",), stream=s, name="on and off")


def test_no_buckets_and_all_buckets_empty(ctx):
    z = np.zeros(0)
    for off in ([0], [0, 0, 0, 0]):
        exp = check(ctx, (z.astype(np.uint64), z.astype(np.int32), z.astype(np.uint8), z.astype(np.uint32), np.array(off, np.uint64), 7),
                    hist_bins=16)
        assert not exp["dist"].any() and not exp["count_pre"].any() and len(exp["umi_entry"]) == 0


def fails(code, call):
    import umi_collapse_rs_amd as umi
    with pytest.raises(umi.UmiHipError) as e:
        call()
    assert e.value.code == code, e.value
    return str(e.value)


def call_only(c, case, form, hist_bins=65536):
    """one call without the model (which has no answer for what the library refuses)"""
    keys, freq, kept, root, off, L = case
    if form == "host":
        return c.dedup_stats(keys, freq, kept, root, off, L, n_words=sm.n_words_of(L), hist_bins=hist_bins)
    return device_call(c, case, 0, hist_bins, True)


@pytest.mark.parametrize("form", ["host", "device"])
def test_argument_errors(ctx, form):
    from umi_collapse_rs_amd import _lib
    keys, freq, kept, root, off, L = good = made_case(61, [3, 0, 12, 70], 12)
    kept[15:], root[15:] = 1, np.arange(15, 85)  # (the last bucket: everything kept, whatever the forest drew)
    check(ctx, good, forms=(form,), name="good")
    refused = lambda case, **kw: fails(_lib.UMI_ERR_ARG, lambda: call_only(ctx, case, form, **kw))
    bad_keys = keys.copy()
    bad_keys[40] = (int(bad_keys[40]) & ~(7 << 15)) | (1 << 15)  # code 001 at base 5
    assert "code" in refused((bad_keys, freq, kept, root, off, L))
    other, kept2 = root.copy(), kept.copy()
    other[20], kept2[20] = 0, 0  # an entry of the last bucket under one of the first
    assert "root" in refused((keys, freq, kept2, other, off, L))
    unkept, kept3 = root.copy(), kept.copy()
    kept3[20], kept3[21] = 0, 0
    unkept[20], unkept[21] = 15, 20  # entry 21 under entry 20, which was not kept
    assert "root" in refused((keys, freq, kept3, unkept, off, L))
    not_self = root.copy()
    not_self[16] = 17  # a kept entry under another
    assert "root" in refused((keys, freq, kept, not_self, off, L))
    falling = off.copy()
    falling[1], falling[2] = 5, 3
    assert "monotone" in refused((keys, freq, kept, root, falling, L))
    assert "hist_bins" in refused(good, hist_bins=1)
    import ctypes as C
    import umi_collapse_rs_amd as umi
    one = np.zeros(8, np.uint64)
    p64 = _lib.ptr(one, C.c_uint64)
    rc = umi.load().umi_dedup_stats(ctx._h, None, 4, None, None, None, _lib.ptr(np.zeros(1, np.uint64), C.c_uint64), 0, 86, 0, 16, p64,
                                    p64, p64, None, None, None, None, None, None)
    assert rc == _lib.UMI_ERR_ARG and "umi_len" in umi.load().umi_last_error().decode()
    check(ctx, good, forms=(form,), name="good")  # (and the context still works)


def test_sizes_are_refused_before_anything_is_read(ctx):
    import ctypes as C
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    out = np.zeros(64, np.uint64)
    p = _lib.ptr(out, C.c_uint64)
    fake = C.c_void_p(4096)
    for off, what in (([0, 2 ** 28], "2^28"), ([0, 2 ** 27] + [2 ** 27 * (i + 2) for i in range(15)], "31-bit")):
        o = np.array(off, np.uint64)
        rc = umi.load().umi_dedup_stats_device(ctx._h, fake, 1, fake, fake, fake, _lib.ptr(o, C.c_uint64), len(off) - 1, 12, 0, 16,
                                               fake, fake, fake, None, None, None, None, None, None, None)
        assert rc == _lib.UMI_ERR_ARG and what in umi.load().umi_last_error().decode()


def test_multi_device_context_uses_its_first_device():
    import umi_collapse_rs_amd as umi
    c = umi.Context([0, 0])
    try:
        check(c, made_case(51, SIZES + [300], 12), seed=7, name="on and off")
    finally:
        c.close()


def test_while_a_deferred_call_is_out(ctx):
    """umi_dedup_batch_device_begin leaves a call out; the stats call lets it end first, and its result is still handed
    out, and right, afterwards -- and is what the stats of that very call take as input"""
    import torch
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
    check(ctx, made_case(51, SIZES + [300], 12), seed=7, name="on and off")
    stats = ctx.dedup_batch_end()
    s.synchronize()
    assert (t_kept.cpu().numpy() == okept).all()
    assert (t_root.cpu().numpy().view(np.uint32) == oroot).all()
    assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(keys)
    exp = check(ctx, (keys, freq, okept, oroot, off, 12), seed=11)
    assert int(exp["count_post"].sum()) == stats["n_kept"]
