"""UMI_ALGO_CLUSTER on the GPU: one UMI per connected component of "within k", on every entry point and path.

Every case is checked against tests/cluster_model.py (union-find over the distance matrix, from the definition)
and, where every freq is below 2^31 - 1, bit for bit against the same entry point called with
algo = DIRECTIONAL, percentage = inf -- code that the mode does not touch, and the same answer (a directional
threshold that admits every pair makes every pair within k a symmetric one).  Each runs with and without root[]
and asserts n_kept, n_buckets, max_bucket, n_pairs and n_rounds <= 1.  Everything is integer and bit-exact."""
import contextlib
import ctypes as C
import functools
import itertools

import numpy as np
import pytest

import chain_inputs as ci
import cluster_model as cm
import edit_model as em
import kept_only_inputs as ko
import oracle as orc
import seg_probe_inputs as sp
import seq_model as sm
import test_gpu_deferred as df
from helpers import canonical, clustered_bucket, hamming_matrix, one_word_batch, seq_buckets, wide_batch

pytestmark = pytest.mark.gpu

DIR, ADJ, CLUSTER = 0, 1, 2
INF = float("inf")
INT32_MAX = 2 ** 31 - 1


@contextlib.contextmanager
def context(opts=None, device=0):
    import umi_collapse_rs_amd as umi
    c = umi.Context(device)
    try:
        for name, v in (opts or {}).items():
            c.set_option(name, v)
        yield c
    finally:
        c.close()


class Call:
    """One call's arrays (keys [n] or [n, w], nm, fr, off), how to run it -- run(ctx, want_root, algo, p, amf)
    -> (kept, root or None, stats) -- and the model's (kept, root), computed once."""

    def __init__(self, keys, nm, fr, off, L, k, form="one", blen=None, model=None):
        self.keys, self.nm, self.fr, self.off, self.L, self.k, self.form, self.blen = keys, nm, fr, off, L, k, form, blen
        self.nmask = nm if nm is not None and nm.any() else None
        kept, root = model if model is not None else cm.batch_of_keys(keys, nm, off, k)
        kept.setflags(write=False)
        root.setflags(write=False)
        self.kept, self.root = kept, root
        sizes = np.diff(off.astype(np.int64))
        self.n_buckets, self.max_bucket = len(sizes), int(sizes.max()) if len(sizes) else 0
        self.n_pairs = int((sizes * (sizes - 1) // 2).sum())

    def run(self, ctx, want_root, algo=CLUSTER, p=0.5, amf=0):
        a = (self.keys, self.nmask, self.fr, self.off)
        if self.form == "one":
            return ctx.dedup_batch(*a, self.L, self.k, p, algo, amf, want_root=want_root)
        if self.form == "wide":
            return ctx.dedup_batch_wide(*a, self.L, self.k, p, algo, amf, want_root=want_root)
        if self.form == "edit":
            return ctx.dedup_batch_edit(*a, self.L, self.k, p, algo, amf, want_root=want_root)
        return ctx.dedup_seqs(self.keys, self.nm, self.fr, self.off, self.blen, self.k, p, algo, amf, want_root=want_root)


def same(what, kept, root, st, ekept, eroot):
    bad = np.nonzero(np.asarray(kept) != ekept)[0]
    assert bad.size == 0, "%s: kept differs at %d entries, first %d" % (what, bad.size, bad[0])
    assert st["n_kept"] == int(ekept.sum()), (what, st["n_kept"], int(ekept.sum()))
    if root is not None:
        bad = np.nonzero(np.asarray(root) != eroot)[0]
        assert bad.size == 0, "%s: root differs at %d entries, first %d (%d, expected %d)" % (
            what, bad.size, bad[0], root[bad[0]], eroot[bad[0]])


def check(call, ctx, what, run=None, directional=True, stats=True):
    """The assertions every case makes on run(ctx, want_root, algo, p, amf) (default: the call's host-buffer form).
    Returns the stats of the cluster call with root."""
    run = run or call.run
    out = None
    for want_root in (True, False):
        kept, root, st = run(ctx, want_root, CLUSTER, 0.5, 0)
        assert (root is not None) == want_root
        w = "%s, want_root %s" % (what, want_root)
        same(w + ": against the model", kept, root, st, call.kept, call.root)
        assert st["n_rounds"] <= 1, (w, st["n_rounds"])
        if stats:
            assert (st["n_buckets"], st["max_bucket"], st["n_pairs"]) == (call.n_buckets, call.max_bucket, call.n_pairs), (w, st)
        if directional:
            assert int(call.fr.max(initial=0)) < INT32_MAX
            dkept, droot, dst = run(ctx, want_root, DIR, INF, 0)
            same(w + ": against directional at p = inf", kept, root, st, np.asarray(dkept), call.root if droot is None else np.asarray(droot))
            for f in ("n_umis", "n_buckets", "max_bucket", "n_pairs", "n_pairs_evaluated", "n_kept"):
                assert st[f] == dst[f], (w, f, st[f], dst[f])
        out = out or st
    return out


def assemble(buckets, wide=False):
    umis = [u for b in buckets for u in b[0]]
    fr = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    if not umis:
        return np.zeros(0, np.uint64), np.zeros(0, np.uint64), fr, off
    keys, nm = (orc.encode_keys_wide if wide else orc.encode_keys)(umis)
    return keys, nm, fr, off


# ---- 1. the fused kernel -------------------------------------------------------------------------------------
FUSED_SIZES = (1, 2, 3, 31, 32, 33, 63, 64, 65, 127, 128)


@functools.lru_cache(maxsize=None)
def fused_call(k, n_frac, top):
    rng = np.random.default_rng(8100 + k + int(100 * n_frac))
    buckets = [clustered_bucket(rng, n, 12, n_frac) for n in FUSED_SIZES]
    if top:
        buckets = [(u, [INT32_MAX] * len(u)) for u, _ in buckets]
    call = Call(*assemble(buckets), 12, k)
    assert call.max_bucket == 128 and (n_frac > 0) == (call.nmask is not None)
    return call


@pytest.mark.parametrize("sliced", [0, 1])
@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("k", [0, 1, 2, 3, 4])
def test_fused_kernel(k, n_frac, sliced):
    """Buckets of 1 .. 128 entries in one call, L = 12 (k = 4: the body that walks the columns), and the same
    call with every freq INT32_MAX -- legal, and nothing there to wrap."""
    with context(dict(fused_sliced=sliced)) as ctx:
        call = fused_call(k, n_frac, False)
        st = check(call, ctx, "fused k=%d N=%g sliced=%d" % (k, n_frac, sliced))
        assert st["n_edges"] == 0 and st["n_rounds"] == 0  # (nothing left the fused kernel)
        if k:
            assert st["n_kept"] < st["n_umis"]
        top = fused_call(k, n_frac, True)
        assert np.array_equal(top.kept, call.kept)
        check(top, ctx, "fused, freq INT32_MAX, k=%d N=%g sliced=%d" % (k, n_frac, sliced), directional=False)


# ---- 2. the tile kernels -------------------------------------------------------------------------------------
TILE_SIZES = (129, 600, 1100, 2100)


@functools.lru_cache(maxsize=None)
def tile_call(k, n_frac):
    rng = np.random.default_rng(8200 + k + int(100 * n_frac))
    buckets = [clustered_bucket(rng, n, 12, n_frac) for n in TILE_SIZES]
    return Call(*assemble(buckets), 12, k)


@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("k", [1, 2])
def test_tile_kernels(k, n_frac):
    """seg_index = 0: buckets on both sides of fused_max, small_max and the 2,048-row tile go to the popcount
    tile kernels, whose pairs all reach the list flagged and are united by the list's union pass."""
    call = tile_call(k, n_frac)
    with context(dict(seg_index=0)) as ctx:
        st = check(call, ctx, "tiles k=%d N=%g" % (k, n_frac))
        assert st["n_edges"] > 0 and st["n_rounds"] == 1
        ctx.set_option("fused_max", 0)
        ctx.set_option("small_max", 200)
        check(call, ctx, "tiles, fused_max 0, small_max 200, k=%d N=%g" % (k, n_frac))


# ---- 3. the segment index ------------------------------------------------------------------------------------
SEG_OPTS = ("seg_unite", "seg_local", "seg_probe", "seg_lds", "seg_ckey", "seg_sliced")


@functools.lru_cache(maxsize=None)
def seg_call(L, k, n_frac):
    return Call(*one_word_batch(L, k, n_frac), L, k)


@pytest.mark.parametrize("n_frac", [0.0, 0.01])
@pytest.mark.parametrize("L,k", [(12, 1), (20, 2)])
def test_segment_index(L, k, n_frac):
    """Every kernel boundary in one call (helpers.one_word_batch), seg_min = 500, under all 64 settings of the
    segment index's six switches: 32-bit compare keys, the LDS kernel and the lookups at L = 12, k = 1; 64-bit keys
    at L = 20, k = 2."""
    call = seg_call(L, k, n_frac)
    assert call.max_bucket >= 2000
    n_edges = set()
    with context(dict(seg_min=500)) as ctx:
        for bits in itertools.product((0, 1), repeat=len(SEG_OPTS)):
            for name, v in zip(SEG_OPTS, bits):
                ctx.set_option(name, v)
            st = check(call, ctx, "segment index L=%d k=%d N=%g %s" % (L, k, n_frac, dict(zip(SEG_OPTS, bits))))
            assert st["n_edges"] > 0 and st["n_rounds"] == 1
            n_edges.add(st["n_edges"])
    assert len(n_edges) == 1, n_edges  # (each pair within k once, united in place or listed)


PROBE_SHAPES = ("first_eligible", "dense", "duplicated", "with_n")


@pytest.mark.parametrize("shape", PROBE_SHAPES)
def test_lookup_path(shape):
    """tests/seg_probe_inputs.py: part-0 sub-buckets decided by bitmap lookups (seg_probe_min = 2 and the default),
    a key that is there twice (walked by tiles), N bases (not taken by lookups)."""
    b = getattr(sp, shape)()
    call = Call(b.keys, b.nm, b.fr, b.off, b.L, 1)
    with context() as ctx:
        for least in (2, 129):
            for probe in (1, 0):
                ctx.set_option("seg_probe", probe)
                ctx.set_option("seg_probe_min", least)
                st = check(call, ctx, "%s seg_probe=%d seg_probe_min=%d" % (shape, probe, least))
                assert st["n_edges"] > 0


def test_overflow_retry():
    """edge_capacity = 1: the list of the first attempt runs over (its floor is 1,024 entries), the pairs and the
    write-out run again with a list of the size that was counted."""
    call = tile_call(2, 0.0)
    for opts in (dict(seg_index=0, fused_max=0), dict(seg_unite=0, seg_min=500)):
        with context(dict(opts, edge_capacity=1)) as ctx:
            st = check(call, ctx, "edge_capacity 1 %s" % opts)
            assert st["n_edges"] > 1024
            check(fused_call(1, 0.0, False), ctx, "a fused call behind it")


# ---- 4. deep unions ------------------------------------------------------------------------------------------
LADDERS = [("sym", o) for o in ci.ORDERS] + [("step2", "forward"), ("comb", "forward")]


def chain_model(buckets):
    """A path is one component: its rank-0 entry survives.  The buckets between the paths: the model."""
    kept, root, at = [], [], 0
    for umis, freq, is_chain in buckets:
        r = np.zeros(len(umis), np.uint32) if is_chain else cm.components(hamming_matrix(umis), 1)
        root.append(r + at)
        at += len(umis)
    root = np.concatenate(root).astype(np.uint32)
    return cm.kept_of(root), root


@functools.lru_cache(maxsize=None)
def chain_call(n, alone):
    """Paths of n entries (1 apart along the path, everything else farther) in every order and ladder: 129 as
    wide keys of 43 bases, 513 and 769 as whole reads of 256."""
    L = 43 if n == 129 else 256
    chains = [ci.chain(lad, L, 1, o, n=n) for lad, o in LADDERS]
    assert all(c.n == n for c in chains)
    if alone:
        buckets = [(c.umis, c.freq, True) for c in chains]
    else:
        buckets = ko.interleave(chains, ko.randoms(n, L, sizes=(25, 10, 35, 20, 30, 15)))
    model = chain_model(buckets)
    if L == 43:
        keys, nm, fr, off = assemble(buckets, wide=True)
        return Call(keys, nm, fr, off, L, 1, "wide", model=model)
    keys, nm = sm.encode([u.encode() for b in buckets for u in b[0]], sm.words(L))
    _, _, fr, off = assemble([([], b[1]) for b in buckets])
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    return Call(keys, nm, fr, off, L, 1, "seqs", blen=[L] * len(buckets), model=model)


@pytest.mark.parametrize("alone", [True, False], ids=["alone", "interleaved"])
@pytest.mark.parametrize("n", [129, 513, 769])
def test_deep_unions(n, alone):
    """A path of n entries is one component whatever its order and freqs: exactly one survivor, its rank-0 entry.
    The reverse and zig-zag orders leave union-find trees as deep as the path for the write-out to climb."""
    call = chain_call(n, alone)
    assert int(call.kept.sum()) >= len(LADDERS) and all(call.kept[int(call.off[2 * i if not alone else i])] for i in range(len(LADDERS)))
    opt_sets = [dict(fused_max=0), dict(fused_max=0, seg_min=2)] if n == 129 else [{}]
    for opts in opt_sets:
        with context(opts) as ctx:
            st = check(call, ctx, "paths of %d %s" % (n, opts), stats=call.form != "seqs")
            assert st["n_edges"] >= len(LADDERS) * (n - 1)
            if alone:
                assert st["n_kept"] == len(LADDERS)


# ---- 5. wide keys, whole reads, edit distance ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wide_call(L):
    return Call(*wide_batch(L, 4), L, 4, "wide")


@pytest.mark.parametrize("L", [24, 43, 85])
def test_wide_keys(L):
    """helpers.wide_batch at k = 4: buckets of the fused range (all through the chunk kernel in this mode), one for
    the chunk kernel and one deep, N at the bases that straddle key words."""
    call = wide_call(L)
    for opts in ({}, dict(seg_min=129), dict(seg_index=0)):
        with context(opts) as ctx:
            st = check(call, ctx, "wide L=%d %s" % (L, opts))
            assert st["n_edges"] > 0 and st["n_kept"] < st["n_umis"]


@functools.lru_cache(maxsize=None)
def seq_call(L, k):
    buckets = seq_buckets(L, k)
    keys, nm = sm.encode([s for b in buckets for s in b[0]], sm.words(L))
    fr = np.array([f for b in buckets for f in b[1]], np.int32)
    off = np.cumsum([0] + [len(b[0]) for b in buckets]).astype(np.uint64)
    return Call(keys, nm, fr, off, L, k, "seqs", blen=[L] * len(buckets))


@pytest.mark.parametrize("L,k", [(100, 2), (256, 3)])
def test_whole_reads(L, k):
    """helpers.seq_buckets: a pair, a bucket evaluated by all pairs and one through the partition."""
    call = seq_call(L, k)
    with context() as ctx:
        st = check(call, ctx, "whole reads L=%d k=%d" % (L, k), stats=False)
        assert st["n_edges"] > 0 and st["n_kept"] < st["n_umis"]
        assert (st["n_buckets"], st["max_bucket"], st["n_pairs"]) == (call.n_buckets, call.max_bucket, call.n_pairs)


@functools.lru_cache(maxsize=None)
def edit_call(n_frac, k):
    buckets, mats, (keys, nm, fr, off) = em.batch(12, n_frac)
    return Call(keys, nm, fr, off, 12, k, "edit", model=cm.batch(mats, off, k))


@pytest.mark.parametrize("n_frac", [0.0, 0.05])
@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_edit_distance(k, n_frac):
    """umi_dedup_batch_edit against the model over edit_matrix; at k = 0 and 1 an indel cannot show between UMIs of
    one length, and the call equals the Hamming cluster call bit for bit."""
    call = edit_call(n_frac, k)
    with context() as ctx:
        st = check(call, ctx, "edit k=%d N=%g" % (k, n_frac))
        if k:
            assert st["n_edges"] > 0
        if k <= 1:
            for want_root in (True, False):
                kept, root, _ = call.run(ctx, want_root)
                hkept, hroot, _ = ctx.dedup_batch(call.keys, call.nmask, call.fr, call.off, 12, k, 0.5, CLUSTER, 0,
                                                  want_root=want_root)
                assert np.array_equal(kept, hkept) and (root is None or np.array_equal(root, hroot))
        else:
            hkept, _ = cm.batch_of_keys(call.keys, call.nm, call.off, k)
            assert not np.array_equal(hkept, call.kept)  # (the edit graph is another graph from k = 2 on)


# ---- 6. entry points ------------------------------------------------------------------------------------------
def dev(a):
    a = np.ascontiguousarray(a)
    return df.dev_t(a if a.size else np.zeros(1, a.dtype))


def back(t, n):
    return t.cpu().numpy().reshape(-1)[:n]


def device_run(call, form):
    """run(ctx, want_root, algo, p, amf) through a device-pointer entry point"""
    def run(ctx, want_root, algo, p, amf):
        import torch
        n = len(call.keys)
        t_keys, t_fr, t_off = dev(call.keys), dev(call.fr), dev(call.off)
        t_nm = dev(call.nmask) if call.nmask is not None else None
        kept = df.zeros(n, torch.uint8)
        root = df.zeros(n, torch.int32) if want_root else None
        a = (t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0, t_fr.data_ptr(), call.off, call.L,
             kept.data_ptr(), root.data_ptr() if want_root else 0)
        kw = dict(k=call.k, percentage=p, algo=algo, adj_max_freq=amf)
        if form == "device":
            st = ctx.dedup_batch_device(*a, **kw)
        elif form == "table":
            st = ctx.dedup_batch_device(*a, d_bucket_off=t_off.data_ptr(), **kw)
        elif form == "begin":
            ctx.dedup_batch_device_begin(*a, **kw)
            st = ctx.dedup_batch_end()
        elif form == "multi":
            st = ctx.dedup_batch_device_multi([dict(d_keys=a[0], d_nmask=a[1], d_freq=a[2], bucket_off=call.off,
                                                    d_kept=a[5], d_root=a[6])], call.L, (n + 7) // 8, gather=False, **kw)
        elif form == "edit":
            st = ctx.dedup_batch_edit_device(*a, **kw)
        else:
            raise ValueError(form)
        torch.cuda.synchronize()
        return back(kept, n), (back(root, n).view(np.uint32) if want_root else None), st
    return run


@functools.lru_cache(maxsize=None)
def deep_bucket_call():
    """fused buckets and one deep bucket (the segment index's) in one call"""
    rng = np.random.default_rng(8600)
    buckets = [clustered_bucket(rng, n, 12, 0.0) for n in (40, 128, 7, 1500, 90)]
    return Call(*assemble(buckets), 12, 1)


@pytest.mark.parametrize("form", ["device", "table", "begin"])
def test_device_entry_points_all_fused(form):
    """An all-fused batch through the device-pointer forms: each equals the plain call."""
    call = fused_call(1, 0.05, False)
    with context() as ctx:
        plain = check(call, ctx, "plain call")
        st = check(call, ctx, form, run=device_run(call, form))
        assert st["n_kept"] == plain["n_kept"] and st["n_edges"] == plain["n_edges"] == 0


def test_begin_end_around_another_call_on_an_all_fused_batch():
    """umi_dedup_batch_device_begin may leave the end of an all-fused call on the stream (the cluster path defers
    under the directional path's condition): another entry point called in between lets the pending call end and
    keeps its result for umi_dedup_batch_end, for both algorithms alike."""
    import torch
    call, other = fused_call(1, 0.0, False), fused_call(2, 0.0, False)
    with context() as ctx:
        for algo, p in ((DIR, INF), (CLUSTER, 0.5)):
            n = len(call.keys)
            t_keys, t_fr = dev(call.keys), dev(call.fr)
            kept, root = df.zeros(n, torch.uint8), df.zeros(n, torch.int32)
            ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_fr.data_ptr(), call.off, 12, kept.data_ptr(),
                                         root.data_ptr(), k=1, percentage=p, algo=algo)
            k2, r2, _ = other.run(ctx, True)  # (settles the pending call, keeps its result)
            assert np.array_equal(k2, other.kept) and np.array_equal(r2, other.root)
            st = ctx.dedup_batch_end()
            torch.cuda.synchronize()
            same("begin / end around another call, algo %d" % algo, back(kept, n), back(root, n).view(np.uint32), st,
                 call.kept, call.root)
            with pytest.raises(Exception):
                ctx.dedup_batch_end()  # (handed out once)


@pytest.mark.parametrize("form", ["device", "table", "begin", "multi"])
def test_device_entry_points_with_a_deep_bucket(form):
    call = deep_bucket_call()
    with context(None, [0] if form == "multi" else 0) as ctx:
        st = check(call, ctx, form + ", one deep bucket", run=device_run(call, form))
        assert st["n_edges"] > 0 and st["n_rounds"] == 1


def test_edit_device_entry_point():
    call = edit_call(0.05, 2)
    with context() as ctx:
        check(call, ctx, "dedup_batch_edit_device", run=device_run(call, "edit"))


def wide_seqs_device_run(call):
    def run(ctx, want_root, algo, p, amf):
        import torch
        from umi_collapse_rs_amd import _lib
        n = len(call.keys)
        t_keys, t_nm, t_fr = dev(call.keys), dev(call.nm), dev(call.fr)
        kept = df.zeros(n, torch.uint8)
        root = df.zeros(n, torch.int32) if want_root else None
        if call.form == "wide":
            st = ctx.dedup_batch_wide_device(t_keys.data_ptr(), t_nm.data_ptr() if call.nmask is not None else 0,
                                             call.keys.shape[1], t_fr.data_ptr(), call.off, call.L, kept.data_ptr(),
                                             root.data_ptr() if want_root else 0, k=call.k, percentage=p, algo=algo,
                                             adj_max_freq=amf)
        else:
            blen = np.array(call.blen, np.int32)
            stats = _lib.Stats()
            _lib.check(_lib.load().umi_dedup_seqs_device(
                ctx._h, t_keys.data_ptr(), t_nm.data_ptr(), call.keys.shape[1], t_fr.data_ptr(),
                _lib.ptr(call.off, C.c_uint64), _lib.ptr(blen, C.c_int32), len(blen), call.k, p, algo, amf, kept.data_ptr(),
                root.data_ptr() if want_root else None, None, C.byref(stats)))
            st = stats.as_dict()
        torch.cuda.synchronize()
        return back(kept, n), (back(root, n).view(np.uint32) if want_root else None), st
    return run


def test_wide_and_whole_read_device_entry_points():
    with context() as ctx:
        check(wide_call(43), ctx, "dedup_batch_wide_device", run=wide_seqs_device_run(wide_call(43)))
        check(seq_call(100, 2), ctx, "umi_dedup_seqs_device", run=wide_seqs_device_run(seq_call(100, 2)), stats=False)


@functools.lru_cache(maxsize=None)
def split_call():
    """one bucket of 3,000 entries that dominates the call, small buckets around it"""
    rng = np.random.default_rng(8700)
    buckets = [clustered_bucket(rng, n, 12, 0.0) for n in (30, 3000, 100, 64)]
    return Call(*assemble(buckets), 12, 1)


def test_multi_device_context():
    """Context([0, 0]): sharded by buckets, and -- split_min lowered -- the pairs of the giant bucket split over the
    devices, the flagged lists gathered on the first, one union pass and write-out there."""
    for call in (deep_bucket_call(), split_call()):
        with context(None, [0, 0]) as ctx:
            st = check(call, ctx, "Context([0, 0]) sharded")
            assert st["n_edges"] > 0
    call = split_call()
    with context(dict(split_min=2000), [0, 0]) as ctx:
        st = check(call, ctx, "Context([0, 0]) split")
        with context(None, [0, 0]) as sharded:
            _, _, st_sharded = call.run(sharded, True)
        # (the split switches the fused kernel off: the small buckets' pairs are in its lists)
        assert st["n_edges"] > st_sharded["n_edges"] > 0


def test_pairs_partial_then_collapse_edges():
    """umi_pairs_partial_device in two parts: every edge carries the flag; umi_collapse_edges_device over the two
    lists gives the plain call's result."""
    import torch
    call = deep_bucket_call()
    n = len(call.keys)
    with context() as ctx:
        t_keys, t_fr = dev(call.keys), dev(call.fr)
        parts = []
        for part in range(2):
            buf = df.zeros(1 << 18, torch.int64)
            ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), 0, t_fr.data_ptr(), call.off, 12, part, 2, buf.data_ptr(),
                                             1 << 18, k=1, percentage=0.5, algo=CLUSTER)
            assert ne > 0
            parts.append(buf[:ne].cpu().numpy().view(np.uint64))
        edges = np.concatenate(parts)
        src, dst = (edges & np.uint64(0xFFFFFFFF)).astype(np.int64), (edges >> np.uint64(32)).astype(np.int64)
        assert ((src >> 31) == 1).all(), "an edge without the flag"
        src &= 0x7FFFFFFF
        assert (src < dst).all() and len(set(zip(src.tolist(), dst.tolist()))) == len(edges)
        d = [cm.word_distance(call.keys[int(call.off[b]):int(call.off[b + 1])], None) for b in range(call.n_buckets)]
        assert len(edges) == sum(int(np.triu(m <= 1, 1).sum()) for m in d)  # (every pair within k, once)

        def run(ctx, want_root, algo, p, amf):
            t_e = dev(edges)
            kept = df.zeros(n, torch.uint8)
            root = df.zeros(n, torch.int32) if want_root else None
            st = ctx.collapse_edges_device(n, t_e.data_ptr(), len(edges), kept.data_ptr(),
                                           root.data_ptr() if want_root else 0, algo=algo)
            torch.cuda.synchronize()
            return back(kept, n), (back(root, n).view(np.uint32) if want_root else None), st
        check(call, ctx, "collapse_edges_device", run=run, directional=False, stats=False)


# ---- 7. arguments and errors ---------------------------------------------------------------------------------
def test_ignored_arguments():
    """percentage with any bit pattern and adj_max_freq take no part."""
    call = deep_bucket_call()
    with context() as ctx:
        for p in (0.5, 0.0, -1.0, INF, float("nan")):
            for amf in (0, 7, -1):
                for want_root in (True, False):
                    kept, root, st = call.run(ctx, want_root, CLUSTER, p, amf)
                    same("p=%r adj_max_freq=%d" % (p, amf), kept, root, st, call.kept, call.root)


def test_errors():
    """The bucket contract still holds (a rise of freq inside a bucket: UMI_ERR_ORDER, in a fused bucket and in a
    deep one); an algo beyond the three is UMI_ERR_ARG."""
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    call = deep_bucket_call()
    with context() as ctx:
        for at in (1, int(call.off[3]) + 700):
            fr = call.fr.copy()
            fr[at] = fr[at - 1] + 1
            with pytest.raises(umi.UmiHipError) as e:
                ctx.dedup_batch(call.keys, None, fr, call.off, 12, 1, 0.5, CLUSTER)
            assert e.value.code == _lib.UMI_ERR_ORDER
        fr = call.fr.copy()
        fr[-1] = 0
        with pytest.raises(umi.UmiHipError) as e:
            ctx.dedup_batch(call.keys, None, fr, call.off, 12, 1, 0.5, CLUSTER)
        assert e.value.code == _lib.UMI_ERR_ORDER
        for algo in (3, -1):
            with pytest.raises(umi.UmiHipError) as e:
                ctx.dedup_batch(call.keys, None, call.fr, call.off, 12, 1, 0.5, algo)
            assert e.value.code == _lib.UMI_ERR_ARG
        kept, root, st = call.run(ctx, True)  # (the context is whole)
        same("after the errors", kept, root, st, call.kept, call.root)


def test_freq_int32_max_on_every_path():
    """freq = INT32_MAX throughout, buckets for the fused kernel, the chunk kernel and the segment index: legal,
    and equal to the model (the oracle's directional mode at p = inf keeps everything here)."""
    base = tile_call(1, 0.0)
    small = fused_call(1, 0.0, True)
    keys = np.concatenate([small.keys, base.keys])
    fr = np.full(len(keys), INT32_MAX, np.int32)
    off = np.concatenate([small.off, base.off[1:] + small.off[-1]]).astype(np.uint64)
    call = Call(keys, np.zeros_like(keys), fr, off, 12, 1)
    okept, _, _ = orc.dedup_batch(keys, None, fr, off, 12, 1, INF, 0)
    assert okept.all() and not call.kept.all()
    for opts in ({}, dict(seg_index=0), dict(seg_unite=0)):
        with context(opts) as ctx:
            check(call, ctx, "freq INT32_MAX %s" % opts, directional=False)


# ---- 8. the old modes are what they were ----------------------------------------------------------------------
COUNTERS = ("n_umis", "n_buckets", "max_bucket", "n_kept", "n_pairs", "n_pairs_evaluated", "n_candidates", "n_edges",
            "n_pair_launches", "kernel_id")


@pytest.mark.parametrize("which", ["fused", "tiles", "segments"])
def test_unchanged_modes(which):
    """Directional and adjacency on three of the batches above: the oracle's kept and root and the counters that
    follow from the input, call after call; and the counters of every call equal to those of a second context that
    makes the same calls with cluster calls in between: the mode leaves no trace on the old paths.  (n_rounds is
    left out: a round's labels move in place, so how many rounds a directional call takes depends on the order
    its waves happen to run in -- 4 and 5 were seen for one call on the MI355X.)"""
    call = dict(fused=fused_call(1, 0.05, False), tiles=tile_call(1, 0.05), segments=seg_call(12, 1, 0.01))[which]
    opts = dict(seg_index=0) if which == "tiles" else {}
    with context(opts) as plain, context(opts) as mixed:
        for algo, p, amf in ((DIR, 0.5, 0), (DIR, 1.0, 0), (ADJ, 0.5, 0), (ADJ, 0.5, 2)):
            okept, oroot, _ = orc.dedup_batch(call.keys, call.nmask, call.fr, call.off, call.L, call.k, p, algo, amf)
            for i in range(3):
                seen = []
                for ctx in (plain, mixed):
                    kept, root, st = call.run(ctx, True, algo, p, amf)
                    same("algo %d p %g amf %d" % (algo, p, amf), kept, root, st, np.asarray(okept), np.asarray(oroot))
                    assert (st["n_umis"], st["n_buckets"], st["max_bucket"], st["n_pairs"]) == (
                        len(call.keys), call.n_buckets, call.max_bucket, call.n_pairs)
                    seen.append({f: st[f] for f in COUNTERS})
                    if ctx is mixed:
                        call.run(ctx, True)  # cluster calls in between
                        call.run(ctx, False)
                assert seen[0] == seen[1], (algo, p, amf, i, seen)


# ---- 9. the per-bucket path -----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [50, 700])
def test_cluster_class_over_hipnaive(n):
    """Cluster.apply over HipNaive (neighbour lists from the GPU) equals the model."""
    from umi_collapse_rs_amd import Cluster, ReadFreq
    rng = np.random.default_rng(8900 + n)
    umis, freq = clustered_bucket(rng, n, 10, 0.0)
    perm = rng.permutation(len(umis)).tolist()
    reads = {umis[i]: ReadFreq(i, freq[i]) for i in perm}
    ranked, _, _ = canonical([umis[i] for i in perm], [freq[i] for i in perm])
    root = cm.components(hamming_matrix(ranked), 1)
    exp = [reads[ranked[i]].read for i in np.nonzero(cm.kept_of(root))[0]]
    assert Cluster(k=1).apply(reads, None, 10) == exp
    assert len(exp) < len(umis)
