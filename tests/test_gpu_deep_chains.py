"""Deep chains of permitted pairs on every collapse path.

Every other input of the suite is a shallow graph: random or clustered UMIs whose chains of one-way
pairs are two or three steps deep.  Here the permitted pairs of a bucket form one induced path
(tests/chain_inputs.py: 25 to 769 nodes, all symmetric / all one-way / alternating), so that the
collapse has to carry a label over up to 768 hops: the fused kernels' sweeps, the rounds along the
edge list and their continuation on the host, the segment index's unions, the wide and whole-read
pair kernels, the adjacency levels, the split path and the development build's hook / jump rounds.
Every call is compared with the oracle (whole reads: the numpy model of tests/seq_model.py) and, on
the chain buckets, with the closed form; the chains sit next to random buckets so that ranges and
mixed paths are in play."""
import contextlib
import functools

import numpy as np
import pytest

import chain_inputs as ci
import oracle as orc
import seq_model as sm
from helpers import canonical, legacy_mark, random_bucket

pytestmark = pytest.mark.gpu
SYM_FLAG = 1 << 31  # include/umihip.h: an edge is (src | flag << 31, dst), two uint32 in a uint64


@contextlib.contextmanager
def context(opts):
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        for name, v in opts.items():
            c.set_option(name, v)
        yield c
    finally:
        c.close()


def randoms(seed, L, n_frac=0.0, sizes=(25, 10, 35)):
    """Random buckets beside the chains; with these sizes none of them has more than 128 entries, so a
    fused kernel that takes the chains takes them too."""
    rng = np.random.default_rng(52000 + seed)
    return [canonical(*random_bucket(rng, n_mol, L, err=0.06, n_frac=n_frac))[:2] for n_mol in sizes]


class Call:
    """One call's input, its reference (computed once, read-only) and the closed form of its chains."""

    def __init__(self, form, L, k, p, chains, rnd, lengths=None):
        self.form, self.L, self.k, self.p = form, L, k, p
        # chain, random, chain, random, ...: ranges of both kinds next to each other
        self.buckets, self.chains = [], []
        rnd = list(rnd)
        for c in chains:
            self.buckets.append((c.umis, c.freq))
            self.chains.append(c)
            if rnd:
                self.buckets.append(rnd.pop(0))
                self.chains.append(None)
        for b in rnd:
            self.buckets.append(b)
            self.chains.append(None)
        self.umis, self.fr, self.off = ci.assemble(self.buckets)
        self.blen = lengths or [L] * len(self.buckets)
        if form == "one":
            self.keys, self.nm = orc.encode_keys(self.umis)
        elif form == "wide":
            self.keys, self.nm = orc.encode_keys_wide(self.umis)
        else:
            from umi_collapse_rs_amd import to_bitset_seq
            self.keys, self.nm = to_bitset_seq(self.umis, max(sm.words(x) for x in self.blen))
        self._ref = {}

    def reference(self, algo=0, amf=0):
        key = (algo, amf)
        if key not in self._ref:
            if self.form == "one":
                okept, oroot, _ = orc.dedup_batch(self.keys, self.nm, self.fr, self.off, self.L, self.k, self.p, algo, amf)
            elif self.form == "wide":
                okept, oroot, _ = orc.dedup_batch_wide(self.keys, self.nm, self.fr, self.off, self.L, self.k, self.p,
                                                       algo, amf)
            else:
                ent = [(u.encode(), int(f), 0) for u, f in zip(self.umis, self.fr)]
                okept, oroot = sm.dedup(ent, [int(x) for x in self.off], self.blen, self.k, algo, self.p, amf)
                okept, oroot = okept.astype(np.uint8), oroot.astype(np.uint32)
            ekept, eroot, known = ci.expected(self.buckets, self.chains, algo, amf)
            # the builder's closed form and the oracle agree before a kernel is asked
            assert np.array_equal(okept[known], ekept[known]) and np.array_equal(oroot[known], eroot[known])
            for a in (okept, oroot, ekept, eroot, known):
                a.setflags(write=False)
            self._ref[key] = (okept, oroot, ekept, eroot, known)
        return self._ref[key]

    def max_bucket(self):
        return int(np.diff(self.off.astype(np.int64)).max())

    def bucket_of(self, i):
        b = int(np.searchsorted(self.off, i, side="right")) - 1
        return "%s bucket %d, entry %d of %d" % (self.chains[b].name if self.chains[b] else "random", b,
                                                  i - int(self.off[b]), len(self.buckets[b][0]))

    def run(self, ctx, algo=0, amf=0):
        nm = self.nm if self.nm.any() else None
        if self.form == "one":
            return ctx.dedup_batch(self.keys, nm, self.fr, self.off, self.L, self.k, self.p, algo, amf)
        if self.form == "wide":
            return ctx.dedup_batch_wide(self.keys, nm, self.fr, self.off, self.L, self.k, self.p, algo, amf)
        return ctx.dedup_seqs(self.keys, self.nm, self.fr, self.off, self.blen, k=self.k, percentage=self.p,
                              algo=algo, adj_max_freq=amf)

    def verify(self, kept, root, n_kept, what, algo=0, amf=0):
        okept, oroot, ekept, eroot, known = self.reference(algo, amf)
        kept, root = np.asarray(kept).astype(np.uint8), np.asarray(root).astype(np.uint32)
        for name, got, exp in (("kept", kept, okept), ("root", root, oroot)):
            bad = np.nonzero(got != exp)[0]
            assert bad.size == 0, "%s: %s differs from the oracle at %d entries, first in %s (%d, oracle %d)" % (
                what, name, bad.size, self.bucket_of(int(bad[0])), got[bad[0]], exp[bad[0]])
        assert np.array_equal(kept[known], ekept[known]) and np.array_equal(root[known], eroot[known]), what
        assert n_kept == int(okept.sum()), (what, n_kept, int(okept.sum()))

    def check(self, ctx, what, algo=0, amf=0):
        kept, root, st = self.run(ctx, algo, amf)
        self.verify(kept, root, st["n_kept"], what, algo, amf)
        return st


SYM4 = [("sym", o) for o in ci.ORDERS]


@functools.lru_cache(maxsize=None)
def one_word_calls(L, stride, n_frac=0.0):
    """The two calls of one path: p = 0.5 (sym in four orders, halving) and p = 1.0 (step2, comb, sym
    zig-zag), random buckets in between (with n_frac: N bases in those)."""
    half = [ci.chain(lad, L, stride, o) for lad, o in SYM4 + [("halving", "forward")]]
    one = [ci.chain(lad, L, stride, o) for lad, o in (("step2", "forward"), ("comb", "forward"), ("sym", "zigzag"))]
    return (Call("one", L, stride, 0.5, half, randoms(L + stride, L, n_frac)),
            Call("one", L, stride, 1.0, one, randoms(100 + L + stride, L, n_frac)))


@functools.lru_cache(maxsize=None)
def wide_calls(L):
    half = [ci.chain(lad, L, 1, o) for lad, o in SYM4 + [("halving", "forward")]]
    one = [ci.chain(lad, L, 1, o) for lad, o in (("step2", "forward"), ("comb", "forward"), ("sym", "zigzag"))]
    return (Call("wide", L, 1, 0.5, half, randoms(200 + L, L, 0.004)),
            Call("wide", L, 1, 1.0, one, randoms(300 + L, L)))


@functools.lru_cache(maxsize=None)
def seq_calls(lengths):
    """Whole reads: per length sym forward / zig-zag at p = 0.5, and step2, comb, sym zig-zag at p = 1.0."""
    out = []
    for p, which in ((0.5, (("sym", "forward"), ("sym", "zigzag"))),
                     (1.0, (("step2", "forward"), ("comb", "forward"), ("sym", "zigzag")))):
        chains = [ci.chain(lad, L, 1, o) for L in lengths for lad, o in which]
        c = Call("seq", max(lengths), 1, p, chains, [], lengths=[len(ch.umis[0]) for ch in chains])
        out.append(c)
    return tuple(out)


PATHS = [(21, 1), (8, 1), (21, 4), (8, 4)]  # 64, 25, 16 and 7 nodes; k = 4 is above the sliced body's k <= 3


# ---- fused one-wave kernels ---------------------------------------------------------------------------
@pytest.mark.parametrize("sliced", [0, 1])
@pytest.mark.parametrize("L,stride", PATHS)
def test_fused(L, stride, sliced):
    """Up to 64 nodes in one wave: the sweeps of the fused bodies go on while a label moves (63 hops
    against the rank order on the zig-zag and the reverse order)."""
    with context({"fused_sliced": sliced}) as ctx:
        for call in one_word_calls(L, stride):
            st = call.check(ctx, "fused L=%d k=%d sliced=%d p=%g" % (L, stride, sliced, call.p))
            assert call.max_bucket() <= 128  # every bucket is the fused kernel's: nothing reaches the list
            assert st["n_edges"] == 0 and st["n_rounds"] == 0


@pytest.mark.parametrize("sliced", [0, 1])
def test_fused_with_n_elsewhere(sliced):
    """N bases in the random buckets of the call: the N variant of the fused kernel takes the chains too."""
    with context({"fused_sliced": sliced}) as ctx:
        for call in one_word_calls(21, 1, 0.03):
            assert call.nm.any() and call.max_bucket() <= 128
            st = call.check(ctx, "fused with N sliced=%d p=%g" % (sliced, call.p))
            assert st["n_edges"] == 0 and st["n_rounds"] == 0


# ---- the edge list and its rounds ------------------------------------------------------------------------
SEG_OPTS = [dict(fused_max=0, seg_min=2, seg_unite=a, seg_local=b, seg_lds=c, seg_ckey=d)
            for a in (0, 1) for b in (0, 1) for c in (0, 1) for d in (0, 1)]
LIST_OPTS = [dict(fused_max=0), dict(fused_max=0, spin_wait=0), dict(fused_max=0, spin_wait=1),
             dict(fused_max=0, seg_min=2, spin_wait=0)] + SEG_OPTS


def _ident(o):
    return "-".join("%s%d" % (k.replace("fused_max", "fm").replace("seg_", "").replace("spin_wait", "spin"), v)
                    for k, v in o.items())


@pytest.mark.parametrize("opts", LIST_OPTS, ids=_ident)
@pytest.mark.parametrize("L,stride", PATHS)
def test_list_path(L, stride, opts):
    """The same buckets with the fused kernel off: the chunk kernel (seg_min = 2: the segment index where
    its parts apply) feeds the edge list, the symmetric pairs are united, the one-way pairs walked in
    rounds.  The p = 1.0 call holds the step2 ladder: a chain of n - 1 one-way pairs."""
    with context(opts) as ctx:
        for call in one_word_calls(L, stride):
            st = call.check(ctx, "list L=%d k=%d %s p=%g" % (L, stride, opts, call.p))
            assert st["n_edges"] > 0 and st["n_rounds"] >= 2


def test_step2_rounds_beyond_the_first_look():
    """The 64-node step2 ladder on the list path (fused_max = 0): 63 one-way pairs in a row.  The host's
    first look covers the union pass and DAG_ROUNDS = 3 rounds on a fresh context, 1 + 16 on one that has
    seen a deep call; n_rounds beyond 17 means that run_one_sync's continuation (run_rounds in batches of
    4, 8, 16, 16, ..., the CNT_KEPT reset, the second finalize) ran, on either kind of context.

    Measured on the MI355X in five fresh processes, first call on a fresh context / second call on the
    same context: 66 / 66, 66 / 66, 66 / 66, 66 / 66, 66 / 66 (the ladder alone in a call: 66 as well).
    All exceed 17, so the continuation is shown to run and that is asserted; the count itself (here
    about one hop per round: 66 for the union pass and 63 hops) depends on how the waves of
    one_way_round interleave and is not."""
    call = one_word_calls(21, 1)[1]
    with context(dict(fused_max=0)) as ctx:
        st = call.check(ctx, "step2, 64 nodes, list path")
        assert st["n_rounds"] > 17
        st = call.check(ctx, "step2, 64 nodes, list path, second call (16 rounds ahead)")
        assert st["n_rounds"] > 17


# ---- keys of several words -------------------------------------------------------------------------------
@pytest.mark.parametrize("L,opts", [(85, {}), (30, {}), (85, dict(seg_min=129)), (30, dict(fused_max=0))],
                         ids=["L85", "L30-fused", "L85-seg129", "L30-list"])
def test_wide(L, opts):
    """256 nodes of 85 bases (above the fused kernel's 128 entries: the wide pair kernel, with seg_min = 129
    the segment index over the first word) and 91 nodes of 30 bases (the fused wide kernel)."""
    with context(opts) as ctx:
        for call in wide_calls(L):
            st = call.check(ctx, "wide L=%d %s p=%g" % (L, opts, call.p))
            if L == 85 or opts:
                assert st["n_edges"] > 0 and st["n_rounds"] >= 2
            else:  # 91 nodes and random buckets of at most 128 entries: the fused wide kernel's, all of them
                assert call.max_bucket() <= 128
                assert st["n_edges"] == 0 and st["n_rounds"] == 0


# ---- whole reads -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("lengths", [(256,), (100,), (256, 100)], ids=["L256", "L100", "both"])
def test_seqs(lengths):
    """769 nodes of 256 bases (above the cut of 512 entries: the partitioned pair kernel) and 301 nodes of
    100 bases, alone and as buckets of one call."""
    with context({}) as ctx:
        for call in seq_calls(lengths):
            st = call.check(ctx, "seqs %s p=%g" % (lengths, call.p))
            assert st["n_edges"] > 0


# ---- adjacency ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def adjacency_call(form, L):
    chains = [ci.chain("sym", L, 1, o) for o in ci.ORDERS]
    return Call(form, L, 1, 0.5, chains, randoms(400 + L, L, sizes=(30, 12)))


@pytest.mark.parametrize("form,L,opts", [("one", 21, {}), ("one", 21, dict(fused_max=0)), ("one", 8, {}),
                                         ("one", 21, dict(fused_max=0, seg_min=2)), ("wide", 85, {})],
                         ids=["fused", "list", "fused-L8", "seg", "wide"])
def test_adjacency(form, L, opts):
    """adj_max_freq = 1 over all-freq-1 paths: n / 2 decision levels (collapse_adjacency settles one per
    iteration; the fused kernel walks the roots in rank order); adj_max_freq = 0 removes nothing."""
    call = adjacency_call(form, L)
    with context(opts) as ctx:
        for amf in (1, 0):
            call.check(ctx, "adjacency %s L=%d %s amf=%d" % (form, L, opts, amf), algo=1, amf=amf)


# ---- the split path ----------------------------------------------------------------------------------------
def collapse_list(ctx, n, parts, algo):
    import torch
    dev = torch.device("cuda:0")
    edges = torch.cat(parts) if parts else torch.zeros(0, dtype=torch.int64, device=dev)
    t_kept = torch.zeros(n, dtype=torch.uint8, device=dev)
    t_root = torch.zeros(n, dtype=torch.int32, device=dev)
    st = ctx.collapse_edges_device(n, edges.data_ptr() if len(edges) else 0, len(edges), t_kept.data_ptr(),
                                   t_root.data_ptr(), algo=algo)
    torch.cuda.synchronize()
    return t_kept.cpu().numpy(), t_root.cpu().numpy().view(np.uint32), st


def run_split(ctx, call, algo, amf, n_parts=2, cap=1 << 16):
    """As tests/test_gpu_split.py: the parts one after the other, their lists concatenated, one collapse."""
    import torch
    dev = torch.device("cuda:0")
    t_keys = torch.from_numpy(call.keys.view(np.int64)).to(dev)
    t_nm = torch.from_numpy(call.nm.view(np.int64)).to(dev) if call.nm.any() else None
    t_fr = torch.from_numpy(call.fr).to(dev)
    parts = []
    for part in range(n_parts):
        buf = torch.zeros(cap, dtype=torch.int64, device=dev)
        ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), t_nm.data_ptr() if t_nm is not None else 0,
                                         t_fr.data_ptr(), call.off, call.L, part, n_parts, buf.data_ptr(), cap,
                                         k=call.k, percentage=call.p, algo=algo, adj_max_freq=amf)
        parts.append(buf[:ne].clone())
    return collapse_list(ctx, len(call.keys), parts, algo) + ([len(x) for x in parts],)


@pytest.mark.parametrize("algo,amf", [(0, 0), (1, 200)], ids=["directional", "adjacency"])
def test_split_64_nodes(algo, amf):
    """pairs_partial_device in two parts on the step2 and comb ladders (64 nodes, 63 hops), the lists
    concatenated, collapse_edges_device: directional_labels' rounds (batches of 3, 6, 12, 16, ...) and
    the adjacency levels."""
    call = one_word_calls(21, 1)[1]
    with context({}) as ctx:
        kept, root, st, counts = run_split(ctx, call, algo, amf)
        call.verify(kept, root, st["n_kept"], "split algo=%d" % algo, algo, amf)
        assert sum(counts) > 0


def model_edges(call, algo, amf):
    """The edge list of a call from the definition, in the documented layout (include/umihip.h)."""
    out = []
    for b in range(len(call.buckets)):
        lo = int(call.off[b])
        umis, freq = call.buckets[b]
        d = ci.distances(umis)
        thr = [ci.thr_f32(call.p, f) for f in freq]
        for i, j in zip(*np.nonzero(np.triu(d <= call.k, 1))):
            i, j = int(i), int(j)
            if algo == 0:
                fwd, bwd = freq[j] <= thr[i], freq[i] <= thr[j]
            else:
                fwd, bwd = freq[j] <= amf, False
            if fwd and bwd:
                out.append((lo + i) | SYM_FLAG | (lo + j) << 32)
            elif fwd:
                out.append((lo + i) | (lo + j) << 32)
            elif bwd:
                out.append((lo + j) | (lo + i) << 32)
    return np.array(out, np.uint64)


@pytest.mark.parametrize("algo,amf", [(0, 0), (1, 600)], ids=["directional", "adjacency"])
def test_split_collapse_256_nodes(algo, amf):
    """collapse_edges_device 255 hops deep.  pairs_partial_device takes keys of one word (21 bases: a path
    of 64 nodes at most), so the lists of the 256-node ladders over 85 bases are written here from the
    definition, as two parts (every other edge) concatenated."""
    import torch
    call = wide_calls(85)[1]
    edges = model_edges(call, algo, amf)
    dev = torch.device("cuda:0")
    parts = [torch.from_numpy(np.ascontiguousarray(edges[h::2]).view(np.int64)).to(dev) for h in (0, 1)]
    with context({}) as ctx:
        kept, root, st = collapse_list(ctx, len(call.keys), parts, algo)
        call.verify(kept, root, st["n_kept"], "edge list of 256-node ladders algo=%d" % algo, algo, amf)


# ---- one context, deep / shallow / deep ----------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def shallow_call():
    return Call("one", 21, 1, 0.5, [], randoms(900, 21, sizes=(60, 25, 8, 40)))


@functools.lru_cache(maxsize=None)
def many_chains(ladder, n_buckets):
    ch = ci.chain(ladder, 21, 1)
    return Call("one", 21, 1, ch.p, [ch] * n_buckets, randoms(700, 21, sizes=(30, 12)))


@pytest.mark.parametrize("opts", [{}, dict(fused_max=0), dict(fused_max=0, seg_min=2)], ids=_ident)
def test_deep_shallow_deep(opts):
    """ctx->dag_rounds_ahead is carried from call to call: a shallow call after a deep one enqueues 15
    rounds and checks with the 16th; then a deep one again (the halving ladder, top freq 2^30)."""
    deep1, deep2 = one_word_calls(21, 1)[1], one_word_calls(21, 1)[0]
    with context(opts) as ctx:
        for i, call in enumerate((deep1, shallow_call(), deep2, shallow_call(), deep1)):
            call.check(ctx, "call %d of deep / shallow / deep / shallow / deep %s" % (i, opts))


def test_deep_chains_behind_the_overflow_retry():
    """40 buckets of 64-node step2 ladders with fused_max = 0 and edge_capacity = 1: about 2,500 one-way
    pairs against the list's floor of 1,024 entries, so the first attempt runs over and pairs and collapse
    are enqueued again with a deep chain behind them; then a shallow call and 40 halving ladders on the
    same context."""
    with context(dict(fused_max=0, edge_capacity=1)) as ctx:
        call = many_chains("step2", 40)
        st = call.check(ctx, "40 step2 ladders, edge_capacity 1")
        assert st["n_edges"] > 1024
        shallow_call().check(ctx, "shallow call after the overflow")
        many_chains("halving", 40).check(ctx, "40 halving ladders after the overflow")
        call.check(ctx, "40 step2 ladders again")


# ---- the deferred call ---------------------------------------------------------------------------------------
def test_deferred_all_fused_zigzag():
    """dedup_batch_device_begin / end on a call the fused kernel finishes alone: 64-node sym chains in
    zig-zag order (63 sweeps each), the result read after end."""
    import torch
    ch = ci.chain("sym", 21, 1, "zigzag")
    call = Call("one", 21, 1, 0.5, [ch] * 48, randoms(800, 21, sizes=(30, 12)))
    dev = torch.device("cuda:0")
    t_keys = torch.from_numpy(call.keys.view(np.int64)).to(dev)
    t_fr = torch.from_numpy(call.fr).to(dev)
    t_kept = torch.zeros(len(call.keys), dtype=torch.uint8, device=dev)
    t_root = torch.zeros(len(call.keys), dtype=torch.int32, device=dev)
    assert not call.nm.any() and call.max_bucket() <= 128
    with context({}) as ctx:
        for _ in range(2):  # (the second begin finds the first one's workspace)
            ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_fr.data_ptr(), call.off, 21, t_kept.data_ptr(),
                                         t_root.data_ptr(), k=1, percentage=0.5)
            st = ctx.dedup_batch_end()
            torch.cuda.synchronize()
            call.verify(t_kept.cpu().numpy(), t_root.cpu().numpy().view(np.uint32), st["n_kept"], "deferred")
            assert st["n_edges"] == 0
            t_kept.zero_()
            t_root.zero_()


# ---- the collapse variants of the development build ------------------------------------------------------------
@pytest.mark.parametrize("tp", [pytest.param(tp, marks=legacy_mark()) for tp in (0, 1, 2)])
def test_two_phase_variants(tp):
    """two_phase 0 (plain label propagation), 1 (hook / jump rounds: one launch per halving of the longest
    chain) and 2 (union-find, the shipped path, here chosen by the option) on the 64-node ladders with
    fused_max = 0.  The option exists in the development build only; the shipped path at the same
    shapes is test_list_path."""
    with context(dict(fused_max=0, two_phase=tp)) as ctx:
        for call in one_word_calls(21, 1):
            st = call.check(ctx, "two_phase=%d p=%g" % (tp, call.p))
            assert st["n_edges"] > 0 and st["n_rounds"] >= 2
