"""The lists umi_pairs_partial_device writes, whole: every part of a split downloaded, decoded and
concatenated must be, as a multiset, exactly the list of tests/pair_list_model.py -- every permitted pair
once over all parts, with its direction and flag, nothing else -- and its collapse
(umi_collapse_edges_device) the oracle's result.  The inputs and what makes them worth running are
checked without a GPU in tests/test_pair_list_model_cpu.py."""
from collections import Counter

import numpy as np
import pytest

import cluster_model
import oracle as orc
import pair_list_model as plm
from pair_list_model import ALGO_ADJACENCY, ALGO_CLUSTER, ALGO_DIRECTIONAL

pytestmark = pytest.mark.gpu

# (p, algo, adj_max_freq): directional at two percentages, adjacency as an edge list and as the reference
# wrote it (no pair at all), connected components
LISTS = ((0.5, ALGO_DIRECTIONAL, 0), (1.0, ALGO_DIRECTIONAL, 0), (0.5, ALGO_ADJACENCY, 2), (0.5, ALGO_ADJACENCY, 0),
         (0.5, ALGO_CLUSTER, 0))


class Device:
    """One input's arrays in device memory."""

    def __init__(self, inp):
        import torch
        self.torch, self.dev = torch, torch.device("cuda:0")
        self.inp, self.n = inp, len(inp.keys)
        self.keys = torch.from_numpy(inp.keys.view(np.int64)).to(self.dev)
        self.nm = torch.from_numpy(inp.nm.view(np.int64)).to(self.dev) if inp.nm.any() else None
        self.fr = torch.from_numpy(inp.fr).to(self.dev)
        self.cap = max(1024, sum(len(d) * (len(d) - 1) // 2 for _, d in inp.dist))  # every pair there is
        self.buf = torch.zeros(self.cap, dtype=torch.int64, device=self.dev)

    def parts(self, ctx, p, algo, amf, n_parts):
        """[int64 [m, 3] per part] of one split."""
        out = []
        for part in range(n_parts):
            ne, _ = ctx.pairs_partial_device(self.keys.data_ptr(), self.nm.data_ptr() if self.nm is not None else 0,
                                             self.fr.data_ptr(), self.inp.off, self.inp.L, part, n_parts,
                                             self.buf.data_ptr(), self.cap, k=self.inp.k, percentage=p, algo=algo,
                                             adj_max_freq=amf)
            out.append(plm.decode_edges(self.buf[:ne].cpu().numpy()))
        return out

    def collapse(self, ctx, edges, algo):
        torch = self.torch
        words = (edges[:, 0] | (edges[:, 2] << 31) | (edges[:, 1] << 32)).astype(np.int64)
        t = torch.from_numpy(words).to(self.dev)
        kept = torch.zeros(self.n, dtype=torch.uint8, device=self.dev)
        root = torch.zeros(self.n, dtype=torch.int32, device=self.dev)
        ctx.collapse_edges_device(self.n, t.data_ptr() if len(words) else 0, len(words), kept.data_ptr(), root.data_ptr(),
                                  algo=algo)
        torch.cuda.synchronize()
        return kept.cpu().numpy(), root.cpu().numpy().view(np.uint32)


def describe(inp, got, want):
    """The first few missing, extra and doubled edges of a list, with the distance of each."""
    g, w = Counter(map(tuple, got.tolist())), Counter(map(tuple, want.tolist()))

    def dist_of(e):
        for s, d in inp.dist:
            if s <= e[0] < s + len(d) and s <= e[1] < s + len(d):
                return int(d[e[0] - s, e[1] - s])
        return None  # (entries of two buckets, or none of the call's)

    def show(c):
        return ["%d->%d flag %d dist %s x%d" % (e[0], e[1], e[2], dist_of(e), m) for e, m in sorted(c.items())[:6]]
    doubled = Counter({e: m for e, m in g.items() if m > 1})
    return "%d listed, %d expected; missing %d %s; extra %d %s; doubled %d %s" % (
        len(got), len(want), sum((w - g).values()), show(w - g), sum((g - w).values()), show(g - w), len(doubled), show(doubled))


def check_lists(inp, ctx_for, lists=LISTS, splits=(2, 3)):
    """Every list of `lists` under every split: the parts' multiset is the model's, its collapse the oracle's.
    ctx_for(p, algo, amf, n_parts) is the context a split runs on."""
    dev = Device(inp)
    for p, algo, amf in lists:
        want = inp.edges(p, algo, amf)
        if algo == ALGO_CLUSTER:  # (no mode of the oracle's: the components' model of tests/cluster_model.py)
            okept, oroot = cluster_model.batch([d for _, d in inp.dist], inp.off, min(inp.k, plm.BATCH_MAX_K))
        else:
            okept, oroot, _ = orc.dedup_batch(inp.keys, inp.nm, inp.fr, inp.off, inp.L, inp.k, p, algo, amf)
        for n_parts in splits:
            ctx = ctx_for(p, algo, amf, n_parts)
            parts = dev.parts(ctx, p, algo, amf, n_parts)
            got = plm.sort_edges(np.concatenate(parts))
            assert np.array_equal(got, want), "%s p %g algo %d amf %d, %d parts %s: %s" % (
                inp.name, p, algo, amf, n_parts, [len(x) for x in parts], describe(inp, got, want))
            kept, root = dev.collapse(ctx, np.concatenate(parts), algo)
            assert np.array_equal(kept, okept) and np.array_equal(root, oroot), (inp.name, p, algo, amf, n_parts)
            if len(want) > 64 * n_parts and n_parts <= 3:
                assert sum(1 for x in parts if len(x)) >= 2, "the work was not split"


def run_case(name, opts=None, **kw):
    import umi_collapse_rs_amd as umi
    inp = plm.pair_input(name)
    ctx = umi.Context(0)
    try:
        for o, v in dict(inp.opts, **(opts or {})).items():
            ctx.set_option(o, v)
        check_lists(inp, lambda *a: ctx, **kw)
    finally:
        ctx.close()


CHUNK = [n for n in plm.PAIR_INPUTS if n.startswith("chunk_")]
SEG = [n for n in plm.PAIR_INPUTS if n.startswith("seg_")]


@pytest.mark.parametrize("name", CHUNK)
def test_chunk_kernel_lists(name):
    """Default options: buckets of 1 .. 300 entries are small tasks of the chunk kernel (32-bit filter keys at 12
    bases, 64-bit ones at 20); the bucket of 1,100 is the segment index's there (seg_min = 512, small_max = 1,024):
    test_chunk_kernel_second_column_tile sends it to the chunk kernel."""
    run_case(name)


@pytest.mark.parametrize("name", [n for n in CHUNK if "1100" in n])
def test_chunk_kernel_second_column_tile(name):
    """1,100 entries as small tasks: the chunk kernel's second tile of 1,024 columns."""
    run_case(name, plm.SECOND_TILE)


def test_more_parts_than_tasks():
    """Eight parts of a call whose largest bucket is five tasks: some parts list nothing, none lists twice."""
    run_case("chunk_sizes_L12_k2_N", splits=(8,))


def test_big_task_lists():
    """small_max = 0 without the segment index: a partial row tile of 2,048 rows, and two row tiles."""
    run_case("big_300_2100")


@pytest.mark.parametrize("blocks", [0, 1, 3])
@pytest.mark.parametrize("name", SEG)
def test_segment_index_lists(name, blocks):
    """seg_min = 129: every pair once, whichever parts' bins its entries share.  One persistent block does every
    flush itself and leaves the rest in its private slot; three share the tasks unevenly."""
    run_case(name, {"seg_blocks": blocks} if blocks else None)


@pytest.mark.parametrize("name,opt", [("seg_L12_k2_N", "seg_ckey"), ("seg_L12_k3", "seg_ckey"), ("seg_L20_k2_N", "seg_sliced"),
                                      ("seg_L12_k2", "seg_sliced"), ("seg_L18_k5_N", "seg_lds"), ("seg_L12_k1", "seg_lds")])
def test_segment_index_lists_with_an_option_off(name, opt):
    run_case(name, {opt: 0})


def test_dense_lists():
    """Every pair of 300 entries is within k = 8 = L: the blocks' stages run over, edges go to the list directly."""
    run_case("dense_L8_k8")


@pytest.mark.parametrize("name", ["growth_chunk", "growth_seg"])
def test_lists_that_outgrow_the_first_list(name):
    """A context told edge_capacity = 1 starts with a list of 1,024 entries and does the pair work again with a
    longer one: a fresh context for every split of the lists that are sure to outgrow it, one for the others."""
    import umi_collapse_rs_amd as umi
    inp = plm.pair_input(name)
    made = []

    def fresh(*_):
        ctx = umi.Context(0)
        made.append(ctx)
        for o, v in dict(inp.opts, edge_capacity=1).items():
            ctx.set_option(o, v)
        return ctx
    try:
        check_lists(inp, fresh, lists=plm.GROWTH_LISTS)
        shared = fresh()
        check_lists(inp, lambda *a: shared, lists=[x for x in LISTS if x not in plm.GROWTH_LISTS])
    finally:
        for ctx in made:
            ctx.close()
