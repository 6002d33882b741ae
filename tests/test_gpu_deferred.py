"""The device-pointer call in two halves (umi_dedup_batch_device_begin / umi_dedup_batch_end) with
every other entry point called while the first half is still out, and the device-pointer forms
that the suite otherwise reaches only through their host wrappers.

include/umihip.h promises: any other call that needs the context's workspace first lets the pending
call end, whose result then waits for umi_dedup_batch_end (a second begin replaces it); d_kept /
d_root of the pending call are final in stream order.  Each intervening call X here gets inputs of
its own and is checked against its own reference, on the pending call's stream and on another one;
the pending call's outputs, stats and contract verdict are checked after end.

Also here: one context taken through every family of host-buffer calls at changing sizes, each result
compared with the same call on a context of its own."""
import ctypes as C

import numpy as np
import pytest

import oracle as orc
import seq_model as sm
from helpers import grouped_stage_model, random_bucket

pytestmark = pytest.mark.gpu

L = 12
ACGTN = np.frombuffer(b"ACGTN", np.uint8)


# ---- inputs --------------------------------------------------------------------------------------

def dense_ids(pos):
    """alignment keys -> ids numbered by first appearance (what orc.stage_reads takes)"""
    _, first, inv = np.unique(pos, return_index=True, return_inverse=True)
    rank = np.empty(len(first), np.int64)
    rank[np.argsort(first, kind="stable")] = np.arange(len(first))
    return rank[inv.reshape(-1)].astype(np.uint32)


def gen_reads(rng, n, n_pos, umi_len, n_pool=64, err=0.02, n_frac=0.0, sort=False):
    """n reads at n_pos positions; UMIs from a pool of n_pool molecules with base errors (and N bases)"""
    pos = rng.integers(0, n_pos, n)
    if sort:
        pos = np.sort(pos)
    pool = rng.integers(0, 4, (n_pool, umi_len))
    bases = pool[rng.integers(0, n_pool, n)]
    flip = rng.random(bases.shape) < err
    bases[flip] = rng.integers(0, 4, int(flip.sum()))
    if n_frac:
        bases[rng.random(bases.shape) < n_frac] = 4
    umis = ACGTN[bases].reshape(-1)
    score = rng.integers(0, 60, n).astype(np.int32)
    return pos.astype(np.uint64), umis, score


def staged(rng, n, n_pos, **kw):
    """a batch in the batched path's canonical order, staged by the oracle"""
    pos, umis, score = gen_reads(rng, n, n_pos, L, **kw)
    st = orc.stage_reads(dense_ids(pos), umis, score, L, 1)
    return st["keys"], st["nmask"], st["freq"], st["bucket_off"]


def with_deep(small, rng, n_deep):
    """small positions and one deep one (more than the fused kernel takes: the host decides there)"""
    pos, umis, score = gen_reads(rng, n_deep, 1, L, n_pool=400, err=0.03)
    d = orc.stage_reads(dense_ids(pos), umis, score, L, 1)
    keys, nm, fr, off = small
    return (np.concatenate([keys, d["keys"]]), np.concatenate([nm, d["nmask"]]), np.concatenate([fr, d["freq"]]),
            np.concatenate([off, off[-1] + d["bucket_off"][1:]]).astype(np.uint64))


@pytest.fixture(scope="module")
def batches():
    rng = np.random.default_rng(2611)
    a = staged(rng, 75000, 3000, n_frac=0.002, sort=True)  # A: ~3,000 positions of a few tens of entries
    x = with_deep(staged(rng, 8000, 800), rng, 1500)       # X: smaller, one position beyond the fused kernel
    big = with_deep(staged(rng, 300000, 9000), rng, 6000)   # X larger than A: the workspace grows while A is out
    return dict(a=a, x=x, big=big)


@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def dev_t(a):
    import torch
    a = np.ascontiguousarray(a)
    if a.dtype == np.uint64:
        a = a.view(np.int64)
    elif a.dtype == np.uint32:
        a = a.view(np.int32)
    return torch.from_numpy(a.copy()).to("cuda:0")


def zeros(n, dtype):
    import torch
    return torch.zeros(max(1, n), dtype=dtype, device="cuda:0")


def ready(s):
    """stream s (None: the NULL stream) waits for what the default stream has enqueued (the uploads):
    an event wait, not a wait of the host -- a pending call keeps running meanwhile"""
    import torch
    if s is not None:
        s.wait_stream(torch.cuda.default_stream())


def read_back(t, stream):
    """the tensor on the host through a copy enqueued on `stream` (a torch stream, or None for the NULL
    stream): stream-ordered, nothing else waited for"""
    import torch
    with torch.cuda.stream(stream if stream is not None else torch.cuda.default_stream()):
        return t.cpu().numpy()


class Pending:
    """A: the deferred call, begun on stream sA (its inputs on the device, its outputs zeroed)"""

    def __init__(self, ctx, batch, stream, bad=False):
        import torch
        keys, nm, fr, off = batch
        n_b = np.diff(off.astype(np.int64))
        assert n_b.max() <= 128 and len(n_b) >= 1000  # every position the fused kernel's: begin returns early
        self.batch, self.stream = batch, stream
        if bad:  # a rise in freq inside the first bucket of two or more entries: UMI_ERR_ORDER at end
            fr = fr.copy()
            b = int(np.nonzero(n_b >= 2)[0][0])
            fr[int(off[b])], fr[int(off[b]) + 1] = 1, 5
        self.t = [dev_t(keys), dev_t(nm), dev_t(fr), dev_t(off)]
        self.kept = zeros(len(keys), torch.uint8)
        self.root = zeros(len(keys), torch.int32)
        ready(stream)
        ctx.dedup_batch_device_begin(self.t[0].data_ptr(), self.t[1].data_ptr(), self.t[2].data_ptr(), off, L,
                                     self.kept.data_ptr(), self.root.data_ptr(), k=1, stream=stream.cuda_stream,
                                     d_bucket_off=self.t[3].data_ptr())

    def check_outputs(self):
        keys, nm, fr, off = self.batch
        okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
        kept = read_back(self.kept, self.stream)[:len(keys)]
        root = read_back(self.root, self.stream)[:len(keys)].view(np.uint32)
        assert (kept == okept).all(), np.nonzero(kept != okept)[0][:10]
        assert (root == oroot).all(), np.nonzero(root != oroot)[0][:10]
        return int(okept.sum())

    def end_and_check(self, ctx):
        import umi_collapse_rs_amd as umi
        st = ctx.dedup_batch_end()
        n_kept = self.check_outputs()
        assert st["n_kept"] == n_kept and st["n_umis"] == len(self.batch[0])
        with pytest.raises(umi.UmiHipError):
            ctx.dedup_batch_end()  # (handed out: nothing is out now)


# ---- the intervening calls: each runs on `s` (a torch stream, or None: the NULL stream) and checks
#      its own result against its own reference --------------------------------------------------

def x_dedup_batch(ctx, b, s):
    keys, nm, fr, off = b["x"]
    kept, root, st = ctx.dedup_batch(keys, nm, fr, off, L, k=1)
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
    assert (kept == okept).all() and (root == oroot).all() and st["n_kept"] == int(okept.sum())


def _dedup_device(ctx, batch, s, table):
    import torch
    keys, nm, fr, off = batch
    t_keys, t_nm, t_fr, t_off = dev_t(keys), dev_t(nm), dev_t(fr), dev_t(off)
    kept, root = zeros(len(keys), torch.uint8), zeros(len(keys), torch.int32)
    ready(s)
    st = ctx.dedup_batch_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(), off, L, kept.data_ptr(),
                                root.data_ptr(), k=1, stream=s.cuda_stream if s is not None else 0,
                                d_bucket_off=t_off.data_ptr() if table else 0)
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
    assert (read_back(kept, s)[:len(keys)] == okept).all()
    assert (read_back(root, s)[:len(keys)].view(np.uint32) == oroot).all()
    assert st["n_kept"] == int(okept.sum()) and st["n_umis"] == len(keys)


def x_dedup_batch_device(ctx, b, s):
    _dedup_device(ctx, b["x"], s, table=False)


def x_dedup_batch_device_table(ctx, b, s):
    _dedup_device(ctx, b["x"], s, table=True)


def wide_batch(seed, umi_len, n_buckets=120, n_mol_max=12):
    rng = np.random.default_rng(seed)
    keys, nm, fr, off = [], [], [], [0]
    for i in range(n_buckets):
        umis, freq = random_bucket(rng, 400 if i == 0 else int(rng.integers(1, n_mol_max + 1)), umi_len, err=0.02,
                                   n_frac=0.002)
        order = sorted(range(len(umis)), key=lambda j: (-freq[j], j))
        umis, freq = [umis[j] for j in order], [freq[j] for j in order]
        k, m = orc.encode_keys_wide(umis)
        keys.append(k); nm.append(m); fr.extend(freq); off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


def _dedup_wide(ctx, s, umi_len, device):
    import torch
    keys, nm, fr, off = wide_batch(umi_len, umi_len)
    okept, oroot, _ = orc.dedup_batch_wide(keys, nm, fr, off, umi_len, 1)
    if not device:
        kept, root, st = ctx.dedup_batch_wide(keys, nm, fr, off, umi_len, k=1)
    else:
        t_keys, t_nm, t_fr = dev_t(keys), dev_t(nm), dev_t(fr)
        t_kept, t_root = zeros(len(keys), torch.uint8), zeros(len(keys), torch.int32)
        ready(s)
        st = ctx.dedup_batch_wide_device(t_keys.data_ptr(), t_nm.data_ptr(), keys.shape[1], t_fr.data_ptr(), off,
                                         umi_len, t_kept.data_ptr(), t_root.data_ptr(), k=1,
                                         stream=s.cuda_stream if s is not None else 0)
        kept, root = read_back(t_kept, s)[:len(keys)], read_back(t_root, s)[:len(keys)].view(np.uint32)
    assert (kept == okept).all() and (root == oroot).all() and st["n_kept"] == int(okept.sum())


def x_dedup_batch_wide_22(ctx, b, s):
    _dedup_wide(ctx, s, 22, False)


def x_dedup_batch_wide_85(ctx, b, s):
    _dedup_wide(ctx, s, 85, False)


def x_dedup_batch_wide_device_22(ctx, b, s):
    _dedup_wide(ctx, s, 22, True)


def x_dedup_batch_wide_device_85(ctx, b, s):
    _dedup_wide(ctx, s, 85, True)


def seq_input(seed):
    from umi_collapse_rs_amd import synth
    seqs, quals = synth.fastq_reads(seed, 1500, 500, lengths=[30, 100, 151], err=0.01, n_frac=0.002)
    return seqs, quals


def _dedup_seqs(ctx, s, device):
    import torch
    from umi_collapse_rs_amd import _lib
    seqs, quals = seq_input(31)
    ent, off, blen = sm.stage(seqs, quals, 1)
    w = max(sm.words(x) for x in blen)
    keys, nm = sm.encode([e[0] for e in ent], w)
    fr = np.array([e[1] for e in ent], np.int32)
    off, blen = np.array(off, np.uint64), np.array(blen, np.int32)
    okept, oroot = sm.dedup(ent, list(off), list(blen), 1)
    if not device:
        kept, root, st = ctx.dedup_seqs(keys, nm, fr, off, blen, k=1)
    else:
        t_keys, t_nm, t_fr = dev_t(keys), dev_t(nm), dev_t(fr)
        t_kept, t_root = zeros(len(ent), torch.uint8), zeros(len(ent), torch.int32)
        ready(s)
        stats = _lib.Stats()
        _lib.check(_lib.load().umi_dedup_seqs_device(
            ctx._h, t_keys.data_ptr(), t_nm.data_ptr(), w, t_fr.data_ptr(), _lib.ptr(off, C.c_uint64),
            _lib.ptr(blen, C.c_int32), len(blen), 1, 0.5, 0, 0, t_kept.data_ptr(), t_root.data_ptr(),
            s.cuda_stream if s is not None else None, C.byref(stats)))
        st = stats.as_dict()
        kept, root = read_back(t_kept, s)[:len(ent)], read_back(t_root, s)[:len(ent)].view(np.uint32)
    assert (kept == okept).all() and (root == oroot).all() and st["n_kept"] == int(okept.sum())


def x_dedup_seqs(ctx, b, s):
    _dedup_seqs(ctx, s, False)


def x_dedup_seqs_device(ctx, b, s):
    _dedup_seqs(ctx, s, True)


def same(got, exp):
    for f in ("keys", "nmask", "freq", "rep", "bucket_off"):
        a, e = np.asarray(got[f]), np.asarray(exp[f])
        assert a.shape == e.shape and (a.astype(np.uint64) == e.astype(np.uint64)).all(), f


def stage_device(ctx, form, align, group, umis, score, umi_len, s, abits=64, gbits=0, shift=0, nmask=True,
                 merge=1):
    """one of the four device forms of the read staging on the caller's stream `s`: the UMI text `shift`
    bytes past a 4-byte boundary, d_score / d_nmask NULL where score / nmask is None / False; the outputs
    read behind the call through stream-ordered copies only.  Guard words behind every output's capacity
    must come back untouched."""
    import torch
    from umi_collapse_rs_amd import _lib
    n = len(align)
    w = (3 * umi_len + 63) // 64 if form in ("wide", "grouped_wide") else 1
    G = 16
    d_align, d_group = dev_t(align if n else np.zeros(1, np.uint64)), dev_t(group if n else np.zeros(1, np.uint64))
    raw = torch.zeros(len(umis) + 8, dtype=torch.uint8, device="cuda:0")
    if n:
        raw[shift:shift + len(umis)] = torch.from_numpy(umis.copy()).to("cuda:0")
    d_score = dev_t(score) if (score is not None and n) else None
    sentinel = -0x5A5A5A5A5A5A5A5B
    outs = {f: torch.full((n * w + G,), sentinel, dtype=torch.int64, device="cuda:0") for f in ("keys", "nmask")}
    outs["rep"] = torch.full((n + G,), sentinel, dtype=torch.int64, device="cuda:0")
    outs["bucket_off"] = torch.full((n + 1 + G,), sentinel, dtype=torch.int64, device="cuda:0")
    outs["freq"] = torch.full((n + G,), -0x5A5A5A5B, dtype=torch.int32, device="cuda:0")
    ready(s)
    ne, nb = C.c_uint64(0), C.c_uint64(0)
    p = {f: t.data_ptr() for f, t in outs.items()}
    stream = s.cuda_stream if s is not None else None
    sc = d_score.data_ptr() if d_score is not None else None
    nm = p["nmask"] if nmask else None
    lib = _lib.load()
    if form == "wide":
        rc = lib.umi_stage_reads_wide_device(ctx._h, d_align.data_ptr(), abits, raw.data_ptr() + shift, sc, n, umi_len,
                                             w, merge, p["keys"], nm, p["freq"], p["rep"], p["bucket_off"],
                                             C.byref(ne), C.byref(nb), stream)
    elif form == "grouped":
        rc = lib.umi_stage_reads_grouped_device(ctx._h, d_align.data_ptr(), abits, d_group.data_ptr() if gbits else None,
                                                gbits, raw.data_ptr() + shift, sc, n, umi_len, merge, p["keys"], nm,
                                                p["freq"], p["rep"], p["bucket_off"], C.byref(ne), C.byref(nb), stream)
    elif form == "grouped_wide":
        rc = lib.umi_stage_reads_grouped_wide_device(ctx._h, d_align.data_ptr(), abits,
                                                     d_group.data_ptr() if gbits else None, gbits,
                                                     raw.data_ptr() + shift, sc, n, umi_len, w, merge, p["keys"], nm,
                                                     p["freq"], p["rep"], p["bucket_off"], C.byref(ne), C.byref(nb),
                                                     stream)
    else:
        rc = lib.umi_stage_reads_device(ctx._h, d_align.data_ptr(), abits, raw.data_ptr() + shift, sc, n, umi_len,
                                        merge, p["keys"], nm, p["freq"], p["rep"], p["bucket_off"], C.byref(ne),
                                        C.byref(nb), stream)
    _lib.check(rc)
    e, b = int(ne.value), int(nb.value)
    host = {f: read_back(t, s) for f, t in outs.items()}
    for f, cap in (("keys", n * w), ("nmask", n * w), ("rep", n), ("freq", n), ("bucket_off", n + 1)):
        assert (host[f][cap:] == host[f].dtype.type(sentinel if f != "freq" else -0x5A5A5A5B)).all(), f
    shape = (e, w) if form in ("wide", "grouped_wide") else (e,)
    got = dict(keys=host["keys"][:e * w].view(np.uint64).reshape(shape), freq=host["freq"][:e],
               rep=host["rep"][:e].view(np.uint64), bucket_off=host["bucket_off"][:b + 1].view(np.uint64))
    got["nmask"] = host["nmask"][:e * w].view(np.uint64).reshape(shape) if nmask else np.zeros(shape, np.uint64)
    return got


def stage_expected(form, align, group, umis, score, umi_len, abits, gbits, merge=1):
    """the model of the staging: positions = (align & abits mask, group & gbits mask) by first appearance"""
    amask = np.uint64((1 << abits) - 1) if abits < 64 else np.uint64(0xFFFFFFFFFFFFFFFF)
    w = (3 * umi_len + 63) // 64 if form in ("wide", "grouped_wide") else 1
    if len(align) == 0:
        z = np.zeros((0, w) if form in ("wide", "grouped_wide") else 0, np.uint64)
        return dict(keys=z, nmask=z, freq=np.zeros(0, np.int32), rep=np.zeros(0, np.uint64),
                    bucket_off=np.zeros(1, np.uint64))
    g = group if form in ("grouped", "grouped_wide") else np.zeros_like(group)
    exp = grouped_stage_model(align & amask, g, umis, score, umi_len, merge, gbits if form.startswith("grouped") else 0)
    if form in ("wide", "grouped_wide") and umi_len <= 21:  # a one-word key as a column
        exp = dict(exp, keys=exp["keys"].reshape(-1, 1), nmask=exp["nmask"].reshape(-1, 1))
    return exp


def stage_input(seed, n, umi_len, n_frac=0.005):
    rng = np.random.default_rng(seed)
    pos, umis, score = gen_reads(rng, n, max(1, n // 40), umi_len, n_frac=n_frac)
    align = rng.integers(0, 1 << 62, max(1, n // 40), dtype=np.uint64)[pos.astype(np.int64)] if n else pos
    group = rng.integers(0, 1 << 40, 7, dtype=np.uint64)[rng.integers(0, 7, n)]
    return align, group, umis, score


def _stage(ctx, s, form, umi_len, device):
    align, group, umis, score = stage_input(umi_len + len(form), 6000, umi_len)
    gb = 8 if form.startswith("grouped") else 0
    exp = stage_expected(form, align, group, umis, score, umi_len, 64, gb)
    if device:
        same(stage_device(ctx, form, align, group, umis, score, umi_len, s, gbits=gb), exp)
        return
    if form == "plain":
        got = ctx.stage_reads(align, umis, score, umi_len)
    elif form == "wide":
        got = ctx.stage_reads_wide(align, umis, score, umi_len)
    elif form == "grouped":
        got = ctx.stage_reads_grouped(align, group, umis, score, umi_len, group_key_bits=gb)
    else:
        got = ctx.stage_reads_grouped_wide(align, group, umis, score, umi_len, group_key_bits=gb)
    same(got, exp)


def x_stage_reads(ctx, b, s):
    _stage(ctx, s, "plain", L, False)


def x_stage_reads_device(ctx, b, s):
    _stage(ctx, s, "plain", L, True)


def x_stage_reads_wide(ctx, b, s):
    _stage(ctx, s, "wide", 30, False)


def x_stage_reads_wide_device(ctx, b, s):
    _stage(ctx, s, "wide", 30, True)


def x_stage_reads_grouped(ctx, b, s):
    _stage(ctx, s, "grouped", L, False)


def x_stage_reads_grouped_device(ctx, b, s):
    _stage(ctx, s, "grouped", L, True)


def x_stage_reads_grouped_wide(ctx, b, s):
    _stage(ctx, s, "grouped_wide", 24, False)


def x_stage_reads_grouped_wide_device(ctx, b, s):
    _stage(ctx, s, "grouped_wide", 24, True)


def _stage_seqs(ctx, s, device):
    import torch
    seqs, quals = seq_input(32)
    ent, off, blen = sm.stage(seqs, quals, 1)
    w = max(sm.words(len(x)) for x in seqs)
    keys, nm = sm.encode([e[0] for e in ent], w)
    freq, rep = np.array([e[1] for e in ent], np.int32), np.array([e[2] for e in ent], np.uint64)
    if not device:
        got = ctx.stage_seqs(seqs, quals, merge=1)
        g_keys, g_nm, g_freq, g_rep = got["keys"], got["nmask"], got["freq"], got["rep"]
        g_off, g_len = got["bucket_off"], got["bucket_len"]
    else:
        n = len(seqs)
        lens = np.array([len(x) for x in seqs], np.uint32)
        pos = np.zeros(n, np.uint64)
        pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
        pos = np.concatenate([pos, pos + np.uint64(int(lens.sum()))])
        d_text = dev_t(np.frombuffer(b"".join(seqs) + b"".join(quals), np.uint8))
        d_pos, d_len = dev_t(pos), dev_t(lens)
        d_keys, d_nm = zeros(n * w, torch.int64), zeros(n * w, torch.int64)
        d_freq, d_rep = zeros(n, torch.int32), zeros(n, torch.int64)
        ready(s)
        g_off, g_len, e, _ = ctx.stage_seqs_device(d_text.data_ptr(), d_pos.data_ptr(), d_pos.data_ptr() + 8 * n,
                                                   d_len.data_ptr(), n, w, d_keys.data_ptr(), d_nm.data_ptr(),
                                                   d_freq.data_ptr(), d_rep.data_ptr(), merge=1,
                                                   stream=s.cuda_stream if s is not None else 0)
        g_keys = read_back(d_keys, s)[:e * w].view(np.uint64).reshape(e, w)
        g_nm = read_back(d_nm, s)[:e * w].view(np.uint64).reshape(e, w)
        g_freq, g_rep = read_back(d_freq, s)[:e], read_back(d_rep, s)[:e].view(np.uint64)
    assert list(g_off) == off and list(g_len) == blen
    assert np.array_equal(g_keys, keys) and np.array_equal(g_nm, nm)
    assert np.array_equal(g_freq, freq) and np.array_equal(g_rep, rep)


def x_stage_seqs(ctx, b, s):
    _stage_seqs(ctx, s, False)


def x_stage_seqs_device(ctx, b, s):
    _stage_seqs(ctx, s, True)


def split_edges(ctx, batch, s, n_parts=2, cap=1 << 20):
    """every part of the pairs (umi_pairs_partial_device), concatenated as an all-gather would"""
    import torch
    keys, nm, fr, off = batch
    t_keys, t_nm, t_fr = dev_t(keys), dev_t(nm), dev_t(fr)
    ready(s)
    parts = []
    for part in range(n_parts):
        buf = zeros(cap, torch.int64)
        ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(), off, L, part, n_parts,
                                         buf.data_ptr(), cap, k=1, stream=s.cuda_stream if s is not None else 0)
        parts.append(buf[:ne])
    assert sum(1 for p in parts if len(p)) == n_parts  # the work really was split
    return torch.cat(parts)


def collapse_and_check(ctx, batch, edges, s):
    import torch
    keys, nm, fr, off = batch
    n = len(keys)
    kept, root = zeros(n, torch.uint8), zeros(n, torch.int32)
    ready(s)
    st = ctx.collapse_edges_device(n, edges.data_ptr(), len(edges), kept.data_ptr(), root.data_ptr(),
                                   stream=s.cuda_stream if s is not None else 0)
    okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
    assert (read_back(kept, s)[:n] == okept).all() and (read_back(root, s)[:n].view(np.uint32) == oroot).all()
    assert st["n_kept"] == int(okept.sum())


def x_pairs_partial_then_collapse(ctx, b, s):
    collapse_and_check(ctx, b["x"], split_edges(ctx, b["x"], s, n_parts=3), s)


def x_collapse_edges(ctx, b, s):
    collapse_and_check(ctx, b["x"], b["x_edges"], s)


def x_hipnaive(ctx, b, s):
    import umi_collapse_rs_amd as umi
    rng = np.random.default_rng(77)
    for umi_len, k in ((8, 1), (20, 2), (30, 1)):
        umis, freq = random_bucket(rng, 60, umi_len, err=0.1, n_frac=0.02)
        d = umi.HipNaive.new(dict(zip(umis, freq)), umi_len, k, ctx=ctx)
        o = orc.Naive(umis, freq)
        for q in rng.permutation(len(umis))[:20]:
            kk, mf = int(rng.integers(0, k + 1)), int(rng.integers(0, 6))
            assert d.remove_near(umis[q], kk, mf) == {umis[i] for i in o.remove_near(int(q), kk, mf)}
            assert all(d.contains(u) == o.contains(i) for i, u in enumerate(umis))


X_HOST = ["dedup_batch", "dedup_batch_wide_22", "dedup_batch_wide_85", "dedup_seqs", "stage_reads",
          "stage_reads_wide", "stage_reads_grouped", "stage_reads_grouped_wide", "stage_seqs", "hipnaive"]
X_DEVICE = ["dedup_batch_device", "dedup_batch_device_table", "dedup_batch_wide_device_22",
            "dedup_batch_wide_device_85", "dedup_seqs_device", "stage_reads_device", "stage_reads_wide_device",
            "stage_reads_grouped_device", "stage_reads_grouped_wide_device", "stage_seqs_device",
            "pairs_partial_then_collapse", "collapse_edges"]
CASES = [(x, "own") for x in X_HOST] + [(x, s) for x in X_DEVICE for s in ("same", "other", "null")]


@pytest.mark.parametrize("x,where", CASES)
def test_call_while_a_deferred_call_is_out(ctx, batches, x, where):
    """begin(A) -> X -> end: X gives its own reference's result, A's outputs and stats the oracle's.
    where: X on A's stream, on another stream, on the NULL stream (host forms: the context's own)."""
    import torch
    b = dict(batches)
    if x == "collapse_edges":  # (the edge list is made before A begins)
        b["x_edges"] = split_edges(ctx, b["x"], None)
        torch.cuda.synchronize()
    s_a = torch.cuda.Stream()
    a = Pending(ctx, b["a"], s_a)
    s_x = {"same": s_a, "other": torch.cuda.Stream(), "null": None, "own": None}[where]
    globals()["x_" + x](ctx, b, s_x)
    a.end_and_check(ctx)


@pytest.mark.parametrize("where", ["same", "other"])
def test_second_begin_replaces_the_pending_call(ctx, batches, where):
    """begin(A) -> begin(B) -> end: end hands out B's stats; A's outputs are final and the oracle's"""
    import torch
    s_a = torch.cuda.Stream()
    a = Pending(ctx, batches["a"], s_a)
    rng = np.random.default_rng(5)
    bb = staged(rng, 40000, 1500)
    pb = Pending(ctx, bb, s_a if where == "same" else torch.cuda.Stream())
    a.check_outputs()  # (final: the second begin let A end)
    pb.end_and_check(ctx)  # (B's stats; A's result was dropped)
    a.check_outputs()


def test_a_larger_call_grows_the_workspace_while_a_call_is_out(batches):
    """X larger than A on a fresh context: every workspace buffer A uses is reallocated under it"""
    import torch
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    try:
        s_a = torch.cuda.Stream()
        a = Pending(c, batches["a"], s_a)
        assert len(batches["big"][0]) > 3 * len(batches["a"][0])
        _dedup_device(c, batches["big"], torch.cuda.Stream(), table=False)
        a.end_and_check(c)
        a = Pending(c, batches["a"], s_a)
        keys, nm, fr, off = batches["big"]
        kept, root, _ = c.dedup_batch(keys, nm, fr, off, L, k=1)
        okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
        assert (kept == okept).all() and (root == oroot).all()
        a.end_and_check(c)
    finally:
        c.close()


# ---- the pending call's contract violation survives the call in between ----------------------------

def _fails(code, fn):
    import umi_collapse_rs_amd as umi
    with pytest.raises(umi.UmiHipError) as e:
        fn()
    assert e.value.code == code, str(e.value)


@pytest.mark.parametrize("x", ["plain", "pairs_partial", "collapse_null_kept", "pairs_partial_small_buffer",
                               "refused_before_settling"])
def test_contract_violation_of_the_pending_call_is_reported_at_end(ctx, batches, x):
    """begin(A with a rank-order violation) -> X -> end: end raises UMI_ERR_ORDER with the contract's text,
    whatever X did -- succeeded, failed after letting A end (settle), or was refused before that"""
    import torch
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    s = torch.cuda.Stream()
    keys, nm, fr, off = batches["x"]
    t_keys, t_nm, t_fr = dev_t(keys), dev_t(nm), dev_t(fr)
    t_kept = zeros(len(keys), torch.uint8)
    buf = zeros(1 << 20, torch.int64)
    torch.cuda.synchronize()
    a = Pending(ctx, batches["a"], s, bad=True)
    if x == "plain":
        x_dedup_batch_device(ctx, batches, s)
    elif x == "pairs_partial":
        ne, _ = ctx.pairs_partial_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(), off, L, 0, 2,
                                         buf.data_ptr(), 1 << 20, k=1, stream=s.cuda_stream)
        assert ne > 0
    elif x == "collapse_null_kept":
        _fails(_lib.UMI_ERR_ARG, lambda: ctx.collapse_edges_device(len(keys), buf.data_ptr(), 1, 0,
                                                                    stream=s.cuda_stream))
    elif x == "pairs_partial_small_buffer":
        _fails(_lib.UMI_ERR_NOMEM, lambda: ctx.pairs_partial_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(),
                                                                     off, L, 0, 2, buf.data_ptr(), 1, k=1,
                                                                     stream=s.cuda_stream))
    else:
        _fails(_lib.UMI_ERR_ARG, lambda: ctx.dedup_batch_device(t_keys.data_ptr(), t_nm.data_ptr(), t_fr.data_ptr(), off,
                                                                0, t_kept.data_ptr(), stream=s.cuda_stream))
    with pytest.raises(umi.UmiHipError) as e:
        ctx.dedup_batch_end()
    assert e.value.code == _lib.UMI_ERR_ORDER
    assert "break the input contract" in str(e.value)
    with pytest.raises(umi.UmiHipError) as e:
        ctx.dedup_batch_end()
    assert e.value.code == _lib.UMI_ERR_ARG
    # the context is whole: the next call in two halves is the oracle's
    Pending(ctx, batches["a"], s).end_and_check(ctx)


def test_close_with_a_call_out(batches):
    """ctx.close() with a deferred call out returns, A's outputs are final; the next context gives the oracle's"""
    import torch
    import umi_collapse_rs_amd as umi
    s = torch.cuda.Stream()
    c = umi.Context(0)
    a = Pending(c, batches["a"], s)
    c.close()
    a.check_outputs()
    c = umi.Context(0)
    try:
        Pending(c, batches["a"], s).end_and_check(c)
        _dedup_device(c, batches["x"], s, table=True)
    finally:
        c.close()


# ---- the device forms on their own -----------------------------------------------------------------

@pytest.mark.parametrize("form,umi_len", [("wide", 12), ("wide", 30), ("grouped", 12), ("grouped_wide", 24)])
@pytest.mark.parametrize("n_reads", [0, 1, 255, 70001])
@pytest.mark.parametrize("shift,abits,gbits,score,nmask", [
    (0, 64, 0, True, True),      # word-aligned text, no group key: the plain staging
    (1, 20, 8, False, False),    # text off the word boundary, no score (rep = first read), no N and no nmask
    (3, 1, 64, True, True),      # one alignment bit, a full 64-bit group key
])
def test_stage_device_forms(ctx, form, umi_len, n_reads, shift, abits, gbits, score, nmask):
    import torch
    align, group, umis, sc = stage_input(n_reads + umi_len + shift, n_reads, umi_len, n_frac=0.004 if nmask else 0.0)
    s = torch.cuda.Stream()
    gbits = gbits if form.startswith("grouped") else 0
    got = stage_device(ctx, form, align, group, umis, sc if score else None, umi_len, s, abits=abits, gbits=gbits,
                       shift=shift, nmask=nmask)
    same(got, stage_expected(form, align, group, umis, sc if score else None, umi_len, abits, gbits))


@pytest.mark.parametrize("umi_len", [22, 40, 85])
@pytest.mark.parametrize("nmask,root", [(True, True), (False, False)])
def test_dedup_batch_wide_device(ctx, umi_len, nmask, root):
    """umi_dedup_batch_wide_device on the caller's stream: NULL d_nmask (no N) and NULL d_root; the results are
    final when the call returns (read behind a stream-ordered copy)"""
    import torch
    keys, nm, fr, off = wide_batch(umi_len * 3, umi_len) if nmask else _without_n(umi_len)
    okept, oroot, _ = orc.dedup_batch_wide(keys, nm, fr, off, umi_len, 1)
    s = torch.cuda.Stream()
    t_keys, t_nm, t_fr = dev_t(keys), dev_t(nm), dev_t(fr)
    t_kept, t_root = zeros(len(keys), torch.uint8), zeros(len(keys), torch.int32)
    torch.cuda.synchronize()
    st = ctx.dedup_batch_wide_device(t_keys.data_ptr(), t_nm.data_ptr() if nmask else 0, keys.shape[1],
                                     t_fr.data_ptr(), off, umi_len, t_kept.data_ptr(),
                                     t_root.data_ptr() if root else 0, k=1, stream=s.cuda_stream)
    assert (read_back(t_kept, s)[:len(keys)] == okept).all()
    if root:
        assert (read_back(t_root, s)[:len(keys)].view(np.uint32) == oroot).all()
    assert st["n_kept"] == int(okept.sum()) and st["n_umis"] == len(keys)


def _without_n(umi_len):
    rng = np.random.default_rng(umi_len)
    keys, nm, fr, off = [], [], [], [0]
    for i in range(80):
        umis, freq = random_bucket(rng, 300 if i == 0 else int(rng.integers(1, 10)), umi_len, err=0.03)
        order = sorted(range(len(umis)), key=lambda j: (-freq[j], j))
        k, m = orc.encode_keys_wide([umis[j] for j in order])
        assert not m.any()
        keys.append(k); nm.append(m); fr.extend(freq[j] for j in order); off.append(off[-1] + len(umis))
    return np.concatenate(keys), np.concatenate(nm), np.array(fr, np.int32), np.array(off, np.uint64)


# ---- one context, every family of host-buffer calls in turn ----------------------------------------------
# The host-buffer forms lay their arrays into one staging block of the context, afresh per call, and the
# single-shot device forms share one workspace.  So: the calls below in a row on one context, with about 300
# items each, then about 70,000 (the block and the workspace grow, every offset moves), then about 300 again
# (small calls inside a large block), arrays that a call may leave out coming and going.  Every result is,
# byte for byte, that of the same call on a context of its own.

def _mix_bam_case(rng, n_clusters):
    """test_gpu_consensus_bam's mixed case with the voters drawn from a pool of families (a family per read
    would take seconds at 70,000 reads)"""
    from test_gpu_consensus_bam import Case, family
    from umi_collapse_rs_amd._lib import UMI_NO_CLUSTER
    lengths = (36, 75, 100, 151)
    pool = {L: [family(rng, L, 25, odd_codes=0.02) for _ in range(8)] for L in lengths}
    reads, clen = [], []
    for c in range(n_clusters):
        L = int(lengths[int(rng.integers(0, 4))])
        clen.append(L)
        if c % 97 == 5:
            continue  # a cluster without a voter
        fam = pool[L][int(rng.integers(0, 8))]
        for j in rng.integers(0, 25, int(rng.geometric(0.25))):
            reads.append(fam[int(j)] + (L, c))
    for _ in range(len(reads) // 9):  # reads that vote nowhere
        L = int(lengths[int(rng.integers(0, 4))])
        reads.append(pool[L][0][int(rng.integers(0, 25))] + (L, UMI_NO_CLUSTER))
    order = rng.permutation(len(reads))
    return Case([reads[i] for i in order], clen)


def _mix_inputs(seed, n, batch_a=None):
    """the inputs of every call of the sequence, about n items each, from the generators of the calls' own tests"""
    import barcode_model as bm
    import barcode_multi_model as mm
    from umi_collapse_rs_amd import synth
    rng = np.random.default_rng(seed)
    inp = dict(a=batch_a if batch_a is not None else staged(rng, n, max(1, n // 25), n_frac=0.002, sort=True),
               plain=staged(rng, n, max(1, n // 25)))  # (no N: a call without nmask)
    assert inp["a"][1].any() and not inp["plain"][1].any()
    wl, pairs = bm.random_list(rng, 5003, 16)
    inp["bc"] = (wl,) + mm.multi_reads(rng, wl, n, pairs)
    inp["stage"] = stage_input(seed + 1, n, 24)
    inp["bam"] = _mix_bam_case(rng, max(1, n // 4))
    nb = len(inp["a"][3]) - 1
    inp["rowcol"] = (rng.integers(0, 700, nb).astype(np.uint32), rng.integers(0, 90, nb).astype(np.uint32))
    few = min(n, 10000)  # (the generator takes a loop per read: a file of 10,000 reads, then the same again)
    seqs, quals = synth.fastq_reads(seed + 2, few, max(1, few // 3), lengths=[30, 100, 151], err=0.01, n_frac=0.002)
    inp["fastq"] = (seqs * (n // few), quals * (n // few))
    return inp


# every step: (context, inputs, the earlier results of this run) -> result
def _m_dedup(c, i, r):
    keys, nm, fr, off = i["a"]
    kept, root, st = c.dedup_batch(keys, nm, fr, off, L, k=1)
    return kept, root, st["n_kept"], st["n_umis"]


def _m_barcodes(c, i, r):
    wl, reads, quals = i["bc"]
    return c.correct_barcodes_multi(reads, quals, 16, wl)


def _m_stage(c, i, r):
    align, group, umis, score = i["stage"]
    return c.stage_reads_grouped_wide(align, group, umis, score, 24, merge=1, group_key_bits=8)


def _m_bam(c, i, r):
    case = i["bam"]
    return c.consensus_bam(case.data, case.seq_pos, case.qual_pos, case.lens, case.cluster, case.clen, want_disagree=True)


def _m_count(c, i, r):
    return c.count_matrix(r["dedup"][0], i["a"][2], i["a"][3], i["rowcol"][0], i["rowcol"][1], 700, 90)


def _m_stats(c, i, r):
    keys, _, fr, off = i["a"]
    return c.dedup_stats(keys, fr, r["dedup"][0], r["dedup"][1], off, L, seed=7, hist_bins=4096, per_umi=True)


def _m_stage_seqs(c, i, r):
    return c.stage_seqs(i["fastq"][0], i["fastq"][1], merge=1)


def _m_dedup_seqs(c, i, r):
    st = r["stage_seqs"]
    kept, root, _ = c.dedup_seqs(st["keys"], st["nmask"] if st["any_n"] else None, st["freq"], st["bucket_off"],
                                 st["bucket_len"], k=1)
    return kept, root


def _m_consensus(c, i, r):
    return c.consensus_seqs(i["fastq"][0], i["fastq"][1], r["stage_seqs"], r["dedup_seqs"][0], r["dedup_seqs"][1])


def _m_dedup_plain(c, i, r):
    keys, _, fr, off = i["plain"]
    kept, root, st = c.dedup_batch(keys, None, fr, off, L, k=1, want_root=False)
    assert root is None
    return kept, st["n_kept"]


MIX = [("dedup", _m_dedup), ("barcodes_multi", _m_barcodes), ("stage_reads_grouped_wide", _m_stage),
       ("consensus_bam", _m_bam), ("count_matrix", _m_count), ("dedup_stats", _m_stats), ("stage_seqs", _m_stage_seqs),
       ("dedup_seqs", _m_dedup_seqs), ("consensus_seqs", _m_consensus), ("dedup_plain", _m_dedup_plain)]


def _blob(x):
    """a result as nested tuples of bytes"""
    if isinstance(x, dict):
        return tuple((k, _blob(x[k])) for k in sorted(x))
    if isinstance(x, (list, tuple)):
        return tuple(_blob(v) for v in x)
    if isinstance(x, np.ndarray):
        return (str(x.dtype), x.shape, x.tobytes())
    return x


def _mix_run(inp, ctx_of):
    """the sequence, step s on the context ctx_of(s) gives; every step sees this run's earlier results"""
    res = {}
    for name, step in MIX:
        c, done = ctx_of(name)
        try:
            res[name] = step(c, inp, res)
        finally:
            done(c)
    return res


def test_one_context_across_every_family_while_the_staging_block_grows_and_shrinks(batches):
    import umi_collapse_rs_amd as umi
    small, large = _mix_inputs(3001, 300), _mix_inputs(3002, 70000, batch_a=batches["a"])
    assert 200 <= len(small["a"][0]) <= 300 and len(large["a"][0]) >= 50000 and len(large["bam"].lens) >= 60000
    alone = {}
    for size, inp in (("small", small), ("large", large)):  # every call on a context of its own
        alone[size] = _mix_run(inp, lambda name: (umi.Context(0), lambda c: c.close()))
        assert alone[size]["stage_seqs"]["any_n"] and len(alone[size]["count_matrix"][0]) > 5
        assert len(alone[size]["dedup_stats"]["umi_entry"]) > 100 and (alone[size]["barcodes_multi"]["counts"][:4] > 0).all()
    shared = umi.Context(0)
    try:
        for size, inp in (("small", small), ("large", large), ("small", small)):
            got = _mix_run(inp, lambda name: (shared, lambda c: None))
            for name, _ in MIX:
                assert _blob(got[name]) == _blob(alone[size][name]), (size, name)
    finally:
        shared.close()


# ---- the multi-device call's error exit --------------------------------------------------------------

def _multi_shards(batches, bad, devices):
    import torch
    shards, ref = [], []
    for r, (batch, dev) in enumerate(zip((batches["a"], batches["x"]), devices)):
        keys, nm, fr, off = batch
        if bad and r == 1:
            fr = fr.copy()
            fr[0], fr[1] = 1, 7  # (bucket 0 of X has two entries or more)
        t = [torch.from_numpy(np.ascontiguousarray(a).view(np.int64) if a.dtype == np.uint64 else a.copy()).to(dev)
             for a in (keys, nm, fr)]
        kept = torch.zeros(len(keys), dtype=torch.uint8, device=dev)
        root = torch.zeros(len(keys), dtype=torch.int32, device=dev)
        shards.append(dict(d_keys=t[0].data_ptr(), d_nmask=t[1].data_ptr(), d_freq=t[2].data_ptr(), bucket_off=off,
                           d_kept=kept.data_ptr(), d_root=root.data_ptr(), _keep=(t, kept, root)))
        ref.append(batch)
    return shards, ref


def _multi_error_then_good(batches, devices, gather):
    import torch
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    assert int(np.diff(batches["x"][3].astype(np.int64))[0]) >= 2
    slice_bytes = (max(len(batches["a"][0]), len(batches["x"][0])) + 7) // 8
    bits = [torch.zeros(2 * slice_bytes, dtype=torch.uint8, device=d) for d in devices]
    c = umi.Context([int(torch.device(d).index) for d in devices])
    try:
        bad, _ = _multi_shards(batches, True, devices)
        for sh, t in zip(bad, bits):
            sh["d_bits_all"] = t.data_ptr()
        for d in devices:
            torch.cuda.synchronize(d)
        with pytest.raises(umi.UmiHipError) as e:
            c.dedup_batch_device_multi(bad, L, slice_bytes, k=1, gather=gather)
        assert e.value.code == _lib.UMI_ERR_ORDER
        good, ref = _multi_shards(batches, False, devices)
        for sh, t in zip(good, bits):
            sh["d_bits_all"] = t.data_ptr()
        for d in devices:
            torch.cuda.synchronize(d)
        st = c.dedup_batch_device_multi(good, L, slice_bytes, k=1, gather=gather)
        n_kept = 0
        okepts = []
        for sh, (keys, nm, fr, off) in zip(good, ref):
            t, kept, root = sh["_keep"]
            okept, oroot, _ = orc.dedup_batch(keys, nm, fr, off, L, 1)
            assert (kept.cpu().numpy() == okept).all() and (root.cpu().numpy().view(np.uint32) == oroot).all()
            n_kept += int(okept.sum())
            okepts.append(okept)
        assert st["n_kept"] == n_kept
        if gather:
            for t in bits:
                got = t.cpu().numpy()
                for r, okept in enumerate(okepts):
                    sl = got[r * slice_bytes:(r + 1) * slice_bytes]
                    assert (np.unpackbits(sl, bitorder="little")[:len(okept)] == okept).all()
    finally:
        c.close()


def test_multi_device_call_with_a_failing_shard_leaves_the_context_whole(batches):
    """Context([0, 0]), no gathered mask: shard 1 breaks the input contract, shard 0 is ~3,000 positions; the
    call raises, and the next call on the context gives the oracle's result on both shards"""
    _multi_error_then_good(batches, ["cuda:0", "cuda:0"], gather=False)


def _two_devices():
    import torch
    return torch.cuda.device_count() >= 2


@pytest.mark.skipif("not _two_devices()", reason="the RCCL gather wants two distinct devices")
def test_multi_device_gather_with_a_failing_shard_leaves_the_context_whole(batches):
    _multi_error_then_good(batches, ["cuda:0", "cuda:1"], gather=True)
