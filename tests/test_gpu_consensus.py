"""umi_consensus_seqs / umi_consensus_seqs_device on the MI355X against the plain-Python model of the
definition (tests/consensus_model.py), bit for bit: the fastq suite's mixed workload over both
algorithms and merges, lengths at the lane and word edges, a cluster deep enough for the split path
under three settings of "cons_split", qualities at both ends, sums beyond 32 bits, the contract
violations, and a call made while a deferred batched call is out."""
import numpy as np
import pytest

import consensus_model as cm
import seq_model as sm
from umi_collapse_rs_amd import Context, UmiHipError, synth
from umi_collapse_rs_amd._lib import UMI_ERR_ARG, UMI_ERR_ORDER

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    c = Context(0)
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


def device_call(ctx, seqs, quals, staged, kept, root, odd=0, fill=0, qual_null=False):
    """consensus_seqs_device on torch buffers; the text starts `odd` bytes into its buffer.  Returns what
    consensus_seqs returns, plus the raw output buffers (filled with `fill` before the call)."""
    import torch
    n, ne = len(seqs), len(staged["freq"])
    lens = np.array([len(s) for s in seqs], np.uint32)
    total = int(lens.sum())
    pos = np.zeros(n, np.uint64)
    pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    pos = np.concatenate([pos, pos + np.uint64(total)])
    text = np.frombuffer(b"\0" * odd + b"".join(seqs) + b"".join(quals) + b"\0", np.uint8)
    t_text, t_pos, t_len = dev_t(text), dev_t(pos), dev_t(lens)
    t_eor, t_freq = dev_t(staged["entry_of_read"]), dev_t(staged["freq"])
    t_kept, t_root = dev_t(np.asarray(kept, np.uint8)), dev_t(np.asarray(root, np.uint32))
    o_seq = torch.full((total + 8,), fill, dtype=torch.uint8, device="cuda:0")
    o_qual = torch.full((total + 8,), fill, dtype=torch.uint8, device="cuda:0")
    o_off = torch.full((ne,), -1, dtype=torch.int64, device="cuda:0")
    o_cr = torch.full((ne,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    try:
        nbytes = ctx.consensus_seqs_device(t_text.data_ptr() + odd, t_pos.data_ptr(), 0 if qual_null else t_pos.data_ptr() + 8 * n,
                                           t_len.data_ptr(), n, t_eor.data_ptr(), t_freq.data_ptr(), t_kept.data_ptr(),
                                           t_root.data_ptr(), ne, staged["bucket_off"], staged["bucket_len"],
                                           o_seq.data_ptr(), o_qual.data_ptr(), o_off.data_ptr(), o_cr.data_ptr())
    finally:
        torch.cuda.synchronize()
        raw = (o_seq.cpu().numpy(), o_qual.cpu().numpy(), o_off.cpu().numpy(), o_cr.cpu().numpy())
    sb, qb, off, cr = raw[0].tobytes(), raw[1].tobytes(), raw[2], raw[3].view(np.uint32)
    ks = np.flatnonzero(np.asarray(kept))
    boff, blen = staged["bucket_off"], staged["bucket_len"]
    out_s, out_q, at = [], [], 0
    for r in ks:
        L = int(blen[np.searchsorted(boff, r, side="right") - 1])
        assert int(off[r]) == at  # dense, in ascending entry order
        out_s.append(sb[at:at + L])
        out_q.append(qb[at:at + L])
        at += L
    assert nbytes == at
    if fill == 0:  # nothing behind the last one
        assert not raw[0][at:].any() and not raw[1][at:].any()
    return (out_s, out_q, cr[ks]), raw


def same(got, want):
    gs, gq, gn = got
    assert len(gs) == len(want)
    for j, (r, s, q, m) in enumerate(want):
        assert gs[j] == s and gq[j] == q and int(gn[j]) == m, (j, r, gs[j], s, gq[j], q, int(gn[j]), m)


def both_forms(ctx, seqs, quals, staged, kept, root, want, odd=1):
    same(ctx.consensus_seqs(seqs, quals, staged, kept, root), want)
    got, _ = device_call(ctx, seqs, quals, staged, kept, root, odd=odd)
    same(got, want)


def staged_of_model(seqs, ent, off, blen):
    """the dict stage_seqs gives, from the model's staging"""
    return dict(freq=np.array([e[1] for e in ent], np.int32), entry_of_read=np.array(cm.entry_of_reads(seqs, ent), np.uint32),
                bucket_off=np.array(off, np.uint64), bucket_len=np.array(blen, np.int32))


@pytest.mark.parametrize("algo", [0, 1])
@pytest.mark.parametrize("merge", [0, 1])
def test_mixed_workload(ctx, algo, merge):
    seqs, quals = synth.fastq_reads(41, 4000, 900, lengths=[18, 60, 100, 150], err=0.01, n_frac=0.002)
    ent, off, blen = sm.stage(seqs, quals, merge)
    kept, root = sm.dedup(ent, off, blen, 2, algo, join=True)
    want = cm.clusters(seqs, quals, cm.entry_of_reads(seqs, ent), kept, root)
    # the library's own staging and collapse give the same entries (their own suites), so the whole
    # chain is checked here, not the model's arrays fed back
    st = ctx.stage_seqs(seqs, quals, merge=merge)
    k2, r2, _ = ctx.dedup_seqs(st["keys"], st["nmask"] if st["any_n"] else None, st["freq"], st["bucket_off"],
                               st["bucket_len"], k=2, algo=algo)
    assert np.array_equal(k2.astype(bool), kept) and np.array_equal(r2, root)
    if algo == 0:  # (adjacency with max_freq 0 unites equal sequences only: there the consensus is the read)
        assert sum(1 for r, s, q, m in want if s != seqs[ent[r][2]]) >= 100  # a copy of the kept read would fail
    both_forms(ctx, seqs, quals, st, k2, r2, want)


def test_lane_and_word_edges(ctx):
    lengths = [0, 1, 3, 4, 5, 63, 64, 255, 256]
    rng = np.random.default_rng(77)
    seqs, quals = [], []
    for L in lengths:  # per length: three molecules, each read a few times with errors and an N here and there
        for m in range(3):
            mol = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
            for c in range(int(rng.integers(1, 7))):
                r = mol.copy()
                hit = rng.random(L) < 0.05
                r[hit] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(hit.sum()))
                seqs.append(r.tobytes())
                quals.append(rng.integers(33, 127, L, dtype=np.uint8).tobytes())
    order = rng.permutation(len(seqs))
    seqs, quals = [seqs[i] for i in order], [quals[i] for i in order]
    ent, off, blen = sm.stage(seqs, quals, 1)
    kept, root = sm.dedup(ent, off, blen, 40, 0)  # k far beyond the errors: the copies of a molecule unite
    want = cm.clusters(seqs, quals, cm.entry_of_reads(seqs, ent), kept, root)
    assert sorted(set(blen)) == lengths and max(m for *_, m in want) >= 4
    st = staged_of_model(seqs, ent, off, blen)
    for odd in (1, 2, 3):  # the text at every byte offset of a word
        got, _ = device_call(ctx, seqs, quals, st, kept, root, odd=odd)
        same(got, want)
    same(ctx.consensus_seqs(seqs, quals, st, kept, root), want)


def test_deep_cluster_three_settings():
    """one molecule read 50,000 times beside 2,000 small ones: the split path by default, for every
    cluster of two reads or more, and for none"""
    rng = np.random.default_rng(5)
    L = 60
    small_s, small_q = synth.fastq_reads(12, 6000, 2000, length=L, err=0.01)
    mol = rng.choice(np.frombuffer(b"ACGT", np.uint8), L)
    deep = np.tile(mol, (50_000, 1))
    hit = rng.random(deep.shape) < 0.01
    deep[hit] = rng.choice(np.frombuffer(b"ACGT", np.uint8), int(hit.sum()))
    deep_q = rng.integers(35, 74, deep.shape, dtype=np.uint8)
    seqs = small_s + [r.tobytes() for r in deep]
    quals = small_q + [r.tobytes() for r in deep_q]
    order = rng.permutation(len(seqs))
    seqs, quals = [seqs[i] for i in order], [quals[i] for i in order]
    results = []
    want = None
    for split in (None, 2, 1 << 30):
        c = Context(0)
        try:
            if split is not None:
                c.set_option("cons_split", split)
            st = c.stage_seqs(seqs, quals, merge=1)
            kept, root, _ = c.dedup_seqs(st["keys"], None, st["freq"], st["bucket_off"], st["bucket_len"], k=1)
            if want is None:  # the collapse is the library's (its own suites check it); the vote is the model's
                want = cm.clusters(seqs, quals, st["entry_of_read"], kept, root)
                assert max(m for *_, m in want) >= 40_000 and len(want) >= 1500
            got = c.consensus_seqs(seqs, quals, st, kept, root)
            same(got, want)
            dgot, _ = device_call(c, seqs, quals, st, kept, root, odd=3)
            same(dgot, want)
            results.append(got)
        finally:
            c.close()
    for g in results[1:]:
        assert g[0] == results[0][0] and g[1] == results[0][1] and np.array_equal(g[2], results[0][2])


def one_cluster(seqs):
    """every read in one cluster, by hand: entries by freq descending, the first one kept"""
    ent, off, blen = sm.stage(seqs, [b"I" * len(s) for s in seqs], 0)
    assert len(blen) == 1
    kept = np.zeros(len(ent), bool)
    kept[0] = True
    return ent, off, blen, kept, np.zeros(len(ent), np.uint32)


def test_all_qualities_zero(ctx):
    """every S is 0: the vote falls to n, then to the order of ACGT"""
    seqs = [b"ACGTACGTTT"] * 3 + [b"ACGTACGTCC"] * 3 + [b"CCGTACGTGN"] * 2
    quals = [b"!" * 10] * len(seqs)
    ent, off, blen, kept, root = one_cluster(seqs)
    want = cm.clusters(seqs, quals, cm.entry_of_reads(seqs, ent), kept, root)
    assert want[0][1:] == (b"ACGTACGTCC", b"!" * 10, 8)
    both_forms(ctx, seqs, quals, staged_of_model(seqs, ent, off, blen), kept, root, want)


def test_highest_qualities_and_the_cap(ctx):
    rng = np.random.default_rng(9)
    mol = rng.choice(np.frombuffer(b"ACGT", np.uint8), 100)
    reads = np.tile(mol, (5000, 1))
    hit = rng.random(reads.shape) < 0.3
    reads[hit] = rng.choice(np.frombuffer(b"ACGTN", np.uint8), int(hit.sum()))
    reads[:, 7] = ord("N")
    reads[:2500, 8], reads[2500:, 8] = ord("G"), ord("T")  # a tie at the top: 2500 x 93 each
    seqs = [r.tobytes() for r in reads]
    quals = [b"~" * 100] * len(seqs)
    ent, off, blen, kept, root = one_cluster(seqs)
    want = cm.clusters(seqs, quals, cm.entry_of_reads(seqs, ent), kept, root)
    s, q = want[0][1], want[0][2]
    assert s[7:9] == b"NG" and q[7:9] == b"!!" and q.count(b"~") >= 90 and want[0][3] == 5000
    st = staged_of_model(seqs, ent, off, blen)
    both_forms(ctx, seqs, quals, st, kept, root, want)
    for split in (2, 1 << 30):
        c = Context(0)
        try:
            c.set_option("cons_split", split)
            same(c.consensus_seqs(seqs, quals, st, kept, root), want)
        finally:
            c.close()


def test_sums_beyond_32_bits(ctx):
    """2^26 reads of one base, all A with quality '~', one cluster: S_A = 93 * 2^26 > 2^32"""
    import torch
    n = 1 << 26
    dev = "cuda:0"
    text = torch.empty(2 * n + 8, dtype=torch.uint8, device=dev)
    text[:n] = ord("A")
    text[n:] = ord("~")
    pos = torch.arange(2 * n, dtype=torch.int64, device=dev)  # seq_pos, then qual_pos = n + i
    lens = torch.ones(n, dtype=torch.int32, device=dev)
    eor = torch.zeros(n, dtype=torch.int32, device=dev)
    freq, kept, root = dev_t(np.array([n], np.int32)), dev_t(np.array([1], np.uint8)), dev_t(np.array([0], np.uint32))
    o_seq = torch.zeros(n, dtype=torch.uint8, device=dev)
    o_qual = torch.zeros(n, dtype=torch.uint8, device=dev)
    o_off = torch.full((1,), -1, dtype=torch.int64, device=dev)
    o_cr = torch.zeros(1, dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    nbytes = ctx.consensus_seqs_device(text.data_ptr(), pos.data_ptr(), pos.data_ptr() + 8 * n, lens.data_ptr(), n,
                                       eor.data_ptr(), freq.data_ptr(), kept.data_ptr(), root.data_ptr(), 1,
                                       np.array([0, 1], np.uint64), np.array([1], np.int32), o_seq.data_ptr(),
                                       o_qual.data_ptr(), o_off.data_ptr(), o_cr.data_ptr())
    torch.cuda.synchronize()
    assert nbytes == 1 and int(o_off[0]) == 0 and int(o_cr[0]) == n
    assert bytes(o_seq[:2].cpu().numpy()) == b"A\0" and bytes(o_qual[:2].cpu().numpy()) == b"~\0"
    # the other way round no quality is left: 2^25 A against 2^25 C, and one more A decides by n alone
    text[: n // 2] = ord("C")
    text[n:] = ord("!")
    torch.cuda.synchronize()
    ctx.consensus_seqs_device(text.data_ptr(), pos.data_ptr(), pos.data_ptr() + 8 * n, lens.data_ptr(), n,
                              eor.data_ptr(), freq.data_ptr(), kept.data_ptr(), root.data_ptr(), 1,
                              np.array([0, 1], np.uint64), np.array([1], np.int32), o_seq.data_ptr(),
                              o_qual.data_ptr(), o_off.data_ptr(), o_cr.data_ptr())
    torch.cuda.synchronize()
    assert bytes(o_seq[:1].cpu().numpy()) == b"A" and bytes(o_qual[:1].cpu().numpy()) == b"!"  # a tie: the first of ACGT
    text[n // 2] = ord("C")
    torch.cuda.synchronize()
    ctx.consensus_seqs_device(text.data_ptr(), pos.data_ptr(), pos.data_ptr() + 8 * n, lens.data_ptr(), n,
                              eor.data_ptr(), freq.data_ptr(), kept.data_ptr(), root.data_ptr(), 1,
                              np.array([0, 1], np.uint64), np.array([1], np.int32), o_seq.data_ptr(),
                              o_qual.data_ptr(), o_off.data_ptr(), o_cr.data_ptr())
    torch.cuda.synchronize()
    assert bytes(o_seq[:1].cpu().numpy()) == b"C" and bytes(o_qual[:1].cpu().numpy()) == b"!"


def small_case():
    seqs, quals = synth.fastq_reads(3, 600, 150, lengths=[20, 50], err=0.01)
    ent, off, blen = sm.stage(seqs, quals, 1)
    kept, root = sm.dedup(ent, off, blen, 1, 0)
    assert (~kept).any()
    return seqs, quals, staged_of_model(seqs, ent, off, blen), kept, root.astype(np.uint32)


def untouched(raw):
    return all((a.view(np.uint8) == 0xAB).all() for a in raw[:2]) and (raw[2] == -1).all() and (raw[3] == -1).all()


def refused(ctx, code, match, seqs, quals, st, kept, root, **kw):
    with pytest.raises(UmiHipError, match=match) as ei:
        ctx.consensus_seqs(seqs, quals, st, kept, root)
    assert ei.value.code == code
    import torch
    # the device form: the same status, and the outputs as they were
    n, ne = len(seqs), len(st["freq"])
    total = sum(map(len, seqs))
    lens = np.array([len(s) for s in seqs], np.uint32)
    pos = np.zeros(n, np.uint64)
    pos[1:] = np.cumsum(lens[:-1], dtype=np.uint64)
    pos = np.concatenate([pos, pos + np.uint64(total)])
    t = [dev_t(np.frombuffer(b"".join(seqs) + b"".join(quals) + b"\0", np.uint8)), dev_t(pos), dev_t(lens),
         dev_t(st["entry_of_read"]), dev_t(st["freq"]), dev_t(np.asarray(kept, np.uint8)), dev_t(np.asarray(root, np.uint32))]
    o_seq = torch.full((total + 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
    o_qual = torch.full((total + 8,), 0xAB, dtype=torch.uint8, device="cuda:0")
    o_off = torch.full((ne,), -1, dtype=torch.int64, device="cuda:0")
    o_cr = torch.full((ne,), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    with pytest.raises(UmiHipError, match=match) as ei:
        ctx.consensus_seqs_device(t[0].data_ptr(), t[1].data_ptr(), 0 if kw.get("qual_null") else t[1].data_ptr() + 8 * n,
                                  t[2].data_ptr(), n, t[3].data_ptr(), t[4].data_ptr(), t[5].data_ptr(), t[6].data_ptr(), ne,
                                  st["bucket_off"], st["bucket_len"], o_seq.data_ptr(), o_qual.data_ptr(), o_off.data_ptr(),
                                  o_cr.data_ptr())
    assert ei.value.code == code
    torch.cuda.synchronize()
    assert untouched((o_seq.cpu().numpy(), o_qual.cpu().numpy(), o_off.cpu().numpy(), o_cr.cpu().numpy()))


def test_root_to_an_entry_that_is_not_kept(ctx):
    seqs, quals, st, kept, root = small_case()
    bad = root.copy()
    bad[int(np.flatnonzero(kept)[3])] = int(np.flatnonzero(~kept)[0])
    refused(ctx, UMI_ERR_ORDER, "not a kept entry", seqs, quals, st, kept, bad)
    bad = root.copy()
    bad[5] = len(root) + 7
    refused(ctx, UMI_ERR_ORDER, "root outside the entries", seqs, quals, st, kept, bad)


def test_entry_of_read_out_of_range(ctx):
    seqs, quals, st, kept, root = small_case()
    st = dict(st)
    st["entry_of_read"] = st["entry_of_read"].copy()
    st["entry_of_read"][17] = len(root)
    st["entry_of_read"][400] = 0xFFFFFFFF
    refused(ctx, UMI_ERR_ORDER, "2 reads break the input contract .entry_of_read outside", seqs, quals, st, kept, root)


def test_multi_device_context_and_null_qualities(ctx):
    seqs, quals, st, kept, root = small_case()
    multi = Context([0, 0])
    try:
        refused(multi, UMI_ERR_ARG, "single-device context", seqs, quals, st, kept, root)
    finally:
        multi.close()
    import torch
    n, ne = len(seqs), len(st["freq"])
    with pytest.raises(UmiHipError, match="qual_pos is NULL") as ei:
        ctx.consensus_seqs_device(8, 8, 0, 8, n, 8, 8, 8, 8, ne, st["bucket_off"], st["bucket_len"], 8, 8, 8, 8)
    assert ei.value.code == UMI_ERR_ARG  # (refused before any pointer is followed)
    with pytest.raises(UmiHipError) as ei:
        ctx.consensus_seqs_device(8, 8, 8, 8, 1 << 30, 8, 8, 8, 8, ne, st["bucket_off"], st["bucket_len"], 8, 8, 8, 8)
    assert ei.value.code == UMI_ERR_ARG
    with pytest.raises(UmiHipError) as ei:
        ctx.consensus_seqs_device(8, 8, 8, 8, n, 8, 8, 8, 8, ne, st["bucket_off"], st["bucket_len"], 0, 8, 8, 8)
    assert ei.value.code == UMI_ERR_ARG
    # and the context still works
    want = cm.clusters(seqs, quals, st["entry_of_read"], kept, root)
    both_forms(ctx, seqs, quals, st, kept, root, want)


def test_while_a_deferred_call_is_out(ctx):
    """begin(A) -> consensus -> end: the consensus is right, and so are A's outputs and counts"""
    import torch
    import oracle as orc
    pos, bases = synth.molecule_reads(seed=31, n_positions=3000, reads_per_position=25, umi_len=12, err=0.02)
    a = synth.stage(pos, synth.bases_to_keys(bases))
    assert int(np.diff(a["bucket_off"].astype(np.int64)).max()) <= 128
    seqs, quals, st, kept, root = small_case()
    want = cm.clusters(seqs, quals, st["entry_of_read"], kept, root)
    okept, oroot, _ = orc.dedup_batch(a["keys"], None, a["freq"], a["bucket_off"], 12, 1)
    for form in ("host", "device"):
        t_keys, t_freq, t_off = dev_t(a["keys"]), dev_t(a["freq"]), dev_t(a["bucket_off"])
        d_kept = torch.zeros(len(a["keys"]), dtype=torch.uint8, device="cuda:0")
        d_root = torch.zeros(len(a["keys"]), dtype=torch.int32, device="cuda:0")
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.default_stream())
        ctx.dedup_batch_device_begin(t_keys.data_ptr(), 0, t_freq.data_ptr(), a["bucket_off"], 12, d_kept.data_ptr(),
                                     d_root.data_ptr(), k=1, stream=s.cuda_stream, d_bucket_off=t_off.data_ptr())
        if form == "host":
            same(ctx.consensus_seqs(seqs, quals, st, kept, root), want)
        else:
            got, _ = device_call(ctx, seqs, quals, st, kept, root, odd=1)
            same(got, want)
        stats = ctx.dedup_batch_end()
        torch.cuda.synchronize()
        assert np.array_equal(d_kept.cpu().numpy(), okept)
        assert np.array_equal(d_root.cpu().numpy().view(np.uint32), oroot)
        assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(a["keys"])
