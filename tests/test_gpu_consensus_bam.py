"""umi_consensus_bam / umi_consensus_bam_device on the MI355X against the plain-Python model of the
definition (tests/bam_consensus_model.py), bit for bit: a mixed workload at odd byte offsets, lengths at
the lane, word and pass edges with the output buffers guarded, a cluster deep enough for the split path
under three settings of "cons_split", qualities at both ends, sums beyond 32 bits, a cluster without a
voter, the contract violations, and a call made while a deferred batched call is out."""
import numpy as np
import pytest

import bam_consensus_model as bm
from umi_collapse_rs_amd import Context, UmiHipError, synth
from umi_collapse_rs_amd._lib import UMI_ERR_ARG, UMI_ERR_ORDER, UMI_NO_CLUSTER

pytestmark = pytest.mark.gpu
FILL = 0xAB


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


class Case:
    """reads = [(packed sequence, quality bytes, length, cluster)], laid into one buffer the way a BAM
    holds them -- qualities right behind the sequence -- each read `gap(i)` bytes behind the one before"""

    def __init__(self, reads, cluster_len, gap=lambda i: 1 + i % 3):
        buf, sp, qp = bytearray(b"\x5a"), [], []
        for i, (s, q, L, c) in enumerate(reads):
            buf += b"\x5a" * gap(i)
            sp.append(len(buf))
            buf += s
            qp.append(len(buf))
            buf += q
        self.data = bytes(buf) + b"\x5a"
        self.seq_pos, self.qual_pos = np.array(sp, np.uint64), np.array(qp, np.uint64)
        self.lens = np.array([r[2] for r in reads], np.uint32)
        self.cluster = np.array([r[3] for r in reads], np.uint32)
        self.clen = np.array(cluster_len, np.uint32)
        self.reads = reads

    def want(self):
        voters = [[] for _ in self.clen]
        for s, q, L, c in self.reads:
            if c != UMI_NO_CLUSTER:
                voters[c].append((s, q))
        return [bm.vote(v, int(L)) for v, L in zip(voters, self.clen)]


def same(got, want):
    gs, gq, gd, ge = got
    assert len(gs) == len(want)
    for c, (s, q, d, e) in enumerate(want):
        assert gs[c] == s and gq[c] == q and int(gd[c]) == d and int(ge[c]) == e, (c, gs[c], s, gq[c], q, gd[c], d, ge[c], e)


def host_call(ctx, case):
    return ctx.consensus_bam(case.data, case.seq_pos, case.qual_pos, case.lens, case.cluster, case.clen)


def device_call(ctx, case, odd=1, disagree=True):
    """consensus_bam_device on torch buffers, the data `odd` bytes into its buffer; the outputs are filled
    with FILL first.  Returns what consensus_bam returns, and the raw output arrays."""
    import torch
    n, nc = len(case.lens), len(case.clen)
    t_data = dev_t(np.frombuffer(b"\0" * odd + case.data, np.uint8))
    t_sp, t_qp, t_len, t_cl, t_clen = (dev_t(case.seq_pos), dev_t(case.qual_pos), dev_t(case.lens), dev_t(case.cluster),
                                       dev_t(case.clen))
    cap_s, cap_q = int(((case.clen.astype(np.int64) + 1) // 2).sum()), int(case.clen.astype(np.int64).sum())
    o_seq = torch.full((cap_s + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    o_qual = torch.full((cap_q + 16,), FILL, dtype=torch.uint8, device="cuda:0")
    o_so = torch.full((max(nc, 1),), -1, dtype=torch.int64, device="cuda:0")
    o_qo = torch.full((max(nc, 1),), -1, dtype=torch.int64, device="cuda:0")
    o_d = torch.full((max(nc, 1),), -1, dtype=torch.int32, device="cuda:0")
    o_e = torch.full((max(nc, 1),), -1, dtype=torch.int32, device="cuda:0")
    torch.cuda.synchronize()
    try:
        sb, qb = ctx.consensus_bam_device(t_data.data_ptr() + odd, t_sp.data_ptr(), t_qp.data_ptr(), t_len.data_ptr(),
                                          t_cl.data_ptr(), n, t_clen.data_ptr(), nc, o_seq.data_ptr(), o_qual.data_ptr(),
                                          o_so.data_ptr(), o_qo.data_ptr(), o_d.data_ptr(), o_e.data_ptr() if disagree else 0)
    finally:
        torch.cuda.synchronize()
        raw = [t.cpu().numpy() for t in (o_seq, o_qual, o_so, o_qo, o_d, o_e)]
    s, q = raw[0].tobytes(), raw[1].tobytes()
    out_s, out_q, at_s, at_q = [], [], 0, 0
    for c in range(nc):  # dense, in ascending order
        L = int(case.clen[c])
        assert int(raw[2][c]) == at_s and int(raw[3][c]) == at_q
        out_s.append(s[at_s:at_s + (L + 1) // 2])
        out_q.append(q[at_q:at_q + L])
        at_s += (L + 1) // 2
        at_q += L
    assert (sb, qb) == (at_s, at_q) == (cap_s, cap_q)
    assert (raw[0][at_s:] == FILL).all() and (raw[1][at_q:] == FILL).all()  # nothing behind the last one
    return (out_s, out_q, raw[4].view(np.uint32)[:nc], raw[5].view(np.uint32)[:nc]), raw


def both_forms(ctx, case, want=None, odd=1):
    want = want or case.want()
    same(host_call(ctx, case), want)
    got, _ = device_call(ctx, case, odd=odd)
    same(got, want)
    return want


def family(rng, L, copies, err=0.01, odd_codes=0.0, qlo=0, qhi=61):
    """`copies` reads of one random molecule of L bases: (packed, quals) each"""
    mol = rng.integers(0, 4, L)
    out = []
    for _ in range(copies):
        s = np.where(rng.random(L) < err, rng.integers(0, 4, L), mol)
        nib = (1 << s).astype(np.int64)
        hit = rng.random(L) < odd_codes
        nib[hit] = rng.integers(0, 16, int(hit.sum()))
        out.append((bm.pack(nib), rng.integers(qlo, qhi, L).astype(np.uint8).tobytes()))
    return out


def mixed_case(seed=11, n_clusters=900):
    rng = np.random.default_rng(seed)
    reads, clen = [], []
    for c in range(n_clusters):
        L = int(rng.choice([36, 75, 100, 151]))
        clen.append(L)
        if c % 97 == 5:
            continue  # a cluster without a voter
        for s, q in family(rng, L, int(rng.geometric(0.25)), odd_codes=0.02):
            reads.append((s, q, L, c))
    for _ in range(len(reads) // 9):  # reads that vote nowhere, of any length
        L = int(rng.integers(0, 200))
        s, q = family(rng, L, 1)[0] if L else (b"", b"")
        reads.append((s, q, L, UMI_NO_CLUSTER))
    order = rng.permutation(len(reads))
    return Case([reads[i] for i in order], clen)


def test_mixed_workload(ctx):
    case = mixed_case()
    assert 3500 <= len(case.reads) <= 4800 and (case.cluster == UMI_NO_CLUSTER).sum() >= 300
    assert {int(p) & 3 for p in case.seq_pos} == {0, 1, 2, 3} and any(int(p) & 1 for p in case.qual_pos)
    want = both_forms(ctx, case)
    assert sum(1 for s, q, d, e in want if e > 0) >= 200 and sum(1 for s, q, d, e in want if d == 0) >= 5
    for odd in (2, 3):  # the buffer at every byte offset of a word
        got, _ = device_call(ctx, case, odd=odd)
        same(got, want)
    got, raw = device_call(ctx, case, disagree=False)  # disagree may be NULL
    same((got[0], got[1], got[2], [w[3] for w in want]), want)
    assert (raw[5] == -1).all()


def test_length_edges(ctx):
    lengths = [1, 2, 3, 7, 8, 9, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1023, 1024]
    rng = np.random.default_rng(77)
    reads, clen = [], []
    for L in lengths:
        for rep in range(2):
            c = len(clen)
            clen.append(L)
            for s, q in family(rng, L, 4 + int(rng.integers(0, 4)), err=0.05, odd_codes=0.02):
                if L & 1:  # the voters' own padding nibble is not 0: it must not vote, nor show
                    s = s[:-1] + bytes([s[-1] | int(rng.integers(1, 16))])
                reads.append((s, q, L, c))
    order = rng.permutation(len(reads))
    case = Case([reads[i] for i in order], clen)
    want = case.want()
    assert all(d >= 4 for s, q, d, e in want) and all(s[-1] & 15 == 0 for (s, q, d, e), L in zip(want, clen) if L & 1)
    for odd in (1, 2, 3, 4):  # (device_call checks the fill pattern behind the outputs, and the dense offsets)
        got, _ = device_call(ctx, case, odd=odd)
        same(got, want)
    same(host_call(ctx, case), want)


def vote_np(nib, qual):
    """the model's vote over arrays [voters, L] (int64 sums: exact here), for the cluster that plain Python
    would take a minute over; checked against the model below"""
    w = np.minimum(qual.astype(np.int64), 93)
    S = np.stack([(w * (nib == (1 << b))).sum(0) for b in range(4)])
    n = np.stack([(nib == (1 << b)).sum(0) for b in range(4)]).astype(np.int64)
    win = np.zeros(nib.shape[1], np.int64)
    for b in range(1, 4):
        ar = np.arange(len(win))
        better = (S[b] > S[win, ar]) | ((S[b] == S[win, ar]) & (n[b] > n[win, ar]))
        win = np.where(better, b, win)
    ar = np.arange(len(win))
    sw, nw = S[win, ar], n[win, ar]
    q = np.clip(sw - (S.sum(0) - sw), 0, 93)
    out_n = np.where(nw == 0, 15, 1 << win)
    q = np.where(nw == 0, 0, q)
    return bm.pack(out_n), q.astype(np.uint8).tobytes(), nib.shape[0], int((n.sum(0) - nw).sum())


def test_deep_cluster_three_settings():
    """one molecule read 50,000 times beside 2,000 small clusters: the split path by default, for every
    cluster of two voters or more, and for none"""
    rng = np.random.default_rng(5)
    L, n_deep = 300, 50_000
    small, clen = [], []
    for c in range(2000):
        clen.append(60)
        for s, q in family(rng, 60, int(rng.integers(1, 6))):
            small.append((s, q, 60, c))
    mol = rng.integers(0, 4, L)
    s = np.where(rng.random((n_deep, L)) < 0.01, rng.integers(0, 4, (n_deep, L)), mol)
    nib = (1 << s).astype(np.uint8)
    hit = rng.random(nib.shape) < 0.002
    nib[hit] = rng.integers(0, 16, int(hit.sum()))
    qual = rng.integers(0, 61, (n_deep, L)).astype(np.uint8)
    packed = ((nib[:, 0::2] << 4) | nib[:, 1::2]).astype(np.uint8)
    rows = np.concatenate([np.full((n_deep, 3), 0x5A, np.uint8), packed, qual], axis=1)  # three bytes, sequence, qualities
    case = Case(small, clen + [L])
    base = len(case.data)
    stride = rows.shape[1]
    case.data += rows.tobytes() + b"\x5a"
    at = base + 3 + stride * np.arange(n_deep, dtype=np.uint64)
    case.seq_pos = np.concatenate([case.seq_pos, at])
    case.qual_pos = np.concatenate([case.qual_pos, at + np.uint64(L // 2)])
    case.lens = np.concatenate([case.lens, np.full(n_deep, L, np.uint32)])
    case.cluster = np.concatenate([case.cluster, np.full(n_deep, 2000, np.uint32)])
    order = rng.permutation(len(case.lens))
    case.seq_pos, case.qual_pos, case.lens, case.cluster = (case.seq_pos[order], case.qual_pos[order], case.lens[order],
                                                            case.cluster[order])
    case.clen = np.array(clen + [L], np.uint32)
    case.clen[-1] = 60  # (want() over the small clusters only ...)
    want = case.want()[:-1]
    case.clen[-1] = L
    # ... the deep one from arrays, by a restatement that agrees with the model on a cluster it can take
    few = [(bm.pack(nib[i]), qual[i].tobytes()) for i in range(40)]
    assert vote_np(nib[:40].astype(np.int64), qual[:40]) == bm.vote(few, L)
    want.append(vote_np(nib.astype(np.int64), qual))
    assert want[-1][2] == n_deep and want[-1][3] > 100_000
    results = []
    for split in (None, 2, 1 << 30):
        c = Context(0)
        try:
            if split is not None:
                c.set_option("cons_split", split)
            got = host_call(c, case)
            same(got, want)
            dgot, _ = device_call(c, case, odd=3)
            same(dgot, want)
            results.append(got)
        finally:
            c.close()
    for g in results[1:]:
        assert g[0] == results[0][0] and g[1] == results[0][1]


def test_all_qualities_zero(ctx):
    """every S is 0: the vote falls to n, then to the order of ACGT"""
    seqs = ["ACGTACGTTT"] * 3 + ["ACGTACGTCC"] * 3 + ["CCGTACGTGN"] * 2
    case = Case([(bm.pack(s), bytes(10), 10, 0) for s in seqs], [10])
    want = case.want()
    assert want[0] == (bm.pack("ACGTACGTCC"), bytes(10), 8, 2 + 5 + 3)
    both_forms(ctx, case, want)


def test_highest_qualities_and_the_cap(ctx):
    rng = np.random.default_rng(9)
    n, L = 600, 100
    mol = rng.integers(0, 4, L)
    s = np.where(rng.random((n, L)) < 0.3, rng.integers(0, 4, (n, L)), mol)
    nib = 1 << s
    nib[:, 7] = 15
    nib[:n // 2, 8], nib[n // 2:, 8] = 4, 8                # a tie at the top: 300 x 93 each, G before T
    q93 = [(bm.pack(r), bytes([93]) * L, L, 0) for r in nib]
    q255 = [(bm.pack(r), bytes([93 if i & 1 else 255]) * L, L, 0) for i, r in enumerate(nib)]
    a, b = Case(q93, [L]), Case(q255, [L])
    want = a.want()
    assert b.want() == want                                  # 93 and 255 weigh the same
    s0, q0, d0, e0 = want[0]
    assert bm.nibbles(s0, L)[7:9] == [15, 4] and q0[7:9] == bytes(2) and q0.count(93) >= 90 and max(q0) == 93 and d0 == n
    both_forms(ctx, a, want)
    both_forms(ctx, b, want, odd=2)
    for split in (2, 1 << 30):
        c = Context(0)
        try:
            c.set_option("cons_split", split)
            same(host_call(c, b), want)
        finally:
            c.close()


def test_sums_beyond_32_bits(ctx):
    """2^26 voters of one base and quality 93 in one cluster, 2^24 of them C, the others A: S_A = 93 * 3 * 2^24
    is beyond 32 bits, and what is left of it in 32 bits is below S_C"""
    import torch
    n = 1 << 26
    dev = "cuda:0"
    data = torch.empty(2 * n + 8, dtype=torch.uint8, device=dev)  # the sequences' bytes, then the qualities
    data[:n] = 0x10
    data[: n // 4] = 0x2F   # (C; the padding nibble of a voter is not looked at)
    data[n:] = 93
    pos = torch.arange(2 * n, dtype=torch.int64, device=dev)  # seq_pos, then qual_pos = n + i
    lens = torch.ones(n, dtype=torch.int32, device=dev)
    cluster = torch.zeros(n, dtype=torch.int32, device=dev)
    clen = dev_t(np.array([1], np.uint32))
    o_seq = torch.full((8,), FILL, dtype=torch.uint8, device=dev)
    o_qual = torch.full((8,), FILL, dtype=torch.uint8, device=dev)
    o_off = torch.full((2,), -1, dtype=torch.int64, device=dev)
    o_de = torch.full((2,), -1, dtype=torch.int32, device=dev)

    def call():
        torch.cuda.synchronize()
        got = ctx.consensus_bam_device(data.data_ptr(), pos.data_ptr(), pos.data_ptr() + 8 * n, lens.data_ptr(),
                                       cluster.data_ptr(), n, clen.data_ptr(), 1, o_seq.data_ptr(), o_qual.data_ptr(),
                                       o_off.data_ptr(), o_off.data_ptr() + 8, o_de.data_ptr(), o_de.data_ptr() + 4)
        torch.cuda.synchronize()
        assert got == (1, 1) and o_off.tolist() == [0, 0]
        return bytes(o_seq[:2].cpu().numpy()), bytes(o_qual[:2].cpu().numpy()), o_de.tolist()

    assert call() == (bytes([0x10, FILL]), bytes([93, FILL]), [n, n // 4])
    # the other way round no quality is left: 2^25 A against 2^25 C, and one more C decides by n alone
    data[: n // 2] = 0x20
    data[n:] = 0
    assert call() == (bytes([0x10, FILL]), bytes([0, FILL]), [n, n // 2])  # a tie: the first of ACGT
    data[n // 2] = 0x20
    assert call() == (bytes([0x20, FILL]), bytes([0, FILL]), [n, n // 2 - 1])


def test_cluster_without_a_voter(ctx):
    reads = [(bm.pack("ACG"), bytes([30, 30, 30]), 3, 1), (bm.pack("ACGTA"), bytes(5), 5, UMI_NO_CLUSTER)]
    case = Case(reads, [5, 3, 0, 4])
    want = case.want()
    assert want[0] == (bytes([0xFF, 0xFF, 0xF0]), bytes(5), 0, 0) and want[2] == (b"", b"", 0, 0)
    assert want[3] == (bytes([0xFF, 0xFF]), bytes(4), 0, 0)
    both_forms(ctx, case, want)
    none = Case([(bm.pack("ACG"), bytes(3), 3, UMI_NO_CLUSTER)], [2])  # no voter at all
    both_forms(ctx, none, [(bytes([0xFF]), bytes(2), 0, 0)])


def small_case():
    rng = np.random.default_rng(3)
    reads, clen = [], []
    for c in range(150):
        L = (20, 51)[c & 1]
        clen.append(L)
        for s, q in family(rng, L, int(rng.integers(1, 7)), err=0.03):
            reads.append((s, q, L, c))
    return Case(reads, clen)


def refused(ctx, code, match, case):
    with pytest.raises(UmiHipError, match=match) as ei:
        host_call(ctx, case)
    assert ei.value.code == code
    with pytest.raises(UmiHipError, match=match) as ei:  # the device form: the same status
        device_call(ctx, case)
    assert ei.value.code == code


def device_outputs_untouched(ctx, case):
    """the device form once more, by hand: every output keeps its fill"""
    import torch
    n, nc = len(case.lens), len(case.clen)
    t = [dev_t(np.frombuffer(case.data, np.uint8)), dev_t(case.seq_pos), dev_t(case.qual_pos), dev_t(case.lens),
         dev_t(case.cluster), dev_t(case.clen)]
    outs = [torch.full((4096 * 8,), FILL, dtype=torch.uint8, device="cuda:0") for _ in range(6)]
    torch.cuda.synchronize()
    with pytest.raises(UmiHipError):
        ctx.consensus_bam_device(*[x.data_ptr() for x in t[:5]], n, t[5].data_ptr(), nc, *[o.data_ptr() for o in outs])
    torch.cuda.synchronize()
    assert all((o.cpu().numpy() == FILL).all() for o in outs)


def test_cluster_id_out_of_range(ctx):
    case = small_case()
    case.cluster[17] = len(case.clen)
    case.cluster[400] = 0xFFFFFFFE
    refused(ctx, UMI_ERR_ORDER, "2 reads break the input contract .cluster outside", case)
    device_outputs_untouched(ctx, case)


def test_voter_of_the_wrong_length(ctx):
    case = small_case()
    case.lens[5] += 1
    case.lens[9] = 1 << 31  # (nothing of it may be read)
    refused(ctx, UMI_ERR_ORDER, "2 voters break the input contract", case)
    device_outputs_untouched(ctx, case)
    ok = small_case()
    for i in (5, 9):  # a read that does not vote may have any length
        ok.cluster[i] = UMI_NO_CLUSTER
        ok.reads[i] = ok.reads[i][:3] + (UMI_NO_CLUSTER,)
    ok.lens[5] += 1
    ok.lens[9] = 1 << 31
    both_forms(ctx, ok)


def test_cluster_len_1025(ctx):
    case = small_case()
    case.clen[3] = 1025
    refused(ctx, UMI_ERR_ORDER, "1 clusters break the input contract .cluster_len above 1024", case)
    device_outputs_untouched(ctx, case)


def test_argument_errors(ctx):
    case = small_case()
    multi = Context([0, 0])
    try:
        with pytest.raises(UmiHipError, match="single-device context") as ei:
            host_call(multi, case)
        assert ei.value.code == UMI_ERR_ARG
        with pytest.raises(UmiHipError, match="single-device context") as ei:
            multi.consensus_bam_device(8, 8, 8, 8, 8, 4, 8, 2, 8, 8, 8, 8, 8, 8)
        assert ei.value.code == UMI_ERR_ARG
    finally:
        multi.close()
    # refused before any pointer is followed: n_reads = 2^30, and a NULL in every required place
    with pytest.raises(UmiHipError) as ei:
        ctx.consensus_bam_device(8, 8, 8, 8, 8, 1 << 30, 8, 2, 8, 8, 8, 8, 8, 8)
    assert ei.value.code == UMI_ERR_ARG
    for hole in (0, 1, 2, 3, 4, 6, 8, 9, 10, 11, 12):
        args = [8, 8, 8, 8, 8, 4, 8, 2, 8, 8, 8, 8, 8, 8]
        args[hole] = 0
        with pytest.raises(UmiHipError, match="NULL") as ei:
            ctx.consensus_bam_device(*args)
        assert ei.value.code == UMI_ERR_ARG
    both_forms(ctx, case)  # and the context still works


def test_while_a_deferred_call_is_out(ctx):
    """begin(A) -> consensus_bam -> end: the consensus is right, and so are A's outputs and counts"""
    import torch
    import oracle as orc
    pos, bases = synth.molecule_reads(seed=31, n_positions=3000, reads_per_position=25, umi_len=12, err=0.02)
    a = synth.stage(pos, synth.bases_to_keys(bases))
    assert int(np.diff(a["bucket_off"].astype(np.int64)).max()) <= 128
    case = small_case()
    want = case.want()
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
            same(host_call(ctx, case), want)
        else:
            got, _ = device_call(ctx, case, odd=1)
            same(got, want)
        stats = ctx.dedup_batch_end()
        torch.cuda.synchronize()
        assert np.array_equal(d_kept.cpu().numpy(), okept)
        assert np.array_equal(d_root.cpu().numpy().view(np.uint32), oroot)
        assert stats["n_kept"] == int(okept.sum()) and stats["n_umis"] == len(a["keys"])
