"""The consensus of BAM mode's clusters (--call-consensus), from its definition (include/umihip.h,
umi_consensus_bam) in plain Python with unbounded integers, a record builder that takes a real
sequence, a synthetic BAM whose clusters hold voters and non-voters, and the CLI's expected output on
top of bamio's / tag_model's staging and the oracle's collapse.  Nothing of the library is used."""
import struct

import numpy as np

import bamio
import oracle as orc

NIBBLES = "=ACMGRSVTWYHKDBN"
MAX_CONS_LEN = 1024
NO_CLUSTER = 0xFFFFFFFF


def pack(seq):
    """ASCII bases (str / bytes) or a sequence of nibble codes -> BAM's 4-bit packing, high nibble first,
    the unused low nibble of an odd length 0"""
    if isinstance(seq, (str, bytes)):
        s = seq.decode() if isinstance(seq, bytes) else seq
        nib = [NIBBLES.index(c) for c in s]
    else:
        nib = [int(x) for x in seq]
    nib = nib + [0] * (len(nib) & 1)
    return bytes((nib[i] << 4) | nib[i + 1] for i in range(0, len(nib), 2))


def nibbles(packed, length):
    return [(packed[c >> 1] >> (0 if c & 1 else 4)) & 15 for c in range(length)]


def vote(voters, length):
    """voters = [(packed sequence, quality bytes)] of `length` bases -> (packed consensus, its quality
    bytes, depth, disagree)"""
    out_n, out_q, disagree = [], [], 0
    rows = [(nibbles(s, length), q) for s, q in voters]
    for c in range(length):
        S, n = [0, 0, 0, 0], [0, 0, 0, 0]
        for nib, q in rows:
            if nib[c] in (1, 2, 4, 8):
                b = (1, 2, 4, 8).index(nib[c])
                S[b] += min(q[c], 93)
                n[b] += 1
        win = 0
        for b in range(1, 4):
            if (S[b], n[b]) > (S[win], n[win]):
                win = b
        if n[win] == 0:
            out_n.append(15)
            out_q.append(0)
        else:
            out_n.append(1 << win)
            out_q.append(min(93, max(0, S[win] - (sum(S) - S[win]))))
        disagree += sum(n) - n[win]
    return pack(out_n), bytes(out_q), len(voters), disagree


def make_record(qname, flag, tid, pos, mapq, cigar, seq, quals, tags=b"", mtid=-1, mpos=-1, tlen=0):
    """bamio.make_record's layout with a real sequence (see pack)"""
    qn = qname.encode() + b"\0"
    cig = b"".join(struct.pack("<I", (l << 4) | bamio.CIGAR_OPS.index(op)) for op, l in cigar)
    quals = bytes(quals)
    l_seq = len(quals)
    ps = pack(seq)
    assert len(ps) == (l_seq + 1) // 2
    body = struct.pack("<iiBBHHHiiii", tid, pos, len(qn), mapq, 4680, len(cigar), flag, l_seq, mtid, mpos,
                       tlen) + qn + cig + ps + quals + tags
    return struct.pack("<i", len(body)) + body


def fields(rec):
    """(offset of the sequence, l_seq, cigar bytes) of a record"""
    l_rn, n_cig, l_seq = rec[4 + 8], struct.unpack_from("<H", rec, 4 + 12)[0], struct.unpack_from("<i", rec, 4 + 16)[0]
    o = 4 + 32 + l_rn
    return o + 4 * n_cig, l_seq, rec[o:o + 4 * n_cig]


def seq_qual(rec):
    o, l_seq, _ = fields(rec)
    sb = (l_seq + 1) // 2
    return rec[o:o + sb], rec[o + sb:o + sb + l_seq]


CIGARS = {"50M": [("M", 50)], "5S45M": [("S", 5), ("M", 45)], "20M2D30M": [("M", 20), ("D", 2), ("M", 30)],
          "20M1I29M": [("M", 20), ("I", 1), ("M", 29)], "49M": [("M", 49)]}


def pos_for(cigar, reverse, anchor):
    """the POS at which a read of this CIGAR has the unclipped 5' position `anchor`"""
    r = dict(flag=0x10 if reverse else 0, pos=0, cigar=cigar)
    return anchor - bamio.unclipped_pos(r)


def synthetic_bam(seed, n_positions=150, reads_per_position=14, umi_len=10, err=0.01, tags=True):
    """Molecules with a sequence of their own: per position a few molecules (true UMI, 50 true bases), every
    read a copy with `err` errors per base in both.  Most reads are 50M; some 5S45M, 20M2D30M, 20M1I29M at
    the same unclipped position, a few 49 bases long, some without qualities (0xFF, and a MAPQ that makes
    them representatives), a few ambiguity codes; both strands, two references.  With `tags`, RX / CB as
    tag_model.tagged_bam writes them."""
    import tag_model
    rng = np.random.default_rng(seed)
    refs = [("chr1", 10_000_000), ("chr2", 5_000_000)]
    cells = ["".join("ACGT"[x] for x in rng.integers(0, 4, 16)) + "-1" for _ in range(3)]
    items, i = [], 0
    for p in range(n_positions):
        tid = 1 if p % 4 == 0 else 0
        reverse = p % 3 == 0
        anchor = 2000 + 100 * p
        left = reads_per_position
        while left > 0:
            copies = min(left, int(rng.geometric(0.35)))
            left -= copies
            umi = rng.integers(0, 4, umi_len)
            mol = rng.integers(0, 4, 50)
            cell = cells[int(rng.integers(0, len(cells)))]
            for _ in range(copies):
                u = np.where(rng.random(umi_len) < err, rng.integers(0, 4, umi_len), umi)
                s = np.where(rng.random(50) < err, rng.integers(0, 4, 50), mol)
                nib = [1 << int(x) for x in s]
                if rng.random() < 0.05:
                    nib[int(rng.integers(0, 50))] = int(rng.integers(0, 16))
                x = rng.random()
                name = "50M" if x < 0.80 else "5S45M" if x < 0.86 else "20M2D30M" if x < 0.91 else "20M1I29M" if x < 0.96 else "49M"
                cigar = CIGARS[name]
                if name == "49M":
                    nib = nib[:49]
                quals = rng.integers(2, 42, len(nib)).astype(np.uint8).tobytes()
                mapq = int(rng.integers(0, 61))
                if rng.random() < 0.04:
                    quals, mapq = b"\xff" * len(nib), 70
                ustr = "".join("ACGT"[int(b)] for b in u)
                aux = b""
                if tags:
                    aux = tag_model.aux_fields_before(rng)
                    if rng.random() >= 0.03:
                        aux += tag_model.aux_z("RX", ustr)
                    if rng.random() >= 0.03:
                        aux += tag_model.aux_z("CB", cell)
                pos = pos_for(cigar, reverse, anchor)
                items.append((tid, pos, i, make_record("r%d_%s" % (i, ustr), 0x10 if reverse else 0, tid, pos, mapq, cigar,
                                                       nib, quals, tags=aux)))
                i += 1
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    return bamio.make_header(refs), [t[3] for t in items]


def expected_output(recs, k=1, p=0.5, algo="dir", min_reads=1, stage=None, **kw):
    """The CLI's --call-consensus output: the records of a plain run in the same order, each kept record with
    its cluster's consensus and cD / cs / ce.  stage: bamio.stage_like_reference (default) or tag_model.stage.
    Returns (records, dict(kept, below, without, changed): the counts of the summary, and the records whose
    consensus bases differ from the representative's own)."""
    st, pre = (stage or bamio.stage_like_reference)(recs, **kw)
    kept, root, _ = orc.dedup_batch(st["keys"], st["nmask"], st["freq"], st["bucket_off"], st["umi_len"], k, p,
                                    0 if algo == "dir" else 1)
    cluster_reads = np.zeros(len(kept), np.int64)
    np.add.at(cluster_reads, root.astype(np.int64), st["freq"])
    index = {}
    off = st["bucket_off"].astype(np.int64)
    for b in range(len(off) - 1):
        for e in range(off[b], off[b + 1]):
            index[(b, int(st["keys"][e]))] = e
    members = {}
    for ri, b, umi in st["reads"]:
        key, _ = orc.encode_keys([umi.decode()])
        members.setdefault(int(root[index[(b, int(key[0]))]]), []).append(ri)
    out = [recs[i] for i in pre]
    counts = dict(kept=int(kept.sum()), below=0, without=0, changed=0)
    for r in np.flatnonzero(kept):
        rep = recs[int(st["rep"][r])]
        o, l_seq, cigar = fields(rep)
        rs, rq = seq_qual(rep)
        if l_seq == 0 or rq[0] == 0xFF:
            counts["without"] += 1
            out.append(rep)
            continue
        assert l_seq <= MAX_CONS_LEN
        voters = []
        for ri in members[int(r)]:
            _, l2, c2 = fields(recs[ri])
            s2, q2 = seq_qual(recs[ri])
            if l2 == l_seq and c2 == cigar and q2[0] != 0xFF:
                voters.append((s2, q2))
        cs, cq, depth, disagree = vote(voters, l_seq)
        if depth < min_reads:
            counts["below"] += 1
            continue
        counts["changed"] += cs != rs
        sb = (l_seq + 1) // 2
        tags = b"".join(t + b"i" + struct.pack("<i", int(v)) for t, v in
                        ((b"cD", depth), (b"cs", cluster_reads[r]), (b"ce", disagree)))
        body = rep[4:o] + cs + cq + rep[o + sb + l_seq:] + tags
        out.append(struct.pack("<i", len(body)) + body)
    return out, counts
