"""The consensus of fastq mode's clusters, from its definition (include/umihip.h, umi_consensus_seqs) in
plain Python with unbounded integers, and the CLI's --consensus output on top of seq_model's staging,
collapse and record layout.  Nothing of the library is used here."""
import seq_model as sm

ACGT = b"ACGT"


def column(votes):
    """One column: votes = [(base byte, quality byte)] of the members -> (called base, quality byte).
    S_b = sum of max(0, q - 33), n_b = voters of base b; the greatest (S_b, n_b) wins, the first of
    ACGT on a tie; nobody voted (only N): N with '!'; else 33 + min(93, max(0, S_win - S_others))."""
    S = {b: 0 for b in ACGT}
    n = {b: 0 for b in ACGT}
    for b, q in votes:
        if b in S:
            S[b] += max(0, q - 33)
            n[b] += 1
    win = ACGT[0]
    for b in ACGT[1:]:
        if (S[b], n[b]) > (S[win], n[win]):
            win = b
    if n[win] == 0:
        return ord("N"), ord("!")
    others = sum(S.values()) - S[win]
    return win, 33 + min(93, max(0, S[win] - others))


def consensus(members):
    """members = [(seq bytes, qual bytes)] of one length -> (consensus seq, consensus qual)."""
    L = len(members[0][0])
    assert all(len(s) == L and len(q) == L for s, q in members)
    cols = [column([(s[c], q[c]) for s, q in members]) for c in range(L)]
    return bytes(b for b, _ in cols), bytes(q for _, q in cols)


def clusters(seqs, quals, entry_of_read, kept, root):
    """Per kept entry in ascending order: (entry, consensus seq, consensus qual, members)."""
    members = {}
    for i, e in enumerate(entry_of_read):
        members.setdefault(int(root[int(e)]), []).append((seqs[i], quals[i]))
    out = []
    for r in range(len(kept)):
        if kept[r]:
            s, q = consensus(members[r])
            out.append((r, s, q, len(members[r])))
    return out


def entry_of_reads(seqs, ent):
    entry = {e[0]: j for j, e in enumerate(ent)}
    return [entry[s] for s in seqs]


def output(seqs, quals, names, ent, kept, root, trim=0, min_reads=1):
    """The CLI's --consensus output: the records of seq_model.output (the kept entries' representative
    reads in file order), the header with " cluster_size=<members>", sequence and quality replaced by
    the cluster's consensus (trimmed like any read); clusters under min_reads left out.  Returns
    (text, clusters left out)."""
    cons = {r: (s, q, m) for r, s, q, m in clusters(seqs, quals, entry_of_reads(seqs, ent), kept, root)}
    rep_of = {e[2]: j for j, e in enumerate(ent)}
    out, dropped = [], 0
    for i in range(len(seqs)):
        j = rep_of.get(i)
        if j is None or not kept[j]:
            continue
        s, q, m = cons[j]
        if m < min_reads:
            dropped += 1
            continue
        out.append(b"@" + names[i] + b" cluster_size=%d" % m + b"\n" + s[trim:] + b"\n+\n" + q[trim:] + b"\n")
    return b"".join(out), dropped


def expected_cli(seqs, quals, names, k, algo, merge, trim=0, min_reads=1):
    ent, off, blen = sm.stage(seqs, quals, merge)
    kept, root = sm.dedup(ent, off, blen, k, algo)
    return output(seqs, quals, names, ent, kept, root, trim, min_reads)
