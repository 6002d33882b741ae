"""Test-side definition of umi_filter_multigene (csrc/umihip_multigene.hip) and of --umi-filtering multi-gene
(host/umicollapse_main.cpp), in plain Python, independent of the library.

A molecule is an entry with kept != 0; its UMI is its key below bit 3 * umi_len, its reads total[r] = the sum of
freq[i] over root[i] == r.  The molecules of non-empty buckets with the same (group, UMI) form a run.  A run of one
survives; in a longer run the molecule whose total is strictly greater than every other's survives, and where two or
more hold the greatest total none does.  kept_out marks the survivors, freq_out is freq with the entries of removed
roots zeroed, counts = runs of two or more, molecules removed, the sum of their totals.

filter_model states it with a dictionary of runs, brute_filter with a double loop over molecules.  multigene_bam is
a small --per-cell --per-gene BAM in which every case of the rule is planted; expected() is the program's output
on it."""
import struct

import numpy as np

import bamio
import gene_model as gm
import oracle as orc
import stats_model as sm
import tag_model


def _molecules(keys, freq, kept, root, bucket_off, group, umi_len, n_words):
    """[(entry, group, UMI as an integer, total)] over the kept entries, in entry order"""
    nw = n_words or sm.n_words_of(umi_len)
    keys = np.asarray(keys, np.uint64).reshape(-1)
    off = [int(x) for x in np.asarray(bucket_off)]
    n = off[-1] if off else 0
    total = [0] * n
    for i in range(n):
        total[int(root[i])] += int(freq[i])
    mask = (1 << (3 * umi_len)) - 1
    out = []
    for b in range(len(off) - 1):
        for i in range(off[b], off[b + 1]):
            if kept[i]:
                out.append((i, int(group[b]), sm.key_int(keys, i, nw) & mask, total[i]))
    return out, n


def _outputs(mols, removed, runs, n, freq, root):
    kept_out = np.zeros(n, np.uint8)
    for i, _, _, _ in mols:
        if i not in removed:
            kept_out[i] = 1
    freq_out = np.array([0 if int(root[i]) in removed else int(freq[i]) for i in range(n)], np.int32).reshape(n)
    reads = sum(t for i, _, _, t in mols if i in removed)
    return kept_out, freq_out, {"runs": runs, "removed": len(removed), "removed_reads": reads & sm.M64}


def filter_model(keys, freq, kept, root, bucket_off, group, umi_len, n_words=None):
    """(kept_out uint8 [N], freq_out int32 [N], {"runs", "removed", "removed_reads"})"""
    mols, n = _molecules(keys, freq, kept, root, bucket_off, group, umi_len, n_words)
    runs = {}
    for i, g, u, t in mols:
        runs.setdefault((g, u), []).append((t, i))
    removed, longer = set(), 0
    for members in runs.values():
        if len(members) < 2:
            continue
        longer += 1
        top = max(t for t, _ in members)
        holders = [i for t, i in members if t == top]
        removed.update(i for _, i in members if len(holders) > 1 or i != holders[0])
    return _outputs(mols, removed, longer, n, freq, root)


def brute_filter(keys, freq, kept, root, bucket_off, group, umi_len, n_words=None):
    """the same, molecule against molecule: a molecule is removed iff another of its group and UMI has at least as
    many reads; a run is counted at its first molecule"""
    mols, n = _molecules(keys, freq, kept, root, bucket_off, group, umi_len, n_words)
    removed, runs = set(), 0
    for a, (i, g, u, t) in enumerate(mols):
        others_before = others = 0
        for b, (j, g2, u2, t2) in enumerate(mols):
            if a == b or g != g2 or u != u2:
                continue
            others += 1
            others_before += b < a
            if t2 >= t:
                removed.add(i)
        runs += others > 0 and others_before == 0
    return _outputs(mols, removed, runs, n, freq, root)


# ---- the program's side

CLASSES = ("two genes, strict winner", "two genes, tie", "three genes, strict winner over a tie", "three genes, tie at the top",
           "a removed entry holds another gene's UMI", "a total through root[] decides", "the same UMI in two cells")


def multigene_bam(seed, umi_len=10, n_cells=3, n_genes=5, background=60):
    """(header, records): reads with UB, CB and GX.  Cell 0 holds, among background molecules of their own UMIs:
    U1 in genes 0 / 1 with 3 and 1 reads; U2 in genes 0 / 1 with 2 and 2; U3 in genes 0 / 1 / 2 with 5, 3, 3; U4 in
    genes 0 / 1 / 2 with 4, 4, 1; U5 in gene 0 with 2 reads, and in gene 1 with 1 read beside a neighbour of 5 reads one
    substitution away, which takes it in; U6 in gene 2 with 4 reads and in gene 3 with 3 reads and a neighbour of 1 read
    that U6 takes in there (4 against 3 + 1: a tie only by the totals); U7 in gene 0 of cells 0 and 1.  Cell 1 holds
    U8 in gene 0 and, with 2 reads each, in a gene of its own that nothing else uses: that (cell, gene) pair is left
    without a molecule."""
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    far = lambda u, pool: all(gm.hamming(u, v) >= 3 for v in pool)
    umis = []
    while len(umis) < 8 + background:
        u = "".join(letters[x] for x in rng.integers(0, 4, umi_len))
        if far(u, umis):
            umis.append(u)
    sub = lambda u, at: u[:at] + letters[(letters.index(u[at]) + 1) % 4] + u[at + 1:]
    u1, u2, u3, u4, u5, u6, u7, u8 = umis[:8]
    cells = ["".join(letters[x] for x in rng.integers(0, 4, 16)) + "-1" for _ in range(n_cells)]
    reads = []  # (cell, gene, UMI, count)
    reads += [(0, 0, u1, 3), (0, 1, u1, 1)]
    reads += [(0, 0, u2, 2), (0, 1, u2, 2)]
    reads += [(0, 0, u3, 5), (0, 1, u3, 3), (0, 2, u3, 3)]
    reads += [(0, 0, u4, 4), (0, 1, u4, 4), (0, 2, u4, 1)]
    reads += [(0, 0, u5, 2), (0, 1, u5, 1), (0, 1, sub(u5, 3), 5)]
    reads += [(0, 2, u6, 4), (0, 3, u6, 3), (0, 3, sub(u6, 5), 1)]
    reads += [(0, 0, u7, 2), (1, 0, u7, 2)]
    reads += [(1, 0, u8, 2), (1, n_genes, u8, 2)]
    for u in umis[8:]:
        reads.append((int(rng.integers(0, n_cells)), int(rng.integers(0, n_genes)), u, int(rng.integers(1, 5))))
        if rng.random() < 0.3:  # (some of them in a second gene or cell as well)
            reads.append((int(rng.integers(0, n_cells)), int(rng.integers(0, n_genes)), u, int(rng.integers(1, 5))))
    items, i = [], 0
    for c, g, u, count in reads:
        for _ in range(count):
            pos = 1000 + 10 * int(rng.integers(0, 200))
            tags = tag_model.aux_z("UB", u) + tag_model.aux_z("CB", cells[c]) + tag_model.aux_z("GX", "GENE%02d" % g)
            tags += b"xxi" + struct.pack("<i", i)
            quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
            items.append((pos, i, bamio.make_record("r%d" % i, 0, 0, pos, int(rng.integers(0, 61)), [("M", 50)], 50, quals, tags=tags)))
            i += 1
    items.sort(key=lambda t: (t[0], t[1]))
    return bamio.make_header([("chr1", 10_000_000)]), [t[2] for t in items]


def collapse(st, k=1, p=0.5, algo="dir", dedup=None):
    """(kept, root) of a staged dict: the oracle's batched call, or dedup(st, k, p, algo) -> (kept, root)"""
    if dedup is not None:
        kept, root = dedup(st, k, p, algo)
        return np.asarray(kept, np.uint8), np.asarray(root, np.uint32)
    call = orc.dedup_batch_wide if st["keys"].ndim == 2 else orc.dedup_batch
    kept, root, _ = call(st["keys"], st["nmask"], st["freq"], st["bucket_off"], max(st["umi_len"], 1), k, p, 0 if algo == "dir" else 1)
    return np.asarray(kept, np.uint8), np.asarray(root, np.uint32)


def groups_of(st):
    nb = len(st["bucket_off"]) - 1
    return (st["bucket_cell"], len(st["cells"])) if st["per_cell"] else (np.zeros(nb, np.uint32), 1)


def expected(recs, per_cell=True, k=1, p=0.5, algo="dir", dedup=None, **kw):
    """what --umi-filtering multi-gene writes: dict of records (in output order), files (the four of --count-matrix),
    st, kept / root (the collapse's), kept_out / freq_out / counts (the filter's)"""
    st = gm.stage(recs, per_cell=per_cell, **kw)
    kept, root = collapse(st, k, p, algo, dedup)
    group, _ = groups_of(st)
    kept_out, freq_out, counts = filter_model(st["keys"], st["freq"], kept, root, st["bucket_off"], group, st["umi_len"])
    row, col, mol, reads = gm.count_model(kept_out, freq_out, st["bucket_off"], st["bucket_gene"], group)
    some = mol != 0  # (a pair that lost all its molecules is left out)
    files = gm.matrix_files(st["genes"], st["cells"], len(st["genes"]), len(st["cells"]), (row[some], col[some], mol[some], reads[some]))
    return dict(records=[recs[int(st["rep"][i])] for i in np.nonzero(kept_out)[0]], files=files, st=st, kept=kept, root=root,
                kept_out=kept_out, freq_out=freq_out, counts=counts)


def classes(e):
    """the cases of the rule that occur in an expected() dict, as a set of CLASSES"""
    st, kept, root, kept_out = e["st"], e["kept"], e["root"], e["kept_out"]
    group, _ = groups_of(st)
    off = st["bucket_off"].astype(np.int64)
    bucket = np.repeat(np.arange(len(off) - 1), np.diff(off))
    keys = np.asarray(st["keys"], np.uint64).reshape(-1)
    total = np.zeros(len(keys), np.int64)
    np.add.at(total, root.astype(np.int64), st["freq"].astype(np.int64))
    runs, by_umi = {}, {}
    for i in np.nonzero(kept)[0]:
        runs.setdefault((int(group[bucket[i]]), int(keys[i])), []).append(int(i))
        by_umi.setdefault(int(keys[i]), set()).add(int(group[bucket[i]]))
    found = set()
    for (g, u), members in runs.items():
        t = sorted((int(total[i]) for i in members), reverse=True)
        alive = [i for i in members if kept_out[i]]
        if len(members) == 2:
            found.add(CLASSES[0] if t[0] > t[1] else CLASSES[1])
            assert len(alive) == (1 if t[0] > t[1] else 0)
            f = sorted((int(st["freq"][i]) for i in members), reverse=True)
            if t[0] == t[1] and f[0] != f[1]:
                found.add(CLASSES[5])
        if len(members) == 3 and t[0] > t[1] == t[2]:
            found.add(CLASSES[2])
            assert len(alive) == 1 and int(total[alive[0]]) == t[0]
        if len(members) == 3 and t[0] == t[1] > t[2]:
            found.add(CLASSES[3])
            assert not alive
        if len(members) == 1 and len(by_umi[u]) > 1:
            found.add(CLASSES[6])
            assert len(alive) == 1
        # an entry that its bucket's collapse removed, with this run's UMI, in another bucket of the group
        for i in np.nonzero((keys == np.uint64(u)) & (kept == 0))[0]:
            if int(group[bucket[i]]) == g and len(members) == 1 and kept_out[members[0]] and bucket[i] != bucket[members[0]]:
                found.add(CLASSES[4])
    return found
