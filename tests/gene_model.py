"""Test-side definition of --per-gene / --count-matrix (host/staging.hpp, umicollapse_main.cpp) and of
umi_count_matrix (csrc/umihip_count.hip), in plain Python over tests/bamio.py and tests/tag_model.py.

--per-gene: a staged read's gene is the value of its gene tag (GX, type Z); a bucket is (gene), with --per-cell
(cell, gene), whatever the alignment.  Reads without the tag, with an empty value, "-", or a value starting with
"__" or "Unassigned" have no gene; a value with ';' or ',' names several; both kinds are dropped and counted.
Genes and cells are numbered by first appearance among the staged reads, buckets by first appearance of the pair,
entries by the oracle's staging (freq descending, then first appearance).  Survivors come from the oracle's
batched dedup; the matrix is the count of kept entries (molecules) and the sum of freq (reads) per (cell, gene),
written as the four files of --count-matrix.  Also: a synthetic single-cell BAM in which one molecule -- the
same (cell, gene, UMI) -- is fragmented at several positions of its gene."""
import struct

import numpy as np

import bamio
import oracle as orc
import tag_model

GENE_TYPE = "Gene Expression"


def count_model(kept, freq, off, row, col):
    """umi_count_matrix in dictionaries: (out_row, out_col, molecules, reads) over the distinct (col, row) of the
    non-empty buckets, sorted by col, then row"""
    kept, freq, off = np.asarray(kept), np.asarray(freq), np.asarray(off).astype(np.int64)
    cells = {}
    for b in range(len(off) - 1):
        lo, hi = int(off[b]), int(off[b + 1])
        if lo == hi:
            continue
        c = cells.setdefault((int(col[b]), int(row[b])), [0, 0])
        c[0] += int(np.count_nonzero(kept[lo:hi]))
        c[1] += int(freq[lo:hi].astype(np.int64).sum())
    order = sorted(cells)
    return (np.array([r for _, r in order], np.uint32), np.array([c for c, _ in order], np.uint32),
            np.array([cells[p][0] for p in order], np.uint32), np.array([cells[p][1] for p in order], np.uint64))


def hamming(a, b):
    return sum(x != y or x == "N" for x, y in zip(a, b))


def correct_cell(raw, whitelist):
    """--cell-whitelist's rule on one barcode: itself where listed, else the one listed barcode a single
    substitution away (an N differs from every base), else None"""
    if raw in whitelist:
        return raw
    near = [w for w in whitelist if len(w) == len(raw) and hamming(raw, w) == 1]
    return near[0] if len(near) == 1 else None


def gene_bam(seed, n_positions=120, reads_per_position=15, n_cells=7, n_genes=12, umi_len=10, pool=4, err=0.03,
             no_gene=0.05, dash_gene=0.04, several=0.04, raw_err=0.15):
    """(header, records, cell barcodes): a coordinate-ordered BAM whose reads carry UB (the UMI), CB ("<16 bases>-1"),
    CR (the 16 bases, with a substitution in a share of the reads) and GX.  A gene spans n_positions / n_genes
    neighbouring positions; the UMIs of a (cell, gene) come from a pool of `pool`, so the same (cell, gene, UMI)
    occurs at several positions.  A share of the reads has no GX, GX:Z:-, a "__" / "Unassigned" value or GX:Z:a;b."""
    rng = np.random.default_rng(seed)
    letters = "ACGT"
    while True:
        cells = ["".join(letters[x] for x in rng.integers(0, 4, 16)) for _ in range(n_cells)]
        if all(hamming(a, b) >= 4 for i, a in enumerate(cells) for b in cells[:i]):  # (a substitution stays unambiguous)
            break
    pools = {}
    refs = [("chr1", 10_000_000), ("chr2", 5_000_000)]
    items, i = [], 0
    for p in range(n_positions):
        g = p * n_genes // n_positions
        for _ in range(reads_per_position):
            c = int(rng.integers(0, n_cells))
            if (c, g) not in pools:
                pools[(c, g)] = ["".join(letters[x] for x in rng.integers(0, 4, umi_len)) for _ in range(pool)]
            umi = pools[(c, g)][int(rng.integers(0, pool))]
            if rng.random() < err:
                at = int(rng.integers(0, umi_len))
                umi = umi[:at] + letters[(letters.index(umi[at]) + 1 + int(rng.integers(0, 3))) % 4] + umi[at + 1:]
            raw = cells[c]
            if rng.random() < raw_err:
                at = int(rng.integers(0, 16))
                raw = raw[:at] + ("N" if rng.random() < 0.2 else letters[(letters.index(raw[at]) + 1) % 4]) + raw[at + 1:]
            u = rng.random()
            if u < no_gene:
                gene = None
            elif u < no_gene + dash_gene:
                gene = ["-", "__no_feature", "Unassigned_NoFeatures", ""][int(rng.integers(0, 4))]
            elif u < no_gene + dash_gene + several:
                gene = "GENE%02d%sGENE%02d" % (g, ";,"[int(rng.integers(0, 2))], (g + 1) % n_genes)
            else:
                gene = "GENE%02d" % g
            tid, p0 = (0 if p % 5 else 1), 1000 + 10 * p
            flag = (0x10 if rng.random() < 0.2 else 0) | (0x4 if rng.random() < 0.02 else 0)
            tags = tag_model.aux_fields_before(rng)
            if rng.random() >= 0.02:
                tags += tag_model.aux_z("UB", umi)
            if rng.random() >= 0.02:
                tags += tag_model.aux_z("CB", cells[c] + "-1") + tag_model.aux_z("CR", raw)
            if gene is not None:
                tags += tag_model.aux_z("GX", gene)
            tags += b"xxi" + struct.pack("<i", i)
            quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
            items.append((tid, p0, i, bamio.make_record("r%d" % i, flag, tid, p0, int(rng.integers(0, 61)), [("M", 50)], 50,
                                                        quals, tags=tags)))
            i += 1
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    return bamio.make_header(refs), [t[3] for t in items], cells


def gene_class(value):
    """'none', 'several' or 'one' for a gene tag's value (None: no tag)"""
    if value is None or value == b"" or value == b"-" or value.startswith(b"__") or value.startswith(b"Unassigned"):
        return "none"
    return "several" if b";" in value or b"," in value else "one"


def stage(recs, per_gene=True, per_cell=False, umi_tag="UB", cell_tag="CB", gene_tag="GX", merge="mapqual", umi_len=0,
          cell_list=None):
    """The staging of umicollapse --per-gene: returns the staged dict -- keys, nmask, freq, rep (record indices),
    bucket_off, bucket_cell, bucket_gene, genes and cells (their names in id order), umi_len, counters."""
    assert per_gene
    rows = []  # (record index, cell name, gene name, UMI bytes, score)
    counters = dict(total=0, unmapped=0, no_umi=0, no_cell=0, no_gene=0, several=0, unlisted=0)
    for i, rec in enumerate(recs):
        r = bamio.parse_record(rec)
        counters["total"] += 1
        if r["flag"] & 0x4:
            counters["unmapped"] += 1
            continue
        aux = tag_model.parse_aux(rec)
        for t in (umi_tag, cell_tag if per_cell else None, gene_tag):
            assert t is None or t not in aux or aux[t][0] == "Z"
        gene = aux[gene_tag][1] if gene_tag in aux else None
        assert gene is None or all(0x21 <= ch <= 0x7e for ch in gene)
        miss = False
        if umi_tag not in aux:
            counters["no_umi"] += 1
            miss = True
        if per_cell and cell_tag not in aux:
            counters["no_cell"] += 1
            miss = True
        if gene_class(gene) == "none":
            counters["no_gene"] += 1
            miss = True
        if miss:
            continue
        if gene_class(gene) == "several":
            counters["several"] += 1
            continue
        umi = aux[umi_tag][1]
        if umi_len == 0:
            umi_len = len(umi)
        assert len(umi) == umi_len
        cell = aux[cell_tag][1] if per_cell else b""
        if per_cell and cell_list is not None:
            fixed = correct_cell(cell.decode(), cell_list)
            if fixed is None:
                counters["unlisted"] += 1
                continue
            cell = fixed.encode()
        score = r["mapq"] if merge == "mapqual" else orc.avg_qual(list(r["qual"]))
        rows.append((i, cell, gene, umi, score))
    cell_id, gene_id, group_id = {}, {}, {}
    bucket_ids, bucket_cell, bucket_gene = [], [], []
    for _, cell, gene, _, _ in rows:
        c = cell_id.setdefault(cell, len(cell_id))
        g = gene_id.setdefault(gene, len(gene_id))
        b = group_id.get((c, g))
        if b is None:
            b = group_id[(c, g)] = len(group_id)
            bucket_cell.append(c)
            bucket_gene.append(g)
        bucket_ids.append(b)
    umis = [u for _, _, _, u, _ in rows]
    ub = np.frombuffer(b"".join(umis), dtype=np.uint8) if umis else np.zeros(0, np.uint8)
    st = orc.stage_reads(bucket_ids, ub, [s for _, _, _, _, s in rows], max(umi_len, 1), merge=0 if merge == "any" else 1)
    rec_idx = np.array([i for i, _, _, _, _ in rows], dtype=np.int64)
    st["rep"] = rec_idx[st["rep"].astype(np.int64)] if rows else np.zeros(0, np.int64)
    st["bucket_cell"] = np.array(bucket_cell, np.uint32)
    st["bucket_gene"] = np.array(bucket_gene, np.uint32)
    st["genes"] = sorted(gene_id, key=gene_id.get)
    st["cells"] = sorted(cell_id, key=cell_id.get) if per_cell else [b"all"]
    st["per_cell"] = per_cell
    st["umi_len"] = umi_len
    counters["genes"], counters["groups"] = len(gene_id), len(group_id)
    st["counters"] = counters
    return st


def expected_output(recs, k=1, p=0.5, algo="dir", dedup=None, **kw):
    """(expected records in output order, staged dict, kept mask); dedup(st, k, p, algo) -> kept replaces the
    oracle's batched call (the Levenshtein model of --distance edit)"""
    st = stage(recs, **kw)
    if dedup is not None:
        kept = np.asarray(dedup(st, k, p, algo), np.uint8)
    else:
        call = orc.dedup_batch_wide if st["keys"].ndim == 2 else orc.dedup_batch
        kept, _, _ = call(st["keys"], st["nmask"], st["freq"], st["bucket_off"], max(st["umi_len"], 1), k, p,
                          0 if algo == "dir" else 1)
    return [recs[int(st["rep"][i])] for i in np.nonzero(kept)[0]], st, kept


def matrix_files(genes, cells, n_rows, n_cols, triplets):
    """the four files' bytes; triplets = (row, col, molecules, reads) arrays in the call's order"""
    row, col, mol, reads = triplets
    head = "%%%%MatrixMarket matrix coordinate integer general\n%d %d %d\n" % (n_rows, n_cols, len(row))
    body = lambda v: "".join("%d %d %d\n" % (int(r) + 1, int(c) + 1, int(x)) for r, c, x in zip(row, col, v))
    return {"features.tsv": b"".join(g + b"\t" + g + b"\t" + GENE_TYPE.encode() + b"\n" for g in genes),
            "barcodes.tsv": b"".join(c + b"\n" for c in cells),
            "matrix.mtx": (head + body(mol)).encode(), "reads.mtx": (head + body(reads)).encode()}


def expected_matrix(st, kept):
    """the four files of --count-matrix for a staged dict and its kept mask"""
    nb = len(st["bucket_off"]) - 1
    col = st["bucket_cell"] if st["per_cell"] else np.zeros(nb, np.uint32)
    trip = count_model(kept, st["freq"], st["bucket_off"], st["bucket_gene"], col)
    return matrix_files(st["genes"], st["cells"], len(st["genes"]), len(st["cells"]), trip)


def read_staging(path, per_cell=False):
    """the --dump-staging file of a --per-gene run: tag_model's fields, then every bucket's gene id"""
    with open(path, "rb") as f:
        n, nb, umi_len, w = struct.unpack("<4Q", f.read(32))
        keys = np.frombuffer(f.read(8 * n * w), np.uint64).reshape(n, w)
        nmask = np.frombuffer(f.read(8 * n * w), np.uint64).reshape(n, w)
        freq = np.frombuffer(f.read(4 * n), np.int32)
        rep = np.frombuffer(f.read(4 * n), np.uint32)
        off = np.frombuffer(f.read(8 * (nb + 1)), np.uint64)
        cell = np.frombuffer(f.read(4 * nb), np.uint32) if per_cell else None
        gene = np.frombuffer(f.read(4 * nb), np.uint32)
        assert len(gene) == nb and f.read() == b""
    if w == 1:
        keys, nmask = keys[:, 0], nmask[:, 0]
    return dict(keys=keys, nmask=nmask, freq=freq, rep=rep, bucket_off=off, bucket_cell=cell, bucket_gene=gene,
                umi_len=umi_len)


def histogram(records, cell_tag="CB", gene_tag="GX", per_cell=True):
    """{(cell bytes, gene bytes): records} over written records"""
    out = {}
    for rec in records:
        aux = tag_model.parse_aux(rec)
        key = (aux[cell_tag][1] if per_cell else b"all", aux[gene_tag][1])
        out[key] = out.get(key, 0) + 1
    return out


def parse_matrix(files):
    """{(cell bytes, gene bytes): value} of matrix.mtx, and of reads.mtx, by the names in the two .tsv files"""
    genes = [l.split(b"\t")[0] for l in files["features.tsv"].splitlines()]
    cells = files["barcodes.tsv"].splitlines()
    out = []
    for name in ("matrix.mtx", "reads.mtx"):
        lines = files[name].decode().splitlines()
        assert lines[0] == "%%MatrixMarket matrix coordinate integer general"
        g, c, nnz = (int(x) for x in lines[1].split())
        assert (g, c, nnz) == (len(genes), len(cells), len(lines) - 2)
        out.append({(cells[int(l.split()[1]) - 1], genes[int(l.split()[0]) - 1]): int(l.split()[2]) for l in lines[2:]})
        assert len(out[-1]) == nnz
    return out
