"""umicollapse --per-gene / --gene-tag / --count-matrix without a GPU: the refusals that end a run with status 101
before the GPU is woken, the staging (--dump-staging) against tests/gene_model.py, and the model's own
invariants -- the generator really fragments molecules over positions, per-gene grouping keeps fewer reads than
per-position grouping, count_model agrees with a brute-force count, and the model's matrix is the histogram of
its own output records."""
import os
import struct
import subprocess

import numpy as np
import pytest

import bamio
import gene_model as gm
import tag_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


@pytest.fixture(scope="module")
def bam():
    return gm.gene_bam(21)


def run(args):
    return subprocess.run([CLI] + args, capture_output=True, text=True, timeout=120)


def small_file(tmp_path, tags=None):
    header = bamio.make_header([("chr1", 100000)])
    z = tag_model.aux_z
    good = z("UB", "ACGTACGTAC") + z("CB", "AAAC-1")
    recs = [bamio.make_record("r0", 0, 0, 500, 60, [("M", 50)], 50, bytes([30] * 50), tags=good + z("GX", "G1")),
            bamio.make_record("r1", 0, 0, 700, 60, [("M", 50)], 50, bytes([30] * 50),
                              tags=good + (z("GX", "G1") if tags is None else tags))]
    src = str(tmp_path / "in.bam")
    tag_model.write_bam(src, header, recs)
    return src


REFUSALS = [
    (["--per-gene", "--two-pass"], "--per-gene does not go with --two-pass"),
    (["--per-gene", "--paired"], "--per-gene does not go with --paired"),
    (["--per-gene", "--keep-unmapped"], "--per-gene does not go with --keep-unmapped"),
    (["--per-gene", "--tag"], "--per-gene does not go with --tag"),
    (["--per-gene", "--call-consensus"], "--per-gene does not go with --call-consensus"),
    (["--per-gene", "--passthrough"], "--per-gene does not go with --passthrough"),
    (["--gene-tag", "GX"], "--gene-tag goes with --per-gene only"),
    (["--per-gene", "--gene-tag", "GXX"], "--gene-tag wants a tag name of two characters"),
    (["--per-gene", "--gene-tag", "G"], "--gene-tag wants a tag name of two characters"),
    (["--per-gene", "--gene-tag", "1X"], "--gene-tag wants a tag name of two characters"),
    (["--count-matrix", "DIR"], "--count-matrix goes with --per-gene only"),
    (["--per-gene", "--count-matrix", "DIR", "--dump-staging", "DUMP"], "--count-matrix does not go with --dump-staging"),
]


@pytest.mark.parametrize("flags,text", REFUSALS, ids=[" ".join(f) for f, _ in REFUSALS])
def test_refusals(tmp_path, flags, text):
    src = small_file(tmp_path)
    flags = [str(tmp_path / "m") if x == "DIR" else str(tmp_path / "s.bin") if x == "DUMP" else x for x in flags]
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB"] + flags)
    assert r.returncode == 101, r.stderr
    assert text in r.stderr, r.stderr
    assert not os.path.exists(str(tmp_path / "m")) and not os.path.exists(str(tmp_path / "o.bam"))


def test_fastq_mode_refuses_per_gene(tmp_path):
    src = tmp_path / "in.fq"
    src.write_text("@r1\nACGT\n+\nIIII\n")
    r = run(["-m", "fastq", "-i", str(src), "-o", str(tmp_path / "o.fq"), "--per-gene"])
    assert r.returncode == 101 and "--per-gene is defined in bam/sam mode only" in r.stderr, r.stderr


def test_count_matrix_directory(tmp_path):
    """made while the flags are looked at: a missing parent, or a file in its place, is status 101; a directory
    that is there is used (the run then goes on and ends without a GPU, which is not this test's matter)"""
    src = small_file(tmp_path)
    common = ["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB", "--per-gene", "--count-matrix"]
    r = run(common + [str(tmp_path / "no" / "such" / "dir")])
    assert r.returncode == 101 and "cannot make the directory" in r.stderr, r.stderr
    (tmp_path / "file").write_text("x")
    r = run(common + [str(tmp_path / "file")])
    assert r.returncode == 101 and "cannot make the directory" in r.stderr, r.stderr


def dump(tmp_path, header, recs, flags):
    src, out = str(tmp_path / "in.bam"), str(tmp_path / "stage.bin")
    tag_model.write_bam(src, header, recs)
    return run(["-i", src, "-o", str(tmp_path / "unused.bam"), "--dump-staging", out] + flags), out


@pytest.mark.parametrize("threads", [1, 4])
@pytest.mark.parametrize("per_cell", [False, True])
def test_staging_matches_the_model(tmp_path, bam, per_cell, threads):
    header, recs, _ = bam
    flags = ["--umi-tag", "UB", "--per-gene", "--merge", "avgqual", "--num-threads", str(threads)]
    r, out = dump(tmp_path, header, recs, flags + (["--per-cell"] if per_cell else []))
    assert r.returncode == 0, r.stderr
    got = gm.read_staging(out, per_cell=per_cell)
    exp = gm.stage(recs, per_cell=per_cell, merge="avgqual")
    assert got["umi_len"] == exp["umi_len"] == 10
    for f in ("keys", "nmask", "freq", "bucket_off", "bucket_gene") + (("bucket_cell",) if per_cell else ()):
        assert got[f].shape == exp[f].shape and (got[f] == exp[f]).all(), f
    assert (got["rep"].astype(np.int64) == exp["rep"].astype(np.int64)).all()
    c = exp["counters"]
    assert min(c["no_gene"], c["several"], c["no_umi"], c["genes"]) > 0
    assert "Number of reads without a gene tag: %d\n" % c["no_gene"] in r.stderr
    assert "Number of reads assigned to several genes: %d\n" % c["several"] in r.stderr
    assert "Number of genes: %d\n" % c["genes"] in r.stderr
    assert ("Number of (cell, gene) groups: %d\n" if per_cell else "Number of gene groups: %d\n") % c["groups"] in r.stderr
    assert "alignment positions" not in r.stderr
    assert c["groups"] == (c["genes"] if not per_cell else len(set(zip(exp["bucket_cell"], exp["bucket_gene"]))))


def test_gene_tag_names_another_tag(tmp_path):
    header = bamio.make_header([("chr1", 100000)])
    z = tag_model.aux_z
    recs = [bamio.make_record("r%d" % i, 0, 0, 500 + 100 * i, 60, [("M", 50)], 50, bytes([30] * 50),
                              tags=z("UB", "ACGTACGTAC") + z("GX", "A") + z("gn", g))
            for i, g in enumerate(["X", "Y", "X", "-"])]
    r, out = dump(tmp_path, header, recs, ["--umi-tag", "UB", "--per-gene", "--gene-tag", "gn"])
    assert r.returncode == 0, r.stderr
    got = gm.read_staging(out)
    assert list(got["bucket_off"]) == [0, 1, 2] and list(got["freq"]) == [2, 1] and list(got["bucket_gene"]) == [0, 1]
    assert "Number of reads without a gene tag: 1\n" in r.stderr


def test_the_input_fragments_molecules_and_per_gene_keeps_fewer(bam):
    _, recs, _ = bam
    seen = {}
    for rec in recs:
        r, aux = bamio.parse_record(rec), tag_model.parse_aux(rec)
        if r["flag"] & 0x4 or not all(t in aux for t in ("UB", "CB", "GX")) or gm.gene_class(aux["GX"][1]) != "one":
            continue
        seen.setdefault((aux["CB"][1], aux["GX"][1], aux["UB"][1]), set()).add((r["tid"], r["pos"], r["flag"] & 0x10))
    assert sum(len(v) >= 2 for v in seen.values()) > 0
    per_gene, st, kept = gm.expected_output(recs, per_cell=True)
    # the same reads grouped by (position, cell): the reads --per-gene would drop taken out first
    staged = [rec for rec in recs if gm.gene_class(tag_model.parse_aux(rec).get("GX", (None, None))[1]) == "one"]
    per_position, _, _ = tag_model.expected_output(staged, umi_tag="UB", per_cell=True)
    assert 0 < len(per_gene) < len(per_position)
    assert int(kept.sum()) == len(per_gene)
    # ... and on the records as they are (the reads without a gene then count on the other side as well)
    assert len(per_gene) < len(tag_model.expected_output(recs, umi_tag="UB", per_cell=True)[0])


def test_wrong_type_and_unprintable_value_end_the_run(tmp_path):
    src = small_file(tmp_path, b"GXi" + struct.pack("<i", 5))
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB", "--per-gene", "--dump-staging", str(tmp_path / "s")])
    assert r.returncode == 101 and "tag GX of read r1 is of type i, not Z" in r.stderr, r.stderr
    src = small_file(tmp_path, tag_model.aux_z("GX", "G\t1"))
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB", "--per-gene", "--dump-staging", str(tmp_path / "s")])
    assert r.returncode == 101 and "tag GX of read r1 holds a byte that is not a printable character: 9" in r.stderr, r.stderr
    src = small_file(tmp_path, b"GXZabc")  # (no NUL: a malformed aux block)
    r = run(["-i", src, "-o", str(tmp_path / "o.bam"), "--umi-tag", "UB", "--per-gene", "--dump-staging", str(tmp_path / "s")])
    assert r.returncode == 101 and "malformed aux block in read r1" in r.stderr, r.stderr


def brute_count(kept, freq, off, row, col):
    cells = {}
    for b in range(len(off) - 1):
        for e in range(int(off[b]), int(off[b + 1])):
            c = cells.setdefault((int(col[b]), int(row[b])), [0, 0])
            c[0] += 1 if kept[e] else 0
            c[1] += int(freq[e])
        # (a bucket without entries never reaches setdefault)
    return sorted((c, r, v[0], v[1]) for (c, r), v in cells.items())


@pytest.mark.parametrize("seed", range(6))
def test_count_model_agrees_with_a_brute_force_count(seed):
    rng = np.random.default_rng(seed)
    nb = int(rng.integers(1, 60))
    sizes = rng.integers(0, 5, nb) * (rng.random(nb) < 0.7)  # empty buckets among them
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
    n = int(off[-1])
    kept = (rng.integers(0, 3, n) * rng.integers(0, 2, n)).astype(np.uint8)  # (values other than 1 count as kept)
    freq = rng.integers(1, 50, n).astype(np.int32)
    row, col = rng.integers(0, 4, nb).astype(np.uint32), rng.integers(0, 3, nb).astype(np.uint32)  # repeated pairs
    r, c, m, rd = gm.count_model(kept, freq, off, row, col)
    got = list(zip(c.tolist(), r.tolist(), m.tolist(), rd.tolist()))
    assert got == brute_count(kept, freq, off, row, col)
    assert got == sorted(got) and len(set((a, b) for a, b, _, _ in got)) == len(got)


def test_count_model_edges():
    z = np.zeros(0)
    assert all(len(a) == 0 for a in gm.count_model(z, z, [0], z, z))
    assert all(len(a) == 0 for a in gm.count_model(z, z, [0, 0, 0], [9, 9], [9, 9]))
    r, c, m, rd = gm.count_model([0, 0, 0], [2 ** 31 - 1] * 3, [0, 3], [5], [6])
    assert (r.tolist(), c.tolist(), m.tolist(), rd.tolist()) == ([5], [6], [0], [3 * (2 ** 31 - 1)])


@pytest.mark.parametrize("per_cell", [False, True])
def test_the_models_matrix_is_the_histogram_of_its_output(bam, per_cell):
    _, recs, _ = bam
    out, st, kept = gm.expected_output(recs, per_cell=per_cell)
    files = gm.expected_matrix(st, kept)
    mol, reads = gm.parse_matrix(files)
    hist = gm.histogram(out, per_cell=per_cell)
    assert {k: v for k, v in mol.items() if v} == hist and sum(mol.values()) == len(out) > 0
    assert sum(reads.values()) == int(st["freq"].sum())
    assert files["features.tsv"].splitlines()[0] == st["genes"][0] + b"\t" + st["genes"][0] + b"\tGene Expression"
    assert files["barcodes.tsv"] == (b"".join(c + b"\n" for c in st["cells"]) if per_cell else b"all\n")
