"""umicollapse --per-cell --cell-whitelist --cell-whitelist-multi end to end.  File A holds a few hundred reads with
a raw barcode in CR, its qualities in CY and the UMI in UR; file B the same records with every barcode replaced by
the model's answer (tests/barcode_multi_model.py: resolved reads included) and the unlisted and still ambiguous
reads left out.  The flag on A must pick the reads that plain --per-cell picks on B."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import barcode_model as bm
import barcode_multi_model as mm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
L = 16
UMIS = ["ACGTACGTAC", "ACGTACGTAA", "TTGGCCAATT", "GGGGTTTTCC", "CATGCATGCA", "TTTTTTTTTT"]
GENES = ["ENSG01", "ENSG02", "ENSG03"]


def build(barcodes, quals, keep, seed, reads_per_position, qual_tag="CY", spoil=None):
    """records of the reads in `keep`, read i with barcodes[i] in CR and quals[i] in `qual_tag`; everything else
    depends on i alone.  spoil = (i, how): read i's quality tag is left out, cut short or written as an integer"""
    refs = [("chr1", 10_000_000), ("chr2", 5_000_000)]
    items = []
    for i in keep:
        rng = np.random.default_rng([seed, i])
        umi = UMIS[int(rng.integers(0, len(UMIS)))]
        p = i // reads_per_position
        tid, p0 = (0 if p % 5 else 1), 1000 + 10 * p
        flag = 0x10 if rng.random() < 0.1 else 0
        tags = tag_model.aux_fields_before(rng) + tag_model.aux_z("UR", umi) + tag_model.aux_z("CR", barcodes[i])
        how = spoil[1] if spoil and spoil[0] == i else None
        if how == "short":
            tags += tag_model.aux_z(qual_tag, quals[i][:-1])
        elif how == "int":
            tags += qual_tag.encode() + b"C" + bytes([7])
        elif how == "byte":
            tags += tag_model.aux_z(qual_tag, " " + quals[i][1:])
        elif how != "missing":
            tags += tag_model.aux_z(qual_tag, quals[i])
        tags += tag_model.aux_z("GX", GENES[int(rng.integers(0, len(GENES)))])
        seq_quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
        items.append((tid, p0, i, bamio.make_record("r%d" % i, flag, tid, p0, int(rng.integers(0, 61)), [("M", 50)], 50,
                                                    seq_quals, tags=tags)))
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    return bamio.make_header(refs), [t[3] for t in items]


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


class Case:
    def __init__(self, tmp, seed=21, n_positions=6, reads_per_position=80, n_wl=10, permille=975, pseudo=0, qual_tag="CY"):
        rng = np.random.default_rng(seed)
        self.tmp, self.permille, self.pseudo, self.qual_tag = tmp, permille, pseudo, qual_tag
        self.wl, pairs = bm.random_list(rng, n_wl, L)
        self.n = n = n_positions * reads_per_position
        self.raw, q = mm.multi_reads(rng, self.wl, n, pairs)
        self.model = mm.correct_multi(self.raw, q, L, self.wl, permille, pseudo)
        self.plain = bm.correct(self.raw, L, self.wl, 1)
        rows = lambda a: [bytes(r).decode() for r in np.asarray(a).reshape(-1, L)]
        self.wl_rows, self.raw_rows, self.q_rows = rows(self.wl), rows(self.raw), rows(q)
        self.seed, self.rpp = seed, reads_per_position
        self.header, self.recs_a = build(self.raw_rows, self.q_rows, range(n), seed, reads_per_position, qual_tag)
        self.a = str(tmp / "a.bam")
        tag_model.write_bam(self.a, self.header, self.recs_a)
        self.list_file = str(tmp / "cells.txt")
        with open(self.list_file, "w") as f:
            f.write("\n".join(self.wl_rows) + "\n")

    def fixed_file(self, model, name):
        """the records whose barcode `model` matched, with the listed barcode in CR"""
        fixed = [self.wl_rows[m] if m >= 0 else None for m in model["match"]]
        _, recs = build(fixed, self.q_rows, np.flatnonzero(model["match"] >= 0), self.seed, self.rpp, self.qual_tag)
        path = str(self.tmp / name)
        tag_model.write_bam(path, self.header, recs)
        return path

    def run(self, src, extra, name):
        dst = str(self.tmp / name)
        r = subprocess.run([CLI, "-i", src, "-o", dst, "--per-cell", "--cell-tag", "CR", "--umi-tag", "UR"] + extra,
                           capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        return bamio.split_records(bamio.bgzf_decompress(open(dst, "rb").read()))[1], r.stderr

    def multi_flags(self):
        f = ["--cell-whitelist", self.list_file, "--cell-whitelist-multi"]
        if self.permille != 975:
            f += ["--cell-whitelist-min-posterior", "%d.%03d" % (self.permille // 1000, self.permille % 1000)]
        if self.pseudo:
            f += ["--cell-whitelist-pseudocount", str(self.pseudo)]
        if self.qual_tag != "CY":
            f += ["--cell-quality-tag", self.qual_tag]
        return f

    def compare(self, extra):
        got, log = self.run(self.a, extra + self.multi_flags(), "got.bam")
        exp, log_b = self.run(self.fixed_file(self.model, "b.bam"), extra, "exp.bam")
        ident = lambda r: (bamio.parse_record(r)["qname"], bamio.parse_record(r)["flag"])
        assert len(got) == len(exp) > 0 and [ident(r) for r in got] == [ident(r) for r in exp]
        c = self.model["counts"]
        assert int(line(log, "Number of reads with a corrected cell barcode")) == int(c[mm.CORRECTED])
        assert int(line(log, "Number of reads with a resolved cell barcode")) == int(c[mm.RESOLVED])
        assert int(line(log, "Number of reads with an unlisted cell barcode")) == int(c[mm.NONE])
        assert int(line(log, "Number of reads with an ambiguous cell barcode")) == int(c[mm.AMBIGUOUS])
        what = "Number of (cell, gene) groups" if "--per-gene" in extra else "Number of (position, cell) groups"
        assert line(log, what) == line(log_b, what) and line(log, "Number of UMIs") == line(log_b, "Number of UMIs")
        originals = set(self.recs_a)
        assert all(r in originals for r in got)  # written records are the input's, byte for byte
        return got, log


def test_resolved_reads_join_their_cells(tmp_path):
    c = Case(tmp_path)
    assert all(int(x) >= 8 for x in c.model["counts"]), c.model["counts"]  # every status occurs, resolved too
    c.compare(["-k", "1"])


def test_the_same_file_without_the_flag_is_as_before(tmp_path):
    c = Case(tmp_path)
    plain_flags = ["--cell-whitelist", c.list_file]
    got, log = c.run(c.a, ["-k", "1"] + plain_flags, "plain.bam")
    exp, _ = c.run(c.fixed_file(c.plain, "b_plain.bam"), ["-k", "1"], "plain_exp.bam")
    names = lambda recs: [bamio.parse_record(r)["qname"] for r in recs]
    assert names(got) == names(exp) and len(got) > 0
    assert "resolved" not in log
    assert int(line(log, "Number of reads with an ambiguous cell barcode")) == int(c.plain["counts"][bm.AMBIGUOUS])
    multi, _ = c.run(c.a, ["-k", "1"] + c.multi_flags(), "multi.bam")
    assert len(multi) > len(got)  # the resolved reads bring their molecules along
    metrics = str(tmp_path / "plain.tsv")
    c.run(c.a, ["-k", "0", "--cell-whitelist-metrics", metrics] + plain_flags, "m.bam")
    assert open(metrics).readline().rstrip("\n").split("\t") == ["barcode", "reads", "exact", "corrected"]


@pytest.mark.parametrize("extra", [
    ["-k", "0", "--stage", "host"],
    ["-k", "0", "--stage", "gpu"],
    ["-k", "1", "--per-gene", "--stage", "host"],
    ["-k", "1", "--per-gene", "--stage", "gpu"],
    ["-k", "1", "--algo", "cluster", "--num-threads", "4"],
], ids=lambda e: " ".join(e[2:]))
def test_combinations_give_the_models_grouping(tmp_path, extra):
    _, log = Case(tmp_path, seed=22).compare(extra)
    if "--stage" in extra:
        assert "staging (%s)" % extra[-1] in log


@pytest.mark.parametrize("kw", [dict(permille=500, pseudo=1), dict(permille=1000), dict(permille=0, pseudo=1000, qual_tag="QY")],
                         ids=lambda kw: "-".join("%s=%s" % kv for kv in kw.items()))
def test_the_rules_parameters_reach_the_call(tmp_path, kw):
    c = Case(tmp_path, seed=23, **kw)
    default = mm.correct_multi(c.raw, "".join(c.q_rows).encode(), L, c.wl)
    if kw != dict(permille=1000):
        assert int(default["counts"][mm.RESOLVED]) != int(c.model["counts"][mm.RESOLVED])  # (the parameters matter here)
    c.compare(["-k", "1"])


def test_count_matrix_and_metrics(tmp_path):
    c = Case(tmp_path, seed=24)
    out, metrics = str(tmp_path / "mtx"), str(tmp_path / "metrics.tsv")
    extra = ["-k", "1", "--per-gene"]
    c.run(c.a, extra + ["--count-matrix", out, "--cell-whitelist-metrics", metrics] + c.multi_flags(), "cm.bam")
    c.run(c.fixed_file(c.model, "b.bam"), extra + ["--count-matrix", str(tmp_path / "mtx_b")], "cm_b.bam")
    for f in ("features.tsv", "barcodes.tsv", "matrix.mtx", "reads.mtx"):  # the same cells, genes and numbers
        assert open(os.path.join(out, f)).read() == open(str(tmp_path / "mtx_b" / f)).read(), f
    rows = [l.split("\t") for l in open(metrics).read().splitlines()]
    assert rows[0] == ["barcode", "reads", "exact", "corrected", "resolved"]
    match, status = c.model["match"], c.model["status"]
    exp = []
    for w, bc in enumerate(c.wl_rows):  # in list order, the barcodes that took a read
        k = [int(((match == w) & (status == s)).sum()) for s in (mm.EXACT, mm.CORRECTED, mm.RESOLVED)]
        if sum(k):
            exp.append([bc, str(sum(k))] + [str(x) for x in k])
    assert rows[1:] == exp and sum(int(r[4]) for r in rows[1:]) == int(c.model["counts"][mm.RESOLVED]) > 0


@pytest.mark.parametrize("how, word", [("missing", "without the quality tag CY"), ("short", "holds 15 bytes, not 16"),
                                       ("int", "is of type C, not Z"), ("byte", "Unknown character in cell quality tag CY")])
def test_a_read_without_proper_qualities_ends_the_run(tmp_path, how, word):
    c = Case(tmp_path, seed=25, n_positions=3)
    _, recs = build(c.raw_rows, c.q_rows, range(c.n), c.seed, c.rpp, spoil=(101, how))
    bad = str(tmp_path / "bad.bam")
    tag_model.write_bam(bad, c.header, recs)
    dst = str(tmp_path / "x.bam")
    r = subprocess.run([CLI, "-i", bad, "-o", dst, "--per-cell", "--cell-tag", "CR", "--umi-tag", "UR", "-k", "1"] + c.multi_flags(),
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 101 and word in r.stderr and "r101" in r.stderr, r.stderr
    # without the flag the tag is not looked at
    r = subprocess.run([CLI, "-i", bad, "-o", dst, "--per-cell", "--cell-tag", "CR", "--umi-tag", "UR", "-k", "1",
                        "--cell-whitelist", c.list_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
