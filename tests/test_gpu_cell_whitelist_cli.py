"""umicollapse --per-cell --cell-whitelist end to end.  File A holds reads whose CR tag is a listed cell barcode
with sequencing errors (substitutions, N, some beyond correction, some ambiguous); file B the same records with
every barcode replaced by the model's correction (tests/barcode_model.py) and the unlisted and ambiguous reads
left out.  --cell-whitelist on A must pick the reads that plain --per-cell picks on B: the correction changes
how reads are grouped and nothing else."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import barcode_model as bm
import tag_model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
L = 16
UMIS = ["ACGTACGTAC", "ACGTACGTAA", "TTGGCCAATT", "GGGGTTTTCC", "CATGCATGCA", "TTTTTTTTTT"]


def build(barcodes, keep, rng_seed, reads_per_position, in_name=False, paired=False):
    """records of the reads in `keep` (indices), read i with cell barcode barcodes[i] in CR; everything but the
    barcode depends on i alone, so that two calls give the same records apart from it"""
    refs = [("chr1", 10_000_000), ("chr2", 5_000_000)]
    items = []
    for i in keep:
        rng = np.random.default_rng([rng_seed, i])
        umi = UMIS[int(rng.integers(0, len(UMIS)))]
        name = "r%d_%s" % (i, umi) if in_name else "r%d" % i
        p = i // reads_per_position
        tid, p0 = (0 if p % 5 else 1), 1000 + 10 * p
        flag = 0x10 if rng.random() < 0.1 else 0
        tags = tag_model.aux_fields_before(rng)
        if not in_name:
            tags += tag_model.aux_z("RX", umi)
        tags += tag_model.aux_z("CR", barcodes[i])
        quals = rng.integers(20, 41, 50).astype(np.uint8).tobytes()
        mapq = int(rng.integers(0, 61))
        if paired:
            tl = int(rng.choice([180, 200]))
            mp = p0 + tl - 50
            items.append((tid, p0, i, bamio.make_record(name, 0x1 | 0x2 | 0x40 | 0x20, tid, p0, mapq, [("M", 50)], 50, quals,
                                                        tags=tags, mtid=tid, mpos=mp, tlen=tl)))
            items.append((tid, mp, i, bamio.make_record(name, 0x1 | 0x2 | 0x80 | 0x10, tid, mp, mapq, [("M", 50)], 50,
                                                        quals, mtid=tid, mpos=p0, tlen=-tl)))
        else:
            items.append((tid, p0, i, bamio.make_record(name, flag, tid, p0, mapq, [("M", 50)], 50, quals, tags=tags)))
    items.sort(key=lambda t: (t[0], t[1], t[2]))
    return bamio.make_header(refs), [t[3] for t in items]


class Case:
    def __init__(self, tmp, seed=7, n_positions=6, reads_per_position=80, n_wl=10, mm=1, **kw):
        rng = np.random.default_rng(seed)
        self.tmp, self.mm = tmp, mm
        self.wl, pairs = bm.random_list(rng, n_wl, L)
        n = n_positions * reads_per_position
        raw = bm.listed_reads(rng, self.wl, n, pairs)
        self.model = bm.correct(raw, L, self.wl, mm)
        rows = lambda a: [bytes(r).decode() for r in np.asarray(a).reshape(-1, L)]
        self.wl_rows = rows(self.wl)
        matched = np.flatnonzero(self.model["match"] >= 0)
        assert all(int(c) >= 8 for c in bm.correct(raw, L, self.wl, 1)["counts"])  # every status occurs
        fixed = [self.wl_rows[m] if m >= 0 else None for m in self.model["match"]]
        self.header, self.recs_a = build(rows(raw), range(n), seed, reads_per_position, **kw)
        _, self.recs_b = build(fixed, matched, seed, reads_per_position, **kw)
        self.a, self.b = str(tmp / "a.bam"), str(tmp / "b.bam")
        tag_model.write_bam(self.a, self.header, self.recs_a)
        tag_model.write_bam(self.b, self.header, self.recs_b)
        self.list_file = str(tmp / "cells.txt")
        with open(self.list_file, "w") as f:
            f.write("# the kit's cell barcodes\n\n" + "\n".join(self.wl_rows) + "\n")
        self.umi_list = str(tmp / "umis.txt")
        with open(self.umi_list, "w") as f:
            f.write("\n".join(UMIS) + "\n")

    def run(self, src, extra, name):
        dst = str(self.tmp / name)
        r = subprocess.run([CLI, "-i", src, "-o", dst, "--per-cell", "--cell-tag", "CR"] + extra, capture_output=True,
                           text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        stream = bamio.bgzf_decompress(open(dst, "rb").read())
        return stream, bamio.split_records(stream)[1], r.stderr

    def flags(self):
        return ["--cell-whitelist", self.list_file, "--cell-whitelist-max-mismatches", str(self.mm)]

    def compare(self, extra, in_name=False):
        """--cell-whitelist on A against plain --per-cell on B: the same reads in the same order"""
        _, got, log = self.run(self.a, extra + self.flags(), "got.bam")
        _, exp, log_b = self.run(self.b, extra, "exp.bam")
        ident = lambda r: (bamio.parse_record(r)["qname"], bamio.parse_record(r)["flag"])
        assert len(got) == len(exp) > 0
        assert [ident(r) for r in got] == [ident(r) for r in exp]
        c = self.model["counts"]
        assert int(line(log, "Number of reads with a corrected cell barcode")) == int(c[bm.CORRECTED])
        assert int(line(log, "Number of reads with an unlisted cell barcode")) == int(c[bm.NONE])
        assert int(line(log, "Number of reads with an ambiguous cell barcode")) == int(c[bm.AMBIGUOUS])
        assert "cell barcode:" not in log_b.replace("without a cell barcode:", "")
        for what in ("Number of UMIs", "Number of unique alignment positions", "Number of (position, cell) groups"):
            assert line(log, what) == line(log_b, what), what
        if "--tag" not in extra:  # written records are the input's, byte for byte (--tag appends its own tags)
            originals = set(self.recs_a)
            assert all(r in originals for r in got)
        return got, exp, log


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


def test_erroneous_barcodes_collapse_like_the_true_ones(tmp_path):
    c = Case(tmp_path)
    c.compare(["--umi-tag", "RX", "-k", "1"])


def test_without_the_flag_the_same_file_falls_into_more_groups(tmp_path):
    c = Case(tmp_path)
    _, with_flag, log = c.run(c.a, ["--umi-tag", "RX", "-k", "1"] + c.flags(), "w.bam")
    _, without, log0 = c.run(c.a, ["--umi-tag", "RX", "-k", "1"], "wo.bam")
    groups, groups0 = (int(line(l, "Number of (position, cell) groups")) for l in (log, log0))
    assert groups < groups0 and len(with_flag) < len(without)
    assert "corrected cell barcode" not in log0 and "unlisted" not in log0 and "ambiguous" not in log0


@pytest.mark.parametrize("extra", [
    ["--umi-tag", "RX", "-k", "0", "--stage", "host"],
    ["--umi-tag", "RX", "-k", "0", "--stage", "gpu"],
    ["--umi-tag", "RX", "-k", "1", "--algo", "adj", "--merge", "avgqual", "--num-threads", "4"],
    ["--umi-tag", "RX", "-k", "1", "--tag"],
    ["--umi-tag", "RX", "-k", "1", "--umi-whitelist", "UMIS"],
    ["--umi-tag", "RX", "-k", "2", "--distance", "edit"],
    ["--umi-tag", "RX", "-k", "0", "--devices", "0,0"],
], ids=lambda e: " ".join(e[2:]))
def test_combinations_give_the_models_grouping(tmp_path, extra):
    c = Case(tmp_path, seed=8)
    extra = [c.umi_list if x == "UMIS" else x for x in extra]
    _, _, log = c.compare(extra)
    if "--stage" in extra:
        assert "staging (%s)" % extra[-1] in log


def test_max_mismatches_zero(tmp_path):
    c = Case(tmp_path, seed=9, mm=0)
    assert int(c.model["counts"][bm.CORRECTED]) == 0
    c.compare(["--umi-tag", "RX", "-k", "1"])


def test_name_umis(tmp_path):
    Case(tmp_path, seed=10, in_name=True).compare(["-k", "1"])


def test_paired(tmp_path):
    c = Case(tmp_path, seed=12, paired=True)
    got, _, _ = c.compare(["--umi-tag", "RX", "--paired", "-k", "0"])
    assert any(bamio.parse_record(r)["flag"] & 0x80 for r in got)  # second mates follow


def test_metrics_file(tmp_path):
    c = Case(tmp_path, seed=15)
    metrics = str(tmp_path / "metrics.tsv")
    c.run(c.a, ["--umi-tag", "RX", "-k", "0", "--cell-whitelist-metrics", metrics] + c.flags(), "m.bam")
    rows = [l.split("\t") for l in open(metrics).read().splitlines()]
    assert rows[0] == ["barcode", "reads", "exact", "corrected"]
    match, status = c.model["match"], c.model["status"]
    exp = []
    for w, bc in enumerate(c.wl_rows):  # in list order, the barcodes that took a read
        exact = int(((match == w) & (status == bm.EXACT)).sum())
        corrected = int(((match == w) & (status == bm.CORRECTED)).sum())
        if exact + corrected:
            exp.append([bc, str(exact + corrected), str(exact), str(corrected)])
    assert rows[1:] == exp and 0 < len(exp)
    assert sum(int(r[1]) for r in rows[1:]) == int(c.model["counts"][0] + c.model["counts"][1])


def test_a_tag_of_another_length_or_another_byte_ends_the_run(tmp_path):
    c = Case(tmp_path, seed=16, n_positions=3)
    short = str(tmp_path / "short.txt")
    with open(short, "w") as f:
        f.write("ACGTACGTAC\nTTTTACGTAC\n")
    r = subprocess.run([CLI, "-i", c.a, "-o", str(tmp_path / "x.bam"), "--umi-tag", "RX", "--per-cell", "--cell-tag", "CR",
                        "--cell-whitelist", short], capture_output=True, text=True, timeout=600)
    assert r.returncode == 101 and "holds 16 bases, not 10" in r.stderr
    header, recs = build(["ACGTACGTACGTACGT", "ACGTACGTACGTAC-1", "ACGTACGTACGTACGT"], range(3), 1, 3)
    odd = str(tmp_path / "odd.bam")
    tag_model.write_bam(odd, header, recs)
    r = subprocess.run([CLI, "-i", odd, "-o", str(tmp_path / "y.bam"), "--umi-tag", "RX", "--per-cell", "--cell-tag", "CR",
                        "--cell-whitelist", c.list_file], capture_output=True, text=True, timeout=600)
    assert r.returncode == 101 and "Unknown character in cell barcode tag CR of read r1" in r.stderr
