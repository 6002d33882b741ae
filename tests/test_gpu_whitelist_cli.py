"""umicollapse --umi-whitelist end to end.  File A holds reads whose UMIs are listed UMIs with errors, some
beyond correction; file B the same records with every UMI replaced by the model's correction
(tests/whitelist_model.py) and the unmatched reads left out.  --umi-whitelist on A must pick the reads that a
plain run picks on B: the correction changes how reads are grouped and nothing else."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import tag_model
import whitelist_model as wm

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
L = 12


def build(umis, keep, rng_seed, reads_per_position, in_name=False, paired=False, n_cells=0):
    """records of the reads in `keep` (indices), read i with UMI umis[i]; everything but the UMI depends on i
    alone, so that two calls give the same records apart from it"""
    refs = [("chr1", 10_000_000), ("chr2", 5_000_000)]
    items = []
    for i in keep:
        rng = np.random.default_rng([rng_seed, i])
        umi = umis[i]
        name = "r%d_%s" % (i, umi) if in_name else "r%d" % i
        p = i // reads_per_position
        tid, p0 = (0 if p % 5 else 1), 1000 + 10 * p
        flag = 0x10 if rng.random() < 0.1 else 0
        tags = tag_model.aux_fields_before(rng)
        if not in_name:
            tags += tag_model.aux_z("RX", umi)
        if n_cells:
            tags += tag_model.aux_z("CB", "CELL%02d-1" % int(rng.integers(0, n_cells)))
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
    def __init__(self, tmp, seed=7, n_positions=150, reads_per_position=14, n_wl=48, mm=1, md=1, **kw):
        rng = np.random.default_rng(seed)
        self.tmp, self.mm, self.md = tmp, mm, md
        self.wl = wm.random_list(rng, n_wl, L)
        n = n_positions * reads_per_position
        raw = wm.noisy_reads(rng, self.wl, L, n)
        self.model = wm.correct(raw, L, self.wl, mm, md)
        rows = lambda a: [bytes(r).decode() for r in np.asarray(a).reshape(-1, L)]
        matched = np.flatnonzero(self.model["match"] >= 0)
        assert 0 < len(matched) < n
        self.header, self.recs_a = build(rows(raw), range(n), seed, reads_per_position, **kw)
        _, self.recs_b = build(rows(self.model["out"]), matched, seed, reads_per_position, **kw)
        self.a, self.b = str(tmp / "a.bam"), str(tmp / "b.bam")
        tag_model.write_bam(self.a, self.header, self.recs_a)
        tag_model.write_bam(self.b, self.header, self.recs_b)
        self.list_file = str(tmp / "kit.txt")
        with open(self.list_file, "w") as f:
            f.write("# the kit's UMIs\n\n" + "\n".join(rows(self.wl)) + "\n")

    def run(self, src, extra, name):
        dst = str(self.tmp / name)
        r = subprocess.run([CLI, "-i", src, "-o", dst] + extra, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        stream = bamio.bgzf_decompress(open(dst, "rb").read())
        return stream, bamio.split_records(stream)[1], r.stderr

    def whitelist_flags(self):
        return ["--umi-whitelist", self.list_file, "--whitelist-max-mismatches", str(self.mm), "--whitelist-min-distance",
                str(self.md)]

    def compare(self, extra, in_name=False):
        """--umi-whitelist on A against a plain run on B: the same reads in the same order"""
        _, got, log = self.run(self.a, extra + self.whitelist_flags(), "got.bam")
        _, exp, log_b = self.run(self.b, extra, "exp.bam")
        ident = lambda r: bamio.parse_record(r)["qname"].split(b"_")[0] if in_name else bamio.parse_record(r)["qname"]
        assert len(got) == len(exp) > 0
        assert [ident(r) for r in got] == [ident(r) for r in exp]
        assert int(line(log, "Number of reads with a corrected UMI")) == int(self.model["counts"][1])
        assert int(line(log, "Number of reads with an uncorrectable UMI")) == int(self.model["counts"][2])
        assert "corrected UMI" not in log_b and "uncorrectable" not in log_b
        for what in ("Number of UMIs", "Number of unique alignment positions"):
            assert line(log, what) == line(log_b, what), what
        return got, exp, log


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


@pytest.mark.parametrize("extra", [
    ["--umi-tag", "RX", "-k", "0"],
    ["--umi-tag", "RX", "-k", "1"],
    ["--umi-tag", "RX", "-k", "0", "--stage", "host"],
    ["--umi-tag", "RX", "-k", "1", "--algo", "adj", "--merge", "avgqual", "--num-threads", "4"],
    ["--umi-tag", "RX", "-k", "0", "--devices", "0,0"],
], ids=lambda e: " ".join(e[2:]))
def test_whitelist_run_picks_what_a_plain_run_picks_on_corrected_umis(tmp_path, extra):
    c = Case(tmp_path)
    assert all(int(x) > 0 for x in c.model["counts"])  # exact, corrected and uncorrectable reads all occur
    got, _, _ = c.compare(extra)
    originals = set(c.recs_a)
    assert all(r in originals for r in got)  # written records are the input's, byte for byte


def test_other_parameters(tmp_path):
    Case(tmp_path, seed=8, mm=2, md=2).compare(["--umi-tag", "RX", "-k", "0"])
    Case(tmp_path, seed=9, mm=0, md=0).compare(["--umi-tag", "RX", "-k", "0"])


def test_name_umis(tmp_path):
    c = Case(tmp_path, seed=10, in_name=True)
    c.compare(["-k", "0"], in_name=True)
    c.compare(["-k", "1", "--stage", "host"], in_name=True)


def test_per_cell(tmp_path):
    c = Case(tmp_path, seed=11, n_cells=5)
    _, _, log = c.compare(["--umi-tag", "RX", "--per-cell", "-k", "0"])
    assert int(line(log, "Number of (position, cell) groups")) > int(line(log, "Number of unique alignment positions"))
    c.compare(["--umi-tag", "RX", "--per-cell", "-k", "1", "--stage", "host"])


def test_paired(tmp_path):
    c = Case(tmp_path, seed=12, n_positions=80, paired=True)
    got, _, _ = c.compare(["--umi-tag", "RX", "--paired", "-k", "0"])
    assert any(bamio.parse_record(r)["flag"] & 0x80 for r in got)  # second mates follow


def test_tag_mode(tmp_path):
    c = Case(tmp_path, seed=13, n_positions=80)
    got, exp, log = c.compare(["--umi-tag", "RX", "--tag", "-k", "1"])
    # every matched read is written (and no unmatched one), with the cluster tags a plain run gives on B
    assert len(got) == int(c.model["counts"][0] + c.model["counts"][1])
    assert [r[-21:] for r in got] == [r[-21:] for r in exp]
    assert got[0][-21:-19] == b"MI" and got[0][-7:-5] == b"su"


def test_gpu_and_host_staging_write_the_same_file(tmp_path):
    c = Case(tmp_path, seed=14)
    flags = ["--umi-tag", "RX", "-k", "0"] + c.whitelist_flags()
    g, _, lg = c.run(c.a, flags + ["--stage", "gpu"], "g.bam")
    h, _, lh = c.run(c.a, flags + ["--stage", "host"], "h.bam")
    assert g == h and "staging (gpu)" in lg and "staging (host)" in lh


def test_metrics_file(tmp_path):
    c = Case(tmp_path, seed=15)
    metrics = str(tmp_path / "metrics.tsv")
    c.run(c.a, ["--umi-tag", "RX", "-k", "0", "--whitelist-metrics", metrics] + c.whitelist_flags(), "m.bam")
    rows = [l.split("\t") for l in open(metrics).read().splitlines()]
    assert rows[0] == ["umi", "reads", "exact", "corrected"]
    wl = [bytes(r).decode() for r in c.wl.reshape(-1, L)]
    assert len(rows) == 1 + len(wl)
    match, best = c.model["match"], c.model["best"]
    for w, row in enumerate(rows[1:]):
        exact = int(((match == w) & (best == 0)).sum())
        corrected = int(((match == w) & (best > 0)).sum())
        assert row == [wl[w], str(exact + corrected), str(exact), str(corrected)], (w, row)
    assert sum(int(r[1]) for r in rows[1:]) == int(c.model["counts"][0] + c.model["counts"][1])


def test_read_with_a_umi_of_another_length_ends_the_run(tmp_path):
    c = Case(tmp_path, seed=16, n_positions=10)
    short = str(tmp_path / "short.txt")
    with open(short, "w") as f:
        f.write("ACGTACGTAC\nTTTTACGTAC\n")
    r = subprocess.run([CLI, "-i", c.a, "-o", str(tmp_path / "x.bam"), "--umi-tag", "RX", "--umi-whitelist", short],
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 101 and "holds 12 bases, not 10" in r.stderr
