"""--umi-tag / --per-cell on the GPU: umicollapse end to end against tests/tag_model.py (decompressed
output record for record), and the grouped device staging (umi_stage_reads_grouped[_wide]) against
stage_reads and a model, in the composed-key and the extra-pass regimes."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import tag_model
from helpers import grouped_stage_model as model

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


def run_cli(tmp_path, header, recs, extra, name="out.bam"):
    src, dst = str(tmp_path / "in.bam"), str(tmp_path / name)
    if not os.path.exists(src):
        tag_model.write_bam(src, header, recs)
    r = subprocess.run([CLI, "-i", src, "-o", dst] + extra, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    stream = bamio.bgzf_decompress(open(dst, "rb").read())
    out_header, out_recs = bamio.split_records(stream)
    return stream, out_recs, r.stderr


def line(log, what):
    for l in log.splitlines():
        if l.startswith(what + ":"):
            return l.split(":", 1)[1].strip()
    raise AssertionError("no line '%s' in\n%s" % (what, log))


@pytest.mark.parametrize("extra,kw", [
    (["--umi-tag", "RX", "--per-cell", "--stage", "gpu"], dict(umi_tag="RX", per_cell=True)),
    (["--umi-tag", "RX", "--per-cell", "--stage", "host"], dict(umi_tag="RX", per_cell=True)),
    (["--umi-tag", "UB", "--per-cell", "--merge", "any", "--stage", "gpu"], dict(umi_tag="UB", per_cell=True, merge="any")),
    (["--umi-tag", "UB", "--per-cell", "--merge", "avgqual", "--stage", "host", "--algo", "adj"],
     dict(umi_tag="UB", per_cell=True, merge="avgqual", algo="adj")),
    (["--per-cell", "--stage", "gpu", "-k", "2", "--num-threads", "4"], dict(per_cell=True, k=2)),
    (["--umi-tag", "RX", "--stage", "gpu", "--keep-unmapped"], dict(umi_tag="RX", keep_unmapped=True)),
    (["--umi-tag", "RX", "--per-cell", "--cell-tag", "CB", "--devices", "0,0"], dict(umi_tag="RX", per_cell=True)),
])
def test_end_to_end_matches_the_model(tmp_path, extra, kw):
    header, recs = tag_model.tagged_bam(21, 120, 15, n_cells=7)
    k = kw.pop("k", 1)
    algo = kw.pop("algo", "dir")
    exp, st, n_kept = tag_model.expected_output(recs, k=k, algo=algo, **kw)
    _, got, log = run_cli(tmp_path, header, recs, extra)
    assert len(got) == len(exp) and got == exp
    assert int(line(log, "Number of reads after deduplicating")) == n_kept
    c = st["counters"]
    if kw.get("per_cell"):
        assert int(line(log, "Number of unique alignment positions")) == c["positions"]
        assert int(line(log, "Number of (position, cell) groups")) == c["groups"]
        assert int(line(log, "Number of reads without a cell barcode")) == c["no_cell"] > 0
    if kw.get("umi_tag"):
        assert int(line(log, "Number of reads without a UMI tag")) == c["no_umi"] > 0


@pytest.mark.parametrize("umi_len", [12, 24])
def test_gpu_and_host_staging_write_the_same_file(tmp_path, umi_len):
    header, recs = tag_model.tagged_bam(22, 80, 12, umi_len=umi_len, n_cells=9)
    flags = ["--umi-tag", "RX", "--per-cell", "--merge", "avgqual"]
    g, _, lg = run_cli(tmp_path, header, recs, flags + ["--stage", "gpu"], "g.bam")
    h, _, lh = run_cli(tmp_path, header, recs, flags + ["--stage", "host"], "h.bam")
    assert g == h and "staging (gpu)" in lg and "staging (host)" in lh
    exp, _, _ = tag_model.expected_output(recs, umi_tag="RX", per_cell=True, merge="avgqual")
    assert bamio.split_records(g)[1] == exp


def test_paired(tmp_path):
    header, recs = tag_model.tagged_bam(23, 60, 10, n_cells=5, paired=True)
    exp, _, _ = tag_model.expected_output(recs, umi_tag="RX", per_cell=True, paired=True)
    _, got, log = run_cli(tmp_path, header, recs, ["--paired", "--umi-tag", "RX", "--per-cell"])
    assert got == exp
    assert any(bamio.parse_record(r)["flag"] & 0x80 for r in got)  # second mates follow


def test_tag_mode_per_cell_clusters(tmp_path):
    header, recs = tag_model.tagged_bam(24, 60, 12, n_cells=4)
    exp, _, groups = tag_model.expected_tagged_output(recs, umi_tag="UB", per_cell=True)
    _, got, log = run_cli(tmp_path, header, recs, ["--tag", "--umi-tag", "UB", "--per-cell"])
    assert got == exp
    assert int(line(log, "Number of groups of reads")) == groups


@pytest.mark.parametrize("extra", [
    ["--umi-tag", "RX", "--per-cell"],
    ["--umi-tag", "RX", "--per-cell", "--stage", "host", "--merge", "any"],
    ["--per-cell", "--paired"],
])
def test_two_pass_is_identical_to_one_pass(tmp_path, extra):
    paired = "--paired" in extra
    header, recs = tag_model.tagged_bam(25, 150, 8, n_cells=6, paired=paired)
    one, _, log1 = run_cli(tmp_path, header, recs, extra, "one.bam")
    two, _, log2 = run_cli(tmp_path, header, recs, extra + ["--two-pass", "--two-pass-window", "64"], "two.bam")
    assert one == two
    windows = int(line(log2, "two-pass").split()[0])
    assert windows > 1
    for what in ("Number of input reads", "Number of unique alignment positions", "Number of (position, cell) groups",
                 "Number of reads without a cell barcode", "Number of UMIs", "Number of reads after deduplicating"):
        assert line(log1, what) == line(log2, what), what
    exp, _, _ = tag_model.expected_output(recs, per_cell=True, paired=paired,
                                          umi_tag="RX" if "--umi-tag" in extra else None,
                                          merge="any" if "any" in extra else "mapqual")
    assert bamio.split_records(one)[1] == exp


def test_names_and_tags_with_the_same_umis_give_the_same_file(tmp_path):
    header, recs = tag_model.tagged_bam(26, 100, 10, miss_umi=0.0)
    for cell in ([], ["--per-cell"]):
        by_name, _, _ = run_cli(tmp_path, header, recs, cell, "name.bam")
        by_tag, _, _ = run_cli(tmp_path, header, recs, cell + ["--umi-tag", "RX"], "tag.bam")
        assert by_name == by_tag


# ---- the library's grouped staging ---------------------------------------------------------------

@pytest.fixture(scope="module")
def ctx():
    import umi_collapse_rs_amd as umi
    c = umi.Context(0)
    yield c
    c.close()


def reads(seed, n, n_align, n_groups, umi_len, abits, gbits):
    rng = np.random.default_rng(seed)
    align_ids = rng.integers(0, n_align, n)
    align_vals = rng.integers(0, 1 << 62, n_align, dtype=np.uint64) << np.uint64(2) if abits == 64 else \
        rng.integers(0, 1 << abits, n_align, dtype=np.uint64)
    group_vals = rng.integers(0, 1 << min(gbits, 62), max(n_groups, 1), dtype=np.uint64)
    align = align_vals[align_ids]
    group = group_vals[rng.integers(0, max(n_groups, 1), n)]
    # a few UMIs per (alignment, group): repeats make freq > 1
    pool = rng.integers(0, 4, (64, umi_len))
    bases = pool[rng.integers(0, 64, n)]
    bases[rng.random(n) < 0.01, 0] = 4  # some N
    umis = np.frombuffer(b"ACGTN", np.uint8)[bases].reshape(-1)
    score = rng.integers(0, 60, n).astype(np.int32)
    return align, group, umis, score


def same(got, exp):
    for f in ("keys", "nmask", "freq", "rep", "bucket_off"):
        a, b = np.asarray(got[f]), np.asarray(exp[f])
        assert a.shape == b.shape and (a.astype(np.uint64) == b.astype(np.uint64)).all(), f


@pytest.mark.parametrize("abits", [20, 64])
def test_group_bits_zero_is_stage_reads(ctx, abits):
    align, group, umis, score = reads(1, 30000, 500, 50, 12, abits, 17)
    plain = ctx.stage_reads(align, umis, score, 12, merge=1, align_key_bits=abits)
    grouped = ctx.stage_reads_grouped(align, group, umis, score, 12, merge=1, align_key_bits=abits, group_key_bits=0)
    same(grouped, plain)


@pytest.mark.parametrize("n,abits,gbits,umi_len,merge", [
    (40000, 12, 8, 12, 1),         # align + group + 28 UMI bits <= 64: one composed key
    (40000, 30, 17, 12, 0),        # align + group fit a word, the UMI does not: one key word per pass set
    (40000, 64, 17, 12, 1),        # align + group over 64 bits: the group word sorted in passes of its own
    (40000, 50, 30, 10, 1),        # ... and with a group key wider than the alignment's free bits
    (2_000_000, 20, 17, 12, 1),    # 2 M reads, composed key: many sort tiles
    (2_000_000, 64, 17, 12, 0),    # 2 M reads, extra passes
])
def test_grouped_staging_matches_the_model(ctx, n, abits, gbits, umi_len, merge):
    align, group, umis, score = reads(n + abits + gbits, n, max(100, n // 100), 5000, umi_len, abits, gbits)
    got = ctx.stage_reads_grouped(align, group, umis, score, umi_len, merge=merge, align_key_bits=abits,
                                  group_key_bits=gbits)
    exp = model(align, group, umis, score, umi_len, merge, gbits)
    same(got, exp)
    plain = ctx.stage_reads(align, umis, score, umi_len, merge=merge, align_key_bits=abits)
    assert len(got["bucket_off"]) > len(plain["bucket_off"])  # the groups really split positions


@pytest.mark.parametrize("abits,gbits", [(16, 8), (64, 17)])
def test_grouped_wide_matches_the_model(ctx, abits, gbits):
    align, group, umis, score = reads(7, 6000, 80, 30, 24, abits, gbits)
    got = ctx.stage_reads_grouped_wide(align, group, umis, score, 24, merge=1, align_key_bits=abits,
                                       group_key_bits=gbits)
    same(got, model(align, group, umis, score, 24, 1, gbits))


def test_grouped_staging_refuses_bad_group_bits(ctx):
    align, group, umis, score = reads(3, 100, 10, 5, 12, 20, 8)
    for bad in (-1, 65):
        with pytest.raises(Exception):
            ctx.stage_reads_grouped(align, group, umis, score, 12, align_key_bits=20, group_key_bits=bad)
