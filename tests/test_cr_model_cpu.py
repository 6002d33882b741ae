"""The one-mismatch correction after Cell Ranger, the parts that need no GPU: the two statements of the rule in
tests/cr_model.py agree, the known answers, the root contract on every input the GPU tests use, and the program's
refusals of --algo cr -- each with its message, status 101 and nothing written."""
import os
import subprocess

import numpy as np
import pytest

import bamio
import cr_model as cm
import tag_model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")


@pytest.mark.parametrize("n_frac", [0.0, 0.1])
def test_the_two_statements_agree(n_frac):
    rng = np.random.default_rng(1 + int(10 * n_frac))
    chains = 0
    for _ in range(150):
        L = int(rng.integers(1, 9))
        umis, freq = cm.dense_bucket(rng, int(rng.integers(1, 60)), L, n_frac)
        assert cm.targets_loop(umis, freq) == cm.targets_argmax(umis, freq)
        chains += cm.chains(umis, freq)
    assert chains > 50   # dense inputs exercise the non-transitive case


def test_a_chain_keeps_both_of_its_targets():
    umis, freq = ["AACC", "AACA", "AAAA"], [4, 2, 1]          # c, b, a in rank order: a -> b -> c
    kept, root, target = cm.model_bucket(umis, freq)
    assert target.tolist() == [0, 0, 1]
    assert kept.tolist() == [1, 1, 0] and root.tolist() == [0, 1, 1]   # two molecules, root[b] == b
    assert cm.chains(umis, freq) == 1


def test_equal_counts_go_to_the_larger_string():
    kept, root, target = cm.model_bucket(["ACGA", "ACGT"], [3, 3])
    assert target.tolist() == [1, 1] and kept.tolist() == [0, 1]      # the larger string keeps itself
    kept, _, target = cm.model_bucket(["ACGT", "ACGN"], [3, 3])       # N < T in the order of the bytes
    assert target.tolist() == [0, 0]
    # the largest of three equal neighbours, not the first one met
    _, _, target = cm.model_bucket(["AAAA", "CAAA", "TAAA", "GAAA"], [1, 1, 1, 1])
    assert target.tolist() == [2, 2, 2, 2]


def test_n_is_replaced_and_never_substituted_in():
    kept, _, target = cm.model_bucket(["ACGT", "ACNT"], [5, 4])
    assert target.tolist() == [0, 0] and kept.tolist() == [1, 0]       # the N of ACNT is replaced
    kept, _, target = cm.model_bucket(["ACNT", "ACGT"], [9, 1])
    assert target.tolist() == [0, 1] and kept.tolist() == [1, 1]       # ACGT -> ACNT would substitute an N in: no candidate
    _, _, target = cm.model_bucket(["ANNT", "ACNT"], [9, 1])           # (the letter that differs decides, not the others)
    assert target.tolist() == [0, 1]
    assert cm.one_base_pairs(["ACNT", "ACGT"]) == 1                    # n_edges counts the pair, admissible or not


def test_a_bucket_of_one():
    kept, root, target = cm.model_bucket(["ACGT"], [7])
    assert kept.tolist() == [1] and root.tolist() == [0] and target.tolist() == [0]
    assert cm.model_batch([([], []), (["A"], [1]), ([], [])])[0].tolist() == [1]


def test_the_root_contract_holds_on_every_gpu_input():
    names = set()
    for name, buckets, (keys, nm, fr, off), (kept, root, target, pairs) in cm.every_input():
        names.add(name)
        assert len(kept) == len(keys) == int(off[-1])
        assert cm.root_contract_holds(kept, root), name
        assert (kept[target.astype(np.int64)] == 1).all(), name
        assert int(kept.sum()) == len(set(target.tolist())), name
        for umis, freq in buckets:                      # rank order, distinct
            assert all(a >= b for a, b in zip(freq, freq[1:])) and len(set(umis)) == len(umis)
    assert len(names) >= 30
    for L in cm.LENGTHS:
        if L >= 6:
            assert [len(u) for u, _ in cm.batch(L, 0.05)[0]][::2] == list(cm.SIZES)
    # the inputs hold what the rule is about: chains, ties, inadmissible pairs
    buckets = cm.batch(12, 0.05)[0]
    assert sum(cm.chains(u, f) for u, f in buckets) > 10
    assert any(len(u) > 1 and f[0] == f[1] for u, f in buckets)


# ---- the program ------------------------------------------------------------------------------------

@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


@pytest.fixture(scope="module")
def inputs(tmp_path_factory):
    d = tmp_path_factory.mktemp("cr_cli_in")
    header, recs = cm.cr_bam()
    bam = str(d / "in.bam")
    tag_model.write_bam(bam, header, recs)
    long_recs = [bamio.make_record("r%d_%s" % (i, "ACGTACGTACGTACGTACGTAC"), 0, 0, 1000 + i, 60, [("M", 50)], 50, bytes([30] * 50))
                 for i in range(4)]
    long_bam = str(d / "long.bam")
    tag_model.write_bam(long_bam, bamio.make_header([("chr1", 10_000_000)]), long_recs)
    wl = str(d / "wl22.txt")
    with open(wl, "w") as f:
        f.write("ACGTACGTACGTACGTACGTAC\nTTGTACGTACGTACGTACGTAC\n")
    fq = str(d / "in.fastq")
    with open(fq, "w") as f:
        f.write("@r0\nACGTACGTAC\n+\nIIIIIIIIII\n")
    return dict(bam=bam, long_bam=long_bam, wl=wl, fq=fq)


def refused(tmp_path, args, message):
    r = subprocess.run([CLI] + args, capture_output=True, text=True, timeout=300, cwd=str(tmp_path))
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert message in r.stderr, r.stderr
    assert os.listdir(str(tmp_path)) == []


CASES = [
    (["-m", "fastq", "-i", "{fq}"], "--algo cr is defined in bam/sam mode only"),
    (["-i", "{bam}", "--two-pass"], "--algo cr does not go with --two-pass"),
    (["-i", "{bam}", "--devices", "0,1"], "--algo cr runs on one GPU"),
    (["-i", "{bam}", "--distance", "edit"], "--algo cr does not go with --distance edit"),
    (["-i", "{bam}", "-k", "2"], "-k 2 does not go with it"),
    (["-i", "{bam}", "-k", "0"], "-k 0 does not go with it"),
    (["-i", "{bam}", "-u", "22"], "--algo cr takes UMIs of at most 21 bases (-u 22)"),
    (["-i", "{bam}", "--umi-whitelist", "{wl}"], "--algo cr takes UMIs of at most 21 bases (the whitelist's have 22)"),
    (["-i", "{long_bam}", "--stage", "host"], "--algo cr takes UMIs of at most 21 bases (this file's have 22)"),
]


@pytest.mark.parametrize("args,message", CASES, ids=[c[1][:40] for c in CASES])
def test_refusals(tmp_path, inputs, args, message):
    refused(tmp_path, [a.format(**inputs) for a in args] + ["-o", "out.bam", "--algo", "cr"], message)


def test_cc_stays_refused(tmp_path, inputs):
    refused(tmp_path, ["-i", inputs["bam"], "-o", "out.bam", "--algo", "cc"], "Invalid algorithm combination: cc")
    refused(tmp_path, ["-i", inputs["bam"], "-o", "out.bam", "--algo", "CR"], "Invalid algorithm combination: CR")


def test_the_flag_is_taken_and_p_plays_no_part(tmp_path, inputs):
    """the staging runs and does not depend on the rule (--dump-staging stops before the GPU)"""
    dumps = []
    for extra in (["--algo", "cr"], ["--algo", "cr", "-p", "0.1", "-k", "1"], ["--algo", "dir"]):
        dump = str(tmp_path / ("d%d.bin" % len(dumps)))
        r = subprocess.run([CLI, "-i", inputs["bam"], "-o", str(tmp_path / "unused"), "--per-cell", "--dump-staging", dump] + extra,
                           capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stderr
        dumps.append(open(dump, "rb").read())
    assert len(dumps[0]) > 32 and dumps[0] == dumps[1] == dumps[2]


def test_help_names_cr():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True, timeout=60)
    assert r.returncode == 0
    assert "or cr;" in r.stdout and "cr: Cell Ranger's one-mismatch correction" in r.stdout
