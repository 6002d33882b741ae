"""The two tiers of umi_assign_genes_introns under AddressSanitizer + UBSan (CPU build): tests/cpp/
test_intron_index.cpp runs the derivation of the gene bodies, both tiers' tables and the two-phase verdict of a read
of csrc/umihip_gene_index.hpp -- the code the kernel runs -- on the fuzz input, the hand-written cases and a comb
beside the body top's capacity, and prints bodies and verdicts, which are compared with tests/intron_model.py here."""
import os
import subprocess

import pytest

import annotation_model as am
import intron_model as im

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("intron_index") / "test_intron_index")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", path,
                           os.path.join(ROOT, "tests", "cpp", "test_intron_index.cpp")])
    return path


def run(exe, tmp_path, exons, reads):
    src = tmp_path / "input.txt"
    with open(src, "w") as f:
        for ref, s, e, strand, g in exons:
            f.write("E %d %d %d %s %d\n" % (ref, s, e, strand, g))
        for ref, pos, rev, cigar in reads:
            f.write("R %d %d %d %d %s\n" % (ref, pos, 1 if rev else 0, len(cigar), " ".join(map(str, am.cigar_words(cigar)))))
    r = subprocess.run([exe, str(src)], capture_output=True, text=True, timeout=120,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, r.stderr[-2000:]
    assert "intron index ok" in r.stdout
    bodies, verdicts = [], {}
    for line in r.stdout.splitlines():
        w = line.split()
        if w[0] == "B":
            bodies.append((int(w[1]), int(w[2]), int(w[3]), w[4], int(w[5])))
        elif w[0] == "V":
            verdicts.setdefault((int(w[1]), int(w[2])), []).append((int(w[4]), int(w[5]), int(w[6])))
    return bodies, verdicts


def check(exe, tmp_path, exons, reads):
    exons, reads = list(exons), list(reads)
    bodies, verdicts = run(exe, tmp_path, exons, reads)
    assert sorted(bodies) == sorted(im.bodies(exons)) and len(bodies) == len(set(bodies))
    assert sorted(verdicts) == [(s, i) for s in range(3) for i in range(3)]
    for (mode, introns), got in verdicts.items():
        exp = im.assign_all(exons, reads, mode, introns)
        want = list(zip(exp["status"].tolist(), exp["gene"].tolist(), exp["tier"].tolist()))
        bad = [i for i in range(len(reads)) if got[i] != want[i]]
        assert not bad, (mode, introns, bad[:5], [got[i] for i in bad[:5]], [want[i] for i in bad[:5]], [reads[i] for i in bad[:5]])


def test_fuzz_input_against_the_model_under_asan_and_ubsan(exe, tmp_path):
    check(exe, tmp_path, am.fuzz_annotation(), am.fuzz_reads())


def test_hand_cases_against_the_model_under_asan_and_ubsan(exe, tmp_path):
    check(exe, tmp_path, im.HAND_EXONS, [r for _, r in im.hand_reads()])
    check(exe, tmp_path, [], [r for _, r in im.hand_reads()])  # no line at all: every table is empty


@pytest.mark.parametrize("n", [im.GENE_BODY_TOP_CAP, im.GENE_BODY_TOP_CAP + 1])
def test_combs_beside_the_body_top_s_capacity(exe, tmp_path, n):
    check(exe, tmp_path, im.body_comb(n), im.body_comb_reads(n))
