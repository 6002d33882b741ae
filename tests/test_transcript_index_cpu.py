"""The transcript index of umi_assign_genes_transcripts under AddressSanitizer + UBSan (CPU build): tests/cpp/
test_transcript_index.cpp, a program of its own, runs the check, the build, the sampled top and the lookup of a read of
csrc/umihip_transcript_index.hpp -- the code the kernel runs -- on the fuzz inputs, the comb and the hand-written cases
of tests/transcript_cases.py, written out here with the verdicts of tests/transcript_model.py under all three strand
modes."""
import os
import subprocess

import annotation_model as am
import transcript_cases as tc
import transcript_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def case_lines(name, exons, reads, n_transcripts=None):
    exp = [tm.assign_all(exons, reads, mode) for mode in (tm.FORWARD, tm.REVERSE, tm.UNSTRANDED)]
    n_tr = tm.n_transcripts_of(exons) if n_transcripts is None else n_transcripts
    out = ["case %d %d %d %s" % (len(exons), n_tr, len(reads), name.replace(" ", "_").replace(",", ""))]
    out += ["%d %d %d %s %d %d" % e for e in exons]
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        words = am.cigar_words(cigar)
        out.append(" ".join(map(str, [ref, pos, int(rev)] + [int(x["status"][i]) for x in exp] + [int(x["gene"][i]) for x in exp] +
                                [len(words)] + words)))
    return out


def test_the_hand_written_cases_say_what_the_rule_says():
    for name, (exons, reads, want) in tc.CASES.items():
        assert len(reads) >= 1 and (want is None or len(want) == len(reads)), name
        if want is not None:
            got = tm.assign_all(exons, reads, tm.FORWARD)
            assert [(int(s), int(g)) for s, g in zip(got["status"], got["gene"])] == want, name


def test_transcript_index_against_the_model_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "test_transcript_index"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_transcript_index.cpp")])
    lines = case_lines("fuzz", list(tm.fuzz_annotation()), list(tm.fuzz_reads()))
    lines += case_lines("fuzz with spare transcripts", list(tm.fuzz_annotation()), list(tm.fuzz_reads()[:200]), n_transcripts=10 ** 9)
    lines += case_lines("comb", *tc.comb())
    lines += case_lines("comb of one", *tc.comb(1))
    for name, (exons, reads, _) in tc.CASES.items():
        lines += case_lines(name, exons, reads)
    with open(data, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert "transcript index ok" in r.stdout and "%d cases" % (4 + len(tc.CASES)) in r.stdout
