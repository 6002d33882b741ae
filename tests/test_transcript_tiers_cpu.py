"""The lookup of umi_assign_genes_transcripts_classes under AddressSanitizer + UBSan (CPU build): tests/cpp/
test_transcript_tiers.cpp, a program of its own, builds the three indices as the call builds them and runs
transcript_assign_read_tiers of csrc/umihip_transcript_index.hpp -- whole, and phase by phase as the two kernels run
it -- on the hand table, the fuzz inputs, the hand-written cases of tests/transcript_cases.py and two combs, written out
here with the verdicts of tests/transcript_intron_model.py under all three strand modes and all three intron modes."""
import os
import subprocess

import annotation_model as am
import transcript_cases as tc
import transcript_intron_model as ti
import transcript_model as tm

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODES = (tm.FORWARD, tm.REVERSE, tm.UNSTRANDED)
INTRONS = (ti.OFF, ti.EXON_FIRST, ti.ALL)


def case_lines(name, exons, reads, n_genes=None, n_transcripts=None):
    exons, reads = list(exons), list(reads)
    exp = [ti.classify_all(exons, reads, mode, introns) for mode in MODES for introns in INTRONS]
    n_genes = am.n_genes_of(tm.overlap_exons(exons)) if n_genes is None else n_genes
    n_tr = tm.n_transcripts_of(exons) if n_transcripts is None else n_transcripts
    out = ["case %d %d %d %d %s" % (len(exons), n_genes, n_tr, len(reads), name.replace(" ", "_").replace(",", ""))]
    out += ["%d %d %d %s %d %d" % e for e in exons]
    for i, (ref, pos, rev, cigar) in enumerate(reads):
        words = am.cigar_words(cigar)
        verdicts = [int(x[f][i]) for x in exp for f in ("status", "gene", "tier", "cls")]
        out.append(" ".join(map(str, [ref, pos, int(rev)] + verdicts + [len(words)] + words)))
    return out


def test_transcript_tiers_against_the_model_under_asan_and_ubsan(tmp_path):
    exe, data = str(tmp_path / "test_transcript_tiers"), str(tmp_path / "cases.txt")
    subprocess.check_call(["g++", "-O1", "-g", "-std=c++17", "-Wall", "-Wextra", "-Werror", "-fsanitize=address,undefined",
                           "-fno-sanitize-recover=all", "-fno-omit-frame-pointer", "-o", exe,
                           os.path.join(ROOT, "tests", "cpp", "test_transcript_tiers.cpp")])
    lines = case_lines("hand table", ti.HAND_EXONS, ti.hand_reads(), ti.HAND_N_GENES, ti.HAND_N_TRANSCRIPTS)
    lines += case_lines("fuzz", ti.fuzz_annotation(), ti.fuzz_reads(), ti.N_GENES)
    lines += case_lines("transcript comb", tm.comb_annotation(2 * 7 + 1), tm.comb_reads(2 * 7 + 1, reads=400), 50)
    lines += case_lines("body comb", ti.body_comb(7), ti.body_comb_reads(7)[:600])
    n = 4
    for name, (exons, reads, _) in tc.CASES.items():
        lines += case_lines(name, exons, reads)
        n += 1
    with open(data, "w") as f:
        f.write("\n".join(lines) + "\n")
    r = subprocess.run([exe, data], capture_output=True, text=True, timeout=300,
                       env=dict(os.environ, ASAN_OPTIONS="detect_leaks=1:abort_on_error=0"))
    assert r.returncode == 0, (r.stdout[-500:], r.stderr[-2000:])
    assert "transcript tiers ok" in r.stdout and "%d cases" % n in r.stdout
