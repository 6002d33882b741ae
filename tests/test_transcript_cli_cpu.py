"""--gene-rule overlap|transcript and --annotation-transcript-attribute, the parts that need no GPU: every refusal ends
with status 101 and a message of its own before anything is read or written (host/annotation.hpp has the list)."""
import os
import subprocess

import pytest

import annotation_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
GOOD = "chr1\tsrc\texon\t101\t200\t.\t+\t.\tgene_id \"G1\"; transcript_id \"T1\"; tx \"X1\";"


@pytest.fixture(scope="module", autouse=True)
def built():
    subprocess.check_call(["make", "-s", "-C", ROOT, "cli"])


def refused(tmp_path, flags, gtf_lines=None):
    """the program's message for a run that must end with status 101 before anything is read or written"""
    argv = [CLI, "-i", "in.bam", "-o", "out.bam"] + flags
    if gtf_lines is not None:
        am.write_gtf(tmp_path / "a.gtf", gtf_lines)
        argv += ["--gene-annotation", "a.gtf"]
    r = subprocess.run(argv, cwd=tmp_path, capture_output=True, text=True, timeout=60)
    assert r.returncode == 101, (r.returncode, r.stderr)
    assert sorted(os.listdir(tmp_path)) == (["a.gtf"] if gtf_lines is not None else [])
    return r.stderr


def line(attrs):
    return "\t".join(GOOD.split("\t")[:8] + [attrs])


def test_the_flag_wants_the_annotation(tmp_path):
    for value in ("transcript", "overlap"):
        assert "--gene-rule goes with --gene-annotation only" in refused(tmp_path, ["--per-gene", "--gene-rule", value])


@pytest.mark.parametrize("value", ["exon", "Transcript", "", "transcripts"])
def test_any_other_value(tmp_path, value):
    assert "--gene-rule wants overlap or transcript: '%s'" % value in refused(tmp_path, ["--per-gene", "--gene-rule", value], [GOOD])


def test_the_flags_given_twice_with_different_values(tmp_path):
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "overlap", "--gene-rule", "transcript"], [GOOD])
    assert "--gene-rule given twice with different values: 'overlap' and 'transcript'" in msg
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--annotation-transcript-attribute", "a",
                             "--annotation-transcript-attribute", "b"], [GOOD])
    assert "--annotation-transcript-attribute given twice with different values: 'a' and 'b'" in msg
    # twice with one value is one flag: what ends the run is the input that is not there
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--gene-rule", "transcript"], [GOOD])
    assert "in.bam" in msg and "gene-rule" not in msg


def test_the_attribute_flag_wants_the_transcript_rule(tmp_path):
    want = "--annotation-transcript-attribute goes with --gene-rule transcript only"
    assert want in refused(tmp_path, ["--per-gene", "--annotation-transcript-attribute", "tx"])
    assert want in refused(tmp_path, ["--per-gene", "--annotation-transcript-attribute", "tx"], [GOOD])
    assert want in refused(tmp_path, ["--per-gene", "--annotation-transcript-attribute", "tx", "--gene-rule", "overlap"], [GOOD])
    assert "wants an attribute name" in refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--annotation-transcript-attribute", ""], [GOOD])


@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_introns_are_not_built_for_the_rule(tmp_path, introns):
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--gene-introns", introns], [GOOD])
    assert "--gene-rule transcript does not go with --gene-introns " + introns in msg and "Not built" in msg


def test_velocity_is_not_built_for_the_rule(tmp_path):
    for introns in ("off", "exon-first"):
        msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--gene-introns", introns, "--velocity", "--count-matrix", "m"], [GOOD])
        assert "--gene-rule transcript does not go with" in msg and "Not built" in msg
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript", "--velocity", "--count-matrix", "m"], [GOOD])
    assert "--gene-rule transcript does not go with --velocity" in msg and "Not built" in msg


@pytest.mark.parametrize("attrs,flags,word", [
    ('gene_id "G1";', [], "no attribute transcript_id"),
    ('gene_id "G1"; transcript_id "T1";', ["--annotation-transcript-attribute", "tx"], "no attribute tx"),
    ('gene_id "G1"; transcript_id "";', [], "the attribute transcript_id is empty"),
    ('gene_id "G1"; transcript_id "a b";', [], "cannot: 32"), ('gene_id "G1"; transcript_id "a;b";', [], "cannot: 59"),
    ('gene_id "G1"; transcript_id "a,b";', [], "cannot: 44"), ('gene_id "G1"; transcript_id "a\x7fb";', [], "cannot: 127"),
    ('gene_id "G1"; transcript_id "a\tb";', [], "cannot: 9"), ('gene_id "G1"; tx "a\xc3\xa9";', ["--annotation-transcript-attribute", "tx"], "cannot: 195"),
])
def test_a_taken_line_without_a_good_transcript(tmp_path, attrs, flags, word):
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "transcript"] + flags, ["# header", GOOD, "", line(attrs)])
    assert word in msg and "a.gtf, line 4" in msg


def test_lines_not_taken_need_no_transcript_and_the_overlap_rule_needs_none(tmp_path):
    other = "\t".join(["chr1", "src", "gene", "101", "200", ".", "+", ".", 'gene_id "G1";'])
    for flags in (["--gene-rule", "transcript"], ["--gene-rule", "transcript", "--annotation-transcript-attribute", "tx"],
                  ["--gene-rule", "transcript", "--gene-introns", "off"]):
        msg = refused(tmp_path, ["--per-gene"] + flags, [other, GOOD])
        assert "in.bam" in msg and "annotation" not in msg and "gene-rule" not in msg
    msg = refused(tmp_path, ["--per-gene", "--gene-rule", "overlap"], [GOOD, line('gene_id "G1";')])
    assert "in.bam" in msg and "annotation" not in msg


def test_what_the_annotation_refuses_stays_refused(tmp_path):
    assert "--gene-annotation goes with --per-gene only" in refused(tmp_path, ["--gene-rule", "transcript"], [GOOD])
    assert "no attribute gene_id" in refused(tmp_path, ["--per-gene", "--gene-rule", "transcript"], [line('transcript_id "T1";')])


def test_help_names_the_flags():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    for flag in ("--gene-rule", "--annotation-transcript-attribute"):
        assert flag in r.stdout
