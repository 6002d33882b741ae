"""--transcript-introns off|exon-first|all, the parts that need no GPU: every refusal ends with status 101 and a message
of its own before anything is read or written (host/annotation.hpp has the list), the two refusals that stood before the
flag still stand without it, and a run the flag makes legal gets as far as the input that is not there."""
import os
import subprocess

import pytest

import annotation_model as am

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CLI = os.path.join(ROOT, "umi_collapse_rs_amd", "bin", "umicollapse")
GOOD = "chr1\tsrc\texon\t101\t200\t.\t+\t.\tgene_id \"G1\"; transcript_id \"T1\";"
RULE = ["--per-gene", "--gene-rule", "transcript"]


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


@pytest.mark.parametrize("value", ["off", "exon-first", "all"])
def test_the_flag_wants_the_transcript_rule(tmp_path, value):
    want = "--transcript-introns goes with --gene-rule transcript only"
    assert want in refused(tmp_path, ["--per-gene", "--transcript-introns", value])
    assert want in refused(tmp_path, ["--per-gene", "--transcript-introns", value], [GOOD])
    assert want in refused(tmp_path, ["--per-gene", "--gene-rule", "overlap", "--transcript-introns", value], [GOOD])


@pytest.mark.parametrize("value", ["exon", "Exon-first", "", "exon_first", "ALL"])
def test_any_other_value(tmp_path, value):
    assert "--transcript-introns wants off, exon-first or all: '%s'" % value in refused(tmp_path, RULE + ["--transcript-introns", value], [GOOD])


def test_the_flag_given_twice_with_different_values(tmp_path):
    msg = refused(tmp_path, RULE + ["--transcript-introns", "all", "--transcript-introns", "exon-first"], [GOOD])
    assert "--transcript-introns given twice with different values: 'all' and 'exon-first'" in msg
    # twice with one value is one flag: what ends the run is the input that is not there
    msg = refused(tmp_path, RULE + ["--transcript-introns", "all", "--transcript-introns", "all"], [GOOD])
    assert "in.bam" in msg and "transcript-introns" not in msg


@pytest.mark.parametrize("introns", ["off", "exon-first", "all"])
@pytest.mark.parametrize("value", ["off", "exon-first", "all"])
def test_the_flag_does_not_go_with_gene_introns(tmp_path, value, introns):
    msg = refused(tmp_path, RULE + ["--transcript-introns", value, "--gene-introns", introns], [GOOD])
    assert "--transcript-introns does not go with --gene-introns" in msg


@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_gene_introns_stay_refused_for_the_rule_and_point_at_the_flag(tmp_path, introns):
    msg = refused(tmp_path, RULE + ["--gene-introns", introns], [GOOD])
    assert "--gene-rule transcript does not go with --gene-introns " + introns in msg and "Not built" in msg
    assert "--transcript-introns " + introns in msg


def test_velocity_stays_refused_for_the_rule_without_the_flag(tmp_path):
    for flags in ([], ["--transcript-introns", "off"]):
        msg = refused(tmp_path, RULE + flags + ["--velocity", "--count-matrix", "m"], [GOOD])
        assert "--gene-rule transcript does not go with --velocity" in msg and "Not built" in msg
        assert "--transcript-introns exon-first or all" in msg


@pytest.mark.parametrize("value", ["exon-first", "all"])
def test_velocity_goes_with_the_flag_and_keeps_its_own_refusals(tmp_path, value):
    flags = RULE + ["--transcript-introns", value, "--velocity"]
    assert "--velocity goes with --count-matrix DIR only" in refused(tmp_path, flags, [GOOD])
    assert "--stage gpu does not go with" in refused(tmp_path, flags + ["--count-matrix", "m", "--stage", "gpu"], [GOOD])


@pytest.mark.parametrize("flags", [["--transcript-introns", "off"], ["--transcript-introns", "exon-first"], ["--transcript-introns", "all"],
                                   ["--transcript-introns", "all", "--per-cell", "--umi-filtering", "multi-gene", "--stage", "gpu"]])
def test_a_legal_run_ends_at_the_input_that_is_not_there(tmp_path, flags):
    msg = refused(tmp_path, RULE + flags, [GOOD])
    assert "in.bam" in msg and "transcript-introns" not in msg and "annotation" not in msg


def test_help_names_the_flag():
    r = subprocess.run([CLI, "--help"], capture_output=True, text=True)
    assert r.returncode == 0
    assert "--transcript-introns <M> off, exon-first or all [default: off], with --gene-rule transcript" in r.stdout
