"""tests/transcript_intron_model.py, the definition of umi_assign_genes_transcripts_classes / --transcript-introns,
checked on the CPU: the hand table word for word, the rule's properties on transcript_model's fuzz annotation and its
5,000 reads in all three strand modes, and what the fuzz input has to hold for the GPU tests to mean something."""
import numpy as np
import pytest

import annotation_model as am
import intron_model as im
import transcript_intron_model as ti
import transcript_model as tm
import velocity_model as vm

MODES = sorted(tm.MODES)


# ---- the hand table -------------------------------------------------------------------------------------

@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_the_hand_table(introns):
    exons = list(ti.HAND_EXONS)
    want = ti.hand_expected(ti.INTRONS[introns])
    got = [ti.classify(exons, *r, am.FORWARD, ti.INTRONS[introns]) for r in ti.hand_reads()]
    assert got == want
    fast = ti.classify_all(exons, ti.hand_reads(), am.FORWARD, ti.INTRONS[introns])
    assert [tuple(int(fast[f][i]) for f in ("status", "gene", "tier", "cls")) for i in range(len(want))] == want
    assert list(fast["counts"]) == [sum(w[0] == ti.ASSIGNED and w[2] == t for w in want) for t in (0, 1)] + [
        sum(w[0] == s for w in want) for s in (ti.NONE, ti.SEVERAL)]
    assert list(fast["class_counts"]) == [sum(w[3] == c for w in want) for c in range(5)]


def test_the_hand_table_holds_every_verdict():
    want = ti.hand_expected(ti.EXON_FIRST)
    assert {w[0] for w in want} == {ti.ASSIGNED, ti.NONE, ti.SEVERAL}
    assert {(w[2], w[3]) for w in want if w[0] == ti.ASSIGNED} == {
        (ti.TIER_TRANSCRIPT, ti.EXONIC), (ti.TIER_TRANSCRIPT, ti.JUNCTION), (ti.TIER_BODY, ti.EXONIC), (ti.TIER_BODY, ti.JUNCTION),
        (ti.TIER_BODY, ti.SPANNING), (ti.TIER_BODY, ti.INTRONIC)}
    assert sum(full is not None for *_, full in ti.HAND_READS) == 1  # read 8 alone differs under all


def test_the_gene_level_rule_calls_read_3_exonic():
    """a read spliced over the intron that T1 retains: the retained line covers the gap, so umi_assign_genes_classes
    under exon-first says EXONIC, where this rule says JUNCTION"""
    ref, pos, rev, cigar = ti.hand_reads()[ti.HAND_GENE_LEVEL_DIFFERS]
    lines = tm.overlap_exons(ti.HAND_EXONS)
    assert vm.classify(lines, ref, pos, rev, cigar, am.FORWARD, im.EXON_FIRST) == (im.ASSIGNED, 0, im.TIER_EXON, vm.EXONIC)
    assert ti.classify(list(ti.HAND_EXONS), ref, pos, rev, cigar, am.FORWARD, ti.EXON_FIRST) == (ti.ASSIGNED, 0, ti.TIER_TRANSCRIPT, ti.JUNCTION)


def test_off_assigns_as_the_transcript_rule_and_knows_no_body():
    exons = list(ti.HAND_EXONS)
    for (ref, pos, rev, cigar), first in zip(ti.hand_reads(), ti.hand_expected(ti.EXON_FIRST)):
        st, g, tier, cls = ti.classify(exons, ref, pos, rev, cigar, am.FORWARD, ti.OFF)
        assert (st, g) == tm.assign(exons, ref, pos, rev, cigar, am.FORWARD) and tier == 0
        if first[0] == ti.ASSIGNED and first[2] == ti.TIER_TRANSCRIPT:
            assert (st, g, tier, cls) == first
        else:
            assert st != ti.ASSIGNED and cls == ti.C_NONE


# ---- the properties on transcript_model's fuzz ----------------------------------------------------------

@pytest.fixture(scope="module")
def sets():
    """{mode: [(G, E, B)] of transcript_model's 5,000 reads}: G by fit, E and B by overlap, each from the lines"""
    exons, reads = list(tm.fuzz_annotation()), list(tm.fuzz_reads())
    lines = tm.overlap_exons(exons)
    trs = tm.transcripts_of(exons)
    out = {}
    for mode in tm.MODES.values():
        E, B = im.hit_sets(lines, reads, mode), im.hit_sets(im.bodies(lines), reads, mode)
        fit = tm.fuzz_expected(mode)
        G = []
        for i, (ref, pos, rev, cigar) in enumerate(reads):
            # (the sets themselves where the read is near a transcript at all: the status tells the rest)
            G.append({trs[t][2] for t in tm.fitting(trs, ref, pos, rev, cigar, mode)} if fit["status"][i] != tm.NONE else set())
        out[mode] = list(zip(G, E, B))
    return out


@pytest.mark.parametrize("mode", MODES)
def test_G_lies_in_E_and_E_in_B(sets, mode):
    some = 0
    for G, E, B in sets[tm.MODES[mode]]:
        assert G <= E <= B
        some += bool(G) and G != E
    assert some  # (the overlap rule sees genes the read fits no transcript of)


@pytest.mark.parametrize("mode", MODES)
def test_off_equals_the_transcript_rule(mode):
    got = ti.classify_all(tm.fuzz_annotation(), tm.fuzz_reads(), tm.MODES[mode], ti.OFF)
    exp = tm.fuzz_expected(tm.MODES[mode])
    assert (got["gene"] == exp["gene"]).all() and (got["status"] == exp["status"]).all() and not got["tier"].any()
    assert list(got["counts"]) == [int(exp["counts"][0]), 0, int(exp["counts"][1]), int(exp["counts"][2])]


@pytest.mark.parametrize("mode", MODES)
def test_all_assigns_as_the_bodies_do(mode):
    got = ti.classify_all(tm.fuzz_annotation(), tm.fuzz_reads(), tm.MODES[mode], ti.ALL)
    exp = im.assign_all(tm.overlap_exons(tm.fuzz_annotation()), tm.fuzz_reads(), tm.MODES[mode], im.ALL)
    assert (got["gene"] == exp["gene"]).all() and (got["status"] == exp["status"]).all()
    # a read the bodies assign and some transcript fits is tier exon there too; not the other way round
    both = (got["status"] == ti.ASSIGNED)
    assert (exp["tier"][both & (got["tier"] == ti.TIER_TRANSCRIPT)] == im.TIER_EXON).all()
    assert (exp["tier"][both] <= got["tier"][both]).all() and (exp["tier"][both] < got["tier"][both]).any()


@pytest.mark.parametrize("mode", MODES)
def test_exon_first_keeps_the_transcript_rules_gene(sets, mode):
    got = ti.classify_all(tm.fuzz_annotation(), tm.fuzz_reads(), tm.MODES[mode], ti.EXON_FIRST)
    fit = tm.fuzz_expected(tm.MODES[mode])
    by_tr = (got["status"] == ti.ASSIGNED) & (got["tier"] == ti.TIER_TRANSCRIPT)
    assert (by_tr == (fit["status"] == tm.ASSIGNED)).all() and (got["gene"][by_tr] == fit["gene"][by_tr]).all()
    assert ((got["status"] == ti.SEVERAL) >= (fit["status"] == tm.SEVERAL)).all()
    by_body = (got["status"] == ti.ASSIGNED) & (got["tier"] == ti.TIER_BODY)
    for i in np.flatnonzero(by_body):
        G, _, B = sets[tm.MODES[mode]][i]
        assert not G and B == {int(got["gene"][i])}


@pytest.mark.parametrize("mode", MODES)
def test_the_fast_model_is_the_line_by_line_one(mode):
    exons, reads = list(ti.fuzz_annotation()), ti.fuzz_reads()
    for introns in (ti.EXON_FIRST, ti.ALL):
        fast = ti.fuzz_expected(tm.MODES[mode], introns)
        for i in list(range(0, 5000, 23)) + list(range(5000, len(reads), 3)):
            assert ti.classify(exons, *reads[i], tm.MODES[mode], introns) == tuple(int(fast[f][i]) for f in ("status", "gene", "tier", "cls")), i


# ---- what the fuzz input holds --------------------------------------------------------------------------

def test_the_fuzz_reads_begin_with_the_transcript_models():
    assert ti.fuzz_reads()[:5000] == tm.fuzz_reads() and len(ti.fuzz_reads()) == 5600 and ti.fuzz_annotation() == tm.fuzz_annotation()


@pytest.mark.parametrize("mode", MODES)
def test_every_class_and_both_tiers_occur_under_exon_first(mode):
    """a condition on the input: transcript_model's reads alone leave body-tier EXONIC and JUNCTION out under
    "reverse", which is why extra_reads() stands behind them"""
    exp = ti.fuzz_expected(tm.MODES[mode], ti.EXON_FIRST)
    assert (exp["counts"] >= 100).all(), exp["counts"]
    by_tr = np.bincount(exp["cls"][(exp["status"] == ti.ASSIGNED) & (exp["tier"] == ti.TIER_TRANSCRIPT)], minlength=5)
    by_body = np.bincount(exp["cls"][(exp["status"] == ti.ASSIGNED) & (exp["tier"] == ti.TIER_BODY)], minlength=5)
    assert by_tr[ti.EXONIC] >= 100 and by_tr[ti.JUNCTION] >= 100 and not by_tr[[0, 3, 4]].any(), by_tr
    assert (by_body[1:] >= 5).all() and not by_body[0], by_body
    assert (exp["class_counts"] > 0).all()
    full = ti.fuzz_expected(tm.MODES[mode], ti.ALL)
    assert ((full["status"] == ti.SEVERAL) & (exp["status"] == ti.ASSIGNED)).sum() >= 20  # (a fit the bodies overrule)
