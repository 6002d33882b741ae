"""tests/velocity_model.py on its own: the hand vectors, the model against a per-base brute force, its identity with
gene_model.count_model, and what the fuzz inputs hold -- so that the GPU tests cannot pass by never producing a class."""
import numpy as np
import pytest

import annotation_model as am
import gene_model
import intron_model as im
import velocity_model as vm

STRANDS = sorted(am.MODES)


@pytest.mark.parametrize("introns", ["exon-first", "all"])
def test_hand_reads(introns):
    for pos, cigar, want in vm.HAND_READS:
        st, g, tier, cls = vm.classify(vm.HAND_EXONS, 0, pos, False, cigar, am.FORWARD, im.INTRONS[introns])
        assert cls == want, (pos, cigar, cls, want)
        assert (st == im.ASSIGNED) == (want != vm.NONE)
        if want != vm.NONE:
            assert g == 0 and tier == (im.TIER_INTRON if want == vm.INTRONIC else im.TIER_EXON)
    # on the other strand nothing of it is assigned under forward, all of it under reverse
    for pos, cigar, want in vm.HAND_READS:
        assert vm.classify(vm.HAND_EXONS, 0, pos, True, cigar, am.FORWARD, im.INTRONS[introns])[3] == vm.NONE
        assert vm.classify(vm.HAND_EXONS, 0, pos, True, cigar, am.REVERSE, im.INTRONS[introns])[3] == want


def test_a_nested_exon_that_fills_the_intron_does_not_cover_the_gap():
    """the exon table has no uncovered base between G0's exons here, but the gap is not G0's"""
    exons = vm.HAND_EXONS + ((0, 200, 300, "+", 2),)
    read = (180, (("M", 20), ("N", 100), ("M", 20)))
    assert vm.classify(exons, 0, *read[:1], False, read[1], am.FORWARD, im.EXON_FIRST) == (im.ASSIGNED, 0, im.TIER_EXON, vm.JUNCTION)
    own = exons + ((0, 150, 350, "+", 0),)  # G0's own line over it: covered
    assert vm.classify(own, 0, *read[:1], False, read[1], am.FORWARD, im.EXON_FIRST)[3] == vm.EXONIC


def test_clipping():
    top = im.TOP
    exons = ((0, 0, 10, "+", 0), (0, top - 10, top, "+", 0))
    c = lambda pos, cigar: vm.classify(exons, 0, pos, False, cigar, am.FORWARD, im.EXON_FIRST)[3]
    assert c(-5, (("M", 10),)) == vm.EXONIC            # what lies before 0 is cut off
    assert c(-5, (("M", 20),)) == vm.SPANNING
    assert c(top - 5, (("M", 5),)) == vm.EXONIC
    assert c(top - 5, (("M", 6),)) == vm.SPANNING        # (no exon holds base 2^31 - 1: the largest end is 2^31 - 1)
    assert c(top - 5, (("M", 3), ("N", 100), ("M", 5))) == vm.EXONIC  # the second block is empty after the cut: one block
    assert c(-20, (("M", 5), ("N", 15), ("M", 5))) == vm.EXONIC       # the first block is
    assert c(5, (("M", 5), ("N", top - 15), ("M", 5))) == vm.JUNCTION


def test_hand_molecules():
    for classes, want in vm.HAND_MOLECULES:
        assert vm.layer_of_classes(classes) == want
        n = len(classes)
        # entry 0 kept, the others hanging on it, a read each; and the same with the kept entry filtered away
        layer = vm.molecule_layers(np.arange(n), classes, [1] + [0] * (n - 1), np.zeros(n, np.uint32))
        assert list(layer) == [want] + [-1] * (n - 1)
        assert (vm.molecule_layers(np.arange(n), classes, np.zeros(n), np.zeros(n, np.uint32)) == -1).all()
    assert list(vm.molecule_layers([], [], [1, 0], [0, 0])) == [vm.AMBIGUOUS, -1]  # no read at all
    assert list(vm.molecule_layers([vm.UNSTAGED], [vm.JUNCTION], [1], [0])) == [vm.AMBIGUOUS]


# ---- against a per-base brute force ---------------------------------------------------------------------

def brute_class(exons, ref, pos, reverse, cigar, mode, introns):
    st, g, tier = im.assign(exons, ref, pos, reverse, cigar, mode, introns)
    if st != im.ASSIGNED:
        return vm.NONE
    if tier == im.TIER_INTRON:
        return vm.INTRONIC
    own = set()
    for xr, xs, xe, xstrand, xg in exons:
        if xg == g and xr == ref and am.admissible(xstrand, reverse, mode):
            own.update(range(xs, xe))
    bl = [(max(s, 0), e) for s, e in am.blocks(pos, cigar) if e > max(s, 0)]
    if any(p not in own for s, e in bl for p in range(s, e)):
        return vm.SPANNING
    if any(p not in own for a, b in zip(bl, bl[1:]) for p in range(a[1], b[0])):
        return vm.JUNCTION
    return vm.EXONIC


@pytest.mark.parametrize("seed", range(6))
def test_model_against_brute_force(seed):
    rng = np.random.default_rng(seed)
    exons = []
    for g in range(6):
        ref, strand, at = int(rng.integers(0, 2)), "+-."[int(rng.choice(3, p=[0.45, 0.45, 0.1]))], int(rng.integers(0, 300))
        for _ in range(int(rng.integers(1, 5))):
            length = int(rng.integers(3, 40))
            exons.append((ref, at, at + length, strand, g))
            if rng.random() < 0.3:
                exons.append((ref, at + length // 2, at + length + int(rng.integers(0, 30)), strand, g))
            at += length + int(rng.integers(0, 40))  # (0: the next exon touches this one)
    seen = set()
    for _ in range(1500):
        pos = int(rng.integers(-10, 450))
        cigar = [("M", int(rng.integers(1, 30)))]
        for _ in range(int(rng.integers(0, 3))):
            cigar += [(str(rng.choice(["N", "N", "D", "I", "S"])), int(rng.integers(0, 50))), ("M", int(rng.integers(0, 25)))]
        read = (int(rng.integers(0, 2)), pos, bool(rng.random() < 0.5), tuple(cigar))
        for mode in am.MODES.values():
            for introns in (im.EXON_FIRST, im.ALL, im.OFF):
                got = vm.classify(exons, *read, mode, introns)[3]
                assert got == brute_class(exons, *read, mode, introns), (read, mode, introns)
                seen.add(got)
    assert seen == {0, 1, 2, 3, 4}
    # classify_all is classify
    reads = [(0, 5 * i, bool(i & 1), (("M", 12), ("N", 7 + i % 30), ("M", 9))) for i in range(80)]
    allof = vm.classify_all(exons, reads, am.FORWARD, im.EXON_FIRST)
    one = [vm.classify(exons, *r, am.FORWARD, im.EXON_FIRST) for r in reads]
    assert [tuple(int(allof[f][i]) for f in ("status", "gene", "tier", "cls")) for i in range(80)] == one


# ---- the matrix -----------------------------------------------------------------------------------------

def test_identity_with_the_count_model():
    m = vm.fuzz_molecules()
    freq = np.ones(len(m["kept"]), np.int32)
    row, col, mol, _ = gene_model.count_model(m["kept"], freq, m["off"], m["row"], m["col"])
    vrow, vcol, s, u, a = vm.velocity_model(m["read_entry"], m["read_class"], m["kept"], m["root"], m["off"], m["row"], m["col"])
    assert (vrow == row).all() and (vcol == col).all()
    assert (s.astype(np.int64) + u + a == mol).all()
    assert int(mol.sum()) == int(np.count_nonzero(m["kept"]))
    # no reads: every molecule is ambiguous
    _, _, s, u, a = vm.velocity_model([], [], m["kept"], m["root"], m["off"], m["row"], m["col"])
    assert not s.any() and not u.any() and (a == mol).all()


def test_fuzz_molecules_hold_every_layer():
    m = vm.fuzz_molecules()
    layer = vm.molecule_layers(m["read_entry"], m["read_class"], m["kept"], m["root"])
    molecules = int((layer >= 0).sum())
    assert molecules > 5000
    for k in (vm.SPLICED, vm.UNSPLICED, vm.AMBIGUOUS):
        assert (layer == k).sum() >= 0.05 * molecules, k
    own = m["root"] == np.arange(len(m["root"]))
    assert (own & (m["kept"] == 0)).sum() > 100 and (~own).sum() > 500   # filtered roots, and entries that hang on others
    assert (m["read_entry"] == vm.UNSTAGED).sum() > 100
    assert len(set(zip(m["col"].tolist(), m["row"].tolist()))) < len(m["row"])  # several buckets of one pair


# ---- what the classes' fuzz inputs hold -----------------------------------------------------------------

def test_fuzz_annotation_shape():
    lines, prim, _, _ = vm.fuzz_genes()
    assert len(prim) == vm.FUZZ_GENES and 800 <= len(lines) <= 1300
    assert am.n_genes_of(lines) == vm.FUZZ_GENES
    ops = {op for _, _, _, cigar in vm.fuzz_reads() for op, _ in cigar}
    assert ops == set(am.OPS) and len(vm.fuzz_reads()) == 5000
    assert {r[2] for r in vm.fuzz_reads()} == {False, True}


@pytest.mark.parametrize("introns", ["exon-first", "all"])
@pytest.mark.parametrize("mode", STRANDS)
def test_fuzz_reads_hold_every_class(mode, introns):
    exp = vm.fuzz_expected(am.MODES[mode], im.INTRONS[introns])
    assigned = int((exp["status"] == im.ASSIGNED).sum())
    assert assigned > 1000  # (a class's twentieth is then 50 reads or more)
    for c in (vm.EXONIC, vm.JUNCTION, vm.SPANNING, vm.INTRONIC):
        assert exp["class_counts"][c] >= 0.05 * assigned, (vm.CLASS_NAMES[c], exp["class_counts"], assigned)
    assert exp["class_counts"][vm.NONE] == exp["counts"][2] + exp["counts"][3] and exp["class_counts"][vm.INTRONIC] == exp["counts"][1]
    assert exp["counts"][2] >= 20 and exp["counts"][3] >= 20  # every status occurs: none, several
    assert (exp["cls"][exp["status"] != im.ASSIGNED] == vm.NONE).all()
    assert ((exp["cls"] == vm.INTRONIC) == ((exp["status"] == im.ASSIGNED) & (exp["tier"] == im.TIER_INTRON))).all()


def test_fuzz_reads_meet_gaps_the_table_covers_but_the_gene_does_not():
    """reads whose gap another gene's exon fills exactly: the exon table's cover of the gap is its length, the gene's
    is not -- the device must look the gap up in the gene's own exons"""
    lines, reads = vm.fuzz_annotation(), vm.fuzz_reads()
    exp = vm.fuzz_expected(am.FORWARD, im.EXON_FIRST)
    n = 0
    for i in np.flatnonzero(exp["cls"] == vm.JUNCTION):
        ref, pos, rev, cigar = reads[i]
        every = [(xs, xe) for xr, xs, xe, xstrand, _ in lines if xr == ref and am.admissible(xstrand, rev, am.FORWARD)]
        n += all(vm.cover_of(every, s, e) == e - s for s, e in vm.gaps(vm.read_blocks(pos, cigar)))
    assert n >= 5, n
