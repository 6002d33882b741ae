"""umi_assign_genes_transcripts / --gene-rule transcript, the parts that need no GPU: the model of tests/
transcript_model.py on hand-written cases and against a brute force (every transcript tried for every read at every
exon it could start in, no index), what the fuzz inputs of the GPU tests hold, and the library's refusals that come
before a device is looked at."""
import ctypes as C

import numpy as np
import pytest

import annotation_model as am
import transcript_model as tm


# ---- brute force: the rule's words, nothing shared with the model but blocks() and admissible() -----------------

def brute_transcripts(exons):
    trs = {}
    for ref, s, e, strand, g, t in exons:
        trs.setdefault(t, []).append((ref, s, e, strand, g))
    out = []
    for t, lines in sorted(trs.items()):
        covered = set()
        for _, s, e, _, _ in lines:
            covered.update(range(s, e))
        # united exons: the maximal runs of covered bases
        xs = [(p, next(q for q in range(p + 1, max(covered) + 2) if q not in covered)) for p in sorted(covered) if p - 1 not in covered]
        out.append((lines[0][0], lines[0][3], lines[0][4], xs))
    return out


def brute_fit(xs, bl):
    if not bl:
        return False
    for j in range(len(xs)):
        if j + len(bl) > len(xs):
            continue
        ok = all(xs[j + i][0] <= b[0] and b[1] <= xs[j + i][1] for i, b in enumerate(bl))
        ok = ok and all(bl[i][1] == xs[j + i][1] and bl[i + 1][0] == xs[j + i + 1][0] for i in range(len(bl) - 1))
        if ok:
            return True
    return False


def brute_assign_all(exons, reads, mode):
    """[(status, gene, transcripts fitted)]"""
    trs = brute_transcripts(exons)
    out = []
    for ref, pos, rev, cigar in reads:
        bl = am.blocks(pos, cigar)
        fit = [(g, k) for k, (xr, strand, g, xs) in enumerate(trs) if xr == ref and am.admissible(strand, rev, mode) and brute_fit(xs, bl)]
        genes = {g for g, _ in fit}
        out.append((tm.NONE if not genes else tm.ASSIGNED if len(genes) == 1 else tm.SEVERAL, genes.pop() if len(genes) == 1 else -1,
                    len(fit)))
    return out


# ---- the model on hand-written cases ----------------------------------------------------------------------------

T123 = [(0, 100, 200, "+", 0, 0), (0, 300, 400, "+", 0, 0), (0, 500, 600, "+", 0, 0)]


def one(exons, pos, cigar, rev=False, mode=tm.FORWARD, ref=0):
    return tm.assign(exons, ref, pos, rev, cigar, mode)


def test_containment_and_junctions():
    m = [("M", 10)]
    assert one(T123, 100, m) == (tm.ASSIGNED, 0) and one(T123, 99, m) == (tm.NONE, -1)
    assert one(T123, 190, m) == (tm.ASSIGNED, 0) and one(T123, 191, m) == (tm.NONE, -1)
    assert one(T123, 190, [("M", 10), ("N", 100), ("M", 10)]) == (tm.ASSIGNED, 0)
    assert one(T123, 189, [("M", 10), ("N", 101), ("M", 10)]) == (tm.NONE, -1)  # ends one short of the exon's end
    assert one(T123, 191, [("M", 10), ("N", 99), ("M", 10)]) == (tm.NONE, -1)   # one past it
    assert one(T123, 190, [("M", 10), ("N", 99), ("M", 10)]) == (tm.NONE, -1)   # the second block starts one before
    assert one(T123, 190, [("M", 10), ("N", 101), ("M", 10)]) == (tm.NONE, -1)  # one after
    assert one(T123, 190, [("M", 10), ("N", 100), ("M", 100), ("N", 100), ("M", 100)]) == (tm.ASSIGNED, 0)
    assert one(T123, 190, [("M", 10), ("N", 100), ("M", 99), ("N", 101), ("M", 100)]) == (tm.NONE, -1)
    assert one(T123, 190, [("M", 10), ("N", 100), ("M", 100), ("N", 100), ("M", 101)]) == (tm.NONE, -1)


def test_skipped_exons_retained_introns_and_deletions():
    skip = [("M", 10), ("N", 300), ("M", 10)]
    assert one(T123, 190, skip) == (tm.NONE, -1)
    assert one(T123 + [(0, 100, 200, "+", 0, 1), (0, 500, 600, "+", 0, 1)], 190, skip) == (tm.ASSIGNED, 0)
    assert one(T123, 190, [("M", 20)]) == (tm.NONE, -1)
    assert one(T123 + [(0, 100, 400, "+", 0, 1)], 190, [("M", 20)]) == (tm.ASSIGNED, 0)
    assert one(T123, 150, [("M", 10), ("D", 5), ("M", 10)]) == (tm.ASSIGNED, 0)
    assert one(T123, 190, [("M", 10), ("D", 100), ("M", 10)]) == (tm.NONE, -1)
    assert one(T123, 150, [("S", 5), ("M", 10), ("I", 3), ("=", 5), ("X", 1), ("P", 1), ("H", 2)]) == (tm.ASSIGNED, 0)
    assert one(T123, 150, [("M", 10), ("N", 0), ("M", 10)]) == (tm.NONE, -1)  # two abutting blocks: united exons never abut
    assert one(T123, 150, []) == (tm.NONE, -1) and one(T123, 150, [("S", 5), ("I", 5)]) == (tm.NONE, -1)
    # more blocks than the transcript has exons left
    assert one(T123, 590, [("M", 10), ("N", 100), ("M", 10)]) == (tm.NONE, -1)
    assert one(T123 + [(0, 700, 800, "+", 1, 1)], 590, [("M", 10), ("N", 100), ("M", 10)]) == (tm.NONE, -1)


def test_order_union_strands_and_several():
    desc = [(0, 500, 600, "-", 0, 0), (0, 300, 400, "-", 0, 0), (0, 100, 200, "-", 0, 0)]
    j = [("M", 10), ("N", 100), ("M", 10)]
    assert one(desc, 190, j, rev=True) == (tm.ASSIGNED, 0) and one(desc, 190, j) == (tm.NONE, -1)
    assert one(desc, 190, j, mode=tm.REVERSE) == (tm.ASSIGNED, 0) and one(desc, 190, j, mode=tm.UNSTRANDED) == (tm.ASSIGNED, 0)
    dot = [(r, s, e, ".", g, t) for r, s, e, _, g, t in desc]
    assert all(one(dot, 190, j, rev=v, mode=m) == (tm.ASSIGNED, 0) for v in (False, True) for m in (0, 1, 2))
    seam = [(0, 100, 150, "+", 0, 0), (0, 150, 200, "+", 0, 0), (0, 300, 360, "+", 0, 0), (0, 340, 400, "+", 0, 0)]
    assert one(seam, 140, [("M", 20)]) == (tm.ASSIGNED, 0) and one(seam, 330, [("M", 40)]) == (tm.ASSIGNED, 0)
    assert one(seam, 190, j) == (tm.ASSIGNED, 0)
    assert one(seam, 140, [("M", 10), ("N", 150), ("M", 10)]) == (tm.NONE, -1)  # 150 is no exon's end once united
    two = T123 + [(0, 100, 200, "+", 0, 1), (0, 300, 420, "+", 0, 1)]
    assert one(two, 190, j) == (tm.ASSIGNED, 0)
    other = T123 + [(0, 100, 200, "+", 1, 1), (0, 300, 420, "+", 1, 1)]
    assert one(other, 190, j) == (tm.SEVERAL, -1)
    graze = T123 + [(0, 195, 260, "+", 1, 1)]
    assert one(graze, 185, [("M", 15)]) == (tm.ASSIGNED, 0)
    assert am.assign(tm.overlap_exons(graze), 0, 185, False, [("M", 15)], tm.FORWARD) == (tm.SEVERAL, -1)
    assert one(T123, 195, [("M", 15)]) == (tm.NONE, -1)
    assert am.assign(tm.overlap_exons(T123), 0, 195, False, [("M", 15)], tm.FORWARD) == (tm.ASSIGNED, 0)
    with pytest.raises(ValueError):
        tm.transcripts_of(T123 + [(1, 700, 800, "+", 0, 0)])
    with pytest.raises(ValueError):
        tm.transcripts_of(T123 + [(0, 700, 800, "-", 0, 0)])
    with pytest.raises(ValueError):
        tm.transcripts_of(T123 + [(0, 700, 800, "+", 1, 0)])


def test_coordinates_at_the_limit():
    top = 2 ** 31 - 1
    ex = [(0, top - 100, top, "+", 0, 0)]
    assert one(ex, top - 5, [("M", 20)]) == (tm.NONE, -1)
    assert one(ex, top - 20, [("M", 20)]) == (tm.ASSIGNED, 0)
    assert one([(0, 0, 50, "+", 0, 0)], -3, [("M", 10)]) == (tm.NONE, -1)


# ---- the model against the brute force, and what the fuzz inputs hold -------------------------------------------

@pytest.fixture(scope="module")
def brute():
    ex, reads = tm.fuzz_annotation(), tm.fuzz_reads()
    return {mode: brute_assign_all(ex, reads, mode) for mode in (tm.FORWARD, tm.REVERSE, tm.UNSTRANDED)}


@pytest.mark.parametrize("mode", sorted(tm.MODES))
def test_model_against_brute_force_on_the_fuzz(brute, mode):
    mode = tm.MODES[mode]
    exp, b = tm.fuzz_expected(mode), brute[mode]
    assert [int(s) for s in exp["status"]] == [x[0] for x in b]
    assert [int(g) for g in exp["gene"]] == [x[1] for x in b]
    assert int(exp["counts"].sum()) == len(b) and exp["counts"].tolist() == np.bincount(exp["status"], minlength=3).tolist()
    ex, reads = tm.fuzz_annotation(), tm.fuzz_reads()
    for i in range(0, len(reads), 25):
        assert tm.assign(ex, *reads[i], mode) == (exp["status"][i], exp["gene"][i])


@pytest.mark.parametrize("mode", sorted(tm.MODES))
def test_fuzz_inputs_hold_what_the_gpu_tests_need(brute, mode):
    mode = tm.MODES[mode]
    ex, reads = tm.fuzz_annotation(), tm.fuzz_reads()
    exp, over = tm.fuzz_expected(mode), am.assign_all(tm.overlap_exons(ex), reads, mode)
    assert (exp["counts"] >= 200).all(), exp["counts"]
    st, ost = exp["status"], over["status"]
    assert int(((st == tm.ASSIGNED) & (ost == tm.SEVERAL)).sum()) >= 50
    assert int(((st == tm.NONE) & (ost == tm.ASSIGNED)).sum()) >= 50
    assert sum(1 for s, g, k in brute[mode] if s == tm.ASSIGNED and k >= 2) >= 50
    n_blocks = np.array([len(am.blocks(r[1], r[3])) for r in reads])
    assert int(((n_blocks >= 3) & (st == tm.ASSIGNED)).sum()) >= 50
    # G is a subset of E, read by read
    trs = tm.transcripts_of(ex)
    for (ref, pos, rev, cigar) in reads:
        G = {trs[t][2] for t in tm.fitting(trs, ref, pos, rev, cigar, mode)}
        E = {g for s, e in am.blocks(pos, cigar) for xr, xs, xe, strand, g, _ in ex
             if xr == ref and am.admissible(strand, rev, mode) and xs < e and s < xe}
        assert G <= E


def test_fuzz_annotation_shape():
    ex, reads = tm.fuzz_annotation(), tm.fuzz_reads()
    assert len(reads) == 5000 and am.n_genes_of(tm.overlap_exons(ex)) == tm.N_GENES
    trs = tm.transcripts_of(ex)
    per_gene = np.bincount([v[2] for v in trs.values()], minlength=tm.N_GENES)
    assert per_gene.min() >= 2 and per_gene.max() <= 5 and tm.n_transcripts_of(ex) == len(trs)
    assert {e[0] for e in ex} == {0, 1, 2} and {e[3] for e in ex} == {"+", "-", "."}
    assert {op for *_, c in reads for op, _ in c} == set(am.OPS)
    # exons come in descending and in shuffled order, and some transcripts' lines overlap or abut
    by_t = {}
    for e in ex:
        by_t.setdefault(e[5], []).append((e[1], e[2]))
    assert sum(1 for v in by_t.values() if len(v) > 2 and v == sorted(v, reverse=True)) >= 10
    assert sum(1 for v in by_t.values() if v != sorted(v) and v != sorted(v, reverse=True)) >= 3
    assert sum(1 for t, v in by_t.items() if len(v) > len(trs[t][3])) >= 5


@pytest.mark.parametrize("n", [1, am.GENE_TOP_CAP, 2 * am.GENE_TOP_CAP + 1])
def test_comb_inputs_reach_both_ends_of_the_table(n):
    ex, reads = tm.comb_annotation(n), tm.comb_reads(n)
    assert len({(e[1], e[2]) for e in ex}) == n
    got = tm.assign_all(ex, reads, tm.FORWARD)
    assert got["counts"][tm.NONE] > 100 and got["counts"][tm.ASSIGNED] > 100
    firsts = {r[1] // 10 for r, s in zip(reads, got["status"]) if s == tm.ASSIGNED and len(r[3]) == 1 and not r[2]}
    assert {0, n - 1} <= firsts
    if n > 1:
        assert sum(1 for r, s in zip(reads, got["status"]) if s == tm.ASSIGNED and len(r[3]) == 3) > 100


# ---- the library, before a device is looked at ------------------------------------------------------------------

def test_library_refuses_bad_arguments_without_a_context():
    import umi_collapse_rs_amd as umi
    from umi_collapse_rs_amd import _lib
    lib = umi.load()
    for name in ("umi_assign_genes_transcripts", "umi_assign_genes_transcripts_device"):
        assert name in _lib.SIGNATURES and getattr(lib, name)
    p = _lib.ptr
    reads = am.pack_reads([(0, 150, False, (("M", 10),))])
    rd = [p(reads[0], C.c_int32), p(reads[1], C.c_int32), p(reads[2], C.c_uint8), p(reads[3], C.c_uint32), p(reads[4], C.c_uint64)]
    gene, status, counts = np.zeros(1, np.int32), np.zeros(1, np.uint8), np.zeros(3, np.uint64)
    outs = [p(gene, C.c_int32), p(status, C.c_uint8), p(counts, C.c_uint64)]

    def call(ex, n_genes, n_tr, mode):
        a = [np.array([e[0] for e in ex], np.int32), np.array([e[1] for e in ex], np.int32), np.array([e[2] for e in ex], np.int32),
             np.frombuffer("".join(e[3] for e in ex).encode(), np.uint8), np.array([e[4] for e in ex], np.int32),
             np.array([e[5] for e in ex], np.int32)]
        rc = lib.umi_assign_genes_transcripts(None, p(a[0], C.c_int32), p(a[1], C.c_int32), p(a[2], C.c_int32), p(a[3], C.c_uint8),
                                              p(a[4], C.c_int32), p(a[5], C.c_int32), len(ex), n_genes, n_tr, mode, *rd, 1, *outs)
        return rc, lib.umi_last_error().decode()

    ok = (0, 100, 200, "+", 0, 0)
    for ex, n_genes, n_tr, mode, word in (
            ([(0, 5, 5, "+", 0, 0)], 1, 1, 0, "interval"), ([ok, (0, 1, 2, "-", 1, 1)], 1, 2, 0, "gene 1"),
            ([ok], 1, 1, 3, "strand_mode"), ([ok, (0, 300, 400, "+", 0, 1)], 1, 1, 0, "transcript 1"),
            ([ok, (0, 300, 400, "+", 0, -1)], 1, 1, 0, "transcript -1"), ([ok, (1, 300, 400, "+", 0, 0)], 1, 1, 0, "two references"),
            ([ok, (0, 300, 400, "-", 0, 0)], 1, 1, 0, "two strands"), ([ok, (0, 300, 400, "+", 1, 0)], 2, 1, 0, "two genes"),
            ([ok], 1, 1, 0, "ctx is NULL"), ([ok], 1, 7, 0, "ctx is NULL")):
        rc, msg = call(ex, n_genes, n_tr, mode)
        assert rc == _lib.UMI_ERR_ARG and word in msg, (ex, msg)
