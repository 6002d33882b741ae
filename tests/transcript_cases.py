"""The hand-written inputs of umi_assign_genes_transcripts' tests, shared by the GPU test (tests/
test_gpu_assign_genes_transcripts.py) and the CPU test of the lookup (tests/test_transcript_index_cpu.py): CASES maps a
name to (exons, reads, what the rule says: [(status, gene)] or None where the model alone is asked).  Each names the
way the lookup can go wrong."""
import annotation_model as am
import transcript_model as tm

A, N, S = tm.ASSIGNED, tm.NONE, tm.SEVERAL
TOP = 2 ** 31 - 1


def M(pos, length=10, ref=0, rev=False):
    return (ref, pos, rev, (("M", length),))


def R(pos, *cigar, ref=0, rev=False):
    """R(190, "10M", "100N", "10M")"""
    return (ref, pos, rev, tuple((c[-1], int(c[:-1])) for c in cigar))


def tr(t, gene, spans, strand="+", ref=0):
    return [(ref, s, e, strand, gene, t) for s, e in spans]


T123 = tr(0, 0, [(100, 200), (300, 400), (500, 600)])
J = ("10M", "100N", "10M")


def _wide(other):
    ex = []
    for k in range(100):
        ex += tr(k, 1 if k == other else 0, [(100, 200), (300, 400 + k)])
    return ex


def _deep():
    ex = tr(0, 0, [(1000, 9000)])
    for i in range(3000):
        ex += tr(1 + i, 1 + i % 5, [(1001 + 2 * i, 1003 + 2 * i)])
    reads = [M(8950 - i, 40 + i) for i in range(40)] + [M(1001, 2), M(1003, 2), M(6999, 2), M(7001, 2), M(7003, 20), M(1000, 8000),
                                                         M(999, 20), M(8990, 11)]
    want = [(A, 0)] * 40 + [(S, -1), (S, -1), (S, -1), (A, 0), (A, 0), (A, 0), (N, -1), (N, -1)]
    return ex, reads, want


def _long():
    spans = [(1000 + 100 * i, 1050 + 100 * i) for i in range(64)]
    through = ["10M"] + ["50N", "50M"] * 38 + ["50N", "20M"]
    off = list(through)
    off[41] = "51N"  # the 21st junction a base long: the next block starts behind its exon's start
    ex = tr(0, 0, spans) + tr(1, 1, [(s + 20000, e + 20000) for s, e in spans[:3]])
    to_end = ["10M"] + ["50N", "50M"] * 53  # from exon 10 to the last, whole
    over = to_end + ["50N", "50M"]          # one block more than the transcript has exons left
    return ex, [R(2040, *through), R(2040, *off), R(2040, *to_end), R(2040, *over)], [(A, 0), (N, -1), (A, 0), (N, -1)]


CASES = {
    # off by one at both ends of an exon, for a one-block read
    "containment": (tr(0, 0, [(100, 200)]),
                    [M(100, 100), M(99, 10), M(100, 10), M(190, 10), M(191, 10), M(99, 102), M(100, 101), M(99, 101), M(150, 1)],
                    [(A, 0), (N, -1), (A, 0), (A, 0), (N, -1), (N, -1), (N, -1), (N, -1), (A, 0)]),
    # a first block that ends one short of, or one past, the exon's end; a second that starts one before, or after
    "junctions": (T123,
                  [R(190, *J), R(189, "10M", "101N", "10M"), R(191, "10M", "99N", "10M"), R(190, "10M", "99N", "10M"),
                   R(190, "10M", "101N", "10M"), R(190, "10M", "100N", "100M", "100N", "100M"),
                   R(190, "10M", "100N", "99M", "101N", "100M"), R(190, "10M", "100N", "100M", "100N", "101M"),
                   R(190, "10M", "100N", "100M", "99N", "100M"), R(100, "100M", "100N", "100M", "100N", "100M")],
                  [(A, 0), (N, -1), (N, -1), (N, -1), (N, -1), (A, 0), (N, -1), (N, -1), (N, -1), (A, 0)]),
    "skipped exon, 1-2-3 alone": (T123, [R(190, "10M", "300N", "10M")], [(N, -1)]),
    "skipped exon, with 1-3": (T123 + tr(1, 0, [(100, 200), (500, 600)]), [R(190, "10M", "300N", "10M"), R(190, *J)], [(A, 0), (A, 0)]),
    "retained intron, none": (T123, [M(190, 20), M(290, 20)], [(N, -1), (N, -1)]),
    "retained intron, covered": (T123 + tr(1, 0, [(100, 400)]), [M(190, 20), M(290, 20), R(390, "10M", "100N", "10M")],
                                 [(A, 0), (A, 0), (A, 0)]),
    "deletions": (T123, [R(150, "10M", "5D", "10M"), R(190, "10M", "100D", "10M"), R(190, "5M", "5D", "100N", "2D", "8M")],
                  [(A, 0), (N, -1), (A, 0)]),
    "other ops and empty reads": (T123,
                                  [R(150, "5S", "10M", "3I", "5=", "1X", "1P", "2H"), R(150, "10M", "0N", "10M"), R(150), R(150, "5S", "5I", "2H", "1P"),
                                   R(150, "10N"), R(150, "0M"), R(90, "10N", "10M"), R(190, "10M", "50N", "0M", "50N", "10M"),
                                   R(190, "3H", "10M", "4I", "100N", "2S")],
                                  [(A, 0), (N, -1), (N, -1), (N, -1), (N, -1), (N, -1), (A, 0), (A, 0), (A, 0)]),
    "two transcripts of one gene": (T123 + tr(1, 0, [(100, 200), (300, 420)]), [R(190, *J), M(150)], [(A, 0), (A, 0)]),
    "transcripts of two genes": (T123 + tr(1, 1, [(100, 200), (300, 420)]), [R(190, *J), M(150), R(190, "10M", "100N", "110M")],
                                 [(S, -1), (S, -1), (A, 1)]),
    "fits A and grazes B": (T123 + tr(1, 1, [(195, 260)]), [M(185, 15), R(185, "15M", "100N", "10M")], [(A, 0), (A, 0)]),
    "overlaps but fits nothing": (T123, [M(195, 15), R(190, "10M", "100N", "101M")], [(N, -1), (N, -1)]),
    "exons descending": (tr(0, 0, [(500, 600), (300, 400), (100, 200)], "-"), [R(190, *J, rev=True), R(190, *J)], None),
    "exons shuffled": (tr(0, 0, [(300, 400), (700, 800), (100, 200), (500, 600)]),
                       [R(190, "10M", "100N", "100M", "100N", "100M", "100N", "5M"), R(390, *J)], [(A, 0), (A, 0)]),
    "seams": (tr(0, 0, [(100, 150), (150, 200), (300, 360), (340, 400)]),
              [M(140, 20), M(330, 40), R(190, *J), R(140, "10M", "150N", "10M"), R(190, "10M", "140N", "10M")],
              [(A, 0), (A, 0), (A, 0), (N, -1), (N, -1)]),
    "a dot transcript": (tr(0, 0, [(100, 200), (300, 400)], "."), [R(190, *J), R(190, *J, rev=True)], None),
    # transcript 0 ends where the read goes on; transcript 1 follows it in the table and starts where the read's third block lies
    "more blocks than exons left": (tr(0, 0, [(100, 200), (300, 400)]) + tr(1, 1, [(500, 600), (700, 800)]),
                                    [R(190, "10M", "100N", "100M", "100N", "10M"), R(190, *J), R(590, *J)], [(N, -1), (A, 0), (A, 1)]),
    "40 blocks through 64 exons": _long(),
    "wide instance list, one gene": (_wide(-1), [R(190, "10M", "100N", "100M"), R(190, "10M", "100N", "160M"), R(190, "10M", "100N", "200M"), M(150)],
                                     [(A, 0), (A, 0), (N, -1), (A, 0)]),
    "wide instance list, another gene among them": (_wide(50), [R(190, "10M", "100N", "100M"), R(190, "10M", "100N", "160M"),
                                                                R(190, "10M", "100N", "150M"), M(150)],
                                                    [(S, -1), (A, 0), (S, -1), (S, -1)]),
    "deep walk-back": _deep(),
    "coordinates at the limit": (tr(0, 0, [(TOP - 100, TOP)]) + tr(1, 1, [(0, 50), (100, 150)]),
                                 [M(TOP - 4, 20), M(TOP - 20, 20), M(TOP - 20, 21), M(-3, 10), M(0, 10), R(-60, "10M", "50N", "20M"),
                                  R(TOP - 20, "10M", "5N", str(2 ** 28 - 1) + "M"), R(40, "10M", "50N", "10M")],
                                 [(N, -1), (A, 0), (N, -1), (N, -1), (A, 1), (N, -1), (N, -1), (A, 1)]),
    "absent references": (tr(0, 0, [(100, 200)]) + tr(1, 1, [(100, 200)], ref=2), [M(150, ref=r, rev=v) for r in (0, 1, 2, 3, TOP) for v in (False, True)], None),
}


def comb(n=2 * am.GENE_TOP_CAP + 1):
    """the table-size case: (exons, reads)"""
    return list(tm.comb_annotation(n)), list(tm.comb_reads(n))
