// The index of an annotation's transcripts and the lookup of a read in it (umi_assign_genes_transcripts, the
// program's --gene-rule transcript).  One header for the host and the device: the kernel
// (umihip_gene_transcripts.hip) and the CPU test (tests/cpp/test_transcript_index.cpp) run the same lookup code.  No
// HIP call, no allocation in the lookup.
//
// The rule (include/umihip.h has it in full; tests/transcript_model.py defines it): a transcript's exons, ascending and
// united where they overlap or abut, are x_1 < ... < x_n; a read with blocks b_1 .. b_m, m >= 1, fits the transcript
// when there is a j with b_i inside x_{j+i-1} for every i, end(b_i) == end(x_{j+i-1}) and start(b_{i+1}) ==
// start(x_{j+i}) for every i < m.  G: the genes with a transcript the read fits, on its reference and an admissible
// strand.  One gene: assigned; none: none; two or more: several.
//
// Index: one table per strand class, as the overlap index has them (umihip_gene_index.hpp).  A table holds
//   instances: every taken transcript's united exons, transcript-major and ascending: x[] (start, end: the positions
//     alone, a transcript lies on one reference) and of[] (stop: the index behind the last instance of the
//     instance's transcript, and the transcript's gene -- kept per instance, so that a candidate costs one load and
//     no walk through a transcript array);
//   distinct exons: the distinct (start, end) pairs among the instances as keys ref << 32 | pos, sorted by start, then
//     end: start[], end[], dmax[] (the running maximum of end[0 .. i]), label[] (the one gene that owns all the
//     pair's instances, or GENE_MULTI), and the pair's instances inst[off[i] .. off[i + 1]);
//   top: every 2^shift-th start (the last of each chunk), at most `cap`, for LDS: GeneTop, searched as the overlap
//     index's.
//
// Query of a read: a first walk of its CIGAR checks the op codes, counts the non-empty blocks and keeps the first,
// [s, e).  d = the last distinct exon with start <= s (a binary search); d steps back while dmax[d] >= e: no exon
// before that reaches e.  m == 1: every exon passed with end >= e contains the block, and its label is the answer's
// share; no transcript is touched.  m >= 2: only exons with end == e count; for each instance p of such an exon with
// p + m <= stop, the CIGAR is walked again from behind the first block, block i against instance p + i: both ends
// equal for a middle block, start equal and end <= for the last.  The first gene seen is kept; a second one ends the
// query: several.  An instance whose gene is the one already seen is not walked.
//
// Behind the lookup: the gene bodies behind the transcripts and the class of a read (umi_assign_genes_transcripts_classes,
// the program's --transcript-introns): the end of this file; tests/cpp/test_transcript_tiers.cpp runs it on the CPU.
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#include "umihip_gene_index.hpp"

namespace umihip {

struct TrExon {
    int32_t start, end;
};

struct TrOf {
    uint32_t stop; // the index behind the last instance of this instance's transcript
    int32_t gene;
};

struct TranscriptTable {
    std::vector<TrExon> x;
    std::vector<TrOf> of;
    std::vector<uint64_t> start, end, dmax;
    std::vector<int32_t> label;
    std::vector<uint32_t> off, inst;
    std::vector<uint64_t> top;
    int top_shift = 0;
};

struct TranscriptView {
    const TrExon *x;
    const TrOf *of;
    const uint64_t *start, *end, *dmax;
    const int32_t *label;
    const uint32_t *off, *inst;
    uint32_t n; // distinct exons
};

// what is wrong with exon_transcript: 0 nothing; else *bad is the first exon at fault
constexpr int TR_OK = 0, TR_BAD_RANGE = 1, TR_BAD_REF = 2, TR_BAD_STRAND = 3, TR_BAD_GENE = 4;

// The caller has checked the exons as gene_index_build asks.  All exons of a transcript must share ref, strand and gene.
inline int transcript_check(const int32_t *ref, const uint8_t *strand, const int32_t *gene, const int32_t *transcript, uint64_t n_exons,
                            uint32_t n_transcripts, uint64_t *bad)
{
    for (uint64_t i = 0; i < n_exons; i++)
        if (transcript[i] < 0 || (uint32_t)transcript[i] >= n_transcripts) {
            *bad = i;
            return TR_BAD_RANGE;
        }
    // a transcript's first exon (a map, not an array of n_transcripts: the count may lie far above the transcripts used).
    // A file names a transcript's lines one after another, so most lines find their transcript in `last`
    std::unordered_map<int32_t, uint64_t> first_of;
    int32_t last = -1;
    uint64_t f = 0;
    for (uint64_t i = 0; i < n_exons; i++) {
        if (transcript[i] != last) {
            const auto at = first_of.emplace(transcript[i], i);
            last = transcript[i];
            f = at.first->second;
            if (at.second) continue;
        }
        *bad = i;
        if (ref[i] != ref[f]) return TR_BAD_REF;
        if (strand[i] != strand[f]) return TR_BAD_STRAND;
        if (gene[i] != gene[f]) return TR_BAD_GENE;
    }
    return TR_OK;
}

// The table of the transcripts whose strand is in `take` (GENE_TAKE_*).  The exons have passed transcript_check.
inline void transcript_index_build(const int32_t *ref, const int32_t *start, const int32_t *end, const uint8_t *strand,
                                   const int32_t *gene, const int32_t *transcript, uint64_t n_exons, unsigned take, TranscriptTable &t)
{
    t = TranscriptTable();
    std::vector<uint64_t> order;
    order.reserve(n_exons);
    for (uint64_t i = 0; i < n_exons; i++) {
        const unsigned bit = strand[i] == '+' ? GENE_TAKE_PLUS : strand[i] == '-' ? GENE_TAKE_MINUS : GENE_TAKE_DOT;
        if (take & bit) order.push_back(i);
    }
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) {
        if (transcript[a] != transcript[b]) return transcript[a] < transcript[b];
        if (start[a] != start[b]) return start[a] < start[b];
        return end[a] < end[b];
    });
    // instances: a transcript's lines united, and the key of each for the distinct exons
    struct Key {
        uint64_t ks, ke;
        uint32_t inst;
    };
    std::vector<Key> keys;
    for (size_t i = 0; i < order.size();) {
        const int32_t tr = transcript[order[i]];
        const size_t first = t.x.size();
        for (; i < order.size() && transcript[order[i]] == tr; i++) {
            const uint64_t e = order[i];
            if (t.x.size() > first && start[e] <= t.x.back().end)
                t.x.back().end = std::max(t.x.back().end, end[e]);
            else
                t.x.push_back({start[e], end[e]});
        }
        const uint64_t any = order[i - 1];
        for (size_t p = first; p < t.x.size(); p++) {
            t.of.push_back({(uint32_t)t.x.size(), gene[any]});
            keys.push_back({gene_key((uint32_t)ref[any], (uint64_t)t.x[p].start), gene_key((uint32_t)ref[any], (uint64_t)t.x[p].end), (uint32_t)p});
        }
    }
    std::sort(keys.begin(), keys.end(), [](const Key &a, const Key &b) {
        if (a.ks != b.ks) return a.ks < b.ks;
        if (a.ke != b.ke) return a.ke < b.ke;
        return a.inst < b.inst;
    });
    t.inst.reserve(keys.size());
    for (size_t i = 0; i < keys.size(); i++) {
        const int32_t g = t.of[keys[i].inst].gene;
        if (i == 0 || keys[i].ks != keys[i - 1].ks || keys[i].ke != keys[i - 1].ke) {
            t.start.push_back(keys[i].ks);
            t.end.push_back(keys[i].ke);
            t.dmax.push_back(t.dmax.empty() ? keys[i].ke : std::max(t.dmax.back(), keys[i].ke));
            t.label.push_back(g);
            t.off.push_back((uint32_t)i);
        } else if (t.label.back() != g) {
            t.label.back() = GENE_MULTI;
        }
        t.inst.push_back(keys[i].inst);
    }
    t.off.push_back((uint32_t)keys.size());
}

// the top: the last start of each chunk of 2^shift distinct exons, at most cap of them
inline void transcript_index_sample(TranscriptTable &t, uint32_t cap)
{
    const uint64_t n = t.start.size();
    t.top_shift = gene_top_shift(n, cap);
    const uint64_t chunks = (n + ((uint64_t)1 << t.top_shift) - 1) >> t.top_shift;
    t.top.resize(chunks);
    for (uint64_t j = 0; j < chunks; j++) t.top[j] = t.start[std::min<uint64_t>((j + 1) << t.top_shift, n) - 1];
}

inline TranscriptView transcript_view(const TranscriptTable &t)
{
    return {t.x.data(), t.of.data(), t.start.data(), t.end.data(), t.dmax.data(), t.label.data(), t.off.data(), t.inst.data(), (uint32_t)t.start.size()};
}
inline GeneTop transcript_top(const TranscriptTable &t) { return {t.top.data(), (uint32_t)t.top.size(), t.top_shift}; }

// the first distinct exon that starts behind key ks (t.n: none)
UMIHIP_HD inline uint32_t transcript_first_behind(const TranscriptView &t, const GeneTop *top, uint64_t ks)
{
    if (!top) return gene_first_above(t.start, 0, t.n, ks);
    const uint32_t j = gene_first_above(top->top, 0, top->n_top, ks);
    if (j == top->n_top) return t.n;
    const uint64_t a = (uint64_t)j << top->shift, b = (uint64_t)(j + 1) << top->shift;
    return gene_first_above(t.start, (uint32_t)a, (uint32_t)(b < t.n ? b : t.n), ks); // (top[j] > ks: it is in the chunk)
}

// The blocks of a read, one after another, its CIGAR read from memory: c the next word, at the reference position there.
struct TrWalk {
    uint64_t c;
    int64_t at;
};

// the next non-empty block [*s, *e) (the op codes have been checked); false: there is none
UMIHIP_HD inline bool transcript_next_block(const uint32_t *cigar, uint64_t n_cigar, TrWalk &w, int64_t *s, int64_t *e)
{
    int64_t bs = w.at, be = w.at;
    while (w.c < n_cigar) {
        const uint32_t op = cigar[w.c] & 15u, len = cigar[w.c] >> 4;
        w.c++;
        if (op == 0 || op == 2 || op == 7 || op == 8) {
            be += len;
        } else if (op == 3) {
            if (be > bs) {
                w.at = be + len;
                *s = bs, *e = be;
                return true;
            }
            bs = be = be + len;
        }
    }
    w.at = be;
    *s = bs, *e = be;
    return be > bs;
}

// do blocks 2 .. m of the read (w: behind the first) fit instances p + 1 .. p + m - 1; p + m <= the transcript's stop
UMIHIP_HD inline bool transcript_rest_fits(const TranscriptView &t, uint32_t p, uint64_t m, const uint32_t *cigar, uint64_t n_cigar, TrWalk w)
{
    for (uint64_t i = 1; i < m; i++) {
        int64_t s, e;
        transcript_next_block(cigar, n_cigar, w, &s, &e);
        const TrExon x = t.x[p + i];
        if (s != (int64_t)x.start) return false;
        if (i + 1 < m ? e != (int64_t)x.end : e > (int64_t)x.end) return false;
    }
    return true;
}

// A read: GENE_READ_* and *gene (-1 unless assigned); GENE_READ_BAD_OP at an op code above 8.  Coordinates are kept in
// 64 bits: a block that starts before 0 or ends behind 2^31 - 1 lies in no exon, and the read fits nothing.
// steps (may be null): the distinct exons the walk back looked at are added to it.  blocks (may be null): m, the
// number of the read's non-empty blocks, whatever the verdict (0 at a bad op code).
UMIHIP_HD inline int transcript_assign_read(const TranscriptView &t, const GeneTop *top, uint32_t ref, int64_t pos, const uint32_t *cigar,
                                            uint64_t n_cigar, int32_t *gene, uint64_t *steps, uint64_t *blocks = nullptr)
{
    *gene = -1;
    if (blocks) *blocks = 0;
    // the first walk: every op code, the number of non-empty blocks, the first of them and the walk's state behind it
    uint64_t m = 0;
    int64_t s = pos, e = pos, s1 = 0, e1 = 0;
    TrWalk behind = {0, 0};
    bool outside = false;
    for (uint64_t c = 0; c <= n_cigar; c++) {
        uint32_t op = 3, len = 0; // (behind the last word: the open block is closed)
        if (c < n_cigar) {
            op = cigar[c] & 15u;
            len = cigar[c] >> 4;
            if (op > 8) return GENE_READ_BAD_OP;
        }
        if (op == 0 || op == 2 || op == 7 || op == 8) {
            e += len;
            continue;
        }
        if (op != 3) continue;
        if (e > s) {
            if (m++ == 0) {
                s1 = s, e1 = e;
                behind = {c + 1, e + len};
            }
            outside |= s < 0 || e >= GENE_POS_LIMIT;
        }
        s = e = e + len;
    }
    if (blocks) *blocks = m;
    if (m == 0 || outside) return GENE_READ_NONE;
    const uint64_t ks = gene_key(ref, (uint64_t)s1), ke = gene_key(ref, (uint64_t)e1);
    int32_t found = GENE_HIT_NONE;
    // (an exon that starts at or before ks and ends at or behind ke lies on ref: its two keys share their reference)
    for (uint32_t d = transcript_first_behind(t, top, ks); d > 0 && t.dmax[d - 1] >= ke; d--) {
        if (steps) ++*steps;
        const uint64_t end = t.end[d - 1];
        if (m == 1 ? end < ke : end != ke) continue;
        const int32_t label = t.label[d - 1];
        if (label == found) continue;
        if (m == 1) {
            if (label == GENE_MULTI || found >= 0) return GENE_READ_SEVERAL;
            found = label;
            continue;
        }
        for (uint32_t k = t.off[d - 1]; k < t.off[d]; k++) {
            const uint32_t p = t.inst[k];
            const TrOf of = t.of[p];
            if (of.gene == found || (uint64_t)p + m > (uint64_t)of.stop) continue;
            if (!transcript_rest_fits(t, p, m, cigar, n_cigar, behind)) continue;
            if (found >= 0) return GENE_READ_SEVERAL;
            found = of.gene;
            if (label != GENE_MULTI) break; // (the exon's other instances are this gene's too)
        }
    }
    if (found == GENE_HIT_NONE) return GENE_READ_NONE;
    *gene = found;
    return GENE_READ_ASSIGNED;
}

// ---- transcripts first, gene bodies behind them, and the class of a read (umi_assign_genes_transcripts_classes, the
// ---- program's --transcript-introns) ----
// G: the genes with a transcript the read fits (transcript_assign_read).  B: the genes whose body shares a base with a
// block (gene_assign_read against the body table, umihip_gene_index.hpp).  G is in E, the overlap rule's set, and E
// is in B.  exon-first: G one gene: that gene, tier transcript (GENE_TIER_EXON); G several: several; G empty: B's
// verdict, tier body (GENE_TIER_INTRON).  all: G several: several (G is in B); else B's verdict, tier transcript where
// G is not empty, else body.  off: G's verdict.
//
// Class of an assigned read.  Tier transcript: JUNCTION where m >= 2, else EXONIC -- every gap of a fitting read is an
// intron of a transcript it fits, nothing is looked up.  Tier body, gene g: the blocks cut to [0, GENE_POS_LIMIT); c
// the summed cover of the blocks by g's exon lines.  B = {g} gives E in {g}: every segment of the overlap table that a
// block touches carries g's label (another gene's exon there would put that gene into E, and so into B), so the
// table's cover of a block is g's -- the argument umihip_gene_index.hpp makes for tier exon.  c == 0: INTRONIC; c below
// the summed length: SPANNING; else the gaps decide as gene_read_class has them: one that the table or g's own exons
// do not cover whole: JUNCTION (the read is spliced, by an isoform the annotation does not have), else EXONIC.
struct TrCoverView {
    GeneView exons; // the overlap table of the strand class, searched without a top
    const uint64_t *cum;
    GeneOwnView own;
};

// The class of a read assigned to gene g by a body (its CIGAR has passed transcript_assign_read: no bad op code).  One
// walk for the summed cover; the gaps are walked only where the cover is whole and there are two blocks.
UMIHIP_HD inline int transcript_body_class(const TrCoverView &v, int32_t g, uint32_t ref, int64_t pos, const uint32_t *cigar,
                                           uint64_t n_cigar)
{
    uint64_t covered = 0, length = 0;
    uint32_t blocks = 0;
    for (int walk = 0; walk < 2; walk++) {
        int64_t s = pos, e = pos, prev_end = -1;
        for (uint64_t c = 0; c <= n_cigar; c++) {
            uint32_t op = 3, len = 0; // (behind the last word: the open block is closed)
            if (c < n_cigar) {
                op = cigar[c] & 15u;
                len = cigar[c] >> 4;
            }
            if (op == 0 || op == 2 || op == 7 || op == 8) {
                e += len;
                continue;
            }
            if (op != 3) continue;
            const int64_t bs = s < 0 ? 0 : s, be = e > GENE_POS_LIMIT ? GENE_POS_LIMIT : e;
            if (be > bs) {
                if (walk == 0) {
                    blocks++;
                    covered += gene_cover(v.exons, nullptr, v.cum, ref, (uint64_t)bs, (uint64_t)be);
                    length += (uint64_t)(be - bs);
                } else if (prev_end >= 0 && bs > prev_end) {
                    const uint64_t gs = (uint64_t)prev_end, ge = (uint64_t)bs;
                    if (gene_cover(v.exons, nullptr, v.cum, ref, gs, ge) < ge - gs || !gene_own_covers(v.own, g, ref, gs, ge))
                        return GENE_CLASS_JUNCTION;
                }
                prev_end = be;
            }
            s = e = e + len;
        }
        if (covered == 0) return GENE_CLASS_INTRONIC;
        if (covered < length) return GENE_CLASS_SPANNING;
        if (blocks < 2) break;
    }
    return GENE_CLASS_EXONIC;
}

// A read under --transcript-introns, in three phases.  Phase 1 is transcript_assign_read, which looks at every word
// and so finds a bad op code; it also gives m.  Phase 2, gene_assign_read against the bodies, runs only where the
// verdict still depends on B (transcript_needs_bodies).  Phase 3, the body tier's class, runs only for a read that a
// body assigned, and only where classes are asked for (cover given; cover null: *cls is not written).

// does the verdict of a read with phase 1's verdict st still depend on B
UMIHIP_HD inline bool transcript_needs_bodies(int mode, int st)
{
    if (st == GENE_READ_ASSIGNED) return mode == GENE_INTRONS_ALL;
    return st == GENE_READ_NONE && mode != GENE_INTRONS_OFF;
}

// the class of a read that a transcript assigned
UMIHIP_HD inline int transcript_fit_class(bool spliced) { return spliced ? GENE_CLASS_JUNCTION : GENE_CLASS_EXONIC; }

// Phases 2 and 3 of a read that needs them (its CIGAR has passed phase 1).  fits: phase 1 assigned it; spliced: m >= 2.
UMIHIP_HD inline int transcript_assign_read_bodies(const GeneView &bodies, const GeneTop *body_top, const TrCoverView *cover, bool fits,
                                                   bool spliced, uint32_t ref, int64_t pos, const uint32_t *cigar, uint64_t n_cigar,
                                                   int32_t *gene, int *tier, int *cls)
{
    const int st = gene_assign_read(bodies, body_top, ref, pos, cigar, n_cigar, gene);
    *tier = st == GENE_READ_ASSIGNED && !fits ? GENE_TIER_INTRON : GENE_TIER_EXON;
    if (cover)
        *cls = st != GENE_READ_ASSIGNED ? GENE_CLASS_NONE
               : fits                   ? transcript_fit_class(spliced)
                                        : transcript_body_class(*cover, *gene, ref, pos, cigar, n_cigar);
    return st;
}

// The three phases of one read: GENE_READ_*, *gene, *tier (GENE_TIER_EXON unless the read is assigned by a body), *cls.
UMIHIP_HD inline int transcript_assign_read_tiers(const TranscriptView &t, const GeneTop *top, const GeneView &bodies, const GeneTop *body_top,
                                                  const TrCoverView *cover, int mode, uint32_t ref, int64_t pos, const uint32_t *cigar,
                                                  uint64_t n_cigar, int32_t *gene, int *tier, int *cls)
{
    *tier = GENE_TIER_EXON;
    if (cover) *cls = GENE_CLASS_NONE;
    uint64_t m = 0;
    const int st = transcript_assign_read(t, top, ref, pos, cigar, n_cigar, gene, nullptr, &m);
    if (st == GENE_READ_BAD_OP) return st;
    if (transcript_needs_bodies(mode, st))
        return transcript_assign_read_bodies(bodies, body_top, cover, st == GENE_READ_ASSIGNED, m >= 2, ref, pos, cigar, n_cigar, gene, tier, cls);
    if (cover && st == GENE_READ_ASSIGNED) *cls = transcript_fit_class(m >= 2);
    return st;
}

} // namespace umihip
