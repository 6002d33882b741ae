// The index of an annotation and the lookup of a read in it (umi_assign_genes, the program's
// --gene-annotation).  One header for the host and the device: the kernel (umihip_genes.hip) and the CPU
// test (tests/cpp/test_gene_index.cpp) run the same lookup code.  No HIP call, no allocation in the lookup.
//
// The rule (include/umihip.h has it in full): a gene hits a read when one of its exons, on the read's
// reference and on an admissible strand, shares a base with one of the read's blocks; one gene: assigned,
// none: none, two or more: several.
//
// Index: one table per strand class (the exons a read of one strand may hit).  A position is the key
// ref << 32 | pos; the line of keys is cut at every exon boundary, and only the covered elementary segments
// are kept, sorted: start[], end[] (half-open, disjoint), and per segment its label -- the one gene that
// covers it, or GENE_MULTI where two do -- and its run: the number of its maximal stretch of consecutive kept
// segments that share one single-gene label (a GENE_MULTI segment is a run of its own).  Uncovered gaps lie
// between kept segments and belong to no run: a block that spans a gap between two segments of one gene hits
// that gene alone.
//
// Query of a block [s, e), e > s: lo = the first segment with end > s, hi = the last with start < e.
// lo > hi: none.  label[lo] == GENE_MULTI or run[lo] != run[hi]: several.  Otherwise label[lo].
// lo is a binary search over end[]; hi is found from lo by doubling steps over start[] (a block is short:
// hi is lo or a few segments on).
//
// Top: every 2^shift-th end (the last end of each chunk of 2^shift segments), at most `cap` of them, small
// enough for LDS.  A search over the top names the chunk, a search over the chunk's ends the segment.
//
// Gene bodies (umi_assign_genes_introns, --gene-introns) are a second tier of the same tables: the end of this file.
// Behind them: the covered bases of an interval and the class of a read (umi_assign_genes_classes, --velocity).
#pragma once
#include <algorithm>
#include <cstdint>
#include <unordered_map>
#include <vector>

#if defined(__HIPCC__)
#define UMIHIP_HD __host__ __device__
#else
#define UMIHIP_HD
#endif

namespace umihip {

constexpr int32_t GENE_MULTI = -2;      // the label of a segment that two genes cover
constexpr int32_t GENE_HIT_NONE = -1;   // what a block's query gives beside a gene's index
constexpr int32_t GENE_HIT_SEVERAL = -2;
constexpr int64_t GENE_POS_LIMIT = (int64_t)1 << 31; // no exon reaches this coordinate (its end is an int32)
// what a read comes to (UMI_GENE_* of include/umihip.h), and GENE_READ_BAD_OP for a CIGAR op code above 8
constexpr int GENE_READ_ASSIGNED = 0, GENE_READ_NONE = 1, GENE_READ_SEVERAL = 2, GENE_READ_BAD_OP = -1;
// exon strands a table takes (gene_index_build's `take`)
constexpr unsigned GENE_TAKE_PLUS = 1, GENE_TAKE_MINUS = 2, GENE_TAKE_DOT = 4;

struct GeneSeg {
    int32_t label;
    uint32_t run;
};

struct GeneTable {
    std::vector<uint64_t> start, end;
    std::vector<GeneSeg> seg;
    std::vector<uint64_t> top;
    int top_shift = 0;
};

struct GeneView {
    const uint64_t *start, *end;
    const GeneSeg *seg;
    uint32_t n;
};

// (top == nullptr: the whole of end[] is searched)
struct GeneTop {
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

UMIHIP_HD inline uint64_t gene_key(uint32_t ref, uint64_t pos) { return (uint64_t)ref << 32 | pos; }

// The table of the exons whose strand is in `take`.  The caller has checked the exons: 0 <= start < end,
// ref >= 0, 0 <= gene < n_genes, strand one of + - .
inline void gene_index_build(const int32_t *ref, const int32_t *start, const int32_t *end, const uint8_t *strand,
                             const int32_t *gene, uint64_t n_exons, uint32_t n_genes, unsigned take, GeneTable &t)
{
    struct Event {
        uint64_t key;
        int32_t gene, delta;
    };
    std::vector<Event> ev;
    ev.reserve(2 * n_exons);
    for (uint64_t i = 0; i < n_exons; i++) {
        const unsigned bit = strand[i] == '+' ? GENE_TAKE_PLUS : strand[i] == '-' ? GENE_TAKE_MINUS : GENE_TAKE_DOT;
        if (!(take & bit)) continue;
        ev.push_back({gene_key((uint32_t)ref[i], (uint64_t)start[i]), gene[i], 1});
        ev.push_back({gene_key((uint32_t)ref[i], (uint64_t)end[i]), gene[i], -1});
    }
    std::sort(ev.begin(), ev.end(), [](const Event &a, const Event &b) { return a.key < b.key; });
    t.start.clear();
    t.end.clear();
    t.seg.clear();
    // exons open per gene, the genes with one open, and the sum of their indices: with one gene, the gene
    std::vector<uint32_t> open(n_genes, 0);
    uint32_t genes_open = 0;
    uint64_t index_sum = 0;
    for (size_t i = 0; i < ev.size();) {
        const uint64_t key = ev[i].key;
        for (; i < ev.size() && ev[i].key == key; i++) {
            uint32_t &o = open[(size_t)ev[i].gene];
            if (ev[i].delta > 0) {
                if (o++ == 0) genes_open++, index_sum += (uint64_t)ev[i].gene;
            } else if (--o == 0) {
                genes_open--, index_sum -= (uint64_t)ev[i].gene;
            }
        }
        if (!genes_open) continue; // (every exon ends on its own reference: nothing is open across two)
        const int32_t label = genes_open == 1 ? (int32_t)index_sum : GENE_MULTI;
        uint32_t run = 0;
        if (!t.seg.empty()) {
            const GeneSeg &p = t.seg.back();
            run = (label == GENE_MULTI || label != p.label) ? p.run + 1 : p.run;
        }
        t.start.push_back(key);
        t.end.push_back(ev[i].key);
        t.seg.push_back({label, run});
    }
    t.top.clear();
    t.top_shift = 0;
}

// the smallest shift at which n segments have at most cap chunks of 2^shift
inline int gene_top_shift(uint64_t n, uint32_t cap)
{
    int s = 0;
    while (((n + ((uint64_t)1 << s) - 1) >> s) > cap) s++;
    return s;
}

inline void gene_index_sample(GeneTable &t, uint32_t cap)
{
    const uint64_t n = t.end.size();
    t.top_shift = gene_top_shift(n, cap);
    const uint64_t chunks = (n + ((uint64_t)1 << t.top_shift) - 1) >> t.top_shift;
    t.top.resize(chunks);
    for (uint64_t j = 0; j < chunks; j++) t.top[j] = t.end[std::min<uint64_t>((j + 1) << t.top_shift, n) - 1];
}

inline GeneView gene_view(const GeneTable &t) { return {t.start.data(), t.end.data(), t.seg.data(), (uint32_t)t.end.size()}; }
inline GeneTop gene_top(const GeneTable &t) { return {t.top.data(), (uint32_t)t.top.size(), t.top_shift}; }

// the first of v[a, b) above key; b where none is
UMIHIP_HD inline uint32_t gene_first_above(const uint64_t *v, uint32_t a, uint32_t b, uint64_t key)
{
    while (a < b) {
        const uint32_t m = a + (b - a) / 2;
        if (v[m] > key)
            b = m;
        else
            a = m + 1;
    }
    return a;
}

// lo: the first segment that ends behind key ks (t.n: none)
UMIHIP_HD inline uint32_t gene_first_segment(const GeneView &t, const GeneTop *top, uint64_t ks)
{
    if (!top) return gene_first_above(t.end, 0, t.n, ks);
    const uint32_t j = gene_first_above(top->top, 0, top->n_top, ks);
    if (j == top->n_top) return t.n;
    const uint64_t a = (uint64_t)j << top->shift, b = (uint64_t)(j + 1) << top->shift;
    return gene_first_above(t.end, (uint32_t)a, (uint32_t)(b < t.n ? b : t.n), ks); // (top[j] > ks: it is in the chunk)
}

// one block [s, e) on reference ref, e > s, 0 <= s, e <= GENE_POS_LIMIT: a gene's index, GENE_HIT_NONE or GENE_HIT_SEVERAL
UMIHIP_HD inline int32_t gene_query(const GeneView &t, const GeneTop *top, uint32_t ref, uint64_t s, uint64_t e)
{
    const uint64_t ke = gene_key(ref, e);
    const uint32_t lo = gene_first_segment(t, top, gene_key(ref, s));
    if (lo >= t.n || t.start[lo] >= ke) return GENE_HIT_NONE;
    // hi, the last segment that starts before ke: start[a] < ke throughout, start[b] >= ke or b == n
    uint32_t a = lo, step = 1;
    while (a + step < t.n && t.start[a + step] < ke) {
        a += step;
        step <<= 1;
    }
    uint32_t b = a + step < t.n ? a + step : t.n;
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (t.start[m] < ke)
            a = m;
        else
            b = m;
    }
    const GeneSeg l = t.seg[lo];
    if (l.label == GENE_MULTI) return GENE_HIT_SEVERAL;
    if (a != lo && t.seg[a].run != l.run) return GENE_HIT_SEVERAL;
    return l.label;
}

// A read: its blocks from pos and its CIGAR (BAM's words, len << 4 | op), each looked up, the answers
// combined.  M = X D (0 7 8 2) extend the block, N (3) closes it and skips, I S H P (1 4 5 6) consume nothing.
// Coordinates are kept in 64 bits and a block is cut to [0, GENE_POS_LIMIT), where every exon lies.
// GENE_READ_* and *gene (-1 unless assigned); GENE_READ_BAD_OP at an op code above 8.
UMIHIP_HD inline int gene_assign_read(const GeneView &t, const GeneTop *top, uint32_t ref, int64_t pos, const uint32_t *cigar,
                                      uint64_t n_cigar, int32_t *gene)
{
    int32_t found = GENE_HIT_NONE;
    int64_t s = pos, e = pos;
    *gene = -1;
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
        const int64_t bs = s < 0 ? 0 : s, be = e > GENE_POS_LIMIT ? GENE_POS_LIMIT : e;
        if (be > bs && found != GENE_HIT_SEVERAL) {
            const int32_t h = gene_query(t, top, ref, (uint64_t)bs, (uint64_t)be);
            if (h == GENE_HIT_SEVERAL || (h >= 0 && found >= 0 && h != found))
                found = GENE_HIT_SEVERAL;
            else if (h >= 0)
                found = h;
        }
        s = e = e + len;
    }
    if (found == GENE_HIT_SEVERAL) return GENE_READ_SEVERAL;
    if (found == GENE_HIT_NONE) return GENE_READ_NONE;
    *gene = found;
    return GENE_READ_ASSIGNED;
}

// ---- the second tier: gene bodies (umi_assign_genes_introns, the program's --gene-introns) ----
// A gene's lines are grouped by (reference, strand as written); each group gives one body, [the group's smallest
// start, its largest end).  The bodies are lines like any other: gene_index_build makes their tables with the same
// `take` per strand class as the exons', and gene_query serves them unchanged.  Bodies nest, so GENE_MULTI segments
// are the rule here where genes overlap.  Every exon lies inside its group's body: the genes E that hit a read by an
// exon are among the genes B that hit it by a body.
constexpr int GENE_INTRONS_OFF = 0, GENE_INTRONS_EXON_FIRST = 1, GENE_INTRONS_ALL = 2; // UMI_INTRONS_*
constexpr int GENE_TIER_EXON = 0, GENE_TIER_INTRON = 1;                                // UMI_GENE_TIER_*

struct GeneBodies {
    std::vector<int32_t> ref, start, end, gene;
    std::vector<uint8_t> strand;
};

// The bodies of the checked exons (gene_index_build's), in the order their groups first appear.
inline void gene_bodies_derive(const int32_t *ref, const int32_t *start, const int32_t *end, const uint8_t *strand,
                               const int32_t *gene, uint64_t n_exons, GeneBodies &b)
{
    b = GeneBodies();
    // (gene and ref are below 2^31, the strand takes two bits: a group is one 64-bit key).  A file names a gene's
    // lines one after another, so most lines find their group in `last` and not in the map
    std::unordered_map<uint64_t, size_t> body_of;
    uint64_t last_key = ~(uint64_t)0;
    size_t last = 0;
    for (uint64_t i = 0; i < n_exons; i++) {
        const uint64_t sc = strand[i] == '+' ? 0 : strand[i] == '-' ? 1 : 2;
        const uint64_t key = (uint64_t)gene[i] << 33 | (uint64_t)ref[i] << 2 | sc;
        if (key != last_key) {
            const auto at = body_of.emplace(key, b.gene.size());
            if (at.second) {
                b.ref.push_back(ref[i]);
                b.start.push_back(start[i]);
                b.end.push_back(end[i]);
                b.strand.push_back(strand[i]);
                b.gene.push_back(gene[i]);
            }
            last_key = key;
            last = at.first->second;
        }
        b.start[last] = std::min(b.start[last], start[i]);
        b.end[last] = std::max(b.end[last], end[i]);
    }
}

// A read under --gene-introns: phase 1 is gene_assign_read against the exon table and gives E's verdict; a read
// whose verdict still depends on B walks its CIGAR again, against the body table.  exon-first: E one gene: that gene,
// tier exon; E several: several; E empty: B's verdict, tier intron.  all: E several: several (E is in B); else B's
// verdict, tier exon where E is not empty, else intron.  off: E's verdict.  *tier is GENE_TIER_EXON unless the read is
// assigned by an intron.  (A bad op code is found by phase 1, which looks at every word.)
UMIHIP_HD inline int gene_assign_read_tiers(const GeneView &exons, const GeneTop *exon_top, const GeneView &bodies,
                                            const GeneTop *body_top, int mode, uint32_t ref, int64_t pos, const uint32_t *cigar,
                                            uint64_t n_cigar, int32_t *gene, int *tier)
{
    *tier = GENE_TIER_EXON;
    int st = gene_assign_read(exons, exon_top, ref, pos, cigar, n_cigar, gene);
    if (st == GENE_READ_BAD_OP || st == GENE_READ_SEVERAL || mode == GENE_INTRONS_OFF) return st;
    const bool by_exon = st == GENE_READ_ASSIGNED;
    if (by_exon && mode == GENE_INTRONS_EXON_FIRST) return st;
    st = gene_assign_read(bodies, body_top, ref, pos, cigar, n_cigar, gene);
    if (st == GENE_READ_ASSIGNED && !by_exon) *tier = GENE_TIER_INTRON;
    return st;
}

// ---- covered bases and the class of a read (umi_assign_genes_classes, the program's --velocity) ----
// cover of [s, e): the positions of it that lie in a kept segment of a table.  Beside the table travels a prefix array,
// cum[i] = the summed lengths of segments 0 .. i-1 (n + 1 words): cover = cum[hi + 1] - cum[lo] less what the block
// leaves of segment lo in front of s and of segment hi behind e; lo and hi are gene_query's.  The table, its view and
// its top are as they were: the array is built and uploaded only by the call that wants classes.
//
// The blocks of a read assigned to gene g by an exon touch only segments that carry g's label (otherwise E would be
// several), so the table's cover of a block is g's.  The stretch an N skipped is another matter: a nested gene's exon
// may lie in g's intron, and the table's cover of a gap is then an upper bound of g's.  A gap the table covers whole
// is therefore looked up once more, in g's own exons: GeneOwn holds, per gene, the union of its lines of the table's
// strand class as disjoint, non-touching intervals in key order (own_off[g] .. own_off[g + 1]); the gap is g's where
// the interval that holds its first base reaches its end.
constexpr int GENE_CLASS_NONE = 0, GENE_CLASS_EXONIC = 1, GENE_CLASS_JUNCTION = 2, GENE_CLASS_SPANNING = 3,
              GENE_CLASS_INTRONIC = 4; // UMI_READ_CLASS_*

inline void gene_cover_prefix(const GeneTable &t, std::vector<uint64_t> &cum)
{
    const size_t n = t.end.size();
    cum.assign(n + 1, 0);
    for (size_t i = 0; i < n; i++) cum[i + 1] = cum[i] + (t.end[i] - t.start[i]); // (a segment lies on one reference)
}

// hi: the last segment that starts before key ke, from lo on (start[lo] < ke), found as gene_query finds it
UMIHIP_HD inline uint32_t gene_last_segment(const GeneView &t, uint32_t lo, uint64_t ke)
{
    uint32_t a = lo, step = 1;
    while (a + step < t.n && t.start[a + step] < ke) {
        a += step;
        step <<= 1;
    }
    uint32_t b = a + step < t.n ? a + step : t.n;
    while (b - a > 1) {
        const uint32_t m = a + (b - a) / 2;
        if (t.start[m] < ke)
            a = m;
        else
            b = m;
    }
    return a;
}

// the covered bases of [s, e) on reference ref, e > s, 0 <= s, e <= GENE_POS_LIMIT
UMIHIP_HD inline uint64_t gene_cover(const GeneView &t, const GeneTop *top, const uint64_t *cum, uint32_t ref, uint64_t s, uint64_t e)
{
    const uint64_t ks = gene_key(ref, s), ke = gene_key(ref, e);
    const uint32_t lo = gene_first_segment(t, top, ks);
    if (lo >= t.n || t.start[lo] >= ke) return 0;
    const uint32_t hi = gene_last_segment(t, lo, ke);
    uint64_t c = cum[hi + 1] - cum[lo]; // (segments lo .. hi end behind ks and start before ke: all on ref)
    const uint64_t first = t.start[lo], last = t.end[hi];
    if (first < ks) c -= ks - first;
    if (last > ke) c -= last - ke;
    return c;
}

struct GeneOwn {
    std::vector<uint64_t> start, end; // keys, as the table's
    std::vector<uint32_t> off;        // [n_genes + 1]
};

struct GeneOwnView {
    const uint64_t *start, *end;
    const uint32_t *off;
};

// The checked exons (gene_index_build's) whose strand is in `take`, united per gene.
inline void gene_own_build(const int32_t *ref, const int32_t *start, const int32_t *end, const uint8_t *strand, const int32_t *gene,
                           uint64_t n_exons, uint32_t n_genes, unsigned take, GeneOwn &o)
{
    struct Line {
        int32_t gene;
        uint64_t ks, ke;
    };
    std::vector<Line> lines;
    lines.reserve(n_exons);
    for (uint64_t i = 0; i < n_exons; i++) {
        const unsigned bit = strand[i] == '+' ? GENE_TAKE_PLUS : strand[i] == '-' ? GENE_TAKE_MINUS : GENE_TAKE_DOT;
        if (take & bit) lines.push_back({gene[i], gene_key((uint32_t)ref[i], (uint64_t)start[i]), gene_key((uint32_t)ref[i], (uint64_t)end[i])});
    }
    std::sort(lines.begin(), lines.end(), [](const Line &a, const Line &b) { return a.gene != b.gene ? a.gene < b.gene : a.ks < b.ks; });
    o.start.clear();
    o.end.clear();
    o.off.assign((size_t)n_genes + 1, 0);
    int32_t g = -1;
    for (const Line &l : lines) {
        // (an end never reaches the next reference's keys: lines that touch lie on one reference)
        if (l.gene == g && l.ks <= o.end.back()) {
            o.end.back() = std::max(o.end.back(), l.ke);
            continue;
        }
        g = l.gene;
        o.start.push_back(l.ks);
        o.end.push_back(l.ke);
        o.off[(size_t)g + 1]++;
    }
    for (size_t i = 0; i < n_genes; i++) o.off[i + 1] += o.off[i];
}

// what travels beside an exon table for the classes: its prefix array and its genes' own exons
struct GeneCover {
    std::vector<uint64_t> cum;
    GeneOwn own;
};

inline GeneOwnView gene_own_view(const GeneOwn &o) { return {o.start.data(), o.end.data(), o.off.data()}; }

// does every base of [s, e), e > s, lie in an exon of gene g
UMIHIP_HD inline bool gene_own_covers(const GeneOwnView &o, int32_t g, uint32_t ref, uint64_t s, uint64_t e)
{
    const uint32_t a = o.off[g], b = o.off[g + 1];
    const uint32_t i = gene_first_above(o.start, a, b, gene_key(ref, s)); // the first interval that starts behind s
    return i > a && o.end[i - 1] >= gene_key(ref, e);
}

// The class of a read that is assigned to gene g with tier exon (its CIGAR has passed gene_assign_read: no bad op
// code).  The blocks are gene_assign_read's, cut to [0, GENE_POS_LIMIT), the empty ones left out; a gap is the stretch
// between one block's end and the next one's start.  A block not covered whole: SPANNING.  Otherwise a gap not covered
// whole by g: JUNCTION.  Otherwise EXONIC.  The gaps are walked only where every block is covered and there are two.
UMIHIP_HD inline int gene_read_class(const GeneView &t, const GeneTop *top, const uint64_t *cum, const GeneOwnView &own, int32_t g,
                                     uint32_t ref, int64_t pos, const uint32_t *cigar, uint64_t n_cigar)
{
    for (int walk = 0; walk < 2; walk++) {
        int64_t s = pos, e = pos, prev_end = -1;
        uint32_t blocks = 0;
        for (uint64_t c = 0; c <= n_cigar; c++) {
            uint32_t op = 3, len = 0;
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
                blocks++;
                if (walk == 0) {
                    if (gene_cover(t, top, cum, ref, (uint64_t)bs, (uint64_t)be) < (uint64_t)(be - bs)) return GENE_CLASS_SPANNING;
                } else if (prev_end >= 0 && bs > prev_end) {
                    const uint64_t gs = (uint64_t)prev_end, ge = (uint64_t)bs;
                    if (gene_cover(t, top, cum, ref, gs, ge) < ge - gs || !gene_own_covers(own, g, ref, gs, ge)) return GENE_CLASS_JUNCTION;
                }
                prev_end = be;
            }
            s = e = e + len;
        }
        if (blocks < 2) break;
    }
    return GENE_CLASS_EXONIC;
}

} // namespace umihip
