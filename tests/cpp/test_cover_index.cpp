// The cover lookup of umi_assign_genes_classes on the CPU (csrc/umihip_gene_index.hpp: the prefix array of covered
// bases, gene_cover, the genes' own exons and gene_read_class -- the code the kernel runs) against a per-base brute
// force over random small annotations on two neighbouring references: every block that begins or ends on, one before
// or one behind a segment's start or end (so: blocks that end on an edge, span an uncovered gap, touch the first and
// the last segment), random longer blocks over the edges of the top's chunks, the whole of a reference from 0 to
// 2^31, and reads cut at 0 and at 2^31.  Everything without a top and under tops of several caps.
// Stand-alone: built with -fsanitize=address,undefined by tests/test_cover_index_cpu.py.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_gene_index.hpp"

using namespace umihip;

namespace {

int failures = 0;
int seen[5] = {0, 0, 0, 0, 0}; // the reads of the random annotations by class
#define EXPECT(cond, ...)                                        \
    do {                                                         \
        if (!(cond) && failures++ < 20) {                        \
            fprintf(stderr, "%s:%d: ", __FILE__, __LINE__);      \
            fprintf(stderr, __VA_ARGS__);                        \
            fprintf(stderr, "\n");                               \
        }                                                        \
    } while (0)

struct Lines {
    std::vector<int32_t> ref, start, end, gene;
    std::vector<uint8_t> strand;
    uint32_t n_genes = 0;
    void add(int32_t r, int32_t s, int32_t e, char st, int32_t g)
    {
        ref.push_back(r), start.push_back(s), end.push_back(e), strand.push_back((uint8_t)st), gene.push_back(g);
        if ((uint32_t)g + 1 > n_genes) n_genes = (uint32_t)g + 1;
    }
};

const uint32_t CAPS[] = {1, 3, 7, 4096};
constexpr int LEN = 700, REFS = 2;
const unsigned TAKE_PLUS = GENE_TAKE_PLUS | GENE_TAKE_DOT;

// covered[r][p]: the genes (a bit each, up to 32) with a taken line over base p of reference r
struct Brute {
    std::vector<uint32_t> over[REFS];
    Brute(const Lines &x, unsigned take)
    {
        for (auto &v : over) v.assign(LEN, 0);
        for (size_t i = 0; i < x.ref.size(); i++) {
            const unsigned bit = x.strand[i] == '+' ? GENE_TAKE_PLUS : x.strand[i] == '-' ? GENE_TAKE_MINUS : GENE_TAKE_DOT;
            if (!(take & bit)) continue;
            for (int32_t p = x.start[i]; p < x.end[i]; p++) over[x.ref[i]][(size_t)p] |= 1u << x.gene[i];
        }
    }
    uint64_t cover(int r, int64_t s, int64_t e, uint32_t genes = ~0u) const
    {
        uint64_t c = 0;
        for (int64_t p = s < 0 ? 0 : s; p < e && p < LEN; p++) c += (over[r][(size_t)p] & genes) != 0;
        return c;
    }
};

Lines random_lines(std::mt19937 &rng, int n_genes)
{
    Lines x;
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    for (int g = 0; g < n_genes; g++) {
        const int r = rnd(0, REFS - 1);
        const char st = "++-."[rnd(0, 3)];
        int at = rnd(0, LEN - 200);
        for (int k = rnd(1, 6); k > 0 && at < LEN - 10; k--) {
            const int len = rnd(1, 40), e = at + len < LEN ? at + len : LEN;
            x.add(r, at, e, st, g);
            const int longer = e + rnd(0, 20);
            if (rnd(0, 3) == 0 && at + len / 2 < e) x.add(r, at + len / 2, longer < LEN ? longer : LEN, st, g);
            at = e + rnd(0, 30); // (0: the next exon touches this one)
        }
    }
    // the first and the last base of both references
    x.add(0, 0, 3, '+', 0);
    x.add(1, LEN - 2, LEN, '+', 1);
    return x;
}

struct Tables {
    GeneTable plain;
    std::vector<GeneTable> sampled;
    GeneCover cover;
};

void build(const Lines &x, unsigned take, Tables &t)
{
    gene_index_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.ref.size(), x.n_genes, take, t.plain);
    for (uint32_t cap : CAPS) {
        GeneTable s = t.plain;
        gene_index_sample(s, cap);
        t.sampled.push_back(std::move(s));
    }
    gene_cover_prefix(t.plain, t.cover.cum);
    gene_own_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.ref.size(), x.n_genes, take,
                   t.cover.own);
}

// gene_cover of one block, without a top and under every cap, against the brute force
void check_block(const Tables &t, const Brute &b, int r, int64_t s, int64_t e)
{
    if (s < 0) s = 0;
    if (e > LEN + 5) e = LEN + 5;
    if (e <= s) return;
    const uint64_t want = b.cover(r, s, e);
    const uint64_t got = gene_cover(gene_view(t.plain), nullptr, t.cover.cum.data(), (uint32_t)r, (uint64_t)s, (uint64_t)e);
    EXPECT(got == want, "ref %d [%" PRId64 ", %" PRId64 "): cover %" PRIu64 ", brute force %" PRIu64, r, s, e, got, want);
    for (size_t k = 0; k < t.sampled.size(); k++) {
        const GeneTop top = gene_top(t.sampled[k]);
        const uint64_t g2 = gene_cover(gene_view(t.sampled[k]), &top, t.cover.cum.data(), (uint32_t)r, (uint64_t)s, (uint64_t)e);
        EXPECT(g2 == want, "ref %d [%" PRId64 ", %" PRId64 "): cover %" PRIu64 " under a cap of %u, brute force %" PRIu64, r, s, e, g2,
               CAPS[k], want);
    }
}

int brute_class(const Brute &b, int r, int32_t g, int64_t pos, const std::vector<uint32_t> &cigar)
{
    std::vector<std::pair<int64_t, int64_t>> blocks;
    int64_t s = pos, e = pos;
    for (size_t c = 0; c <= cigar.size(); c++) {
        const uint32_t op = c < cigar.size() ? cigar[c] & 15u : 3u, len = c < cigar.size() ? cigar[c] >> 4 : 0u;
        if (op == 0 || op == 2 || op == 7 || op == 8) {
            e += len;
            continue;
        }
        if (op != 3) continue;
        const int64_t bs = s < 0 ? 0 : s;
        if (e > bs) blocks.push_back({bs, e});
        s = e = e + len;
    }
    for (auto &bl : blocks)
        if (b.cover(r, bl.first, bl.second, 1u << g) < (uint64_t)(bl.second - bl.first)) return GENE_CLASS_SPANNING;
    for (size_t i = 0; i + 1 < blocks.size(); i++)
        if (b.cover(r, blocks[i].second, blocks[i + 1].first, 1u << g) < (uint64_t)(blocks[i + 1].first - blocks[i].second))
            return GENE_CLASS_JUNCTION;
    return GENE_CLASS_EXONIC;
}

void one_annotation(uint32_t seed)
{
    std::mt19937 rng(seed);
    auto rnd = [&](int lo, int hi) { return lo + (int)(rng() % (uint32_t)(hi - lo + 1)); };
    const Lines x = random_lines(rng, 4 + (int)(seed % 20));
    for (unsigned take : {TAKE_PLUS, GENE_TAKE_MINUS | GENE_TAKE_DOT, GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT}) {
        Tables t;
        build(x, take, t);
        const Brute b(x, take);
        const GeneView v = gene_view(t.plain);
        EXPECT(t.cover.cum.size() == (size_t)v.n + 1 && t.cover.cum[0] == 0, "the prefix array has n + 1 words");
        // every block on, before and behind the edges of two segments (neighbouring ones, and any two)
        for (uint32_t i = 0; i < v.n; i++) {
            const int r = (int)(v.start[i] >> 32);
            const int64_t si = (int64_t)(v.start[i] & 0xFFFFFFFFu), ei = (int64_t)(v.end[i] & 0xFFFFFFFFu);
            for (uint32_t j : {i, i + 1 < v.n ? i + 1 : i, (uint32_t)rnd(0, (int)v.n - 1)}) {
                if ((int)(v.start[j] >> 32) != r) continue;
                const int64_t sj = (int64_t)(v.start[j] & 0xFFFFFFFFu), ej = (int64_t)(v.end[j] & 0xFFFFFFFFu);
                for (int64_t s : {si - 1, si, si + 1, ei - 1, ei, ei + 1})
                    for (int64_t e : {sj - 1, sj, sj + 1, ej - 1, ej, ej + 1}) check_block(t, b, r, s, e);
            }
        }
        for (int k = 0; k < 400; k++) { // longer blocks, over the chunks' edges and the uncovered stretches
            const int s = rnd(0, LEN - 1);
            check_block(t, b, rnd(0, REFS - 1), s, s + rnd(1, LEN));
        }
        for (int r = 0; r < REFS + 1; r++) { // a whole reference, and one behind the last with lines
            const uint64_t got = gene_cover(v, nullptr, t.cover.cum.data(), (uint32_t)r, 0, (uint64_t)GENE_POS_LIMIT);
            EXPECT(got == (r < REFS ? b.cover(r, 0, LEN) : 0), "reference %d from 0 to 2^31: %" PRIu64, r, got);
        }
        // a gene's own exons: [s, e) wholly in gene g
        const GeneOwnView own = gene_own_view(t.cover.own);
        EXPECT(t.cover.own.off.size() == (size_t)x.n_genes + 1 && t.cover.own.off.back() == t.cover.own.start.size(), "own_off");
        for (int k = 0; k < 2000; k++) {
            const int r = rnd(0, REFS - 1), g = rnd(0, (int)x.n_genes - 1), s = rnd(0, LEN - 1), e = s + rnd(1, 60);
            const bool want = e <= LEN && b.cover(r, s, e, 1u << g) == (uint64_t)(e - s);
            EXPECT(gene_own_covers(own, g, (uint32_t)r, (uint64_t)s, (uint64_t)e) == want, "gene %d ref %d [%d, %d): own %d", g, r, s, e, !want);
        }
        // reads: the class of every read an exon assigns, against the per-base class
        for (int k = 0; k < 3000; k++) {
            const int r = rnd(0, REFS - 1);
            const int64_t pos = rnd(-10, LEN - 1);
            std::vector<uint32_t> cigar{(uint32_t)rnd(1, 30) << 4};
            for (int p = rnd(0, 2); p > 0; p--) {
                static const uint32_t ops[] = {3, 3, 3, 2, 1, 4, 6, 7, 8, 5};
                cigar.push_back((uint32_t)rnd(0, 60) << 4 | ops[rnd(0, 9)]);
                cigar.push_back((uint32_t)rnd(0, 25) << 4);
            }
            int32_t g;
            if (gene_assign_read(v, nullptr, (uint32_t)r, pos, cigar.data(), cigar.size(), &g) != GENE_READ_ASSIGNED) continue;
            const int want = brute_class(b, r, g, pos, cigar);
            const int got = gene_read_class(v, nullptr, t.cover.cum.data(), own, g, (uint32_t)r, pos, cigar.data(), cigar.size());
            EXPECT(got == want, "seed %u read %d at %" PRId64 ": class %d, brute force %d", seed, k, pos, got, want);
            for (size_t c = 0; c < t.sampled.size(); c++) {
                const GeneTop top = gene_top(t.sampled[c]);
                const int g2 = gene_read_class(gene_view(t.sampled[c]), &top, t.cover.cum.data(), own, g, (uint32_t)r, pos, cigar.data(),
                                               cigar.size());
                EXPECT(g2 == want, "seed %u read %d: class %d under a cap of %u, brute force %d", seed, k, g2, CAPS[c], want);
            }
            seen[want]++;
        }
    }
}

// the cuts at 0 and at 2^31, and a nested exon that fills an intron exactly
void hand_cases()
{
    const int32_t top = INT32_MAX;
    Lines x;
    x.add(0, 0, 10, '+', 0);
    x.add(0, top - 10, top, '+', 0);
    x.add(1, 100, 200, '+', 1);
    x.add(1, 300, 400, '+', 1);
    x.add(1, 200, 300, '+', 2);
    x.add(2, 100, 200, '+', 3); // (another gene's lines on the next reference, at the same coordinates)
    Tables t;
    build(x, TAKE_PLUS, t);
    const GeneView v = gene_view(t.plain);
    const GeneOwnView own = gene_own_view(t.cover.own);
    auto cls = [&](int32_t g, uint32_t r, int64_t pos, std::vector<uint32_t> cigar) {
        const int a = gene_read_class(v, nullptr, t.cover.cum.data(), own, g, r, pos, cigar.data(), cigar.size());
        for (size_t c = 0; c < t.sampled.size(); c++) {
            const GeneTop tp = gene_top(t.sampled[c]);
            EXPECT(gene_read_class(gene_view(t.sampled[c]), &tp, t.cover.cum.data(), own, g, r, pos, cigar.data(), cigar.size()) == a,
                   "a hand case differs under a cap of %u", CAPS[c]);
        }
        return a;
    };
    auto M = [](uint32_t n) { return n << 4; };
    auto N = [](uint32_t n) { return n << 4 | 3u; };
    EXPECT(gene_cover(v, nullptr, t.cover.cum.data(), 0, 0, (uint64_t)GENE_POS_LIMIT) == 20, "reference 0 holds 20 covered bases");
    EXPECT(gene_cover(v, nullptr, t.cover.cum.data(), 0, 5, (uint64_t)top - 5) == 10, "5 bases of either exon");
    EXPECT(gene_cover(v, nullptr, t.cover.cum.data(), 1, 150, 350) == 200 && gene_cover(v, nullptr, t.cover.cum.data(), 2, 150, 350) == 50,
           "neighbouring references");
    EXPECT(cls(0, 0, -5, {M(10)}) == GENE_CLASS_EXONIC, "what lies before 0 is cut off");
    EXPECT(cls(0, 0, -5, {M(20)}) == GENE_CLASS_SPANNING, "... and what lies behind the exon is not");
    EXPECT(cls(0, 0, top - 5, {M(5)}) == GENE_CLASS_EXONIC, "the last bases an exon can hold");
    EXPECT(cls(0, 0, top - 5, {M(6)}) == GENE_CLASS_SPANNING, "base 2^31 - 1 lies in no exon");
    EXPECT(cls(0, 0, top - 5, {M(3), N(100), M(5)}) == GENE_CLASS_EXONIC, "a block behind 2^31 is no block");
    EXPECT(cls(0, 0, -20, {M(5), N(15), M(5)}) == GENE_CLASS_EXONIC, "a block before 0 is no block");
    const uint32_t far = (1u << 28) - 1; // (the longest operation; the gap from 10 to 2^31 - 6 in eight of them)
    EXPECT(cls(0, 0, 5, {M(5), N(far), N(far), N(far), N(far), N(far), N(far), N(far), N(far - 8), M(5)}) == GENE_CLASS_JUNCTION,
           "from the first exon to the last");
    EXPECT(cls(0, 0, (int64_t)top - 3, {M(0xFFFFFFF), M(0xFFFFFFF)}) == GENE_CLASS_SPANNING, "far beyond 2^31");
    EXPECT(cls(1, 1, 180, {M(20), N(100), M(20)}) == GENE_CLASS_JUNCTION, "gene 2 fills gene 1's intron: the gap is not gene 1's");
    EXPECT(cls(1, 1, 110, {M(10), N(5), M(10)}) == GENE_CLASS_EXONIC, "a gap inside the exon");
    EXPECT(cls(1, 1, 150, {M(20), 2u << 4 | 2u, M(20)}) == GENE_CLASS_EXONIC, "a deletion is part of the block");
    EXPECT(cls(1, 1, 150, {M(20), N(0), M(20)}) == GENE_CLASS_EXONIC, "an N that skips nothing");
}

} // namespace

int main()
{
    hand_cases();
    for (uint32_t seed = 0; seed < 40; seed++) one_annotation(seed);
    EXPECT(seen[1] > 100 && seen[2] > 100 && seen[3] > 100, "classes seen: %d %d %d", seen[1], seen[2], seen[3]);
    if (failures) {
        fprintf(stderr, "%d failures\n", failures);
        return 1;
    }
    printf("cover index ok\n");
    return 0;
}
