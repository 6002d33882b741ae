// The annotation index of umi_assign_genes on the CPU (csrc/umihip_gene_index.hpp: the build, the sampled top,
// the block query and the walk of a read -- the code the kernel runs) against brute force over the exons.
// Stand-alone: built with -fsanitize=address,undefined by tests/test_gene_index_cpu.py.
#include <cstdio>
#include <cstdlib>
#include <random>
#include <set>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_gene_index.hpp"

using namespace umihip;

namespace {

struct Exons {
    std::vector<int32_t> ref, start, end, gene;
    std::vector<uint8_t> strand;
    uint32_t n_genes = 0;
    void add(int32_t r, int32_t s, int32_t e, char st, int32_t g)
    {
        ref.push_back(r), start.push_back(s), end.push_back(e), strand.push_back((uint8_t)st), gene.push_back(g);
        if ((uint32_t)g + 1 > n_genes) n_genes = (uint32_t)g + 1;
    }
    size_t size() const { return ref.size(); }
};

unsigned bit_of(uint8_t st) { return st == '+' ? GENE_TAKE_PLUS : st == '-' ? GENE_TAKE_MINUS : GENE_TAKE_DOT; }

// the rule, exon by exon: the genes with an exon of a taken strand on ref that shares a base with [s, e)
int32_t brute_block(const Exons &x, unsigned take, int32_t ref, int64_t s, int64_t e, std::set<int32_t> *into = nullptr)
{
    std::set<int32_t> hit;
    for (size_t i = 0; i < x.size(); i++)
        if ((take & bit_of(x.strand[i])) && x.ref[i] == ref && x.start[i] < e && s < x.end[i]) hit.insert(x.gene[i]);
    if (into) into->insert(hit.begin(), hit.end());
    return hit.empty() ? GENE_HIT_NONE : hit.size() > 1 ? GENE_HIT_SEVERAL : *hit.begin();
}

int brute_read(const Exons &x, unsigned take, int32_t ref, int64_t pos, const std::vector<uint32_t> &cigar, int32_t *gene)
{
    std::set<int32_t> hit;
    int64_t s = pos, e = pos;
    *gene = -1;
    for (uint32_t w : cigar) {
        const uint32_t op = w & 15, len = w >> 4;
        if (op > 8) return GENE_READ_BAD_OP;
        if (op == 0 || op == 2 || op == 7 || op == 8) e += len;
        if (op == 3) {
            if (e > s) brute_block(x, take, ref, s, e, &hit);
            s = e = e + len;
        }
    }
    if (e > s) brute_block(x, take, ref, s, e, &hit);
    if (hit.empty()) return GENE_READ_NONE;
    if (hit.size() > 1) return GENE_READ_SEVERAL;
    *gene = *hit.begin();
    return GENE_READ_ASSIGNED;
}

long checks = 0, verdicts[3] = {0, 0, 0};
int failures = 0;

#define EXPECT(cond, ...)                              \
    do {                                               \
        checks++;                                      \
        if (!(cond)) {                                 \
            if (failures++ < 20) {                     \
                fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);          \
                fprintf(stderr, "\n");                 \
            }                                          \
        }                                              \
    } while (0)

struct Built {
    GeneTable t;
    std::vector<GeneTable> sampled; // the same table under several caps
};

void build(const Exons &x, unsigned take, Built &b)
{
    gene_index_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.size(), x.n_genes, take, b.t);
    const size_t n = b.t.end.size();
    EXPECT(b.t.start.size() == n && b.t.seg.size() == n, "array sizes");
    for (size_t i = 0; i < n; i++) {
        EXPECT(b.t.start[i] < b.t.end[i], "segment %zu is empty", i);
        if (i) EXPECT(b.t.end[i - 1] <= b.t.start[i], "segments %zu and %zu overlap", i - 1, i);
        if (i) EXPECT(b.t.seg[i].run == b.t.seg[i - 1].run || b.t.seg[i].run == b.t.seg[i - 1].run + 1, "run numbers skip at %zu", i);
    }
    b.sampled.clear();
    for (uint32_t cap : {1u, 2u, 3u, 7u, 64u, 4096u}) {
        GeneTable s = b.t;
        gene_index_sample(s, cap);
        EXPECT(s.top.size() <= cap, "top of %zu entries over a cap of %u", s.top.size(), cap);
        EXPECT(n == 0 || s.top.size() == ((n - 1) >> s.top_shift) + 1, "top size");
        EXPECT(s.top_shift == 0 || ((n - 1) >> (s.top_shift - 1)) + 1 > cap, "a smaller shift would do");
        b.sampled.push_back(std::move(s));
    }
}

void check_block(const Exons &x, unsigned take, const Built &b, int32_t ref, int64_t s, int64_t e)
{
    const int32_t want = brute_block(x, take, ref, s, e);
    const GeneView v = gene_view(b.t);
    const int32_t got = gene_query(v, nullptr, (uint32_t)ref, (uint64_t)s, (uint64_t)e);
    EXPECT(got == want, "block ref %d [%lld, %lld): %d, brute force %d", ref, (long long)s, (long long)e, got, want);
    for (const GeneTable &st : b.sampled) {
        const GeneTop top = gene_top(st);
        const int32_t g2 = gene_query(gene_view(st), &top, (uint32_t)ref, (uint64_t)s, (uint64_t)e);
        EXPECT(g2 == want, "block ref %d [%lld, %lld) with a top of shift %d: %d, brute force %d", ref, (long long)s, (long long)e,
               st.top_shift, g2, want);
    }
    verdicts[want >= 0 ? 0 : want == GENE_HIT_NONE ? 1 : 2]++;
}

void check_read(const Exons &x, unsigned take, const Built &b, int32_t ref, int64_t pos, const std::vector<uint32_t> &cigar)
{
    int32_t wg, gg;
    const int want = brute_read(x, take, ref, pos, cigar, &wg);
    for (size_t k = 0; k <= b.sampled.size(); k++) {
        const GeneTable &st = k ? b.sampled[k - 1] : b.t;
        const GeneTop top = gene_top(st);
        const int got = gene_assign_read(gene_view(st), k ? &top : nullptr, (uint32_t)ref, pos, cigar.data(), cigar.size(), &gg);
        EXPECT(got == want && gg == wg, "read ref %d pos %lld, %zu words: %d gene %d, brute force %d gene %d", ref, (long long)pos,
               cigar.size(), got, gg, want, wg);
    }
}

const unsigned TAKES[3] = {GENE_TAKE_PLUS | GENE_TAKE_DOT, GENE_TAKE_MINUS | GENE_TAKE_DOT, GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT};

// every block with both ends in [lo, hi) on the references given
void sweep(const Exons &x, int64_t lo, int64_t hi, std::initializer_list<int32_t> refs)
{
    for (unsigned take : TAKES) {
        Built b;
        build(x, take, b);
        for (int32_t r : refs)
            for (int64_t s = lo; s < hi; s++)
                for (int64_t e = s + 1; e <= hi; e++) check_block(x, take, b, r, s, e);
    }
}

void fixed_cases()
{
    Exons none;
    sweep(none, 0, 6, {0, 3});
    {
        Built b;
        build(none, TAKES[2], b);
        EXPECT(b.t.end.empty() && b.sampled[0].top.empty(), "an empty annotation has an empty table");
        check_read(none, TAKES[2], b, 0, 5, {50u << 4});
    }
    Exons one;
    one.add(1, 3, 6, '+', 0);
    sweep(one, 0, 9, {0, 1, 2, 7}); // (references 0, 2 and 7: the annotation lacks them)
    Exons same; // all exons of one gene: overlapping, nested, abutting, apart
    for (auto se : {std::pair<int, int>{2, 6}, {4, 9}, {5, 6}, {9, 12}, {15, 18}}) same.add(0, se.first, se.second, '+', 0);
    sweep(same, 0, 20, {0});
    Exons mix; // nested and abutting exons of several genes on both strands, a gene inside another's intron
    mix.add(0, 2, 10, '+', 0), mix.add(0, 4, 6, '+', 1), mix.add(0, 10, 14, '+', 2), mix.add(0, 14, 16, '+', 0);
    mix.add(0, 20, 24, '-', 3), mix.add(0, 22, 26, '.', 4), mix.add(0, 30, 32, '+', 0), mix.add(0, 34, 36, '+', 5),
        mix.add(0, 38, 40, '+', 0);
    mix.add(2, 0, 3, '-', 1), mix.add(2, 3, 5, '-', 1), mix.add(2, 3, 5, '-', 1);
    sweep(mix, 0, 42, {0, 1, 2, 3});
    // coordinates at 0 and at 2^31 - 2, and a reference id near the top of its range
    Exons edge;
    const int32_t top = 0x7FFFFFFF;
    edge.add(0, 0, 1, '+', 0), edge.add(0, top - 2, top, '+', 1), edge.add(0, top - 1, top, '-', 2), edge.add(top, top - 3, top, '.', 3);
    for (unsigned take : TAKES) {
        Built b;
        build(edge, take, b);
        for (int32_t r : {0, 1, top - 1, top}) {
            for (int64_t s : {(int64_t)0, (int64_t)1, (int64_t)top - 4, (int64_t)top - 3, (int64_t)top - 2, (int64_t)top - 1})
                for (int64_t e : {(int64_t)1, (int64_t)2, (int64_t)top - 2, (int64_t)top - 1, (int64_t)top, (int64_t)top + 1})
                    if (e > s) check_block(edge, take, b, r, s, e);
            // reads that start before 0 or run beyond 2^31: their blocks are cut to the line
            check_read(edge, take, b, r, -3, {4u << 4});
            check_read(edge, take, b, r, -3, {3u << 4});
            check_read(edge, take, b, r, top - 2, {9u << 4});
            check_read(edge, take, b, r, top - 5, {(1u << 4) | 0, (0x0FFFFFFFu << 4) | 3, 5u << 4});
            check_read(edge, take, b, r, 0, {(1u << 4) | 0, (0x0FFFFFFFu << 4) | 2, (0x0FFFFFFFu << 4) | 2, (0x0FFFFFFFu << 4) | 2});
        }
    }
    // the walk: every op code, a bad one, no block at all
    Built b;
    build(mix, TAKES[2], b);
    check_read(mix, TAKES[2], b, 0, 3, {});
    check_read(mix, TAKES[2], b, 0, 3, {(5u << 4) | 4, (3u << 4) | 1, (2u << 4) | 5, (1u << 4) | 6});
    check_read(mix, TAKES[2], b, 0, 3, {(0u << 4) | 0, (7u << 4) | 3, (0u << 4) | 0});
    for (uint32_t op = 0; op < 16; op++) {
        check_read(mix, TAKES[2], b, 0, 3, {(2u << 4) | op});
        check_read(mix, TAKES[2], b, 0, 28, {(3u << 4) | 0, (2u << 4) | 3, (2u << 4) | op, (4u << 4) | 3, (2u << 4) | 7});
    }
    int32_t g;
    const uint32_t bad[2] = {(2u << 4) | 0, (2u << 4) | 9};
    EXPECT(gene_assign_read(gene_view(b.t), nullptr, 0, 3, bad, 2, &g) == GENE_READ_BAD_OP, "op code 9 is refused");
}

void random_cases(uint32_t seed, int rounds)
{
    std::mt19937 rng(seed);
    auto upto = [&](int n) { return (int)(rng() % (uint32_t)n); };
    for (int round = 0; round < rounds; round++) {
        Exons x;
        const int n_genes = 1 + upto(12), n_exons = upto(60), span = 40 + upto(260), n_refs = 1 + upto(3);
        for (int i = 0; i < n_exons; i++) {
            const int s = upto(span), len = 1 + upto(1 + upto(30));
            x.add(upto(n_refs), s, s + len, "+-."[upto(8) < 1 ? 2 : upto(2)], upto(n_genes));
        }
        x.n_genes = (uint32_t)n_genes;
        for (unsigned take : TAKES) {
            Built b;
            build(x, take, b);
            for (int q = 0; q < 150; q++) {
                const int s = upto(span + 40), len = 1 + upto(1 + upto(40));
                check_block(x, take, b, upto(n_refs + 1), s, s + len);
            }
            for (int q = 0; q < 60; q++) {
                std::vector<uint32_t> cigar;
                const int words = upto(8);
                for (int w = 0; w < words; w++) cigar.push_back((uint32_t)upto(1 + upto(25)) << 4 | (uint32_t)upto(9));
                check_read(x, take, b, upto(n_refs + 1), upto(span + 40) - 10, cigar);
            }
        }
    }
}

} // namespace

int main()
{
    fixed_cases();
    random_cases(20251, 200);
    printf("gene index: %ld checks, blocks one gene %ld, none %ld, several %ld\n", checks, verdicts[0], verdicts[1], verdicts[2]);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    if (!verdicts[0] || !verdicts[1] || !verdicts[2]) {
        fprintf(stderr, "a verdict never occurred\n");
        return 1;
    }
    printf("gene index ok\n");
    return 0;
}
