// The lookup of umi_assign_genes_transcripts_classes on the CPU (csrc/umihip_transcript_index.hpp:
// transcript_assign_read_tiers and its phases -- the code the kernels run -- over the three indices as the call builds
// them) against the verdicts of tests/transcript_intron_model.py, read from the file that
// tests/test_transcript_tiers_cpu.py writes:
//   case <n_exons> <n_genes> <n_transcripts> <n_reads> <name without blanks>
//   n_exons lines   ref start end strand(+ - .) gene transcript
//   n_reads lines   ref pos reverse  9 x (status gene tier class)  n_words words...
//                   (the nine: forward, reverse, unstranded, each under off, exon-first, all)
// Stand-alone: built with -fsanitize=address,undefined by that test.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_transcript_index.hpp"

using namespace umihip;

namespace {

long checks = 0, seen_class[5] = {0, 0, 0, 0, 0}, seen_tier[2] = {0, 0}, body_class[5] = {0, 0, 0, 0, 0};
int failures = 0;

#define EXPECT(cond, ...)                                       \
    do {                                                        \
        checks++;                                               \
        if (!(cond)) {                                          \
            if (failures++ < 20) {                              \
                fprintf(stderr, "%s:%d: ", __FILE__, __LINE__); \
                fprintf(stderr, __VA_ARGS__);                   \
                fprintf(stderr, "\n");                          \
            }                                                   \
        }                                                       \
    } while (0)

struct Exons {
    std::vector<int32_t> ref, start, end, gene, transcript;
    std::vector<uint8_t> strand;
    void add(int32_t r, int32_t s, int32_t e, char st, int32_t g, int32_t t)
    {
        ref.push_back(r), start.push_back(s), end.push_back(e), strand.push_back((uint8_t)st), gene.push_back(g), transcript.push_back(t);
    }
    size_t size() const { return ref.size(); }
};

struct Verdict {
    int status, gene, tier, cls;
};

struct Read {
    int32_t ref;
    int64_t pos;
    int reverse;
    Verdict want[9];
    std::vector<uint32_t> cigar;
};

const unsigned TAKE_PLUS = GENE_TAKE_PLUS | GENE_TAKE_DOT, TAKE_MINUS = GENE_TAKE_MINUS | GENE_TAKE_DOT,
               TAKE_ALL = GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT;

// the three indices of one strand class, as umi_assign_genes_transcripts_classes builds them, the tops under several caps
struct Built {
    std::vector<TranscriptTable> tr; // [0]: cap 4096, then smaller caps
    std::vector<GeneTable> body;     // [0]: cap 512, then smaller caps
    GeneTable exons;
    GeneCover cover;
};

const uint32_t TR_CAPS[3] = {4096, 7, 1}, BODY_CAPS[3] = {512, 3, 1};

void build(const Exons &x, uint32_t n_genes, unsigned take, Built &b)
{
    TranscriptTable t;
    transcript_index_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.transcript.data(), x.size(), take, t);
    GeneBodies bodies;
    gene_bodies_derive(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.size(), bodies);
    GeneTable bt;
    gene_index_build(bodies.ref.data(), bodies.start.data(), bodies.end.data(), bodies.strand.data(), bodies.gene.data(), bodies.gene.size(),
                     n_genes, take, bt);
    for (int k = 0; k < 3; k++) {
        b.tr.push_back(t);
        transcript_index_sample(b.tr.back(), TR_CAPS[k]);
        b.body.push_back(bt);
        gene_index_sample(b.body.back(), BODY_CAPS[k]);
    }
    gene_index_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.size(), n_genes, take, b.exons);
    gene_cover_prefix(b.exons, b.cover.cum);
    gene_own_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.size(), n_genes, take, b.cover.own);
}

void run_case(const std::string &name, const Exons &x, uint32_t n_genes, uint32_t n_transcripts, const std::vector<Read> &reads)
{
    uint64_t bad = 0;
    EXPECT(transcript_check(x.ref.data(), x.strand.data(), x.gene.data(), x.transcript.data(), x.size(), n_transcripts, &bad) == TR_OK,
           "%s: the exons do not pass the check", name.c_str());
    Built plus, minus, all;
    build(x, n_genes, TAKE_PLUS, plus);
    build(x, n_genes, TAKE_MINUS, minus);
    build(x, n_genes, TAKE_ALL, all);
    for (size_t r = 0; r < reads.size(); r++) {
        const Read &rd = reads[r];
        for (int mode = 0; mode < 3; mode++) { // UMI_STRAND_FORWARD, _REVERSE, _UNSTRANDED
            const Built &b = mode == 2 ? all : ((rd.reverse != 0) != (mode == 1)) ? minus : plus;
            const TrCoverView cover = {gene_view(b.exons), b.cover.cum.data(), gene_own_view(b.cover.own)};
            for (int introns = 0; introns < 3; introns++) { // GENE_INTRONS_OFF, _EXON_FIRST, _ALL
                const Verdict &w = rd.want[mode * 3 + introns];
                for (int k = 0; k <= 3; k++) { // without tops, then with them under three caps
                    const TranscriptTable &tt = b.tr[k ? k - 1 : 0];
                    const GeneTable &bt = b.body[k ? k - 1 : 0];
                    const GeneTop top = transcript_top(tt), btop = gene_top(bt);
                    int32_t g = 77;
                    int tier = 77, cls = 77;
                    int got = transcript_assign_read_tiers(transcript_view(tt), k ? &top : nullptr, gene_view(bt), k ? &btop : nullptr, &cover,
                                                           introns, (uint32_t)rd.ref, rd.pos, rd.cigar.data(), rd.cigar.size(), &g, &tier, &cls);
                    EXPECT(got == w.status && g == w.gene && tier == w.tier && cls == w.cls,
                           "%s: read %zu, mode %d, introns %d, tops %d: %d gene %d tier %d class %d, the model %d gene %d tier %d class %d",
                           name.c_str(), r, mode, introns, k, got, g, tier, cls, w.status, w.gene, w.tier, w.cls);
                    // without classes: the same gene, status and tier, and the class is not written
                    g = 77, tier = 77, cls = 77;
                    got = transcript_assign_read_tiers(transcript_view(tt), k ? &top : nullptr, gene_view(bt), k ? &btop : nullptr, nullptr,
                                                       introns, (uint32_t)rd.ref, rd.pos, rd.cigar.data(), rd.cigar.size(), &g, &tier, &cls);
                    EXPECT(got == w.status && g == w.gene && tier == w.tier && cls == 77, "%s: read %zu, mode %d, introns %d, tops %d, no classes",
                           name.c_str(), r, mode, introns, k);
                }
                // the phases one by one, as the two kernels run them
                const GeneTop top = transcript_top(b.tr[0]), btop = gene_top(b.body[0]);
                int32_t g = 77;
                uint64_t m = 99;
                int st = transcript_assign_read(transcript_view(b.tr[0]), &top, (uint32_t)rd.ref, rd.pos, rd.cigar.data(), rd.cigar.size(), &g,
                                                nullptr, &m);
                int tier = GENE_TIER_EXON, cls = st == GENE_READ_ASSIGNED ? transcript_fit_class(m >= 2) : GENE_CLASS_NONE;
                if (transcript_needs_bodies(introns, st))
                    st = transcript_assign_read_bodies(gene_view(b.body[0]), &btop, &cover, st == GENE_READ_ASSIGNED, m >= 2, (uint32_t)rd.ref,
                                                       rd.pos, rd.cigar.data(), rd.cigar.size(), &g, &tier, &cls);
                EXPECT(st == w.status && g == w.gene && tier == w.tier && cls == w.cls, "%s: read %zu, mode %d, introns %d: the phases apart",
                       name.c_str(), r, mode, introns);
                seen_class[w.cls]++;
                if (w.status == GENE_READ_ASSIGNED) seen_tier[w.tier]++;
                if (w.status == GENE_READ_ASSIGNED && w.tier == GENE_TIER_INTRON) body_class[w.cls]++;
            }
        }
    }
}

void fixed_cases()
{
    // an empty annotation: every read is none, whatever the mode; a bad op code is found by phase 1
    Exons none;
    Built b;
    build(none, 0, TAKE_ALL, b);
    const TrCoverView cover = {gene_view(b.exons), b.cover.cum.data(), gene_own_view(b.cover.own)};
    const uint32_t words[3] = {(2u << 4) | 0, (2u << 4) | 9, (2u << 4) | 3};
    for (int introns = 0; introns < 3; introns++)
        for (int k = 0; k < 3; k++) {
            const GeneTop top = transcript_top(b.tr[k]), btop = gene_top(b.body[k]);
            int32_t g = 77;
            int tier = 77, cls = 77;
            EXPECT(transcript_assign_read_tiers(transcript_view(b.tr[k]), &top, gene_view(b.body[k]), &btop, &cover, introns, 0, 5, words, 1, &g,
                                                &tier, &cls) == GENE_READ_NONE &&
                       g == -1 && tier == 0 && cls == GENE_CLASS_NONE,
                   "no exon: none");
            EXPECT(transcript_assign_read_tiers(transcript_view(b.tr[k]), &top, gene_view(b.body[k]), &btop, &cover, introns, 0, 5, words, 3, &g,
                                                &tier, &cls) == GENE_READ_BAD_OP,
                   "op code 9 is refused");
        }
    uint64_t m = 99;
    int32_t g;
    EXPECT(transcript_assign_read(transcript_view(b.tr[0]), nullptr, 0, 5, words, 3, &g, nullptr, &m) == GENE_READ_BAD_OP && m == 0,
           "a bad op code leaves m at 0");
    const uint32_t three[5] = {(2u << 4) | 0, (0u << 4) | 3, (2u << 4) | 7, (5u << 4) | 3, (1u << 4) | 8};
    EXPECT(transcript_assign_read(transcript_view(b.tr[0]), nullptr, 0, 5, three, 5, &g, nullptr, &m) == GENE_READ_NONE && m == 3, "three blocks");
}

} // namespace

int main(int argc, char **argv)
{
    fixed_cases();
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        unsigned long long n_exons, n_genes, n_tr, n_reads;
        char name[256];
        int cases = 0;
        while (fscanf(f, " case %llu %llu %llu %llu %255s", &n_exons, &n_genes, &n_tr, &n_reads, name) == 5) {
            Exons x;
            for (unsigned long long i = 0; i < n_exons; i++) {
                int r, s, e, g, t;
                char st;
                if (fscanf(f, "%d %d %d %c %d %d", &r, &s, &e, &st, &g, &t) != 6) return 2;
                x.add(r, s, e, st, g, t);
            }
            std::vector<Read> reads((size_t)n_reads);
            for (Read &rd : reads) {
                unsigned long long words;
                if (fscanf(f, "%d %" SCNd64 " %d", &rd.ref, &rd.pos, &rd.reverse) != 3) return 2;
                for (Verdict &v : rd.want)
                    if (fscanf(f, "%d %d %d %d", &v.status, &v.gene, &v.tier, &v.cls) != 4 || v.status < 0 || v.status > 2 || v.tier < 0 ||
                        v.tier > 1 || v.cls < 0 || v.cls > 4)
                        return 2;
                if (fscanf(f, "%llu", &words) != 1) return 2;
                rd.cigar.resize((size_t)words);
                for (uint32_t &w : rd.cigar)
                    if (fscanf(f, "%" SCNu32, &w) != 1) return 2;
            }
            run_case(name, x, (uint32_t)n_genes, (uint32_t)n_tr, reads);
            cases++;
        }
        fclose(f);
        printf("transcript tiers: %d cases from %s\n", cases, argv[1]);
        for (int c = 0; c < 5; c++)
            if (!seen_class[c] || (c && !body_class[c])) {
                fprintf(stderr, "class %d never occurred (in all: %ld, by a body: %ld)\n", c, seen_class[c], body_class[c]);
                return 1;
            }
        if (!seen_tier[0] || !seen_tier[1]) {
            fprintf(stderr, "a tier never occurred\n");
            return 1;
        }
    }
    printf("transcript tiers: %ld checks; by a transcript %ld, by a body %ld (exonic %ld, junction %ld, spanning %ld, intronic %ld)\n", checks,
           seen_tier[0], seen_tier[1], body_class[1], body_class[2], body_class[3], body_class[4]);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("transcript tiers ok\n");
    return 0;
}
