// The transcript index of umi_assign_genes_transcripts on the CPU (csrc/umihip_transcript_index.hpp: the check, the
// build, the sampled top and the lookup of a read -- the code the kernel runs) against the verdicts of
// tests/transcript_model.py, read from the file that tests/test_transcript_index_cpu.py writes:
//   case <n_exons> <n_transcripts> <n_reads> <name without blanks>
//   n_exons lines   ref start end strand(+ - .) gene transcript
//   n_reads lines   ref pos reverse status[3] gene[3] n_words words...     (status, gene: forward, reverse, unstranded)
// A second argument `forward` asks for that mode alone (tools/transcripts_bench.py, which knows no other verdicts).  The
// walk back of the plain lookups under forward is counted and printed.
// Stand-alone: built with -fsanitize=address,undefined by that test; `make` builds it plain.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_transcript_index.hpp"

using namespace umihip;

namespace {

long checks = 0, verdicts[3] = {0, 0, 0}, spliced_fits = 0;
int failures = 0, n_modes = 3;
uint64_t walk_reads = 0, walk_steps = 0, walk_max = 0; // forward, no top: the distinct exons stepped over

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

struct Read {
    int32_t ref;
    int64_t pos;
    int reverse, status[3], gene[3];
    std::vector<uint32_t> cigar;
};

const unsigned TAKE_PLUS = GENE_TAKE_PLUS | GENE_TAKE_DOT, TAKE_MINUS = GENE_TAKE_MINUS | GENE_TAKE_DOT,
               TAKE_ALL = GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT;

struct Built {
    TranscriptTable t;
    std::vector<TranscriptTable> sampled; // the same table under several caps
};

void build(const Exons &x, unsigned take, Built &b)
{
    transcript_index_build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.transcript.data(), x.size(), take, b.t);
    const TranscriptTable &t = b.t;
    const size_t nd = t.start.size(), ni = t.x.size();
    EXPECT(t.end.size() == nd && t.dmax.size() == nd && t.label.size() == nd && t.off.size() == nd + 1, "array sizes");
    EXPECT(t.of.size() == ni && t.inst.size() == ni && t.off.back() == ni && t.off[0] == 0, "instance arrays");
    for (size_t i = 0; i < nd; i++) {
        EXPECT(t.start[i] < t.end[i] && t.off[i] < t.off[i + 1], "distinct exon %zu is empty", i);
        if (i) EXPECT(t.start[i - 1] < t.start[i] || (t.start[i - 1] == t.start[i] && t.end[i - 1] < t.end[i]), "distinct exons %zu: order", i);
        EXPECT(t.dmax[i] >= t.end[i] && (!i || t.dmax[i] >= t.dmax[i - 1]), "dmax at %zu", i);
        for (uint32_t k = t.off[i]; k < t.off[i + 1]; k++) {
            const uint32_t p = t.inst[k];
            EXPECT(p < ni && (uint32_t)t.start[i] == (uint32_t)t.x[p].start && (uint32_t)t.end[i] == (uint32_t)t.x[p].end, "instance %u of exon %zu", p, i);
            EXPECT(t.label[i] == GENE_MULTI || t.label[i] == t.of[p].gene, "label of exon %zu", i);
        }
    }
    for (size_t p = 0; p < ni; p++) {
        EXPECT(t.of[p].stop > p && t.of[p].stop <= ni, "stop of instance %zu", p);
        if (p + 1 < t.of[p].stop) EXPECT(t.x[p].end < t.x[p + 1].start && t.of[p + 1].stop == t.of[p].stop, "instances %zu, %zu touch", p, p + 1);
    }
    b.sampled.clear();
    for (uint32_t cap : {1u, 2u, 3u, 7u, 64u, 4096u}) {
        TranscriptTable s = t;
        transcript_index_sample(s, cap);
        EXPECT(s.top.size() <= cap, "top of %zu entries over a cap of %u", s.top.size(), cap);
        EXPECT(nd == 0 || s.top.size() == ((nd - 1) >> s.top_shift) + 1, "top size");
        b.sampled.push_back(std::move(s));
    }
}

void run_case(const std::string &name, const Exons &x, uint32_t n_transcripts, const std::vector<Read> &reads)
{
    uint64_t bad = 0;
    EXPECT(transcript_check(x.ref.data(), x.strand.data(), x.gene.data(), x.transcript.data(), x.size(), n_transcripts, &bad) == TR_OK,
           "%s: the exons do not pass the check", name.c_str());
    Built plus, minus, all;
    build(x, TAKE_PLUS, plus);
    build(x, TAKE_MINUS, minus);
    build(x, TAKE_ALL, all);
    for (size_t r = 0; r < reads.size(); r++) {
        const Read &rd = reads[r];
        for (int mode = 0; mode < n_modes; mode++) { // UMI_STRAND_FORWARD, _REVERSE, _UNSTRANDED
            const Built &b = mode == 2 ? all : ((rd.reverse != 0) != (mode == 1)) ? minus : plus;
            uint64_t steps0 = 0;
            for (size_t k = 0; k <= b.sampled.size(); k++) {
                const TranscriptTable &st = k ? b.sampled[k - 1] : b.t;
                const GeneTop top = transcript_top(st);
                int32_t g = 77;
                uint64_t steps = 0;
                const int got = transcript_assign_read(transcript_view(st), k ? &top : nullptr, (uint32_t)rd.ref, rd.pos, rd.cigar.data(),
                                                       rd.cigar.size(), &g, &steps);
                EXPECT(got == rd.status[mode] && g == rd.gene[mode], "%s: read %zu, mode %d, top %zu: %d gene %d, the model %d gene %d",
                       name.c_str(), r, mode, k, got, g, rd.status[mode], rd.gene[mode]);
                if (k == 0) steps0 = steps;
                if (k == 0 && mode == 0) walk_reads++, walk_steps += steps, walk_max = steps > walk_max ? steps : walk_max;
                EXPECT(steps == steps0, "%s: read %zu: the walk back differs with a top", name.c_str(), r);
            }
            verdicts[rd.status[mode]]++;
            if (rd.status[mode] == GENE_READ_ASSIGNED) {
                int n_skips = 0;
                for (uint32_t w : rd.cigar) n_skips += (w & 15u) == 3 && (w >> 4) > 0;
                spliced_fits += n_skips > 0;
            }
        }
    }
}

void fixed_cases()
{
    // the check: an entry out of range, a transcript on two references, strands, genes; the first exon at fault is named
    Exons x;
    x.add(0, 100, 200, '+', 0, 0), x.add(0, 300, 400, '+', 0, 0), x.add(1, 100, 200, '-', 1, 2), x.add(0, 500, 600, '+', 0, 0);
    uint64_t bad = 99;
    auto check = [&](uint32_t n_tr) { return transcript_check(x.ref.data(), x.strand.data(), x.gene.data(), x.transcript.data(), x.size(), n_tr, &bad); };
    EXPECT(check(3) == TR_OK && check(1000000000u) == TR_OK, "good exons");
    EXPECT(check(2) == TR_BAD_RANGE && bad == 2, "transcript 2 of 2");
    x.transcript[1] = -1;
    EXPECT(check(3) == TR_BAD_RANGE && bad == 1, "transcript -1");
    x.transcript[1] = 0, x.ref[3] = 1;
    EXPECT(check(3) == TR_BAD_REF && bad == 3, "two references");
    x.ref[3] = 0, x.strand[3] = '.';
    EXPECT(check(3) == TR_BAD_STRAND && bad == 3, "two strands");
    x.strand[3] = '+', x.gene[1] = 1;
    EXPECT(check(3) == TR_BAD_GENE && bad == 1, "two genes");
    x.gene[1] = 0;
    // an empty annotation, and a bad op code
    Exons none;
    Built b;
    build(none, TAKE_ALL, b);
    EXPECT(b.t.start.empty() && b.sampled[0].top.empty(), "an empty annotation has an empty table");
    int32_t g;
    const uint32_t words[3] = {(2u << 4) | 0, (2u << 4) | 9, (2u << 4) | 3};
    for (const TranscriptTable &st : b.sampled) {
        const GeneTop top = transcript_top(st);
        EXPECT(transcript_assign_read(transcript_view(st), &top, 0, 5, words, 1, &g, nullptr) == GENE_READ_NONE && g == -1, "no exon: none");
        EXPECT(transcript_assign_read(transcript_view(st), &top, 0, 5, words, 3, &g, nullptr) == GENE_READ_BAD_OP, "op code 9 is refused");
    }
    Built one;
    build(x, TAKE_ALL, one);
    EXPECT(transcript_assign_read(transcript_view(one.t), nullptr, 0, 150, words, 2, &g, nullptr) == GENE_READ_BAD_OP, "op code 9 is refused");
    EXPECT(transcript_assign_read(transcript_view(one.t), nullptr, 0, 150, words, 1, &g, nullptr) == GENE_READ_ASSIGNED && g == 0, "a read of 2M");
    const uint32_t bad_last[3] = {(10u << 4) | 0, (100u << 4) | 3, (10u << 4) | 15};
    EXPECT(transcript_assign_read(transcript_view(one.t), nullptr, 0, 190, bad_last, 3, &g, nullptr) == GENE_READ_BAD_OP, "op code 15 in the last word");
}

} // namespace

int main(int argc, char **argv)
{
    fixed_cases();
    if (argc > 2 && std::string(argv[2]) == "forward") n_modes = 1;
    if (argc > 1) {
        FILE *f = fopen(argv[1], "r");
        if (!f) {
            fprintf(stderr, "cannot open %s\n", argv[1]);
            return 2;
        }
        unsigned long long n_exons, n_tr, n_reads;
        char name[256];
        int cases = 0;
        while (fscanf(f, " case %llu %llu %llu %255s", &n_exons, &n_tr, &n_reads, name) == 4) {
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
                if (fscanf(f, "%d %" SCNd64 " %d %d %d %d %d %d %d %llu", &rd.ref, &rd.pos, &rd.reverse, &rd.status[0], &rd.status[1], &rd.status[2],
                           &rd.gene[0], &rd.gene[1], &rd.gene[2], &words) != 10)
                    return 2;
                rd.cigar.resize((size_t)words);
                for (uint32_t &w : rd.cigar)
                    if (fscanf(f, "%" SCNu32, &w) != 1) return 2;
            }
            run_case(name, x, (uint32_t)n_tr, reads);
            cases++;
        }
        fclose(f);
        printf("transcript index: %d cases from %s\n", cases, argv[1]);
        printf("walk back: reads %llu, mean %.3f, max %llu\n", (unsigned long long)walk_reads,
               walk_reads ? (double)walk_steps / (double)walk_reads : 0.0, (unsigned long long)walk_max);
        if (!verdicts[0] || !verdicts[1] || !verdicts[2] || !spliced_fits) {
            fprintf(stderr, "a verdict never occurred\n");
            return 1;
        }
    }
    printf("transcript index: %ld checks, reads assigned %ld (spliced %ld), none %ld, several %ld\n", checks, verdicts[0], spliced_fits,
           verdicts[1], verdicts[2]);
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("transcript index ok\n");
    return 0;
}
