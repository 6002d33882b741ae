// The two tiers of umi_assign_genes_introns on the CPU (csrc/umihip_gene_index.hpp: the derivation of the gene
// bodies, both tiers' tables and the two-phase verdict of a read -- the code the kernel runs).  Reads a file of
// lines "E ref start end strand gene" and "R ref pos reverse n_words word..." and prints the derived bodies
// ("B ref start end strand gene") and, for every strand mode and intron mode, every read's verdict ("V strand_mode
// intron_mode read status gene tier"); tests/test_intron_index_cpu.py compares them with tests/intron_model.py.
// Every verdict is computed without a top and under tops of several caps, which must agree.
// Stand-alone: built with -fsanitize=address,undefined by that test.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_gene_index.hpp"

using namespace umihip;

namespace {

struct Lines {
    std::vector<int32_t> ref, start, end, gene;
    std::vector<uint8_t> strand;
    uint32_t n_genes = 0;
};

struct Read {
    int32_t ref;
    int64_t pos;
    int reverse;
    std::vector<uint32_t> cigar;
};

struct Tier {
    GeneTable plain;
    std::vector<GeneTable> sampled;
};

const uint32_t CAPS[] = {1, 3, 7, 512};

void build(const int32_t *ref, const int32_t *start, const int32_t *end, const uint8_t *strand, const int32_t *gene, size_t n,
           uint32_t n_genes, unsigned take, Tier &t)
{
    gene_index_build(ref, start, end, strand, gene, n, n_genes, take, t.plain);
    for (uint32_t cap : CAPS) {
        GeneTable s = t.plain;
        gene_index_sample(s, cap);
        t.sampled.push_back(std::move(s));
    }
}

} // namespace

int main(int argc, char **argv)
{
    if (argc != 2) {
        fprintf(stderr, "usage: test_intron_index FILE\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot read %s\n", argv[1]);
        return 2;
    }
    Lines x;
    std::vector<Read> reads;
    char kind;
    while (fscanf(f, " %c", &kind) == 1) {
        if (kind == 'E') {
            int32_t r, s, e, g;
            char st;
            if (fscanf(f, "%" SCNd32 " %" SCNd32 " %" SCNd32 " %c %" SCNd32, &r, &s, &e, &st, &g) != 5) return 2;
            x.ref.push_back(r), x.start.push_back(s), x.end.push_back(e), x.strand.push_back((uint8_t)st), x.gene.push_back(g);
            if ((uint32_t)g + 1 > x.n_genes) x.n_genes = (uint32_t)g + 1;
        } else if (kind == 'R') {
            Read r;
            size_t n;
            if (fscanf(f, "%" SCNd32 " %" SCNd64 " %d %zu", &r.ref, &r.pos, &r.reverse, &n) != 4) return 2;
            r.cigar.resize(n);
            for (size_t i = 0; i < n; i++)
                if (fscanf(f, "%" SCNu32, &r.cigar[i]) != 1) return 2;
            reads.push_back(std::move(r));
        } else {
            return 2;
        }
    }
    fclose(f);

    GeneBodies b;
    gene_bodies_derive(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.ref.size(), b);
    for (size_t i = 0; i < b.gene.size(); i++) printf("B %d %d %d %c %d\n", b.ref[i], b.start[i], b.end[i], (char)b.strand[i], b.gene[i]);

    int failures = 0;
    for (int strand_mode = 0; strand_mode < 3; strand_mode++) { // forward, reverse, unstranded (UMI_STRAND_*)
        // the tables as the library lays them out: one for unstranded, else what a read on + and on - may hit
        const int n_tables = strand_mode == 2 ? 1 : 2;
        const unsigned take[2] = {n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                                  GENE_TAKE_MINUS | GENE_TAKE_DOT};
        Tier exons[2], bodies[2];
        for (int t = 0; t < n_tables; t++) {
            build(x.ref.data(), x.start.data(), x.end.data(), x.strand.data(), x.gene.data(), x.ref.size(), x.n_genes, take[t], exons[t]);
            build(b.ref.data(), b.start.data(), b.end.data(), b.strand.data(), b.gene.data(), b.gene.size(), x.n_genes, take[t], bodies[t]);
        }
        for (int intron_mode = 0; intron_mode < 3; intron_mode++)
            for (size_t i = 0; i < reads.size(); i++) {
                const Read &r = reads[i];
                const int t = n_tables == 1 ? 0 : ((r.reverse != 0) != (strand_mode == 1) ? 1 : 0);
                int32_t gene;
                int tier;
                const int st = gene_assign_read_tiers(gene_view(exons[t].plain), nullptr, gene_view(bodies[t].plain), nullptr, intron_mode,
                                                      (uint32_t)r.ref, r.pos, r.cigar.data(), r.cigar.size(), &gene, &tier);
                for (size_t k = 0; k < exons[t].sampled.size(); k++) {
                    const GeneTop et = gene_top(exons[t].sampled[k]), bt = gene_top(bodies[t].sampled[k]);
                    int32_t g2;
                    int tier2;
                    const int st2 = gene_assign_read_tiers(gene_view(exons[t].sampled[k]), &et, gene_view(bodies[t].sampled[k]), &bt,
                                                           intron_mode, (uint32_t)r.ref, r.pos, r.cigar.data(), r.cigar.size(), &g2, &tier2);
                    if ((st2 != st || g2 != gene || tier2 != tier) && failures++ < 20)
                        fprintf(stderr, "read %zu, strand mode %d, intron mode %d: %d %d %d without a top, %d %d %d under a cap of %u\n", i,
                                strand_mode, intron_mode, st, gene, tier, st2, g2, tier2, CAPS[k]);
                }
                printf("V %d %d %zu %d %d %d\n", strand_mode, intron_mode, i, st, gene, tier);
            }
    }
    if (failures) {
        fprintf(stderr, "%d verdicts differ under a top\n", failures);
        return 1;
    }
    printf("intron index ok\n");
    return 0;
}
