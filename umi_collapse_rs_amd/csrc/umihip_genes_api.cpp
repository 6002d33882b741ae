// Reads assigned to genes from an annotation: umi_assign_genes*.  The checks, the index (built on the host by
// every call, umihip_gene_index.hpp), the call's workspace and what the device found wrong.
#include <hip/hip_runtime.h>

#include "umihip_gene_index.hpp"
#include "umihip_host.hpp"
#include "umihip_transcript_index.hpp"

using namespace umihip;

namespace {

struct GeneIndex {
    GeneTable tables[2];
    int n_tables = 0;
    bool flip = false;
};

// the checks both forms share, all but the context's: decided without a device
int genes_check_arrays(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                       const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode, const void *read_ref,
                       const void *read_pos, const void *read_reverse, const void *cigar_off, uint64_t n_reads, const void *gene,
                       const void *status, const uint64_t *counts)
{
    if (!counts) return fail(UMI_ERR_ARG, "counts is NULL");
    if (strand_mode != UMI_STRAND_FORWARD && strand_mode != UMI_STRAND_REVERSE && strand_mode != UMI_STRAND_UNSTRANDED)
        return fail(UMI_ERR_ARG, "unknown strand_mode %d", strand_mode);
    if (n_exons >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu exons exceed the 30-bit index space of one call", (unsigned long long)n_exons);
    if (n_genes >= (1u << 31)) return fail(UMI_ERR_ARG, "n_genes %u does not fit a gene index", n_genes);
    if (n_exons && (!exon_ref || !exon_start || !exon_end || !exon_strand || !exon_gene))
        return fail(UMI_ERR_ARG, "a required exon array is NULL");
    if (n_reads >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one call", (unsigned long long)n_reads);
    if (n_reads && (!read_ref || !read_pos || !read_reverse || !cigar_off || !gene || !status))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    for (uint64_t i = 0; i < n_exons; i++) {
        if (exon_start[i] < 0 || exon_end[i] <= exon_start[i])
            return fail(UMI_ERR_ARG, "exon %llu: [%d, %d) is no interval of the reference", (unsigned long long)i, exon_start[i], exon_end[i]);
        if (exon_ref[i] < 0) return fail(UMI_ERR_ARG, "exon %llu: reference %d", (unsigned long long)i, exon_ref[i]);
        if (exon_gene[i] < 0 || (uint32_t)exon_gene[i] >= n_genes)
            return fail(UMI_ERR_ARG, "exon %llu: gene %d outside 0..%u", (unsigned long long)i, exon_gene[i], n_genes);
        if (exon_strand[i] != '+' && exon_strand[i] != '-' && exon_strand[i] != '.')
            return fail(UMI_ERR_ARG, "exon %llu: unknown strand %u", (unsigned long long)i, (unsigned)exon_strand[i]);
    }
    return UMI_OK;
}

// (the context is looked at last)
int genes_check(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode, const void *read_ref,
                const void *read_pos, const void *read_reverse, const void *cigar_off, uint64_t n_reads, const void *gene,
                const void *status, const uint64_t *counts)
{
    const int rc = genes_check_arrays(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, read_ref,
                                      read_pos, read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

void genes_index(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                 const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode, GeneIndex &ix)
{
    ix.flip = strand_mode == UMI_STRAND_REVERSE;
    ix.n_tables = strand_mode == UMI_STRAND_UNSTRANDED ? 1 : 2;
    const unsigned take[2] = {ix.n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                              GENE_TAKE_MINUS | GENE_TAKE_DOT};
    for (int t = 0; t < ix.n_tables; t++) {
        gene_index_build(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, take[t], ix.tables[t]);
        gene_index_sample(ix.tables[t], GENE_TOP_CAP);
    }
}

int genes_run(umi_ctx *ctx, const GeneIndex &ix, const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse,
              const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene, uint8_t *d_status,
              uint64_t *counts, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(genes_workspace_bytes(ix.tables, ix.n_tables)))) return rc;
    uint64_t bad = 0;
    const int r = genes_on_device(ctx->call_ws.p, ix.tables, ix.n_tables, ix.flip, ctx->gene_top, d_ref, d_pos, d_reverse, d_cigar,
                                  d_cigar_off, (uint32_t)n_reads, d_gene, d_status, counts, &bad, (uint32_t)ctx->n_cus,
                                  ctx->h_counters, s);
    if (r == 1)
        return fail(UMI_ERR_ARG, "read %llu: a negative reference, a CIGAR op code above 8, or CIGAR words without an array",
                    (unsigned long long)bad);
    if (r == 2) return fail(UMI_ERR_ORDER, "cigar_off falls at read %llu", (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "gene assignment: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_assign_genes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                            const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                            int strand_mode, const int32_t *d_read_ref, const int32_t *d_read_pos, const uint8_t *d_read_reverse,
                            const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene,
                            uint8_t *d_status, uint64_t counts[3], void *hip_stream)
{
    int rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, d_read_ref,
                         d_read_pos, d_read_reverse, d_cigar_off, n_reads, d_gene, d_status, counts);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (the first device of a multi-device context, as umi_correct_barcodes)
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    GeneIndex ix;
    genes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, ix);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return genes_run(ctx, ix, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene, d_status, counts,
                     (hipStream_t)hip_stream);
}

int umi_assign_genes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                     const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode,
                     const int32_t *read_ref, const int32_t *read_pos, const uint8_t *read_reverse, const uint32_t *cigar,
                     const uint64_t *cigar_off, uint64_t n_reads, int32_t *gene, uint8_t *status, uint64_t counts[3])
{
    int rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, read_ref,
                         read_pos, read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (n_reads && cigar_off[n_reads] && !cigar) return fail(UMI_ERR_ARG, "cigar is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    GeneIndex ix;
    genes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, ix);
    const size_t n = (size_t)n_reads, words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_ref = io.in(read_ref, n * 4), d_pos = io.in(read_pos, n * 4);
    const auto d_reverse = io.in(read_reverse, n);
    const auto d_cigar = io.in(cigar, words * 4);
    const auto d_off = io.in(cigar_off, (n + 1) * 8);
    const auto d_gene = io.out(gene, n * 4);
    const auto d_status = io.out(status, n);
    if ((rc = io.open()) ||
        (rc = genes_run(ctx, ix, d_ref, d_pos, d_reverse, d_cigar, d_off, n_reads, d_gene, d_status, counts, io.stream())) ||
        (rc = io.fetch(gene, d_gene, n)) || (rc = io.fetch(status, d_status, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- umi_assign_genes_introns*: the same checks and the exons' index, and beside it the gene bodies' (derived here,
// ---- umihip_gene_index.hpp), one table per strand class each; the kernel is umihip_gene_introns.hip's

namespace {

struct IntronIndex {
    GeneIndex exons;
    GeneTable bodies[2];
};

int introns_check(int intron_mode, const void *tier, uint64_t n_reads)
{
    if (intron_mode != UMI_INTRONS_OFF && intron_mode != UMI_INTRONS_EXON_FIRST && intron_mode != UMI_INTRONS_ALL)
        return fail(UMI_ERR_ARG, "unknown intron_mode %d", intron_mode);
    if (n_reads && !tier) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    return UMI_OK;
}

void introns_index(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                   const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode, int intron_mode, IntronIndex &ix)
{
    genes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, ix.exons);
    GeneBodies b; // (off: no read looks at a body, and the body tables stay empty)
    if (intron_mode != UMI_INTRONS_OFF) gene_bodies_derive(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, b);
    const unsigned take[2] = {ix.exons.n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                              GENE_TAKE_MINUS | GENE_TAKE_DOT};
    for (int t = 0; t < ix.exons.n_tables; t++) {
        gene_index_build(b.ref.data(), b.start.data(), b.end.data(), b.strand.data(), b.gene.data(), b.gene.size(), n_genes, take[t],
                         ix.bodies[t]);
        gene_index_sample(ix.bodies[t], GENE_BODY_TOP_CAP);
    }
}

int introns_run(umi_ctx *ctx, const IntronIndex &ix, int intron_mode, const int32_t *d_ref, const int32_t *d_pos,
                const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene,
                uint8_t *d_status, uint8_t *d_tier, uint64_t *counts, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(gene_introns_workspace_bytes(ix.exons.tables, ix.bodies, ix.exons.n_tables)))) return rc;
    uint64_t bad = 0;
    const int r = gene_introns_on_device(ctx->call_ws.p, ix.exons.tables, ix.bodies, ix.exons.n_tables, ix.exons.flip, intron_mode,
                                         ctx->gene_top, ctx->gene_body_top, d_ref, d_pos, d_reverse, d_cigar, d_cigar_off,
                                         (uint32_t)n_reads, d_gene, d_status, d_tier, counts, &bad, (uint32_t)ctx->n_cus,
                                         ctx->h_counters, s);
    if (r == 1)
        return fail(UMI_ERR_ARG, "read %llu: a negative reference, a CIGAR op code above 8, or CIGAR words without an array",
                    (unsigned long long)bad);
    if (r == 2) return fail(UMI_ERR_ORDER, "cigar_off falls at read %llu", (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "gene assignment with introns: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_assign_genes_introns_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                    const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                                    int strand_mode, int intron_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                                    const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                                    uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint64_t counts[4],
                                    void *hip_stream)
{
    int rc = introns_check(intron_mode, d_tier, n_reads);
    if (rc) return rc;
    rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, d_read_ref, d_read_pos,
                     d_read_reverse, d_cigar_off, n_reads, d_gene, d_status, counts);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_reads == 0) return UMI_OK;
    IntronIndex ix;
    introns_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, intron_mode, ix);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return introns_run(ctx, ix, intron_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene, d_status,
                       d_tier, counts, (hipStream_t)hip_stream);
}

int umi_assign_genes_introns(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                             const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                             int strand_mode, int intron_mode, const int32_t *read_ref, const int32_t *read_pos,
                             const uint8_t *read_reverse, const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads,
                             int32_t *gene, uint8_t *status, uint8_t *tier, uint64_t counts[4])
{
    int rc = introns_check(intron_mode, tier, n_reads);
    if (rc) return rc;
    rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, read_ref, read_pos,
                     read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (n_reads && cigar_off[n_reads] && !cigar) return fail(UMI_ERR_ARG, "cigar is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_reads == 0) return UMI_OK;
    IntronIndex ix;
    introns_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, intron_mode, ix);
    const size_t n = (size_t)n_reads, words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_ref = io.in(read_ref, n * 4), d_pos = io.in(read_pos, n * 4);
    const auto d_reverse = io.in(read_reverse, n);
    const auto d_cigar = io.in(cigar, words * 4);
    const auto d_off = io.in(cigar_off, (n + 1) * 8);
    const auto d_gene = io.out(gene, n * 4);
    const auto d_status = io.out(status, n);
    const auto d_tier = io.out(tier, n);
    if ((rc = io.open()) ||
        (rc = introns_run(ctx, ix, intron_mode, d_ref, d_pos, d_reverse, d_cigar, d_off, n_reads, d_gene, d_status, d_tier, counts,
                          io.stream())) ||
        (rc = io.fetch(gene, d_gene, n)) || (rc = io.fetch(status, d_status, n)) || (rc = io.fetch(tier, d_tier, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- umi_assign_genes_classes*: umi_assign_genes_introns' checks and index, and beside every exon table its prefix
// ---- array of covered bases and its genes' own exons; the kernel is umihip_gene_classes.hip's

namespace {

struct ClassIndex {
    IntronIndex tiers;
    GeneCover cover[2];
};

int classes_check(const void *cls, const uint64_t *class_counts, uint64_t n_reads)
{
    if (!class_counts) return fail(UMI_ERR_ARG, "class_counts is NULL");
    if (n_reads && !cls) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    return UMI_OK;
}

void classes_index(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                   const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes, int strand_mode, int intron_mode, ClassIndex &ix)
{
    introns_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, intron_mode, ix.tiers);
    const int n_tables = ix.tiers.exons.n_tables;
    const unsigned take[2] = {n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                              GENE_TAKE_MINUS | GENE_TAKE_DOT};
    for (int t = 0; t < n_tables; t++) {
        gene_cover_prefix(ix.tiers.exons.tables[t], ix.cover[t].cum);
        gene_own_build(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, take[t], ix.cover[t].own);
    }
}

int classes_run(umi_ctx *ctx, const ClassIndex &ix, int intron_mode, const int32_t *d_ref, const int32_t *d_pos,
                const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene,
                uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls, uint64_t *counts, uint64_t *class_counts, hipStream_t s)
{
    int rc;
    const GeneIndex &ex = ix.tiers.exons;
    if ((rc = ctx->call_ws.reserve(gene_classes_workspace_bytes(ex.tables, ix.tiers.bodies, ix.cover, ex.n_tables)))) return rc;
    uint64_t bad = 0;
    const int r = gene_classes_on_device(ctx->call_ws.p, ex.tables, ix.tiers.bodies, ix.cover, ex.n_tables, ex.flip, intron_mode,
                                         ctx->gene_top, ctx->gene_body_top, d_ref, d_pos, d_reverse, d_cigar, d_cigar_off,
                                         (uint32_t)n_reads, d_gene, d_status, d_tier, d_cls, counts, class_counts, &bad,
                                         (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r == 1)
        return fail(UMI_ERR_ARG, "read %llu: a negative reference, a CIGAR op code above 8, or CIGAR words without an array",
                    (unsigned long long)bad);
    if (r == 2) return fail(UMI_ERR_ORDER, "cigar_off falls at read %llu", (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "gene assignment with classes: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_assign_genes_classes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                    const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                                    int strand_mode, int intron_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                                    const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                                    uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls,
                                    uint64_t counts[4], uint64_t class_counts[5], void *hip_stream)
{
    int rc = classes_check(d_cls, class_counts, n_reads);
    if (rc) return rc;
    if ((rc = introns_check(intron_mode, d_tier, n_reads))) return rc;
    rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, d_read_ref, d_read_pos,
                     d_read_reverse, d_cigar_off, n_reads, d_gene, d_status, counts);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int c = 0; c < 5; c++) class_counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    ClassIndex ix;
    classes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, intron_mode, ix);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return classes_run(ctx, ix, intron_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene, d_status,
                       d_tier, d_cls, counts, class_counts, (hipStream_t)hip_stream);
}

int umi_assign_genes_classes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                             const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                             int strand_mode, int intron_mode, const int32_t *read_ref, const int32_t *read_pos,
                             const uint8_t *read_reverse, const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads,
                             int32_t *gene, uint8_t *status, uint8_t *tier, uint8_t *cls, uint64_t counts[4],
                             uint64_t class_counts[5])
{
    int rc = classes_check(cls, class_counts, n_reads);
    if (rc) return rc;
    if ((rc = introns_check(intron_mode, tier, n_reads))) return rc;
    rc = genes_check(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, read_ref, read_pos,
                     read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (n_reads && cigar_off[n_reads] && !cigar) return fail(UMI_ERR_ARG, "cigar is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int c = 0; c < 5; c++) class_counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    ClassIndex ix;
    classes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, intron_mode, ix);
    const size_t n = (size_t)n_reads, words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_ref = io.in(read_ref, n * 4), d_pos = io.in(read_pos, n * 4);
    const auto d_reverse = io.in(read_reverse, n);
    const auto d_cigar = io.in(cigar, words * 4);
    const auto d_off = io.in(cigar_off, (n + 1) * 8);
    const auto d_gene = io.out(gene, n * 4);
    const auto d_status = io.out(status, n);
    const auto d_tier = io.out(tier, n);
    const auto d_cls = io.out(cls, n);
    if ((rc = io.open()) ||
        (rc = classes_run(ctx, ix, intron_mode, d_ref, d_pos, d_reverse, d_cigar, d_off, n_reads, d_gene, d_status, d_tier, d_cls, counts,
                          class_counts, io.stream())) ||
        (rc = io.fetch(gene, d_gene, n)) || (rc = io.fetch(status, d_status, n)) || (rc = io.fetch(tier, d_tier, n)) ||
        (rc = io.fetch(cls, d_cls, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- umi_assign_genes_transcripts*: umi_assign_genes' checks, the transcripts' (umihip_transcript_index.hpp), and the
// ---- transcript tables, one per strand class; the kernel is umihip_gene_transcripts.hip's

namespace {

struct TranscriptIndex {
    TranscriptTable tables[2];
    int n_tables = 0;
    bool flip = false;
};

// (after genes_check_arrays: every exon is an exon)
int transcripts_check(const int32_t *exon_ref, const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript,
                      uint64_t n_exons, uint32_t n_transcripts)
{
    if (n_transcripts >= (1u << 31)) return fail(UMI_ERR_ARG, "n_transcripts %u does not fit a transcript index", n_transcripts);
    if (n_exons && !exon_transcript) return fail(UMI_ERR_ARG, "a required exon array is NULL");
    uint64_t bad = 0;
    switch (transcript_check(exon_ref, exon_strand, exon_gene, exon_transcript, n_exons, n_transcripts, &bad)) {
    case TR_BAD_RANGE:
        return fail(UMI_ERR_ARG, "exon %llu: transcript %d outside 0..%u", (unsigned long long)bad, exon_transcript[bad], n_transcripts);
    case TR_BAD_REF:
        return fail(UMI_ERR_ARG, "exon %llu: transcript %d lies on two references", (unsigned long long)bad, exon_transcript[bad]);
    case TR_BAD_STRAND:
        return fail(UMI_ERR_ARG, "exon %llu: transcript %d lies on two strands", (unsigned long long)bad, exon_transcript[bad]);
    case TR_BAD_GENE:
        return fail(UMI_ERR_ARG, "exon %llu: transcript %d lies in two genes", (unsigned long long)bad, exon_transcript[bad]);
    default:
        return UMI_OK;
    }
}

// both forms' checks, in order: the exons, the transcripts, the context
int transcripts_check_all(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                          const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript, uint64_t n_exons,
                          uint32_t n_genes, uint32_t n_transcripts, int strand_mode, const void *read_ref, const void *read_pos,
                          const void *read_reverse, const void *cigar_off, uint64_t n_reads, const void *gene, const void *status,
                          const uint64_t *counts)
{
    int rc = genes_check_arrays(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, n_genes, strand_mode, read_ref, read_pos,
                                read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if ((rc = transcripts_check(exon_ref, exon_strand, exon_gene, exon_transcript, n_exons, n_transcripts))) return rc;
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

void transcripts_index(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                       const int32_t *exon_gene, const int32_t *exon_transcript, uint64_t n_exons, int strand_mode, TranscriptIndex &ix)
{
    ix.flip = strand_mode == UMI_STRAND_REVERSE;
    ix.n_tables = strand_mode == UMI_STRAND_UNSTRANDED ? 1 : 2;
    const unsigned take[2] = {ix.n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                              GENE_TAKE_MINUS | GENE_TAKE_DOT};
    for (int t = 0; t < ix.n_tables; t++) {
        transcript_index_build(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, take[t], ix.tables[t]);
        transcript_index_sample(ix.tables[t], GENE_TOP_CAP);
    }
}

int transcripts_run(umi_ctx *ctx, const TranscriptIndex &ix, const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse,
                    const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene, uint8_t *d_status,
                    uint64_t *counts, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(gene_transcripts_workspace_bytes(ix.tables, ix.n_tables)))) return rc;
    uint64_t bad = 0;
    const int r = gene_transcripts_on_device(ctx->call_ws.p, ix.tables, ix.n_tables, ix.flip, ctx->gene_top, d_ref, d_pos, d_reverse,
                                             d_cigar, d_cigar_off, (uint32_t)n_reads, d_gene, d_status, counts, &bad,
                                             (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r == 1)
        return fail(UMI_ERR_ARG, "read %llu: a negative reference, a CIGAR op code above 8, or CIGAR words without an array",
                    (unsigned long long)bad);
    if (r == 2) return fail(UMI_ERR_ORDER, "cigar_off falls at read %llu", (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "gene assignment by transcripts: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_assign_genes_transcripts_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                        const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript,
                                        uint64_t n_exons, uint32_t n_genes, uint32_t n_transcripts, int strand_mode,
                                        const int32_t *d_read_ref, const int32_t *d_read_pos, const uint8_t *d_read_reverse,
                                        const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene,
                                        uint8_t *d_status, uint64_t counts[3], void *hip_stream)
{
    int rc = transcripts_check_all(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes,
                                   n_transcripts, strand_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar_off, n_reads, d_gene,
                                   d_status, counts);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (the first device of a multi-device context, as umi_assign_genes)
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    TranscriptIndex ix;
    transcripts_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, strand_mode, ix);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return transcripts_run(ctx, ix, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene, d_status, counts,
                           (hipStream_t)hip_stream);
}

int umi_assign_genes_transcripts(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                 const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript, uint64_t n_exons,
                                 uint32_t n_genes, uint32_t n_transcripts, int strand_mode, const int32_t *read_ref,
                                 const int32_t *read_pos, const uint8_t *read_reverse, const uint32_t *cigar, const uint64_t *cigar_off,
                                 uint64_t n_reads, int32_t *gene, uint8_t *status, uint64_t counts[3])
{
    int rc = transcripts_check_all(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes,
                                   n_transcripts, strand_mode, read_ref, read_pos, read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (n_reads && cigar_off[n_reads] && !cigar) return fail(UMI_ERR_ARG, "cigar is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    TranscriptIndex ix;
    transcripts_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, strand_mode, ix);
    const size_t n = (size_t)n_reads, words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_ref = io.in(read_ref, n * 4), d_pos = io.in(read_pos, n * 4);
    const auto d_reverse = io.in(read_reverse, n);
    const auto d_cigar = io.in(cigar, words * 4);
    const auto d_off = io.in(cigar_off, (n + 1) * 8);
    const auto d_gene = io.out(gene, n * 4);
    const auto d_status = io.out(status, n);
    if ((rc = io.open()) ||
        (rc = transcripts_run(ctx, ix, d_ref, d_pos, d_reverse, d_cigar, d_off, n_reads, d_gene, d_status, counts, io.stream())) ||
        (rc = io.fetch(gene, d_gene, n)) || (rc = io.fetch(status, d_status, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- umi_assign_genes_transcripts_classes*: umi_assign_genes_transcripts' checks and tables, the gene bodies' (as
// ---- umi_assign_genes_introns derives them) and, where classes are asked for, the exons' overlap tables with their
// ---- covers (as umi_assign_genes_classes builds them, not sampled); the kernel is umihip_gene_transcript_classes.hip's

namespace {

struct TranscriptClassIndex {
    TranscriptIndex transcripts;
    GeneTable bodies[2], exons[2];
    GeneCover cover[2];
    bool classes = false;
};

// (cls and class_counts come or go together)
int transcript_classes_check(int intron_mode, const void *tier, const void *cls, const uint64_t *class_counts, uint64_t n_reads)
{
    if ((cls == nullptr) != (class_counts == nullptr)) return fail(UMI_ERR_ARG, "cls and class_counts are given together or not at all");
    return introns_check(intron_mode, tier, n_reads);
}

void transcript_classes_index(const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end, const uint8_t *exon_strand,
                              const int32_t *exon_gene, const int32_t *exon_transcript, uint64_t n_exons, uint32_t n_genes, int strand_mode,
                              int intron_mode, bool classes, TranscriptClassIndex &ix)
{
    transcripts_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, strand_mode, ix.transcripts);
    ix.classes = classes;
    const int n_tables = ix.transcripts.n_tables;
    GeneBodies b; // (off: no read looks at a body, and the body tables stay empty)
    if (intron_mode != UMI_INTRONS_OFF) gene_bodies_derive(exon_ref, exon_start, exon_end, exon_strand, exon_gene, n_exons, b);
    const unsigned take[2] = {n_tables == 1 ? GENE_TAKE_PLUS | GENE_TAKE_MINUS | GENE_TAKE_DOT : GENE_TAKE_PLUS | GENE_TAKE_DOT,
                              GENE_TAKE_MINUS | GENE_TAKE_DOT};
    for (int t = 0; t < n_tables; t++) {
        gene_index_build(b.ref.data(), b.start.data(), b.end.data(), b.strand.data(), b.gene.data(), b.gene.size(), n_genes, take[t],
                         ix.bodies[t]);
        gene_index_sample(ix.bodies[t], GENE_BODY_TOP_CAP);
        // (off: no read is assigned by a body, and none looks at the overlap table)
        if (!classes) continue;
        gene_index_build(exon_ref, exon_start, exon_end, exon_strand, exon_gene, intron_mode != UMI_INTRONS_OFF ? n_exons : 0, n_genes,
                         take[t], ix.exons[t]);
        gene_cover_prefix(ix.exons[t], ix.cover[t].cum);
        gene_own_build(exon_ref, exon_start, exon_end, exon_strand, exon_gene, intron_mode != UMI_INTRONS_OFF ? n_exons : 0, n_genes, take[t],
                       ix.cover[t].own);
    }
}

int transcript_classes_run(umi_ctx *ctx, const TranscriptClassIndex &ix, int intron_mode, const int32_t *d_ref, const int32_t *d_pos,
                           const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint64_t n_reads,
                           int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls, uint64_t *counts, uint64_t *class_counts,
                           hipStream_t s)
{
    int rc;
    const TranscriptIndex &tr = ix.transcripts;
    const GeneCover *cover = ix.classes ? ix.cover : nullptr;
    if ((rc = ctx->call_ws.reserve(gene_transcript_classes_workspace_bytes(tr.tables, ix.bodies, ix.exons, cover, tr.n_tables, (uint32_t)n_reads)))) return rc;
    uint64_t bad = 0;
    const int r = gene_transcript_classes_on_device(ctx->call_ws.p, tr.tables, ix.bodies, ix.exons, cover, tr.n_tables, tr.flip, intron_mode,
                                                    ctx->gene_top, ctx->gene_body_top, d_ref, d_pos, d_reverse, d_cigar, d_cigar_off,
                                                    (uint32_t)n_reads, d_gene, d_status, d_tier, d_cls, counts, class_counts, &bad,
                                                    (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r == 1)
        return fail(UMI_ERR_ARG, "read %llu: a negative reference, a CIGAR op code above 8, or CIGAR words without an array",
                    (unsigned long long)bad);
    if (r == 2) return fail(UMI_ERR_ORDER, "cigar_off falls at read %llu", (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "gene assignment by transcripts with classes: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_assign_genes_transcripts_classes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                                const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript,
                                                uint64_t n_exons, uint32_t n_genes, uint32_t n_transcripts, int strand_mode,
                                                int intron_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                                                const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                                                uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls,
                                                uint64_t counts[4], uint64_t class_counts[5], void *hip_stream)
{
    int rc = transcript_classes_check(intron_mode, d_tier, d_cls, class_counts, n_reads);
    if (rc) return rc;
    rc = transcripts_check_all(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes, n_transcripts,
                               strand_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar_off, n_reads, d_gene, d_status, counts);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (the first device of a multi-device context, as umi_assign_genes)
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int c = 0; class_counts && c < 5; c++) class_counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    TranscriptClassIndex ix;
    transcript_classes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes, strand_mode,
                             intron_mode, d_cls != nullptr, ix);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return transcript_classes_run(ctx, ix, intron_mode, d_read_ref, d_read_pos, d_read_reverse, d_cigar, d_cigar_off, n_reads, d_gene,
                                  d_status, d_tier, d_cls, counts, class_counts, (hipStream_t)hip_stream);
}

int umi_assign_genes_transcripts_classes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                         const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript,
                                         uint64_t n_exons, uint32_t n_genes, uint32_t n_transcripts, int strand_mode, int intron_mode,
                                         const int32_t *read_ref, const int32_t *read_pos, const uint8_t *read_reverse,
                                         const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads, int32_t *gene,
                                         uint8_t *status, uint8_t *tier, uint8_t *cls, uint64_t counts[4], uint64_t class_counts[5])
{
    int rc = transcript_classes_check(intron_mode, tier, cls, class_counts, n_reads);
    if (rc) return rc;
    rc = transcripts_check_all(ctx, exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes, n_transcripts,
                               strand_mode, read_ref, read_pos, read_reverse, cigar_off, n_reads, gene, status, counts);
    if (rc) return rc;
    if (n_reads && cigar_off[n_reads] && !cigar) return fail(UMI_ERR_ARG, "cigar is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    for (int c = 0; class_counts && c < 5; c++) class_counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    TranscriptClassIndex ix;
    transcript_classes_index(exon_ref, exon_start, exon_end, exon_strand, exon_gene, exon_transcript, n_exons, n_genes, strand_mode,
                             intron_mode, cls != nullptr, ix);
    const size_t n = (size_t)n_reads, words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_ref = io.in(read_ref, n * 4), d_pos = io.in(read_pos, n * 4);
    const auto d_reverse = io.in(read_reverse, n);
    const auto d_cigar = io.in(cigar, words * 4);
    const auto d_off = io.in(cigar_off, (n + 1) * 8);
    const auto d_gene = io.out(gene, n * 4);
    const auto d_status = io.out(status, n);
    const auto d_tier = io.out(tier, n);
    const auto d_cls = io.out(cls, n); // (absent, and null, where no class is asked for)
    if ((rc = io.open()) ||
        (rc = transcript_classes_run(ctx, ix, intron_mode, d_ref, d_pos, d_reverse, d_cigar, d_off, n_reads, d_gene, d_status, d_tier,
                                     d_cls, counts, class_counts, io.stream())) ||
        (rc = io.fetch(gene, d_gene, n)) || (rc = io.fetch(status, d_status, n)) || (rc = io.fetch(tier, d_tier, n)) ||
        (rc = io.fetch(cls, d_cls, n)))
        return rc;
    return io.close();
}

} // extern "C"
