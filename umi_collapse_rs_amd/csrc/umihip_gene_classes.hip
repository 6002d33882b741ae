// Reads assigned to genes with their introns and their class (umi_assign_genes_classes, the program's --velocity),
// gfx950.
//
// gene, status, tier and the four counts are umi_assign_genes_introns' (umihip_gene_introns.hip), by the same lookup
// code (gene_assign_read_tiers).  New is the class of an assigned read (include/umihip.h has the rule in full): tier
// intron: INTRONIC; tier exon: SPANNING where a block is not covered whole by the gene's exons, else JUNCTION where
// a gap an N skipped is not, else EXONIC.  tests/velocity_model.py defines it.
//
// Beside each exon table travel a prefix array of covered bases (cover of a block: two more loads) and the genes' own
// united exons, for the gaps the table covers whole (umihip_gene_index.hpp says why); both are built on the host and
// uploaded by this call alone.
//
// Kernel: gene_introns_kernel's shape -- a read per lane, GENE_THREADS lanes per block, GENE_BLOCKS_PER_CU blocks per
// CU, a grid stride beyond, the same tops in LDS (72 KiB a block) and the same options.  A lane whose read is assigned
// by an exon walks its CIGAR once more for the blocks' cover (the words are in cache), and a third time for the gaps
// only where every block is covered and there are two.  What the device finds wrong is told through the control
// block, as umihip_genes.hip tells it.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_gene_index.hpp"
#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

static_assert(GENE_CLASS_NONE == UMI_READ_CLASS_NONE && GENE_CLASS_EXONIC == UMI_READ_CLASS_EXONIC &&
                  GENE_CLASS_JUNCTION == UMI_READ_CLASS_JUNCTION && GENE_CLASS_SPANNING == UMI_READ_CLASS_SPANNING &&
                  GENE_CLASS_INTRONIC == UMI_READ_CLASS_INTRONIC,
              "the lookup's classes are the interface's");

namespace {

enum ClassCtl : int {
    CLASS_BAD_ARG = 0,   // smallest read with read_ref < 0 or a bad op code (all ones: none)
    CLASS_BAD_ORDER = 1, // smallest read whose cigar_off falls (all ones: none)
    CLASS_COUNT0 = 2,    // seven words: reads assigned by an exon, by an intron, none, several; exonic, junction, spanning
    CLASS_CTL_COUNT = 9,
};

struct ClassDevTable {
    GeneView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
    const uint64_t *cum; // (the exon tier alone)
    GeneOwnView own;
};

struct ClassArgs {
    ClassDevTable exon[2], body[2]; // forward / reverse: the tables of a read on + and on -; unstranded: [0] for both
    int n_tab, mode;
    const int32_t *ref, *pos;
    const uint8_t *reverse;
    const uint32_t *cigar;
    const uint64_t *cigar_off;
    uint32_t n;
    int32_t *gene;
    uint8_t *status, *tier, *cls;
    unsigned long long *ctl;
};

constexpr uint32_t LDS_BODY0 = 2 * GENE_TOP_CAP; // where the body tops begin

template <bool TOP, bool BTOP> __global__ __launch_bounds__(GENE_THREADS) void gene_classes_kernel(ClassArgs a)
{
    __shared__ uint64_t lds_top[TOP ? 2 * GENE_TOP_CAP + (BTOP ? 2 * GENE_BODY_TOP_CAP : 0) : 1];
    if (TOP) {
        for (int t = 0; t < a.n_tab; t++) {
            for (uint32_t j = threadIdx.x; j < a.exon[t].n_top; j += GENE_THREADS) lds_top[t * GENE_TOP_CAP + j] = a.exon[t].top[j];
            if (BTOP)
                for (uint32_t j = threadIdx.x; j < a.body[t].n_top; j += GENE_THREADS)
                    lds_top[LDS_BODY0 + t * GENE_BODY_TOP_CAP + j] = a.body[t].top[j];
        }
        __syncthreads();
    }
    const uint64_t total = a.cigar_off[a.n];
    uint32_t seen[7] = {0, 0, 0, 0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * GENE_THREADS + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * GENE_THREADS) {
        const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
        if (c0 > c1 || c1 > total) {
            atomicMin(a.ctl + CLASS_BAD_ORDER, (unsigned long long)i);
            continue;
        }
        const int32_t ref = a.ref[i];
        if (ref < 0 || (c1 > c0 && !a.cigar)) {
            atomicMin(a.ctl + CLASS_BAD_ARG, (unsigned long long)i);
            continue;
        }
        const int t = a.n_tab == 1 ? 0 : (a.reverse[i] ? 1 : 0);
        const GeneTop exon_top = {lds_top + (TOP ? t * GENE_TOP_CAP : 0), a.exon[t].n_top, a.exon[t].shift};
        const GeneTop body_top = {lds_top + (TOP && BTOP ? LDS_BODY0 + t * GENE_BODY_TOP_CAP : 0), a.body[t].n_top, a.body[t].shift};
        int32_t g;
        int tier;
        const int st = gene_assign_read_tiers(a.exon[t].view, TOP ? &exon_top : nullptr, a.body[t].view, TOP && BTOP ? &body_top : nullptr,
                                              a.mode, (uint32_t)ref, (int64_t)a.pos[i], a.cigar + c0, c1 - c0, &g, &tier);
        if (st == GENE_READ_BAD_OP) {
            atomicMin(a.ctl + CLASS_BAD_ARG, (unsigned long long)i);
            continue;
        }
        int cls = GENE_CLASS_NONE;
        if (st == GENE_READ_ASSIGNED)
            cls = tier == GENE_TIER_INTRON ? GENE_CLASS_INTRONIC
                                           : gene_read_class(a.exon[t].view, TOP ? &exon_top : nullptr, a.exon[t].cum, a.exon[t].own, g,
                                                             (uint32_t)ref, (int64_t)a.pos[i], a.cigar + c0, c1 - c0);
        a.gene[i] = g;
        a.status[i] = (uint8_t)st;
        a.tier[i] = (uint8_t)tier;
        a.cls[i] = (uint8_t)cls;
        seen[0] += st == GENE_READ_ASSIGNED && tier == GENE_TIER_EXON;
        seen[1] += st == GENE_READ_ASSIGNED && tier == GENE_TIER_INTRON;
        seen[2] += st == GENE_READ_NONE;
        seen[3] += st == GENE_READ_SEVERAL;
        seen[4] += cls == GENE_CLASS_EXONIC;
        seen[5] += cls == GENE_CLASS_JUNCTION;
        seen[6] += cls == GENE_CLASS_SPANNING;
    }
    // the counts: summed over the wave, one atomic per wave and counter
    for (int c = 0; c < 7; c++) {
        uint32_t v = seen[c];
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.ctl + CLASS_COUNT0 + c, (unsigned long long)v);
    }
}

size_t table_bytes(const GeneTable &t)
{
    const size_t n = t.end.size();
    return 2 * align256(n * 8 + 8) + align256(n * sizeof(GeneSeg) + 8) + align256(t.top.size() * 8 + 8);
}

size_t cover_bytes(const GeneCover &c)
{
    const GeneOwn &o = c.own;
    return align256(c.cum.size() * 8) + 2 * align256(o.start.size() * 8 + 8) + align256(o.off.size() * 4 + 8);
}

// one table into the workspace at p (table_bytes of it), p moved on
int upload(const GeneTable &h, char *&p, ClassDevTable &d, hipStream_t s)
{
    const size_t n = h.end.size();
    uint64_t *d_start = (uint64_t *)p;
    p += align256(n * 8 + 8);
    uint64_t *d_end = (uint64_t *)p;
    p += align256(n * 8 + 8);
    GeneSeg *d_seg = (GeneSeg *)p;
    p += align256(n * sizeof(GeneSeg) + 8);
    uint64_t *d_top = (uint64_t *)p;
    p += align256(h.top.size() * 8 + 8);
    if (n) {
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_start, h.start.data(), n * 8, hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_end, h.end.data(), n * 8, hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_seg, h.seg.data(), n * sizeof(GeneSeg), hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_top, h.top.data(), h.top.size() * 8, hipMemcpyHostToDevice, s));
    }
    d = {{d_start, d_end, d_seg, (uint32_t)n}, d_top, (uint32_t)h.top.size(), h.top_shift, nullptr, {nullptr, nullptr, nullptr}};
    return 0;
}

// an exon table's prefix array and its genes' own exons (cover_bytes of them)
int upload_cover(const GeneCover &c, char *&p, ClassDevTable &d, hipStream_t s)
{
    const std::vector<uint64_t> &cum = c.cum;
    const GeneOwn &o = c.own;
    const size_t m = o.start.size();
    uint64_t *d_cum = (uint64_t *)p;
    p += align256(cum.size() * 8);
    uint64_t *d_start = (uint64_t *)p;
    p += align256(m * 8 + 8);
    uint64_t *d_end = (uint64_t *)p;
    p += align256(m * 8 + 8);
    uint32_t *d_off = (uint32_t *)p;
    p += align256(o.off.size() * 4 + 8);
    UMIHIP_TRY_NEG(hipMemcpyAsync(d_cum, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, s));
    if (m) {
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_start, o.start.data(), m * 8, hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_end, o.end.data(), m * 8, hipMemcpyHostToDevice, s));
    }
    UMIHIP_TRY_NEG(hipMemcpyAsync(d_off, o.off.data(), o.off.size() * 4, hipMemcpyHostToDevice, s));
    d.cum = d_cum;
    d.own = {d_start, d_end, d_off};
    return 0;
}

} // namespace

size_t gene_classes_workspace_bytes(const GeneTable *exons, const GeneTable *bodies, const GeneCover *cover, int n_tables)
{
    size_t b = 256;
    for (int t = 0; t < n_tables; t++) b += table_bytes(exons[t]) + table_bytes(bodies[t]) + cover_bytes(cover[t]);
    return b;
}

int gene_classes_on_device(void *workspace, const GeneTable *exons, const GeneTable *bodies, const GeneCover *cover,
                           int n_tables, bool flip, int mode, bool use_top, bool use_body_top, const int32_t *d_ref,
                           const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                           uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls, uint64_t counts[4],
                           uint64_t class_counts[5], uint64_t *bad, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s)
{
    unsigned long long *ctl = (unsigned long long *)workspace;
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl, 0xFF, CLASS_COUNT0 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl + CLASS_COUNT0, 0, 7 * 8, s));
    ClassDevTable dev_exon[2], dev_body[2];
    char *p = (char *)workspace + 256;
    for (int t = 0; t < n_tables; t++) {
        int r;
        if ((r = upload(exons[t], p, dev_exon[t], s)) || (r = upload(bodies[t], p, dev_body[t], s)) ||
            (r = upload_cover(cover[t], p, dev_exon[t], s)))
            return r;
    }
    ClassArgs a;
    a.n_tab = n_tables;
    a.mode = mode;
    // (reverse: a read on + looks among the lines on -)
    const int fwd = n_tables == 2 && flip ? 1 : 0, rev = n_tables == 2 && !flip ? 1 : 0;
    a.exon[0] = dev_exon[fwd];
    a.exon[1] = dev_exon[rev];
    a.body[0] = dev_body[fwd];
    a.body[1] = dev_body[rev];
    a.ref = d_ref;
    a.pos = d_pos;
    a.reverse = d_reverse;
    a.cigar = d_cigar;
    a.cigar_off = d_cigar_off;
    a.n = n_reads;
    a.gene = d_gene;
    a.status = d_status;
    a.tier = d_tier;
    a.cls = d_cls;
    a.ctl = ctl;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(((uint64_t)n_reads + GENE_THREADS - 1) / GENE_THREADS, (uint64_t)n_cus * GENE_BLOCKS_PER_CU));
    if (use_top && use_body_top)
        gene_classes_kernel<true, true><<<grid, GENE_THREADS, 0, s>>>(a);
    else if (use_top)
        gene_classes_kernel<true, false><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_classes_kernel<false, false><<<grid, GENE_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, ctl, CLASS_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    if (h_pinned[CLASS_BAD_ORDER] != ~0ull && h_pinned[CLASS_BAD_ORDER] <= h_pinned[CLASS_BAD_ARG]) {
        *bad = h_pinned[CLASS_BAD_ORDER];
        return 2;
    }
    if (h_pinned[CLASS_BAD_ARG] != ~0ull) {
        *bad = h_pinned[CLASS_BAD_ARG];
        return 1;
    }
    for (int c = 0; c < 4; c++) counts[c] = h_pinned[CLASS_COUNT0 + c];
    class_counts[GENE_CLASS_NONE] = counts[2] + counts[3];
    class_counts[GENE_CLASS_EXONIC] = h_pinned[CLASS_COUNT0 + 4];
    class_counts[GENE_CLASS_JUNCTION] = h_pinned[CLASS_COUNT0 + 5];
    class_counts[GENE_CLASS_SPANNING] = h_pinned[CLASS_COUNT0 + 6];
    class_counts[GENE_CLASS_INTRONIC] = counts[1];
    return 0;
}

} // namespace umihip
