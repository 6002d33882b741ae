// Reads assigned to genes with their introns (umi_assign_genes_introns, the program's --gene-introns), gfx950.
//
// The rule is STARsolo's GeneFull_ExonOverIntron ("exon-first") or GeneFull ("all") with this project's overlap of one
// base, on gene bodies derived from the taken lines (include/umihip.h has it in full).  Two tiers of tables, built on
// the host by umihip_gene_index.hpp and uploaded by every call: the exons' (umi_assign_genes' own) and the bodies',
// one per strand class each.
//
// Kernel: a read per lane, GENE_THREADS lanes per block, GENE_BLOCKS_PER_CU blocks per CU, a grid stride beyond, as
// umihip_genes.hip.  Phase 1 walks the CIGAR against the exon table; a lane whose verdict still depends on the bodies
// (exon-first: no exon hit; all: not already several) walks it again against the body table -- the CIGAR words are
// in cache from the first walk, and under exon-first a wave of exonic reads never touches the body tables.  The
// lanes of a wave diverge between the phases; they meet again at the stores.
// LDS: the exon tops as in umihip_genes.hip (2 x GENE_TOP_CAP ends, 64 KiB) and, behind them, the body tops, 2 x
// GENE_BODY_TOP_CAP ends (8 KiB): 72 KiB a block, so that two blocks of 16 waves stay resident in a CU's 160 KiB.
// Option "gene_top" 0: neither tier has a top; "gene_body_top" 0 (with gene_top 1): the exon tier alone has one.
//
// What the device finds wrong is told through the control block, as umihip_genes.hip tells it.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_gene_index.hpp"
#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

static_assert(GENE_INTRONS_OFF == UMI_INTRONS_OFF && GENE_INTRONS_EXON_FIRST == UMI_INTRONS_EXON_FIRST &&
                  GENE_INTRONS_ALL == UMI_INTRONS_ALL && GENE_TIER_EXON == UMI_GENE_TIER_EXON && GENE_TIER_INTRON == UMI_GENE_TIER_INTRON,
              "the lookup's modes and tiers are the interface's");
static_assert((2 * (size_t)GENE_TOP_CAP + 2 * (size_t)GENE_BODY_TOP_CAP) * 8 * GENE_BLOCKS_PER_CU <= 160 * 1024,
              "the resident blocks' tops fit a CU's LDS");

namespace {

enum IntronCtl : int {
    INTRON_BAD_ARG = 0,   // smallest read with read_ref < 0 or a bad op code (all ones: none)
    INTRON_BAD_ORDER = 1, // smallest read whose cigar_off falls (all ones: none)
    INTRON_COUNT0 = 2,    // four words: reads assigned by an exon, by an intron, none, several
    INTRON_CTL_COUNT = 6,
};

struct IntronDevTable {
    GeneView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

struct IntronArgs {
    IntronDevTable exon[2], body[2]; // forward / reverse: the tables of a read on + and on -; unstranded: [0] for both
    int n_tab, mode;
    const int32_t *ref, *pos;
    const uint8_t *reverse;
    const uint32_t *cigar;
    const uint64_t *cigar_off;
    uint32_t n;
    int32_t *gene;
    uint8_t *status, *tier;
    unsigned long long *ctl;
};

constexpr uint32_t LDS_BODY0 = 2 * GENE_TOP_CAP; // where the body tops begin

template <bool TOP, bool BTOP> __global__ __launch_bounds__(GENE_THREADS) void gene_introns_kernel(IntronArgs a)
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
    uint32_t seen[4] = {0, 0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * GENE_THREADS + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * GENE_THREADS) {
        const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
        if (c0 > c1 || c1 > total) {
            atomicMin(a.ctl + INTRON_BAD_ORDER, (unsigned long long)i);
            continue;
        }
        const int32_t ref = a.ref[i];
        if (ref < 0 || (c1 > c0 && !a.cigar)) {
            atomicMin(a.ctl + INTRON_BAD_ARG, (unsigned long long)i);
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
            atomicMin(a.ctl + INTRON_BAD_ARG, (unsigned long long)i);
            continue;
        }
        a.gene[i] = g;
        a.status[i] = (uint8_t)st;
        a.tier[i] = (uint8_t)tier;
        seen[0] += st == GENE_READ_ASSIGNED && tier == GENE_TIER_EXON;
        seen[1] += st == GENE_READ_ASSIGNED && tier == GENE_TIER_INTRON;
        seen[2] += st == GENE_READ_NONE;
        seen[3] += st == GENE_READ_SEVERAL;
    }
    // the four counts: summed over the wave, one atomic per wave and counter
    for (int c = 0; c < 4; c++) {
        uint32_t v = seen[c];
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.ctl + INTRON_COUNT0 + c, (unsigned long long)v);
    }
}

size_t table_bytes(const GeneTable &t)
{
    const size_t n = t.end.size();
    return 2 * align256(n * 8 + 8) + align256(n * sizeof(GeneSeg) + 8) + align256(t.top.size() * 8 + 8);
}

// one table into the workspace at p (table_bytes of it), p moved on
int upload(const GeneTable &h, char *&p, IntronDevTable &d, hipStream_t s)
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
    d = {{d_start, d_end, d_seg, (uint32_t)n}, d_top, (uint32_t)h.top.size(), h.top_shift};
    return 0;
}

} // namespace

size_t gene_introns_workspace_bytes(const GeneTable *exons, const GeneTable *bodies, int n_tables)
{
    size_t b = 256;
    for (int t = 0; t < n_tables; t++) b += table_bytes(exons[t]) + table_bytes(bodies[t]);
    return b;
}

int gene_introns_on_device(void *workspace, const GeneTable *exons, const GeneTable *bodies, int n_tables, bool flip, int mode,
                           bool use_top, bool use_body_top, const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse,
                           const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint32_t n_reads, int32_t *d_gene, uint8_t *d_status,
                           uint8_t *d_tier, uint64_t counts[4], uint64_t *bad, uint32_t n_cus, unsigned long long *h_pinned,
                           hipStream_t s)
{
    unsigned long long *ctl = (unsigned long long *)workspace;
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl, 0xFF, INTRON_COUNT0 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl + INTRON_COUNT0, 0, 4 * 8, s));
    IntronDevTable dev_exon[2], dev_body[2];
    char *p = (char *)workspace + 256;
    for (int t = 0; t < n_tables; t++) {
        int r;
        if ((r = upload(exons[t], p, dev_exon[t], s)) || (r = upload(bodies[t], p, dev_body[t], s))) return r;
    }
    IntronArgs a;
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
    a.ctl = ctl;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(((uint64_t)n_reads + GENE_THREADS - 1) / GENE_THREADS, (uint64_t)n_cus * GENE_BLOCKS_PER_CU));
    if (use_top && use_body_top)
        gene_introns_kernel<true, true><<<grid, GENE_THREADS, 0, s>>>(a);
    else if (use_top)
        gene_introns_kernel<true, false><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_introns_kernel<false, false><<<grid, GENE_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, ctl, INTRON_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    if (h_pinned[INTRON_BAD_ORDER] != ~0ull && h_pinned[INTRON_BAD_ORDER] <= h_pinned[INTRON_BAD_ARG]) {
        *bad = h_pinned[INTRON_BAD_ORDER];
        return 2;
    }
    if (h_pinned[INTRON_BAD_ARG] != ~0ull) {
        *bad = h_pinned[INTRON_BAD_ARG];
        return 1;
    }
    for (int c = 0; c < 4; c++) counts[c] = h_pinned[INTRON_COUNT0 + c];
    return 0;
}

} // namespace umihip
