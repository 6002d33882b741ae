// Reads assigned to genes from an annotation (umi_assign_genes, the program's --gene-annotation), gfx950.
//
// The rule is featureCounts' default (-t exon -g gene_id, minimum overlap 1, no -O, single-end; include/umihip.h
// has it in full).  The index -- the covered elementary segments of the annotation, one table per strand
// class -- is built on the host (umihip_gene_index.hpp, which also holds the lookup the kernel runs) and
// uploaded by every call.
//
// Kernel: a read per lane, GENE_THREADS lanes per block, GENE_BLOCKS_PER_CU blocks per CU, a grid stride
// beyond.  A lane walks its read's CIGAR (usually 1 to 5 words), closes a block at every N and at the end,
// and looks each block up: a binary search for the first segment that ends behind the block's start, a few
// doubling steps for the last that starts before its end, one 8-byte load for label and run.  With the top
// (option "gene_top", the default) a block first copies every 2^shift-th end of each table into LDS, at most
// GENE_TOP_CAP per table (2 x 32 KiB: two blocks of 16 waves stay resident per CU); the first steps of a
// search are then LDS reads and the last `shift` touch one or two cache lines of the chunk.  Coordinate-sorted
// input keeps a wave's lanes in neighbouring segments.  Integer work only.
//
// What the device finds wrong is told through the control block: the smallest read with read_ref < 0 or a
// CIGAR op code above 8, the smallest read whose cigar_off falls (or lies beyond cigar_off[n_reads]: nothing is
// read outside the CIGAR array).  Such a read writes nothing; the host looks once, at the end.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_gene_index.hpp"
#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

static_assert(GENE_READ_ASSIGNED == UMI_GENE_ASSIGNED && GENE_READ_NONE == UMI_GENE_NONE && GENE_READ_SEVERAL == UMI_GENE_SEVERAL,
              "the lookup's verdicts are the interface's");

namespace {

enum GeneCtl : int {
    GENE_BAD_ARG = 0,   // smallest read with read_ref < 0 or a bad op code (all ones: none)
    GENE_BAD_ORDER = 1, // smallest read whose cigar_off falls (all ones: none)
    GENE_STATUS0 = 2,   // three words: reads assigned, none, several
    GENE_CTL_COUNT = 5,
};

struct GeneDevTable {
    GeneView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

struct GeneArgs {
    GeneDevTable tab[2]; // forward / reverse: the table of a read on + and on -; unstranded: [0] for both
    int n_tab;
    const int32_t *ref, *pos;
    const uint8_t *reverse;
    const uint32_t *cigar;
    const uint64_t *cigar_off;
    uint32_t n;
    int32_t *gene;
    uint8_t *status;
    unsigned long long *ctl;
};

template <bool TOP> __global__ __launch_bounds__(GENE_THREADS) void gene_assign_kernel(GeneArgs a)
{
    __shared__ uint64_t lds_top[TOP ? 2 * GENE_TOP_CAP : 1];
    if (TOP) {
        for (int t = 0; t < a.n_tab; t++)
            for (uint32_t j = threadIdx.x; j < a.tab[t].n_top; j += GENE_THREADS) lds_top[t * GENE_TOP_CAP + j] = a.tab[t].top[j];
        __syncthreads();
    }
    const uint64_t total = a.cigar_off[a.n];
    uint32_t seen[3] = {0, 0, 0};
    for (uint64_t i = (uint64_t)blockIdx.x * GENE_THREADS + threadIdx.x; i < a.n; i += (uint64_t)gridDim.x * GENE_THREADS) {
        const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
        if (c0 > c1 || c1 > total) {
            atomicMin(a.ctl + GENE_BAD_ORDER, (unsigned long long)i);
            continue;
        }
        const int32_t ref = a.ref[i];
        if (ref < 0 || (c1 > c0 && !a.cigar)) {
            atomicMin(a.ctl + GENE_BAD_ARG, (unsigned long long)i);
            continue;
        }
        const int t = a.n_tab == 1 ? 0 : (a.reverse[i] ? 1 : 0);
        const GeneTop top = {lds_top + (TOP ? t * GENE_TOP_CAP : 0), a.tab[t].n_top, a.tab[t].shift};
        int32_t g;
        const int st = gene_assign_read(a.tab[t].view, TOP ? &top : nullptr, (uint32_t)ref, (int64_t)a.pos[i], a.cigar + c0, c1 - c0, &g);
        if (st == GENE_READ_BAD_OP) {
            atomicMin(a.ctl + GENE_BAD_ARG, (unsigned long long)i);
            continue;
        }
        a.gene[i] = g;
        a.status[i] = (uint8_t)st;
        seen[0] += st == GENE_READ_ASSIGNED;
        seen[1] += st == GENE_READ_NONE;
        seen[2] += st == GENE_READ_SEVERAL;
    }
    // the three counts: summed over the wave, one atomic per wave and status
    for (int c = 0; c < 3; c++) {
        uint32_t v = seen[c];
        for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d, 64);
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.ctl + GENE_STATUS0 + c, (unsigned long long)v);
    }
}

size_t table_bytes(const GeneTable &t)
{
    const size_t n = t.end.size();
    return 2 * align256(n * 8 + 8) + align256(n * sizeof(GeneSeg) + 8) + align256(t.top.size() * 8 + 8);
}

} // namespace

size_t genes_workspace_bytes(const GeneTable *tables, int n_tables)
{
    size_t b = 256;
    for (int t = 0; t < n_tables; t++) b += table_bytes(tables[t]);
    return b;
}

int genes_on_device(void *workspace, const GeneTable *tables, int n_tables, bool flip, bool use_top, const int32_t *d_ref,
                    const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                    uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint64_t counts[3], uint64_t *bad, uint32_t n_cus,
                    unsigned long long *h_pinned, hipStream_t s)
{
    unsigned long long *ctl = (unsigned long long *)workspace;
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl, 0xFF, GENE_STATUS0 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl + GENE_STATUS0, 0, 3 * 8, s));
    GeneDevTable dev[2];
    char *p = (char *)workspace + 256;
    for (int t = 0; t < n_tables; t++) {
        const GeneTable &h = tables[t];
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
        dev[t] = {{d_start, d_end, d_seg, (uint32_t)n}, d_top, (uint32_t)h.top.size(), h.top_shift};
    }
    GeneArgs a;
    a.n_tab = n_tables;
    // (reverse: a read on + looks among the exons on -)
    a.tab[0] = dev[n_tables == 2 && flip ? 1 : 0];
    a.tab[1] = dev[n_tables == 2 && !flip ? 1 : 0];
    a.ref = d_ref;
    a.pos = d_pos;
    a.reverse = d_reverse;
    a.cigar = d_cigar;
    a.cigar_off = d_cigar_off;
    a.n = n_reads;
    a.gene = d_gene;
    a.status = d_status;
    a.ctl = ctl;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(((uint64_t)n_reads + GENE_THREADS - 1) / GENE_THREADS, (uint64_t)n_cus * GENE_BLOCKS_PER_CU));
    if (use_top)
        gene_assign_kernel<true><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_assign_kernel<false><<<grid, GENE_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, ctl, GENE_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    if (h_pinned[GENE_BAD_ORDER] != ~0ull && h_pinned[GENE_BAD_ORDER] <= h_pinned[GENE_BAD_ARG]) {
        *bad = h_pinned[GENE_BAD_ORDER];
        return 2;
    }
    if (h_pinned[GENE_BAD_ARG] != ~0ull) {
        *bad = h_pinned[GENE_BAD_ARG];
        return 1;
    }
    for (int c = 0; c < 3; c++) counts[c] = h_pinned[GENE_STATUS0 + c];
    return 0;
}

} // namespace umihip
