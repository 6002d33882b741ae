// Reads assigned to genes by transcript model (umi_assign_genes_transcripts, the program's --gene-rule transcript),
// gfx950.
//
// The rule is STARsolo's Gene (include/umihip.h has it in full): a read belongs to a gene when it fits one of the
// gene's transcripts, every block inside an exon and every N from one exon's end to the next one's start.  The index
// -- per strand class the transcripts' united exons, the distinct exons among them and each one's instances -- is
// built on the host (umihip_transcript_index.hpp, which also holds the lookup the kernel runs) and uploaded by every
// call.
//
// Kernel: gene_assign_kernel's shape (umihip_genes.hip) -- a read per lane, GENE_THREADS lanes per block,
// GENE_BLOCKS_PER_CU blocks per CU, a grid stride beyond.  A lane walks its read's CIGAR once for the op codes, the
// number of blocks and the first block, finds the last distinct exon that starts at or before that block by a binary
// search and steps back while the running maximum of the ends still reaches the block's end.  A one-block read takes
// the labels of the exons that contain it; a spliced read walks its CIGAR again, from memory, against the following
// instances of every transcript that has the first block's exon (nothing of the CIGAR is kept in per-lane arrays).
// With the top (option "gene_top", the default) a block first copies every 2^shift-th start of each table into LDS,
// at most GENE_TOP_CAP per table (2 x 32 KiB: two blocks of 16 waves stay resident per CU).  Integer work only.
//
// What the device finds wrong is told through the control block, as umihip_genes.hip tells it: the smallest read with
// read_ref < 0 or a CIGAR op code above 8, the smallest read whose cigar_off falls (or lies beyond cigar_off[n_reads]:
// nothing is read outside the CIGAR array).  Such a read writes nothing; the host looks once, at the end.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_pair_table.h"
#include "umihip_transcript_index.hpp"

namespace umihip {

static_assert(GENE_READ_ASSIGNED == UMI_GENE_ASSIGNED && GENE_READ_NONE == UMI_GENE_NONE && GENE_READ_SEVERAL == UMI_GENE_SEVERAL,
              "the lookup's verdicts are the interface's");
static_assert(2 * (size_t)GENE_TOP_CAP * 8 * GENE_BLOCKS_PER_CU <= 160 * 1024, "the tops of two resident blocks fit a CU's LDS");

namespace {

enum TrCtl : int {
    TR_CTL_BAD_ARG = 0,   // smallest read with read_ref < 0 or a bad op code (all ones: none)
    TR_CTL_BAD_ORDER = 1, // smallest read whose cigar_off falls (all ones: none)
    TR_CTL_STATUS0 = 2,   // three words: reads assigned, none, several
    TR_CTL_COUNT = 5,
};

struct TrDevTable {
    TranscriptView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

struct TrArgs {
    TrDevTable tab[2]; // forward / reverse: the table of a read on + and on -; unstranded: [0] for both
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

template <bool TOP> __global__ __launch_bounds__(GENE_THREADS) void gene_transcripts_kernel(TrArgs a)
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
            atomicMin(a.ctl + TR_CTL_BAD_ORDER, (unsigned long long)i);
            continue;
        }
        const int32_t ref = a.ref[i];
        if (ref < 0 || (c1 > c0 && !a.cigar)) {
            atomicMin(a.ctl + TR_CTL_BAD_ARG, (unsigned long long)i);
            continue;
        }
        const int t = a.n_tab == 1 ? 0 : (a.reverse[i] ? 1 : 0);
        const GeneTop top = {lds_top + (TOP ? t * GENE_TOP_CAP : 0), a.tab[t].n_top, a.tab[t].shift};
        int32_t g;
        const int st = transcript_assign_read(a.tab[t].view, TOP ? &top : nullptr, (uint32_t)ref, (int64_t)a.pos[i], a.cigar + c0, c1 - c0,
                                              &g, nullptr);
        if (st == GENE_READ_BAD_OP) {
            atomicMin(a.ctl + TR_CTL_BAD_ARG, (unsigned long long)i);
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
        if ((threadIdx.x & 63) == 0 && v) atomicAdd(a.ctl + TR_CTL_STATUS0 + c, (unsigned long long)v);
    }
}

// the arrays of a table in the workspace, in this order, each from a 256-byte boundary (8 bytes spare: none is empty)
struct TrLayout {
    size_t x, of, start, end, dmax, label, off, inst, top, bytes;
};

TrLayout layout_of(const TranscriptTable &t)
{
    TrLayout l;
    size_t p = 0;
    const size_t ni = t.x.size(), nd = t.start.size();
    l.x = p, p += align256(ni * sizeof(TrExon) + 8);
    l.of = p, p += align256(ni * sizeof(TrOf) + 8);
    l.start = p, p += align256(nd * 8 + 8);
    l.end = p, p += align256(nd * 8 + 8);
    l.dmax = p, p += align256(nd * 8 + 8);
    l.label = p, p += align256(nd * 4 + 8);
    l.off = p, p += align256((nd + 1) * 4 + 8);
    l.inst = p, p += align256(ni * 4 + 8);
    l.top = p, p += align256(t.top.size() * 8 + 8);
    l.bytes = p;
    return l;
}

} // namespace

size_t gene_transcripts_workspace_bytes(const TranscriptTable *tables, int n_tables)
{
    size_t b = 256;
    for (int t = 0; t < n_tables; t++) b += layout_of(tables[t]).bytes;
    return b;
}

int gene_transcripts_on_device(void *workspace, const TranscriptTable *tables, int n_tables, bool flip, bool use_top, const int32_t *d_ref,
                               const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                               uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint64_t counts[3], uint64_t *bad, uint32_t n_cus,
                               unsigned long long *h_pinned, hipStream_t s)
{
    unsigned long long *ctl = (unsigned long long *)workspace;
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl, 0xFF, TR_CTL_STATUS0 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl + TR_CTL_STATUS0, 0, 3 * 8, s));
    TrDevTable dev[2];
    char *base = (char *)workspace + 256;
    for (int t = 0; t < n_tables; t++) {
        const TranscriptTable &h = tables[t];
        const TrLayout l = layout_of(h);
        const size_t ni = h.x.size(), nd = h.start.size();
        if (nd) {
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.x, h.x.data(), ni * sizeof(TrExon), hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.of, h.of.data(), ni * sizeof(TrOf), hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.start, h.start.data(), nd * 8, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.end, h.end.data(), nd * 8, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.dmax, h.dmax.data(), nd * 8, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.label, h.label.data(), nd * 4, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.off, h.off.data(), (nd + 1) * 4, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.inst, h.inst.data(), ni * 4, hipMemcpyHostToDevice, s));
            UMIHIP_TRY_NEG(hipMemcpyAsync(base + l.top, h.top.data(), h.top.size() * 8, hipMemcpyHostToDevice, s));
        }
        dev[t] = {{(const TrExon *)(base + l.x), (const TrOf *)(base + l.of), (const uint64_t *)(base + l.start),
                   (const uint64_t *)(base + l.end), (const uint64_t *)(base + l.dmax), (const int32_t *)(base + l.label),
                   (const uint32_t *)(base + l.off), (const uint32_t *)(base + l.inst), (uint32_t)nd},
                  (const uint64_t *)(base + l.top),
                  (uint32_t)h.top.size(),
                  h.top_shift};
        base += l.bytes;
    }
    TrArgs a;
    a.n_tab = n_tables;
    // (reverse: a read on + looks among the transcripts on -)
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
        gene_transcripts_kernel<true><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_transcripts_kernel<false><<<grid, GENE_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, ctl, TR_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    if (h_pinned[TR_CTL_BAD_ORDER] != ~0ull && h_pinned[TR_CTL_BAD_ORDER] <= h_pinned[TR_CTL_BAD_ARG]) {
        *bad = h_pinned[TR_CTL_BAD_ORDER];
        return 2;
    }
    if (h_pinned[TR_CTL_BAD_ARG] != ~0ull) {
        *bad = h_pinned[TR_CTL_BAD_ARG];
        return 1;
    }
    for (int c = 0; c < 3; c++) counts[c] = h_pinned[TR_CTL_STATUS0 + c];
    return 0;
}

} // namespace umihip
