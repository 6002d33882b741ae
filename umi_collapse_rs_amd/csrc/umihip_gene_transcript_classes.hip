// Reads assigned to genes by transcript model, with the gene bodies behind it and the class of every assigned read
// (umi_assign_genes_transcripts_classes, the program's --transcript-introns), gfx950.
//
// The rule (include/umihip.h has it in full; tests/transcript_intron_model.py defines it): a read that fits a
// transcript of one gene is that gene's, tier transcript; a read that fits none falls back to the gene bodies, tier
// body ("exon-first"), or the bodies decide and the fit only names the tier ("all").  Class: tier transcript: JUNCTION
// with two blocks or more, else EXONIC; tier body: INTRONIC, SPANNING, or by its gaps JUNCTION or EXONIC, from the
// cover of the blocks by the gene's exons.  The lookup is transcript_assign_read_tiers (umihip_transcript_index.hpp),
// shared with the CPU test.
//
// Three indices travel with a call, one table of each per strand class: the transcripts' (umihip_transcript_index.hpp),
// the gene bodies' (umihip_gene_index.hpp) and, only where classes are asked for, the exons' overlap table with its
// prefix array of covered bases and the genes' own exons (GeneCover).  All are built on the host and uploaded by the
// call.
//
// Two kernels, each in the siblings' shape (umihip_gene_transcripts.hip, umihip_gene_classes.hip) -- a read per lane,
// GENE_THREADS lanes per block, GENE_BLOCKS_PER_CU blocks per CU, a grid stride beyond.  One kernel over all three phases
// took 67 to 77 vector registers and over 100 scalar ones: at 1,024 lanes a block, two blocks fit a CU only at 64 and
// 96, and the compiler reached them only by spilling.  So the phases run as two passes:
//   fit (phase 1): transcript_assign_read for every read, the transcript tops (2 x GENE_TOP_CAP, 64 KiB) in LDS.  A
//     read whose verdict stands writes it; a read whose verdict still depends on the bodies is put into a queue (its
//     index, whether it fits and whether it has two blocks), one atomic per wave and trip;
//   bodies (phases 2 and 3): transcript_assign_read_bodies for every queued read, the body tops (2 x GENE_BODY_TOP_CAP,
//     8 KiB) in LDS.  The overlap table of phase 3 is searched from global memory, without a top: only a read that a
//     body assigned looks at it.  Under "off" the queue stays empty and the pass is not launched.
// The order of the queue differs from run to run; what is written per read does not.  The counts are kept per wave
// (a trip's verdicts are counted by a ballot) and added with one atomic per wave and counter.  What the device finds
// wrong is told through the control block, as umihip_genes.hip tells it: the first pass looks at every word, and a
// read at fault writes nothing and is not queued.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_pair_table.h"
#include "umihip_transcript_index.hpp"

namespace umihip {

static_assert(GENE_INTRONS_OFF == UMI_INTRONS_OFF && GENE_INTRONS_EXON_FIRST == UMI_INTRONS_EXON_FIRST && GENE_INTRONS_ALL == UMI_INTRONS_ALL,
              "the lookup's modes are the interface's");
static_assert(GENE_TIER_EXON == UMI_GENE_TIER_EXON && GENE_TIER_INTRON == UMI_GENE_TIER_INTRON, "the lookup's tiers are the interface's");
static_assert(2 * (size_t)GENE_TOP_CAP * 8 * GENE_BLOCKS_PER_CU <= 160 * 1024, "the tops of two resident blocks fit a CU's LDS");

namespace {

enum TcCtl : int {
    TC_BAD_ARG = 0,   // smallest read with read_ref < 0 or a bad op code (all ones: none)
    TC_BAD_ORDER = 1, // smallest read whose cigar_off falls (all ones: none)
    TC_COUNT0 = 2,    // seven words: reads assigned by a transcript, by a body, none, several; exonic, junction, spanning
    TC_CTL_COUNT = 9, // (what the host reads)
    TC_QUEUE_N = 9,   // the reads queued for the second pass
};

struct TcTrTable {
    TranscriptView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

struct TcBodyTable {
    GeneView view;
    const uint64_t *top;
    uint32_t n_top;
    int shift;
};

struct TcArgs {
    TcTrTable tr[2]; // forward / reverse: the tables of a read on + and on -; unstranded: [0] for both
    TcBodyTable body[2];
    TrCoverView cover[2]; // (classes alone)
    int n_tab, mode;
    const int32_t *ref, *pos;
    const uint8_t *reverse;
    const uint32_t *cigar;
    const uint64_t *cigar_off;
    uint32_t n;
    int32_t *gene;
    uint8_t *status, *tier, *cls;
    uint32_t *queue; // [n]: TC_Q_* | the read's index
    unsigned long long *ctl;
};

constexpr uint32_t TC_Q_FITS = 1u << 31, TC_Q_SPLICED = 1u << 30, TC_Q_INDEX = TC_Q_SPLICED - 1; // (a call has fewer than 2^30 reads)
constexpr int TC_SKIP = -2, TC_QUEUED = -3; // a read that wrote nothing yet: at fault, or left to the second pass

// The counts are kept per wave in LDS, not in registers: a trip's verdicts are counted by a ballot (the loops run over the
// block's trips, the same for every lane, so a ballot sees the whole wave) and the wave's first lane adds them to its
// wave's seven words.
constexpr int TC_WAVES = GENE_THREADS / 64;

__device__ inline void tc_count(uint32_t *mine, int c, bool p)
{
    const uint32_t v = (uint32_t)__popcll(__ballot(p));
    if ((threadIdx.x & 63) == 0 && v) mine[c] += v;
}

// the counts of one trip (st: GENE_READ_*, or below zero for a lane without a verdict); mine: the wave's words
template <bool CLASSES> __device__ inline void tc_tally(uint32_t *mine, int st, int tier, int cls)
{
    tc_count(mine, 0, st == GENE_READ_ASSIGNED && tier == GENE_TIER_EXON);
    tc_count(mine, 1, st == GENE_READ_ASSIGNED && tier == GENE_TIER_INTRON);
    tc_count(mine, 2, st == GENE_READ_NONE);
    tc_count(mine, 3, st == GENE_READ_SEVERAL);
    if (CLASSES) {
        tc_count(mine, 4, st >= 0 && cls == GENE_CLASS_EXONIC);
        tc_count(mine, 5, st >= 0 && cls == GENE_CLASS_JUNCTION);
        tc_count(mine, 6, st >= 0 && cls == GENE_CLASS_SPANNING);
    }
}

// one atomic per wave and counter (only the wave's first lane has touched its words)
__device__ inline void tc_add(unsigned long long *ctl, const uint32_t *mine)
{
    if ((threadIdx.x & 63) == 0)
        for (int c = 0; c < 7; c++)
            if (mine[c]) atomicAdd(ctl + TC_COUNT0 + c, (unsigned long long)mine[c]);
}

// Phase 1 of one read.  GENE_READ_* where its verdict stands (written); TC_QUEUED with *entry where the bodies have a
// say; TC_SKIP where the read is at fault.
template <bool TOP, bool CLASSES>
__device__ inline int tc_fit_read(const TcArgs &a, const uint64_t *lds_top, uint64_t i, uint64_t total, int *cls, uint32_t *entry)
{
    const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
    if (c0 > c1 || c1 > total) {
        atomicMin(a.ctl + TC_BAD_ORDER, (unsigned long long)i);
        return TC_SKIP;
    }
    const int32_t ref = a.ref[i];
    if (ref < 0 || (c1 > c0 && !a.cigar)) {
        atomicMin(a.ctl + TC_BAD_ARG, (unsigned long long)i);
        return TC_SKIP;
    }
    const int t = a.n_tab == 1 ? 0 : (a.reverse[i] ? 1 : 0);
    const GeneTop top = {lds_top + (TOP ? t * GENE_TOP_CAP : 0), a.tr[t].n_top, a.tr[t].shift};
    int32_t g;
    uint64_t m = 0;
    const int st = transcript_assign_read(a.tr[t].view, TOP ? &top : nullptr, (uint32_t)ref, (int64_t)a.pos[i], a.cigar + c0, c1 - c0, &g,
                                          nullptr, &m);
    if (st == GENE_READ_BAD_OP) {
        atomicMin(a.ctl + TC_BAD_ARG, (unsigned long long)i);
        return TC_SKIP;
    }
    if (transcript_needs_bodies(a.mode, st)) {
        *entry = (uint32_t)i | (st == GENE_READ_ASSIGNED ? TC_Q_FITS : 0) | (m >= 2 ? TC_Q_SPLICED : 0);
        return TC_QUEUED;
    }
    a.gene[i] = g;
    a.status[i] = (uint8_t)st;
    a.tier[i] = (uint8_t)GENE_TIER_EXON;
    if (CLASSES) {
        *cls = st == GENE_READ_ASSIGNED ? transcript_fit_class(m >= 2) : GENE_CLASS_NONE;
        a.cls[i] = (uint8_t)*cls;
    }
    return st;
}

template <bool TOP, bool CLASSES> __global__ __launch_bounds__(GENE_THREADS, 8) void gene_transcript_fit_kernel(TcArgs a)
{
    __shared__ uint64_t lds_top[TOP ? 2 * GENE_TOP_CAP : 1];
    if (TOP) {
        for (int t = 0; t < a.n_tab; t++)
            for (uint32_t j = threadIdx.x; j < a.tr[t].n_top; j += GENE_THREADS) lds_top[t * GENE_TOP_CAP + j] = a.tr[t].top[j];
        __syncthreads();
    }
    __shared__ uint32_t lds_seen[TC_WAVES * 7];
    uint32_t *seen = lds_seen + (threadIdx.x >> 6) * 7;
    if ((threadIdx.x & 63) < 7) seen[threadIdx.x & 63] = 0; // (a wave's words are its own: no barrier)
    const uint64_t total = a.cigar_off[a.n];
    const uint32_t lane = threadIdx.x & 63;
    for (uint64_t base = (uint64_t)blockIdx.x * GENE_THREADS; base < a.n; base += (uint64_t)gridDim.x * GENE_THREADS) {
        const uint64_t i = base + threadIdx.x;
        int st = TC_SKIP, cls = GENE_CLASS_NONE;
        uint32_t entry = 0;
        if (i < a.n) st = tc_fit_read<TOP, CLASSES>(a, lds_top, i, total, &cls, &entry);
        tc_tally<CLASSES>(seen, st, GENE_TIER_EXON, cls);
        // the wave's queued reads take a stretch of the queue, found with one atomic
        const uint64_t queued = __ballot(st == TC_QUEUED);
        if (queued) {
            const int leader = __ffsll((unsigned long long)queued) - 1;
            unsigned long long at = 0;
            if ((int)lane == leader) at = atomicAdd(a.ctl + TC_QUEUE_N, (unsigned long long)__popcll(queued));
            const uint32_t first = __shfl((uint32_t)at, leader, 64);
            if (st == TC_QUEUED) a.queue[first + (uint32_t)__popcll(queued & (((uint64_t)1 << lane) - 1))] = entry;
        }
    }
    tc_add(a.ctl, seen);
}

template <bool BTOP, bool CLASSES> __global__ __launch_bounds__(GENE_THREADS) void gene_transcript_bodies_kernel(TcArgs a)
{
    __shared__ uint64_t lds_top[BTOP ? 2 * GENE_BODY_TOP_CAP : 1];
    if (BTOP) {
        for (int t = 0; t < a.n_tab; t++)
            for (uint32_t j = threadIdx.x; j < a.body[t].n_top; j += GENE_THREADS) lds_top[t * GENE_BODY_TOP_CAP + j] = a.body[t].top[j];
        __syncthreads();
    }
    __shared__ uint32_t lds_seen[TC_WAVES * 7];
    uint32_t *seen = lds_seen + (threadIdx.x >> 6) * 7;
    if ((threadIdx.x & 63) < 7) seen[threadIdx.x & 63] = 0;
    const uint64_t n_queued = a.ctl[TC_QUEUE_N]; // (at most a.n: a read is queued once)
    for (uint64_t base = (uint64_t)blockIdx.x * GENE_THREADS; base < n_queued; base += (uint64_t)gridDim.x * GENE_THREADS) {
        const uint64_t j = base + threadIdx.x;
        int st = TC_SKIP, tier = GENE_TIER_EXON, cls = GENE_CLASS_NONE;
        if (j < n_queued) {
            const uint32_t entry = a.queue[j];
            const uint64_t i = entry & TC_Q_INDEX; // (below a.n, and its offsets have passed the first pass)
            const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
            const int t = a.n_tab == 1 ? 0 : (a.reverse[i] ? 1 : 0);
            const GeneTop top = {lds_top + (BTOP ? t * GENE_BODY_TOP_CAP : 0), a.body[t].n_top, a.body[t].shift};
            int32_t g;
            st = transcript_assign_read_bodies(a.body[t].view, BTOP ? &top : nullptr, CLASSES ? &a.cover[t] : nullptr, (entry & TC_Q_FITS) != 0,
                                               (entry & TC_Q_SPLICED) != 0, (uint32_t)a.ref[i], (int64_t)a.pos[i], a.cigar + c0, c1 - c0, &g,
                                               &tier, &cls);
            a.gene[i] = g;
            a.status[i] = (uint8_t)st;
            a.tier[i] = (uint8_t)tier;
            if (CLASSES) a.cls[i] = (uint8_t)cls;
        }
        tc_tally<CLASSES>(seen, st, tier, cls);
    }
    tc_add(a.ctl, seen);
}

// the arrays of a transcript table in the workspace, in this order, each from a 256-byte boundary (8 bytes spare: none
// is empty)
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

int upload_transcripts(const TranscriptTable &h, char *&p, TcTrTable &d, hipStream_t s)
{
    const TrLayout l = layout_of(h);
    const size_t ni = h.x.size(), nd = h.start.size();
    char *base = p;
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
    d = {{(const TrExon *)(base + l.x), (const TrOf *)(base + l.of), (const uint64_t *)(base + l.start), (const uint64_t *)(base + l.end),
          (const uint64_t *)(base + l.dmax), (const int32_t *)(base + l.label), (const uint32_t *)(base + l.off),
          (const uint32_t *)(base + l.inst), (uint32_t)nd},
         (const uint64_t *)(base + l.top),
         (uint32_t)h.top.size(),
         h.top_shift};
    p += l.bytes;
    return 0;
}

size_t table_bytes(const GeneTable &t)
{
    const size_t n = t.end.size();
    return 2 * align256(n * 8 + 8) + align256(n * sizeof(GeneSeg) + 8) + align256(t.top.size() * 8 + 8);
}

size_t cover_bytes(const GeneCover &c)
{
    const GeneOwn &o = c.own;
    return align256(c.cum.size() * 8 + 8) + 2 * align256(o.start.size() * 8 + 8) + align256(o.off.size() * 4 + 8);
}

// one segment table into the workspace at p (table_bytes of it), p moved on; a table that was not sampled has no top
int upload_table(const GeneTable &h, char *&p, TcBodyTable &d, hipStream_t s)
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
        if (!h.top.empty()) UMIHIP_TRY_NEG(hipMemcpyAsync(d_top, h.top.data(), h.top.size() * 8, hipMemcpyHostToDevice, s));
    }
    d = {{d_start, d_end, d_seg, (uint32_t)n}, d_top, (uint32_t)h.top.size(), h.top_shift};
    return 0;
}

// an overlap table's prefix array and its genes' own exons (cover_bytes of them)
int upload_cover(const GeneCover &c, char *&p, TrCoverView &d, hipStream_t s)
{
    const std::vector<uint64_t> &cum = c.cum;
    const GeneOwn &o = c.own;
    const size_t m = o.start.size();
    uint64_t *d_cum = (uint64_t *)p;
    p += align256(cum.size() * 8 + 8);
    uint64_t *d_start = (uint64_t *)p;
    p += align256(m * 8 + 8);
    uint64_t *d_end = (uint64_t *)p;
    p += align256(m * 8 + 8);
    uint32_t *d_off = (uint32_t *)p;
    p += align256(o.off.size() * 4 + 8);
    if (!cum.empty()) UMIHIP_TRY_NEG(hipMemcpyAsync(d_cum, cum.data(), cum.size() * 8, hipMemcpyHostToDevice, s));
    if (m) {
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_start, o.start.data(), m * 8, hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(d_end, o.end.data(), m * 8, hipMemcpyHostToDevice, s));
    }
    if (!o.off.empty()) UMIHIP_TRY_NEG(hipMemcpyAsync(d_off, o.off.data(), o.off.size() * 4, hipMemcpyHostToDevice, s));
    d.cum = d_cum;
    d.own = {d_start, d_end, d_off};
    return 0;
}

template <bool CLASSES> void launch(bool use_top, bool use_body_top, bool bodies, uint32_t grid, const TcArgs &a, hipStream_t s)
{
    if (use_top)
        gene_transcript_fit_kernel<true, CLASSES><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_transcript_fit_kernel<false, CLASSES><<<grid, GENE_THREADS, 0, s>>>(a);
    if (!bodies) return;
    if (use_top && use_body_top)
        gene_transcript_bodies_kernel<true, CLASSES><<<grid, GENE_THREADS, 0, s>>>(a);
    else
        gene_transcript_bodies_kernel<false, CLASSES><<<grid, GENE_THREADS, 0, s>>>(a);
}

} // namespace

size_t gene_transcript_classes_workspace_bytes(const TranscriptTable *transcripts, const GeneTable *bodies, const GeneTable *exons,
                                               const GeneCover *cover, int n_tables, uint32_t n_reads)
{
    size_t b = 256 + align256((size_t)n_reads * 4 + 8);
    for (int t = 0; t < n_tables; t++) {
        b += layout_of(transcripts[t]).bytes + table_bytes(bodies[t]);
        if (cover) b += table_bytes(exons[t]) + cover_bytes(cover[t]);
    }
    return b;
}

int gene_transcript_classes_on_device(void *workspace, const TranscriptTable *transcripts, const GeneTable *bodies, const GeneTable *exons,
                                      const GeneCover *cover, int n_tables, bool flip, int mode, bool use_top, bool use_body_top,
                                      const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar,
                                      const uint64_t *d_cigar_off, uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier,
                                      uint8_t *d_cls, uint64_t counts[4], uint64_t *class_counts, uint64_t *bad, uint32_t n_cus,
                                      unsigned long long *h_pinned, hipStream_t s)
{
    const bool classes = cover != nullptr;
    unsigned long long *ctl = (unsigned long long *)workspace;
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl, 0xFF, TC_COUNT0 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(ctl + TC_COUNT0, 0, 8 * 8, s)); // (the counts and the queue's length)
    TcTrTable dev_tr[2];
    TcBodyTable dev_body[2], dev_exon[2];
    TrCoverView dev_cover[2];
    char *p = (char *)workspace + 256;
    uint32_t *d_queue = (uint32_t *)p;
    p += align256((size_t)n_reads * 4 + 8);
    for (int t = 0; t < n_tables; t++) {
        int r;
        if ((r = upload_transcripts(transcripts[t], p, dev_tr[t], s)) || (r = upload_table(bodies[t], p, dev_body[t], s))) return r;
        dev_cover[t] = {{nullptr, nullptr, nullptr, 0}, nullptr, {nullptr, nullptr, nullptr}};
        if (classes) {
            if ((r = upload_table(exons[t], p, dev_exon[t], s))) return r;
            dev_cover[t].exons = dev_exon[t].view;
            if ((r = upload_cover(cover[t], p, dev_cover[t], s))) return r;
        }
    }
    TcArgs a;
    a.n_tab = n_tables;
    a.mode = mode;
    // (reverse: a read on + looks among the lines on -)
    const int fwd = n_tables == 2 && flip ? 1 : 0, rev = n_tables == 2 && !flip ? 1 : 0;
    a.tr[0] = dev_tr[fwd];
    a.tr[1] = dev_tr[rev];
    a.body[0] = dev_body[fwd];
    a.body[1] = dev_body[rev];
    a.cover[0] = dev_cover[fwd];
    a.cover[1] = dev_cover[rev];
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
    a.queue = d_queue;
    a.ctl = ctl;
    const uint32_t grid = (uint32_t)std::max<uint64_t>(
        1, std::min<uint64_t>(((uint64_t)n_reads + GENE_THREADS - 1) / GENE_THREADS, (uint64_t)n_cus * GENE_BLOCKS_PER_CU));
    if (classes)
        launch<true>(use_top, use_body_top, mode != GENE_INTRONS_OFF, grid, a, s);
    else
        launch<false>(use_top, use_body_top, mode != GENE_INTRONS_OFF, grid, a, s);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, ctl, TC_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    if (h_pinned[TC_BAD_ORDER] != ~0ull && h_pinned[TC_BAD_ORDER] <= h_pinned[TC_BAD_ARG]) {
        *bad = h_pinned[TC_BAD_ORDER];
        return 2;
    }
    if (h_pinned[TC_BAD_ARG] != ~0ull) {
        *bad = h_pinned[TC_BAD_ARG];
        return 1;
    }
    for (int c = 0; c < 4; c++) counts[c] = h_pinned[TC_COUNT0 + c];
    if (classes) {
        // (a read assigned by a transcript is EXONIC or JUNCTION; by a body, any of the four: INTRONIC is the rest)
        class_counts[GENE_CLASS_NONE] = counts[2] + counts[3];
        class_counts[GENE_CLASS_EXONIC] = h_pinned[TC_COUNT0 + 4];
        class_counts[GENE_CLASS_JUNCTION] = h_pinned[TC_COUNT0 + 5];
        class_counts[GENE_CLASS_SPANNING] = h_pinned[TC_COUNT0 + 6];
        class_counts[GENE_CLASS_INTRONIC] = counts[0] + counts[1] - h_pinned[TC_COUNT0 + 4] - h_pinned[TC_COUNT0 + 5] - h_pinned[TC_COUNT0 + 6];
    }
    return 0;
}

} // namespace umihip
