// Spliced, unspliced and ambiguous molecules per (column, row) pair over the buckets of a batched call
// (umi_velocity_matrix, the program's --velocity), gfx950: the classes of the reads (umi_assign_genes_classes) are
// carried to their molecules, and the molecules counted in three layers, as the sorted triplets umi_count_matrix
// gives.  No counterpart in the reference; tests/velocity_model.py defines it.  Integer work on HBM streams, 64-lane
// waves, no MFMA.
//
// The pair-table pipeline ("The pair-table pipeline"; umihip_pair_table.h) with these parts of its own:
//
//   scatter  a lane per read: its evidence -- 1 for JUNCTION, 2 for SPANNING or INTRONIC, nothing for EXONIC or NONE --
//            is OR-ed onto its molecule's byte of a zeroed evidence array, a byte per entry, at root[read_entry[i]].
//            The OR is atomicOr on the byte's 32-bit word; an integer OR, so the result does not depend on the order.
//            With option "velocity_skip" a lane loads the word first and leaves the atomic out where its bit is set
//            already, and a molecule of 10^5 reads costs a handful of atomics; off by default: at three reads an entry
//            the load costs 5 to 20 % of the call and saves nothing.  A read_entry, read_class or root out of range goes to the control
//            block by atomicMin (the smallest such read is told), and nothing is written for it.
//   reduce   kept[] and the evidence, a queued bucket's a 4-byte word of evidence at a time.  A kept entry counts by
//            its evidence byte: 1 spliced, 2 unspliced, 0 or 3 ambiguous.  Every bucket writes its three counts (16
//            bytes).
//   sum      the runs' scan adds the three counters; a run inside a wave is stored, one that crosses a wave's edge
//            added by atomicAdd onto zeroed outputs.
//
// One synchronisation, at the end, brings nnz, the count of bad ids and the three smallest bad reads.  Workspace:
// umi_count_matrix's per non-empty bucket, and a byte per entry.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

namespace {

constexpr int VEL_THREADS = 256;
constexpr uint32_t VEL_SMALL = 32; // a bucket of more entries is a wave's (umihip_count.hip's COUNT_SMALL)
constexpr uint32_t EV_SPLICED = 1, EV_UNSPLICED = 2;

enum VelCtl : int {
    VEL_BAD_IDS = 0,   // non-empty buckets with an id out of range
    VEL_BAD_ENTRY = 1, // the smallest read with a read_entry out of range (all ones: none)
    VEL_BAD_CLASS = 2, // ... with a read_class above 4
    VEL_BAD_ROOT = 3,  // ... whose entry's root is out of range
    VEL_CTL_COUNT = 4,
};
static_assert(VEL_BAD_IDS == 0, "the bucket walk counts into ctl[0]");

struct VelSum { // what a bucket adds to its pair
    uint32_t spliced, unspliced, ambiguous, pad;
};

struct VelWs : PairTableWs {
    uint32_t *ev; // [ceil(n / 4)] words, a byte per entry
    VelSum *sum;
    size_t ev_bytes, total;
};
VelWs vel_carve(void *ws, uint64_t n, uint32_t m, bool has_idx)
{
    VelWs w;
    Carver c(ws);
    w.ctl = c.take<unsigned long long>(256);
    w.ev_bytes = (((size_t)n + 3) / 4) * 4;
    w.ev = c.take<uint32_t>(w.ev_bytes);
    w.carve_buckets(c, m, has_idx);
    w.sum = c.take<VelSum>((size_t)m * sizeof(VelSum));
    w.carve_temps(c, m, radix_sort_temp_bytes(m));
    w.total = c.o;
    return w;
}

template <bool SKIP_SET>
__global__ __launch_bounds__(VEL_THREADS) void velocity_scatter_kernel(const uint32_t *__restrict__ read_entry,
                                                                       const uint8_t *__restrict__ read_class, uint32_t n_reads,
                                                                       const uint32_t *__restrict__ root, uint64_t n, uint32_t *ev,
                                                                       unsigned long long *ctl)
{
    for (uint64_t i = (uint64_t)blockIdx.x * VEL_THREADS + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * VEL_THREADS) {
        const uint32_t e = read_entry[i];
        if (e == UMI_READ_UNSTAGED) continue;
        if (e >= n) {
            atomicMin(ctl + VEL_BAD_ENTRY, (unsigned long long)i);
            continue;
        }
        const uint32_t cls = read_class[i];
        if (cls > UMI_READ_CLASS_INTRONIC) {
            atomicMin(ctl + VEL_BAD_CLASS, (unsigned long long)i);
            continue;
        }
        const uint32_t r = root[e];
        if (r >= n) {
            atomicMin(ctl + VEL_BAD_ROOT, (unsigned long long)i);
            continue;
        }
        const uint32_t bit = cls == UMI_READ_CLASS_JUNCTION ? EV_SPLICED : cls >= UMI_READ_CLASS_SPANNING ? EV_UNSPLICED : 0u;
        if (!bit) continue;
        const uint32_t mask = bit << (8u * (r & 3u));
        uint32_t *word = ev + (r >> 2);
        // (the load is the device's view, as the atomics': a bit set by another CU is seen; a 0 read too early costs an
        // atomic, never a wrong bit)
        if (SKIP_SET && (__hip_atomic_load(word, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & mask)) continue;
        atomicOr(word, mask);
    }
}

struct VelArgs {
    PairTable t;
    const uint8_t *kept;
    const uint8_t *ev;
    VelSum *sum;
};

// a kept entry into its layer
__device__ __forceinline__ void vel_count(uint32_t kept, uint32_t ev, uint32_t &s, uint32_t &u, uint32_t &a)
{
    if (!kept) return;
    s += ev == EV_SPLICED;
    u += ev == EV_UNSPLICED;
    a += ev != EV_SPLICED && ev != EV_UNSPLICED;
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_reduce_kernel(VelArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    pair_bucket_walk<VEL_THREADS, VEL_SMALL>(
        a.t,
        [&](uint64_t j, uint64_t lo, uint64_t hi, uint32_t, bool) {
            VelSum s{0u, 0u, 0u, 0u};
            for (uint64_t e = lo; e < hi; e++) vel_count(a.kept[e], a.ev[e], s.spliced, s.unspliced, s.ambiguous);
            a.sum[j] = s;
        },
        [&](uint64_t jb, uint64_t lo, uint64_t hi) {
            // the evidence by words from its first aligned entry on (its array begins on a word; kept[] is the caller's
            // and is read by bytes beside it); the entries in front and the rest behind a lane each
            const uint64_t head = std::min<uint64_t>(hi - lo, (4u - (uint32_t)(lo & 3u)) & 3u);
            const uint64_t body = lo + head, words = (hi - body) >> 2, tail = body + 4 * words;
            uint32_t s = 0, u = 0, am = 0;
            if (lane < head) vel_count(a.kept[lo + lane], a.ev[lo + lane], s, u, am);
            for (uint64_t w = lane; w < words; w += 64) {
                const uint64_t e = body + 4 * w;
                const uint32_t we = *(const uint32_t *)(a.ev + e);
                for (int k = 0; k < 4; k++) vel_count(a.kept[e + k], (we >> (8 * k)) & 0xFFu, s, u, am);
            }
            if (tail + lane < hi) vel_count(a.kept[tail + lane], a.ev[tail + lane], s, u, am);
            for (int o = 32; o > 0; o >>= 1) {
                s += __shfl_down(s, o);
                u += __shfl_down(u, o);
                am += __shfl_down(am, o);
            }
            if (lane == 0) a.sum[jb] = VelSum{s, u, am, 0u};
        });
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_sum_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                   const uint64_t *__restrict__ incl, const VelSum *__restrict__ sum,
                                                                   uint32_t m, int rb, uint32_t *__restrict__ out_row,
                                                                   uint32_t *__restrict__ out_col, uint32_t *out_spliced,
                                                                   uint32_t *out_unspliced, uint32_t *out_ambiguous)
{
    const uint64_t i = (uint64_t)blockIdx.x * VEL_THREADS + threadIdx.x;
    const WaveRuns run(incl, i, m);
    VelSum v{0u, 0u, 0u, 0u};
    if (run.valid) v = sum[val[i]];
    uint32_t s = v.spliced, u = v.unspliced, am = v.ambiguous;
    run.scan([](uint32_t x, uint32_t y) { return x + y; }, s, u, am);
    if (run.head) {
        const uint64_t k = key[i];
        out_row[run.slot()] = (uint32_t)(k & ((1ull << rb) - 1ull));
        out_col[run.slot()] = (uint32_t)(k >> rb);
    }
    if (run.tail()) {
        if (run.whole()) {
            out_spliced[run.slot()] = s;
            out_unspliced[run.slot()] = u;
            out_ambiguous[run.slot()] = am;
        } else {
            atomicAdd(out_spliced + run.slot(), s);
            atomicAdd(out_unspliced + run.slot(), u);
            atomicAdd(out_ambiguous + run.slot(), am);
        }
    }
}

} // namespace

size_t velocity_workspace_bytes(uint64_t n, uint32_t m, bool has_idx) { return vel_carve(nullptr, n, m, has_idx).total; }

int velocity_matrix_on_device(void *workspace, const uint32_t *d_read_entry, const uint8_t *d_read_class, uint32_t n_reads,
                              const uint8_t *d_kept, const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx,
                              uint32_t m, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols,
                              uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_spliced, uint32_t *d_out_unspliced,
                              uint32_t *d_out_ambiguous, bool skip_set, uint64_t *nnz, uint64_t *bad_ids, int *bad_kind,
                              uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s)
{
    const VelWs w = vel_carve(workspace, n, m, h_idx != nullptr);
    const int rb = bits_of(n_rows - 1), cb = bits_of(n_cols - 1);
    int r;
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl + VEL_BAD_ENTRY, 0xFF, 3 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ev, 0, w.ev_bytes, s));
    if ((r = pair_table_upload(w, h_off, h_idx, m, s))) return r;
    UMIHIP_TRY_NEG(hipMemsetAsync(d_out_spliced, 0, (size_t)m * 4, s)); // (a run that crosses a wave is added up in place)
    UMIHIP_TRY_NEG(hipMemsetAsync(d_out_unspliced, 0, (size_t)m * 4, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(d_out_ambiguous, 0, (size_t)m * 4, s));
    if (n_reads) {
        const uint32_t grid = std::min(blocks_for(n_reads, VEL_THREADS), n_cus * 16);
        if (skip_set)
            velocity_scatter_kernel<true><<<grid, VEL_THREADS, 0, s>>>(d_read_entry, d_read_class, n_reads, d_root, n, w.ev, w.ctl);
        else
            velocity_scatter_kernel<false><<<grid, VEL_THREADS, 0, s>>>(d_read_entry, d_read_class, n_reads, d_root, n, w.ev, w.ctl);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    const VelArgs a{{w.off, w.idx, d_row, d_col, n_rows, n_cols, m, rb, w.ka, w.va, w.ctl}, d_kept, (const uint8_t *)w.ev, w.sum};
    velocity_reduce_kernel<<<std::min(blocks_for(m, VEL_THREADS), n_cus * 8), VEL_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    const uint64_t *keys;
    const uint32_t *vals;
    uint64_t *incl;
    if ((r = pair_table_sort_and_number<VEL_THREADS>(w, m, rb + cb, blocks_for(m, VEL_THREADS), s, &keys, &vals, &incl))) return r;
    velocity_sum_kernel<<<blocks_for(m, VEL_THREADS), VEL_THREADS, 0, s>>>(keys, vals, incl, w.sum, m, rb, d_out_row, d_out_col,
                                                                         d_out_spliced, d_out_unspliced, d_out_ambiguous);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, w.ctl, VEL_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned + VEL_CTL_COUNT, incl + (m - 1), 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    *bad_ids = h_pinned[VEL_BAD_IDS];
    *nnz = h_pinned[VEL_CTL_COUNT];
    *bad_kind = 0;
    *bad_read = ~0ull;
    for (int k = 1; k <= 3; k++)
        if (h_pinned[k] < *bad_read) {
            *bad_read = h_pinned[k];
            *bad_kind = k;
        }
    return 0;
}

} // namespace umihip
