// Spliced, unspliced and ambiguous molecules per (column, row) pair over the buckets of a batched call
// (umi_velocity_matrix, the program's --velocity), gfx950: the classes of the reads (umi_assign_genes_classes) are
// carried to their molecules, and the molecules counted in three layers, as the sorted triplets umi_count_matrix
// gives.  No counterpart in the reference; tests/velocity_model.py defines it.  Integer work on HBM streams, 64-lane
// waves, no MFMA.
//
// The bucket table is walked on the host exactly as for umi_count_matrix (umihip_count.hip): the m non-empty buckets.
//
//   scatter  a lane per read: its evidence -- 1 for JUNCTION, 2 for SPANNING or INTRONIC, nothing for EXONIC or NONE --
//            is OR-ed onto its molecule's byte of a zeroed evidence array, a byte per entry, at root[read_entry[i]].
//            The OR is atomicOr on the byte's 32-bit word; an integer OR, so the result does not depend on the order.
//            With option "velocity_skip" a lane loads the word first and leaves the atomic out where its bit is set
//            already, and a molecule of 10^5 reads costs a handful of atomics; off by default: at three reads an entry
//            the load costs 5 to 20 % of the call and saves nothing.  A read_entry, read_class or root out of range goes to the control
//            block by atomicMin (the smallest such read is told), and nothing is written for it.
//   reduce   umi_count_matrix's: a bucket of up to VEL_SMALL entries is its lane's, a larger one is queued in LDS
//            and taken by a wave, kept[] and the evidence a 4-byte word at a time.  A kept entry counts by its
//            evidence byte: 1 spliced, 2 unspliced, 0 or 3 ambiguous.  Every bucket writes its three counts (16 bytes),
//            its sort key column << rb | row and its number.
//   sort, heads, sum   as umihip_count.hip, the payload three counters: a segmented inclusive scan over the wave, a
//            run inside a wave stored, one that crosses a wave's edge added by atomicAdd onto zeroed outputs.  No
//            thread walks a run.
//
// One synchronisation, at the end, brings nnz, the count of bad ids and the three smallest bad reads.  Workspace:
// umi_count_matrix's per non-empty bucket, and a byte per entry.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"

namespace umihip {

namespace {

#define VEL_TRY(expr)                            \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

constexpr int VEL_THREADS = 256, VEL_WAVES = VEL_THREADS / 64;
constexpr uint32_t VEL_SMALL = 32; // a bucket of more entries is a wave's (umihip_count.hip's COUNT_SMALL)
constexpr uint32_t EV_SPLICED = 1, EV_UNSPLICED = 2;

enum VelCtl : int {
    VEL_BAD_IDS = 0,   // non-empty buckets with an id out of range
    VEL_BAD_ENTRY = 1, // the smallest read with a read_entry out of range (all ones: none)
    VEL_BAD_CLASS = 2, // ... with a read_class above 4
    VEL_BAD_ROOT = 3,  // ... whose entry's root is out of range
    VEL_CTL_COUNT = 4,
};

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct VelSum { // what a bucket adds to its pair
    uint32_t spliced, unspliced, ambiguous, pad;
};

struct VelWs {
    unsigned long long *ctl;
    uint32_t *ev; // [ceil(n / 4)] words, a byte per entry
    uint64_t *off;
    uint32_t *idx;
    uint64_t *ka, *kb;
    uint32_t *va, *vb;
    VelSum *sum;
    void *radix_tmp, *scan_tmp;
    size_t ev_bytes, radix_bytes, scan_bytes, total;
};
VelWs vel_carve(void *ws, uint64_t n, uint32_t m, bool has_idx)
{
    VelWs w;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = p + o;
        o += align256(bytes);
        return at;
    };
    w.ctl = (unsigned long long *)take(256);
    w.ev_bytes = (((size_t)n + 3) / 4) * 4;
    w.ev = (uint32_t *)take(w.ev_bytes);
    w.off = (uint64_t *)take(((size_t)m + 1) * 8);
    w.idx = has_idx ? (uint32_t *)take((size_t)m * 4) : nullptr;
    w.ka = (uint64_t *)take((size_t)m * 8);
    w.kb = (uint64_t *)take((size_t)m * 8);
    w.va = (uint32_t *)take((size_t)m * 4);
    w.vb = (uint32_t *)take((size_t)m * 4);
    w.sum = (VelSum *)take((size_t)m * sizeof(VelSum));
    w.radix_bytes = radix_sort_temp_bytes(m);
    w.radix_tmp = take(w.radix_bytes);
    w.scan_bytes = scan_temp_bytes(m);
    w.scan_tmp = take(w.scan_bytes);
    w.total = o;
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
    const uint8_t *kept;
    const uint8_t *ev;
    const uint64_t *off;
    const uint32_t *idx; // may be null
    const uint32_t *row, *col;
    uint32_t n_rows, n_cols, m;
    int rb;
    uint64_t *key;
    uint32_t *val;
    VelSum *sum;
    unsigned long long *ctl;
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
    __shared__ uint32_t queue[VEL_THREADS];
    __shared__ uint32_t queued;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t base = (uint64_t)blockIdx.x * VEL_THREADS; base < a.m; base += (uint64_t)gridDim.x * VEL_THREADS) {
        if (tid == 0) queued = 0;
        __syncthreads();
        const uint64_t j = base + tid;
        if (j < a.m) {
            const uint64_t lo = a.off[j], hi = a.off[j + 1];
            const uint32_t b = a.idx ? a.idx[j] : (uint32_t)j;
            const uint32_t row = a.row[b], col = a.col[b];
            const bool bad = row >= a.n_rows || col >= a.n_cols;
            if (bad) atomicAdd(a.ctl + VEL_BAD_IDS, 1ull);
            a.key[j] = bad ? 0ull : ((uint64_t)col << a.rb) | row;
            a.val[j] = (uint32_t)j;
            if (hi - lo <= VEL_SMALL) {
                VelSum s{0u, 0u, 0u, 0u};
                for (uint64_t e = lo; e < hi; e++) vel_count(a.kept[e], a.ev[e], s.spliced, s.unspliced, s.ambiguous);
                a.sum[j] = s;
            } else {
                queue[atomicAdd(&queued, 1u)] = tid;
            }
        }
        __syncthreads();
        const uint32_t nq = queued;
        for (uint32_t t = wave; t < nq; t += VEL_WAVES) {
            const uint64_t jb = base + queue[t];
            const uint64_t lo = a.off[jb], hi = a.off[jb + 1];
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
        }
        __syncthreads(); // (the queue is the next round's as well)
    }
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_heads_kernel(const uint64_t *__restrict__ key, uint32_t m,
                                                                     uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * VEL_THREADS + threadIdx.x;
    if (i < m) flag[i] = i == 0 || key[i] != key[i - 1] ? 1ull : 0ull;
}

__global__ __launch_bounds__(VEL_THREADS) void velocity_sum_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                   const uint64_t *__restrict__ incl, const VelSum *__restrict__ sum,
                                                                   uint32_t m, int rb, uint32_t *__restrict__ out_row,
                                                                   uint32_t *__restrict__ out_col, uint32_t *out_spliced,
                                                                   uint32_t *out_unspliced, uint32_t *out_ambiguous)
{
    const uint64_t i = (uint64_t)blockIdx.x * VEL_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = i < m;
    const uint64_t slot1 = valid ? incl[i] : 0ull; // the slot, counted from 1
    uint64_t prev = __shfl_up(slot1, 1), next = __shfl_down(slot1, 1);
    if (lane == 0) prev = valid && i > 0 ? incl[i - 1] : 0ull;
    if (lane == 63) next = i + 1 < m ? incl[i + 1] : 0ull;
    const bool head = valid && slot1 != prev;
    const bool last = valid && (i + 1 >= m || next != slot1);
    VelSum v{0u, 0u, 0u, 0u};
    if (valid) v = sum[val[i]];
    uint32_t s = v.spliced, u = v.unspliced, am = v.ambiguous;
    for (int d = 1; d < 64; d <<= 1) { // inclusive scan inside runs of one slot
        const uint32_t us = __shfl_up(s, d), uu = __shfl_up(u, d), ua = __shfl_up(am, d);
        const uint64_t uslot = __shfl_up(slot1, d);
        if (lane >= d && uslot == slot1) {
            s += us;
            u += uu;
            am += ua;
        }
    }
    const unsigned long long heads = __ballot(head);
    const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
    if (head) {
        const uint64_t k = key[i];
        out_row[slot1 - 1] = (uint32_t)(k & ((1ull << rb) - 1ull));
        out_col[slot1 - 1] = (uint32_t)(k >> rb);
    }
    if (valid && (last || lane == 63)) { // the run's last lane in this wave holds what the wave adds to it
        if (last && (heads & upto)) {    // (a head at or before this lane: the run began in this wave)
            out_spliced[slot1 - 1] = s;
            out_unspliced[slot1 - 1] = u;
            out_ambiguous[slot1 - 1] = am;
        } else {
            atomicAdd(out_spliced + (slot1 - 1), s);
            atomicAdd(out_unspliced + (slot1 - 1), u);
            atomicAdd(out_ambiguous + (slot1 - 1), am);
        }
    }
}

inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

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
    auto bits = [](uint64_t v) {
        int b = 0;
        while (v >> b) b++;
        return b;
    };
    const int rb = bits(n_rows - 1), cb = bits(n_cols - 1);
    VEL_TRY(hipMemsetAsync(w.ctl, 0, 8, s));
    VEL_TRY(hipMemsetAsync(w.ctl + VEL_BAD_ENTRY, 0xFF, 3 * 8, s));
    VEL_TRY(hipMemsetAsync(w.ev, 0, w.ev_bytes, s));
    VEL_TRY(hipMemcpyAsync(w.off, h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (h_idx) VEL_TRY(hipMemcpyAsync(w.idx, h_idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    VEL_TRY(hipMemsetAsync(d_out_spliced, 0, (size_t)m * 4, s)); // (a run that crosses a wave is added up in place)
    VEL_TRY(hipMemsetAsync(d_out_unspliced, 0, (size_t)m * 4, s));
    VEL_TRY(hipMemsetAsync(d_out_ambiguous, 0, (size_t)m * 4, s));
    if (n_reads) {
        const uint32_t grid = std::min(blocks_for(n_reads, VEL_THREADS), n_cus * 16);
        if (skip_set)
            velocity_scatter_kernel<true><<<grid, VEL_THREADS, 0, s>>>(d_read_entry, d_read_class, n_reads, d_root, n, w.ev, w.ctl);
        else
            velocity_scatter_kernel<false><<<grid, VEL_THREADS, 0, s>>>(d_read_entry, d_read_class, n_reads, d_root, n, w.ev, w.ctl);
        VEL_TRY(hipGetLastError());
    }
    VelArgs a;
    a.kept = d_kept;
    a.ev = (const uint8_t *)w.ev;
    a.off = w.off;
    a.idx = w.idx;
    a.row = d_row;
    a.col = d_col;
    a.n_rows = n_rows;
    a.n_cols = n_cols;
    a.m = m;
    a.rb = rb;
    a.key = w.ka;
    a.val = w.va;
    a.sum = w.sum;
    a.ctl = w.ctl;
    velocity_reduce_kernel<<<std::min(blocks_for(m, VEL_THREADS), n_cus * 8), VEL_THREADS, 0, s>>>(a);
    VEL_TRY(hipGetLastError());
    bool in_b = false;
    VEL_TRY(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, m, 0, rb + cb, w.radix_tmp, w.radix_bytes, &in_b, s));
    const uint64_t *keys = in_b ? w.kb : w.ka;
    const uint32_t *vals = in_b ? w.vb : w.va;
    uint64_t *flag = in_b ? w.ka : w.kb, *incl = w.off; // (the offsets have been read)
    velocity_heads_kernel<<<blocks_for(m, VEL_THREADS), VEL_THREADS, 0, s>>>(keys, m, flag);
    VEL_TRY(hipGetLastError());
    VEL_TRY(scan_inclusive_u64(flag, incl, m, w.scan_tmp, w.scan_bytes, s));
    velocity_sum_kernel<<<blocks_for(m, VEL_THREADS), VEL_THREADS, 0, s>>>(keys, vals, incl, w.sum, m, rb, d_out_row, d_out_col,
                                                                         d_out_spliced, d_out_unspliced, d_out_ambiguous);
    VEL_TRY(hipGetLastError());
    VEL_TRY(hipMemcpyAsync(h_pinned, w.ctl, VEL_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    VEL_TRY(hipMemcpyAsync(h_pinned + VEL_CTL_COUNT, incl + (m - 1), 8, hipMemcpyDeviceToHost, s));
    VEL_TRY(hipStreamSynchronize(s));
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

#undef VEL_TRY

} // namespace umihip
