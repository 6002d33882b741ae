// Molecules and reads per (column, row) pair over the buckets of a batched call (umi_count_matrix, the
// program's --count-matrix), gfx950: kept[] / freq[] of a call and every bucket's row (gene) and column (cell)
// become the sorted triplets of a sparse matrix.  No counterpart in the reference; tests/gene_model.py
// (count_model) defines it.  Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The host walks the bucket table once (it has to copy it to its pinned staging anyway): the table must not
// fall, and its empty buckets are left out there -- a run of equal offsets is one offset, so the m non-empty
// buckets are the m + 1 different values, with a list of their bucket numbers only where something was left
// out.  Everything below works on those m buckets (none: no kernel is launched).
//
//   reduce   one pass over the buckets, 256 per block at a time.  A bucket of up to COUNT_SMALL entries is its
//            lane's: it walks its few neighbouring entries (the typical bucket has one to three; the lanes of a
//            wave read one stretch of kept[] and freq[] between them).  A larger one is queued in LDS and taken by
//            one of the block's four waves: the lanes stride over kept[] a 4-byte word at a time from the first
//            aligned entry on (the entries before it and after the last whole word a lane each), freq[] beside it,
//            and the wave adds up with __shfl_down.  Every bucket writes (reads, molecules) -- 16 bytes -- its sort
//            key column << rb | row (rb = bits of n_rows - 1) and its number as the sort's value; an id out of
//            range counts into the control word and gives key 0.  No global atomic per entry or per bucket.
//   sort     radix_sort_pairs_u64 over the rb + cb bits that are in use (umihip_radix.hip).
//   heads    flag[i] = the sorted key differs from its predecessor's; scan_inclusive_u64 over the flags numbers
//            the output slots (nnz = the last value).
//   sum      a lane per sorted bucket gathers its 16 bytes; a segmented inclusive scan over the wave (six
//            __shfl_up steps that add only across equal slots) leaves a run's sum in its last lane there.  A run
//            that begins and ends inside the wave is stored; one that crosses a wave's edge is added with
//            atomicAdd (u32 molecules, 64-bit reads) onto the zeroed outputs -- one atomic pair per wave and
//            run, integer sums, so the result does not depend on the order.  No thread walks a run.
//
// One synchronisation, at the end, brings nnz and the count of bad ids.  Workspace per non-empty bucket:
// offsets 8 (the slots' scan reuses them), keys 2 x 8 (the buffer the sort leaves free holds the flags), values
// 2 x 4, sums 16, bucket numbers 4 where buckets were left out: 48 to 52 bytes, and the sort's tables.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"

namespace umihip {

namespace {

#define COUNT_TRY(expr)                          \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

constexpr int COUNT_THREADS = 256, COUNT_WAVES = COUNT_THREADS / 64;
constexpr uint32_t COUNT_SMALL = 32; // a bucket of more entries is a wave's

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

struct CountSum { // what a bucket adds to its pair
    unsigned long long reads;
    uint32_t molecules, pad;
};

struct CountWs {
    unsigned long long *ctl; // [0] non-empty buckets with an id out of range
    uint64_t *off;           // [m + 1] the non-empty buckets' offsets; then the inclusive scan of the head flags
    uint32_t *idx;           // [m] their bucket numbers (null: nothing was left out)
    uint64_t *ka, *kb;
    uint32_t *va, *vb;
    CountSum *sum;
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes, total;
};
CountWs count_carve(void *ws, uint32_t m, bool has_idx)
{
    CountWs w;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = p + o;
        o += align256(bytes);
        return at;
    };
    w.ctl = (unsigned long long *)take(256);
    w.off = (uint64_t *)take(((size_t)m + 1) * 8);
    w.idx = has_idx ? (uint32_t *)take((size_t)m * 4) : nullptr;
    w.ka = (uint64_t *)take((size_t)m * 8);
    w.kb = (uint64_t *)take((size_t)m * 8);
    w.va = (uint32_t *)take((size_t)m * 4);
    w.vb = (uint32_t *)take((size_t)m * 4);
    w.sum = (CountSum *)take((size_t)m * sizeof(CountSum));
    w.radix_bytes = radix_sort_temp_bytes(m);
    w.radix_tmp = take(w.radix_bytes);
    w.scan_bytes = scan_temp_bytes(m);
    w.scan_tmp = take(w.scan_bytes);
    w.total = o;
    return w;
}

struct CountArgs {
    const uint8_t *kept;
    const int32_t *freq;
    const uint64_t *off;
    const uint32_t *idx; // may be null
    const uint32_t *row, *col;
    uint32_t n_rows, n_cols, m;
    int rb;
    uint64_t *key;
    uint32_t *val;
    CountSum *sum;
    unsigned long long *ctl;
};

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    return ((w & 0xFFu) != 0u) + ((w & 0xFF00u) != 0u) + ((w & 0xFF0000u) != 0u) + ((w & 0xFF000000u) != 0u);
}

__global__ __launch_bounds__(COUNT_THREADS) void count_reduce_kernel(CountArgs a)
{
    __shared__ uint32_t queue[COUNT_THREADS];
    __shared__ uint32_t queued;
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    for (uint64_t base = (uint64_t)blockIdx.x * COUNT_THREADS; base < a.m; base += (uint64_t)gridDim.x * COUNT_THREADS) {
        if (tid == 0) queued = 0;
        __syncthreads();
        const uint64_t j = base + tid;
        if (j < a.m) {
            const uint64_t lo = a.off[j], hi = a.off[j + 1];
            const uint32_t b = a.idx ? a.idx[j] : (uint32_t)j;
            const uint32_t row = a.row[b], col = a.col[b];
            const bool bad = row >= a.n_rows || col >= a.n_cols;
            if (bad) atomicAdd(a.ctl, 1ull);
            a.key[j] = bad ? 0ull : ((uint64_t)col << a.rb) | row;
            a.val[j] = (uint32_t)j;
            if (hi - lo <= COUNT_SMALL) {
                CountSum s{0ull, 0u, 0u};
                for (uint64_t e = lo; e < hi; e++) {
                    s.molecules += a.kept[e] != 0;
                    s.reads += (unsigned long long)(long long)a.freq[e];
                }
                a.sum[j] = s;
            } else {
                queue[atomicAdd(&queued, 1u)] = tid;
            }
        }
        __syncthreads();
        const uint32_t nq = queued;
        for (uint32_t t = wave; t < nq; t += COUNT_WAVES) {
            const uint64_t jb = base + queue[t];
            const uint64_t lo = a.off[jb], hi = a.off[jb + 1];
            // kept[] by words from the first aligned entry on; the entries in front and the rest behind a lane each
            const uint64_t head = std::min<uint64_t>(hi - lo, (4u - (uint32_t)((uintptr_t)(a.kept + lo) & 3u)) & 3u);
            const uint64_t body = lo + head, words = (hi - body) >> 2, tail = body + 4 * words;
            uint32_t mol = 0;
            unsigned long long reads = 0;
            if (lane < head) {
                mol += a.kept[lo + lane] != 0;
                reads += (unsigned long long)(long long)a.freq[lo + lane];
            }
            for (uint64_t w = lane; w < words; w += 64) {
                const uint64_t e = body + 4 * w;
                mol += nonzero_bytes(*(const uint32_t *)(a.kept + e));
                reads += (unsigned long long)((long long)a.freq[e] + (long long)a.freq[e + 1] + (long long)a.freq[e + 2] +
                                              (long long)a.freq[e + 3]);
            }
            if (tail + lane < hi) {
                mol += a.kept[tail + lane] != 0;
                reads += (unsigned long long)(long long)a.freq[tail + lane];
            }
            for (int o = 32; o > 0; o >>= 1) {
                mol += __shfl_down(mol, o);
                reads += __shfl_down(reads, o);
            }
            if (lane == 0) a.sum[jb] = CountSum{reads, mol, 0u};
        }
        __syncthreads(); // (the queue is the next round's as well)
    }
}

__global__ __launch_bounds__(COUNT_THREADS) void count_heads_kernel(const uint64_t *__restrict__ key, uint32_t m,
                                                                    uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * COUNT_THREADS + threadIdx.x;
    if (i < m) flag[i] = i == 0 || key[i] != key[i - 1] ? 1ull : 0ull;
}

__global__ __launch_bounds__(COUNT_THREADS) void count_sum_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                  const uint64_t *__restrict__ incl, const CountSum *__restrict__ sum,
                                                                  uint32_t m, int rb, uint32_t *__restrict__ out_row,
                                                                  uint32_t *__restrict__ out_col, uint32_t *out_molecules,
                                                                  unsigned long long *out_reads)
{
    const uint64_t i = (uint64_t)blockIdx.x * COUNT_THREADS + threadIdx.x;
    const int lane = (int)(threadIdx.x & 63u);
    const bool valid = i < m;
    const uint64_t slot1 = valid ? incl[i] : 0ull; // the slot, counted from 1
    uint64_t prev = __shfl_up(slot1, 1), next = __shfl_down(slot1, 1);
    if (lane == 0) prev = valid && i > 0 ? incl[i - 1] : 0ull;
    if (lane == 63) next = i + 1 < m ? incl[i + 1] : 0ull;
    const bool head = valid && slot1 != prev;                   // (slot numbers start at 1: the first bucket differs from 0)
    const bool last = valid && (i + 1 >= m || next != slot1);   // the run ends here
    CountSum s{0ull, 0u, 0u};
    if (valid) s = sum[val[i]];
    uint32_t mol = s.molecules;
    unsigned long long reads = s.reads;
    for (int d = 1; d < 64; d <<= 1) { // inclusive scan inside runs of one slot
        const uint32_t um = __shfl_up(mol, d);
        const unsigned long long ur = __shfl_up(reads, d);
        const uint64_t us = __shfl_up(slot1, d);
        if (lane >= d && us == slot1) {
            mol += um;
            reads += ur;
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
            out_molecules[slot1 - 1] = mol;
            out_reads[slot1 - 1] = reads;
        } else {
            atomicAdd(out_molecules + (slot1 - 1), mol);
            atomicAdd(out_reads + (slot1 - 1), reads);
        }
    }
}

inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }

} // namespace

size_t count_workspace_bytes(uint32_t m, bool has_idx) { return count_carve(nullptr, m, has_idx).total; }

int count_matrix_on_device(void *workspace, const uint8_t *d_kept, const int32_t *d_freq, const uint64_t *h_off,
                           const uint32_t *h_idx, uint32_t m, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows,
                           uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules,
                           uint64_t *d_out_reads, uint64_t *nnz, uint64_t *bad_ids, uint32_t n_cus, unsigned long long *h_pinned,
                           hipStream_t s)
{
    const CountWs w = count_carve(workspace, m, h_idx != nullptr);
    auto bits = [](uint64_t v) { // (64 bits wide: a shift by 32 is defined)
        int b = 0;
        while (v >> b) b++; // (v < 2^32, b <= 32)
        return b;
    };
    const int rb = bits(n_rows - 1), cb = bits(n_cols - 1);
    COUNT_TRY(hipMemsetAsync(w.ctl, 0, 256, s));
    COUNT_TRY(hipMemcpyAsync(w.off, h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (h_idx) COUNT_TRY(hipMemcpyAsync(w.idx, h_idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    COUNT_TRY(hipMemsetAsync(d_out_molecules, 0, (size_t)m * 4, s)); // (a run that crosses a wave is added up in place)
    COUNT_TRY(hipMemsetAsync(d_out_reads, 0, (size_t)m * 8, s));
    CountArgs a;
    a.kept = d_kept;
    a.freq = d_freq;
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
    count_reduce_kernel<<<std::min(blocks_for(m, COUNT_THREADS), n_cus * 8), COUNT_THREADS, 0, s>>>(a);
    COUNT_TRY(hipGetLastError());
    bool in_b = false;
    COUNT_TRY(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, m, 0, rb + cb, w.radix_tmp, w.radix_bytes, &in_b, s));
    const uint64_t *keys = in_b ? w.kb : w.ka;
    const uint32_t *vals = in_b ? w.vb : w.va;
    uint64_t *flag = in_b ? w.ka : w.kb, *incl = w.off; // (the offsets have been read)
    count_heads_kernel<<<blocks_for(m, COUNT_THREADS), COUNT_THREADS, 0, s>>>(keys, m, flag);
    COUNT_TRY(hipGetLastError());
    COUNT_TRY(scan_inclusive_u64(flag, incl, m, w.scan_tmp, w.scan_bytes, s));
    count_sum_kernel<<<blocks_for(m, COUNT_THREADS), COUNT_THREADS, 0, s>>>(keys, vals, incl, w.sum, m, rb, d_out_row, d_out_col,
                                                                           d_out_molecules, (unsigned long long *)d_out_reads);
    COUNT_TRY(hipGetLastError());
    COUNT_TRY(hipMemcpyAsync(h_pinned, w.ctl, 8, hipMemcpyDeviceToHost, s));
    COUNT_TRY(hipMemcpyAsync(h_pinned + 1, incl + (m - 1), 8, hipMemcpyDeviceToHost, s));
    COUNT_TRY(hipStreamSynchronize(s));
    *bad_ids = h_pinned[0];
    *nnz = h_pinned[1];
    return 0;
}

#undef COUNT_TRY

} // namespace umihip
