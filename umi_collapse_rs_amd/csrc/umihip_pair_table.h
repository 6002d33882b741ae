// The pair-table pipeline that the tables over a call's result share ("The pair-table pipeline"):
// umi_count_matrix, umi_velocity_matrix and umi_saturation_curve walk the non-empty buckets the same way, sort them
// by (column, row), number the runs of one pair and combine every run's buckets by a segmented scan over the wave;
// umi_dedup_stats' per-UMI table and umi_filter_multigene use the run numbering and the scan.  What differs between
// them -- what a bucket is reduced to, and how two buckets of a pair combine -- is handed in.  gfx950, 64-lane waves.
#pragma once
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"

namespace umihip {

// ---- host helpers -------------------------------------------------------------------------------------------------
// (an *_on_device function returns 0 or minus the HIP error)
#define UMIHIP_TRY_NEG(expr)                     \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }
inline uint32_t blocks_for(uint64_t n, uint32_t per) { return (uint32_t)std::max<uint64_t>(1, (n + per - 1) / per); }
inline int bits_of(uint64_t v)
{
    int b = 0;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// A workspace handed out piece by piece, every piece on a 256-byte boundary; the order of the takes is the layout.
struct Carver {
    char *p;
    size_t o = 0;
    explicit Carver(void *ws) : p((char *)ws) {}
    template <typename T = void> T *take(size_t bytes)
    {
        char *at = p + o;
        o += align256(bytes);
        return (T *)at;
    }
};

// The buffers of a table over m non-empty buckets.  A call's workspace is this and its own fields; it carves ctl
// itself (the words behind [0] are its own) and the two groups below where its layout has them.
struct PairTableWs {
    unsigned long long *ctl; // [0] non-empty buckets with an id out of range
    uint64_t *off;           // [m + 1] the non-empty buckets' offsets; then the inclusive scan of the head flags
    uint32_t *idx;           // [m] their bucket numbers (null: nothing was left out)
    uint64_t *ka, *kb;       // [m] the sort keys (the buffer the sort leaves free holds the head flags)
    uint32_t *va, *vb;       // [m] the sort's values: the buckets' numbers among the non-empty ones
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes;

    void carve_buckets(Carver &c, uint32_t m, bool has_idx)
    {
        off = c.take<uint64_t>(((size_t)m + 1) * 8);
        idx = has_idx ? c.take<uint32_t>((size_t)m * 4) : nullptr;
        ka = c.take<uint64_t>((size_t)m * 8);
        kb = c.take<uint64_t>((size_t)m * 8);
        va = c.take<uint32_t>((size_t)m * 4);
        vb = c.take<uint32_t>((size_t)m * 4);
    }
    void carve_temps(Carver &c, uint32_t m, size_t radix)
    {
        radix_bytes = radix;
        radix_tmp = c.take(radix_bytes);
        scan_bytes = scan_temp_bytes(m);
        scan_tmp = c.take(scan_bytes);
    }
};

// the walked table (umihip_count_api.cpp: cm_walk) from the pinned staging into the workspace
inline int pair_table_upload(const PairTableWs &w, const uint64_t *h_off, const uint32_t *h_idx, uint32_t m, hipStream_t s)
{
    UMIHIP_TRY_NEG(hipMemcpyAsync(w.off, h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (h_idx) UMIHIP_TRY_NEG(hipMemcpyAsync(w.idx, h_idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    return 0;
}

// flag[i] = the sorted key differs from its predecessor's.  Grid-stride: one trip where the grid covers n.
template <int THREADS>
__global__ __launch_bounds__(THREADS) void pair_heads_kernel(const uint64_t *__restrict__ key, uint32_t n, uint64_t *__restrict__ flag)
{
    for (uint64_t i = (uint64_t)blockIdx.x * THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * THREADS)
        flag[i] = i == 0 || key[i] != key[i - 1] ? 1ull : 0ull;
}

// (ka, va) of the m buckets sorted by the low key_bits bits of the key, the head flags of the sorted keys (by
// heads_grid blocks of THREADS) and their inclusive scan: bucket i of the sorted order belongs to output slot incl[i] - 1,
// and incl[m - 1] slots there are.  incl[] takes the offsets' place: they have been read.
template <int THREADS>
int pair_table_sort_and_number(const PairTableWs &w, uint32_t m, int key_bits, uint32_t heads_grid, hipStream_t s,
                               const uint64_t **keys, const uint32_t **vals, uint64_t **incl)
{
    bool in_b = false;
    UMIHIP_TRY_NEG(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, m, 0, key_bits, w.radix_tmp, w.radix_bytes, &in_b, s));
    *keys = in_b ? w.kb : w.ka;
    *vals = in_b ? w.vb : w.va;
    uint64_t *flag = in_b ? w.ka : w.kb;
    *incl = w.off;
    pair_heads_kernel<THREADS><<<heads_grid, THREADS, 0, s>>>(*keys, m, flag);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(scan_inclusive_u64(flag, *incl, m, w.scan_tmp, w.scan_bytes, s));
    return 0;
}

// ---- the bucket walk ----------------------------------------------------------------------------------------------
struct PairTable { // what the walk reads and writes of a table
    const uint64_t *off;
    const uint32_t *idx; // may be null
    const uint32_t *row, *col;
    uint32_t n_rows, n_cols, m;
    int rb; // bits of n_rows - 1
    uint64_t *key;
    uint32_t *val;
    unsigned long long *ctl;
};

// One pass over the m buckets, THREADS per block at a time, the whole block calling.  Every bucket writes its sort key
// column << rb | row and its number as the sort's value; an id out of range counts into ctl[0] and gives key 0.  A
// bucket of up to SMALL entries is its lane's: lane_fn(j, lo, hi, col, bad) with its entries [lo, hi).  A larger one
// is queued in LDS and taken by one of the block's waves: wave_fn(j, lo, hi), all 64 lanes calling.  No global atomic
// per entry or per bucket; three barriers a trip.
template <int THREADS, uint32_t SMALL, typename LaneFn, typename WaveFn>
__device__ __forceinline__ void pair_bucket_walk(const PairTable &a, LaneFn lane_fn, WaveFn wave_fn)
{
    __shared__ uint32_t queue[THREADS];
    __shared__ uint32_t queued;
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    for (uint64_t base = (uint64_t)blockIdx.x * THREADS; base < a.m; base += (uint64_t)gridDim.x * THREADS) {
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
            if (hi - lo <= SMALL) lane_fn(j, lo, hi, col, bad);
            else queue[atomicAdd(&queued, 1u)] = tid;
        }
        __syncthreads();
        const uint32_t nq = queued;
        for (uint32_t t = wave; t < nq; t += THREADS / 64) {
            const uint64_t jb = base + queue[t];
            wave_fn(jb, a.off[jb], a.off[jb + 1]);
        }
        __syncthreads(); // (the queue is the next round's as well)
    }
}

// ---- runs of one slot over a wave ---------------------------------------------------------------------------------
// What lane i of a wave knows of its sorted element's run, from the inclusive scan of the head flags: a lane per
// element, every lane of the wave constructing (elements past n take part as no run's).  scan() leaves in every lane
// what its run holds from the run's first lane in this wave up to it, so the run's last lane in the wave -- tail() --
// holds all the wave adds to the run: stored where whole(), combined by an atomic otherwise.  No thread walks a run.
struct WaveRuns {
    uint64_t slot1; // the slot, counted from 1 (0 past the end)
    unsigned long long heads;
    int lane;
    bool valid, head, last;

    __device__ __forceinline__ WaveRuns(const uint64_t *__restrict__ incl, uint64_t i, uint32_t n)
    {
        lane = (int)(threadIdx.x & 63u);
        valid = i < n;
        slot1 = valid ? incl[i] : 0ull;
        uint64_t prev = __shfl_up(slot1, 1), next = __shfl_down(slot1, 1);
        if (lane == 0) prev = valid && i > 0 ? incl[i - 1] : 0ull;
        if (lane == 63) next = i + 1 < n ? incl[i + 1] : 0ull;
        head = valid && slot1 != prev;                 // (slot numbers start at 1: the first element differs from 0)
        last = valid && (i + 1 >= n || next != slot1); // the run ends here
        heads = __ballot(head);
    }
    uint64_t __device__ __forceinline__ slot() const { return slot1 - 1; }

    // inclusive scan of every value inside runs of one slot: six steps that combine only across equal slots
    template <typename Op, typename... T> __device__ __forceinline__ void scan(Op op, T &...v) const
    {
        for (int d = 1; d < 64; d <<= 1) {
            const uint64_t up = __shfl_up(slot1, d); // (every lane shuffles, whether it combines or not)
            const bool same = lane >= d && up == slot1;
            (step(op, v, d, same), ...);
        }
    }
    // the run's last lane in this wave
    __device__ __forceinline__ bool tail() const { return valid && (last || lane == 63); }
    // at a tail(): the run began in this wave and ends here (a head at or before this lane)
    __device__ __forceinline__ bool whole() const
    {
        const unsigned long long upto = lane == 63 ? ~0ull : (2ull << lane) - 1ull;
        return last && (heads & upto);
    }

private:
    template <typename Op, typename T> static __device__ __forceinline__ void step(Op op, T &v, int d, bool same)
    {
        const T up = __shfl_up(v, d); // (every lane shuffles)
        if (same) v = op(v, up);
    }
};

} // namespace umihip
