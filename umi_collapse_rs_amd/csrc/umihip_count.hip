// Molecules and reads per (column, row) pair over the buckets of a batched call (umi_count_matrix, the
// program's --count-matrix), gfx950: kept[] / freq[] of a call and every bucket's row (gene) and column (cell)
// become the sorted triplets of a sparse matrix.  No counterpart in the reference; tests/gene_model.py
// (count_model) defines it.  Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The pair-table pipeline ("The pair-table pipeline"; umihip_pair_table.h) with these parts of its own:
//
//   reduce   a bucket's lane walks its few neighbouring entries (the typical bucket has one to three; the lanes of a
//            wave read one stretch of kept[] and freq[] between them).  A queued bucket's wave strides over kept[] a
//            4-byte word at a time from the first aligned entry on (the entries before it and after the last whole
//            word a lane each), freq[] beside it, and adds up with __shfl_down.  Every bucket writes (reads,
//            molecules), 16 bytes.
//   sum      a lane per sorted bucket gathers its 16 bytes; the runs' scan adds.  A run inside a wave is stored; one
//            that crosses a wave's edge is added with atomicAdd (u32 molecules, 64-bit reads) onto the zeroed outputs
//            -- one atomic pair per wave and run, integer sums, so the result does not depend on the order.
//
// One synchronisation, at the end, brings nnz and the count of bad ids.  Workspace per non-empty bucket:
// offsets 8 (the slots' scan reuses them), keys 2 x 8 (the buffer the sort leaves free holds the flags), values
// 2 x 4, sums 16, bucket numbers 4 where buckets were left out: 48 to 52 bytes, and the sort's tables.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

namespace {

constexpr int COUNT_THREADS = 256;
constexpr uint32_t COUNT_SMALL = 32; // a bucket of more entries is a wave's

struct CountSum { // what a bucket adds to its pair
    unsigned long long reads;
    uint32_t molecules, pad;
};

struct CountWs : PairTableWs {
    CountSum *sum;
    size_t total;
};
CountWs count_carve(void *ws, uint32_t m, bool has_idx)
{
    CountWs w;
    Carver c(ws);
    w.ctl = c.take<unsigned long long>(256);
    w.carve_buckets(c, m, has_idx);
    w.sum = c.take<CountSum>((size_t)m * sizeof(CountSum));
    w.carve_temps(c, m, radix_sort_temp_bytes(m));
    w.total = c.o;
    return w;
}

struct CountArgs {
    PairTable t;
    const uint8_t *kept;
    const int32_t *freq;
    CountSum *sum;
};

__device__ __forceinline__ uint32_t nonzero_bytes(uint32_t w)
{
    return ((w & 0xFFu) != 0u) + ((w & 0xFF00u) != 0u) + ((w & 0xFF0000u) != 0u) + ((w & 0xFF000000u) != 0u);
}

__global__ __launch_bounds__(COUNT_THREADS) void count_reduce_kernel(CountArgs a)
{
    const uint32_t lane = threadIdx.x & 63u;
    pair_bucket_walk<COUNT_THREADS, COUNT_SMALL>(
        a.t,
        [&](uint64_t j, uint64_t lo, uint64_t hi, uint32_t, bool) {
            CountSum s{0ull, 0u, 0u};
            for (uint64_t e = lo; e < hi; e++) {
                s.molecules += a.kept[e] != 0;
                s.reads += (unsigned long long)(long long)a.freq[e];
            }
            a.sum[j] = s;
        },
        [&](uint64_t jb, uint64_t lo, uint64_t hi) {
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
        });
}

__global__ __launch_bounds__(COUNT_THREADS) void count_sum_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                  const uint64_t *__restrict__ incl, const CountSum *__restrict__ sum,
                                                                  uint32_t m, int rb, uint32_t *__restrict__ out_row,
                                                                  uint32_t *__restrict__ out_col, uint32_t *out_molecules,
                                                                  unsigned long long *out_reads)
{
    const uint64_t i = (uint64_t)blockIdx.x * COUNT_THREADS + threadIdx.x;
    const WaveRuns run(incl, i, m);
    CountSum s{0ull, 0u, 0u};
    if (run.valid) s = sum[val[i]];
    uint32_t mol = s.molecules;
    unsigned long long reads = s.reads;
    run.scan([](auto x, auto y) { return x + y; }, mol, reads);
    if (run.head) {
        const uint64_t k = key[i];
        out_row[run.slot()] = (uint32_t)(k & ((1ull << rb) - 1ull));
        out_col[run.slot()] = (uint32_t)(k >> rb);
    }
    if (run.tail()) {
        if (run.whole()) {
            out_molecules[run.slot()] = mol;
            out_reads[run.slot()] = reads;
        } else {
            atomicAdd(out_molecules + run.slot(), mol);
            atomicAdd(out_reads + run.slot(), reads);
        }
    }
}

} // namespace

size_t count_workspace_bytes(uint32_t m, bool has_idx) { return count_carve(nullptr, m, has_idx).total; }

int count_matrix_on_device(void *workspace, const uint8_t *d_kept, const int32_t *d_freq, const uint64_t *h_off,
                           const uint32_t *h_idx, uint32_t m, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows,
                           uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules,
                           uint64_t *d_out_reads, uint64_t *nnz, uint64_t *bad_ids, uint32_t n_cus, unsigned long long *h_pinned,
                           hipStream_t s)
{
    const CountWs w = count_carve(workspace, m, h_idx != nullptr);
    const int rb = bits_of(n_rows - 1), cb = bits_of(n_cols - 1);
    int r;
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, 256, s));
    if ((r = pair_table_upload(w, h_off, h_idx, m, s))) return r;
    UMIHIP_TRY_NEG(hipMemsetAsync(d_out_molecules, 0, (size_t)m * 4, s)); // (a run that crosses a wave is added up in place)
    UMIHIP_TRY_NEG(hipMemsetAsync(d_out_reads, 0, (size_t)m * 8, s));
    const CountArgs a{{w.off, w.idx, d_row, d_col, n_rows, n_cols, m, rb, w.ka, w.va, w.ctl}, d_kept, d_freq, w.sum};
    count_reduce_kernel<<<std::min(blocks_for(m, COUNT_THREADS), n_cus * 8), COUNT_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    const uint64_t *keys;
    const uint32_t *vals;
    uint64_t *incl;
    if ((r = pair_table_sort_and_number<COUNT_THREADS>(w, m, rb + cb, blocks_for(m, COUNT_THREADS), s, &keys, &vals, &incl))) return r;
    count_sum_kernel<<<blocks_for(m, COUNT_THREADS), COUNT_THREADS, 0, s>>>(keys, vals, incl, w.sum, m, rb, d_out_row, d_out_col,
                                                                           d_out_molecules, (unsigned long long *)d_out_reads);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, w.ctl, 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned + 1, incl + (m - 1), 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    *bad_ids = h_pinned[0];
    *nnz = h_pinned[1];
    return 0;
}

} // namespace umihip
