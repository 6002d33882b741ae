// Sequencing saturation and median genes / molecules per cell as a function of depth (umi_saturation_curve, the
// program's --saturation-curve), gfx950: every read gets a hash of its number and a level in 0..L-1 from it, depth j is
// the reads of level <= j, and a molecule, a (column, row) pair or a column is there at depth j exactly when the
// smallest level among its reads is <= j.  So one pass over the reads and one over the molecules give all L depths.
// The collapse is the full-depth one: nothing is collapsed again per depth.  No counterpart in the reference;
// tests/saturation_model.py defines it.  Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The pair-table pipeline ("The pair-table pipeline"; umihip_pair_table.h) with these parts of its own:
//
//   scatter    a lane per read: its level's bit is OR-ed onto its molecule's word of a zeroed array, a word per entry, at
//              root[read_entry[i]] -- an integer OR, so the result does not depend on the order; the molecule's level
//              is the word's lowest set bit.  A read under a root that is not kept counts nowhere.  Counted reads per
//              level go through the block's LDS histogram and one atomicAdd per bin and block.  With option
//              "saturation_skip" a lane loads the word first and leaves the atomic out where its bit is set already.
//              A read_entry or root out of range goes to the control block by atomicMin, and nothing is written for it.
//   molecules  the bucket walk: a bucket's lane takes its entries one by one, a queued bucket's wave 64 entries at a
//              time, their levels counted by ballots.  Molecules per level through the block's LDS histogram; a
//              molecule adds 1 to its (level, column) count; every bucket writes its smallest level.
//   pairs      the runs' scan takes the minimum and ends in an atomicMin per run and wave (a minimum: no order).  Then
//              a lane per pair: pairs per level, and 1 onto the pair's (level, column) count.
//   columns    a lane per column walks its at most L counts of either table: whether it is selected, its first level,
//              the molecules and pairs of selected columns per level, and for every depth the column's cumulative
//              molecules and pairs as sort keys depth << 33 | count (a column that is not selected: count 2^32, behind
//              every real one).  One radix sort of the 2 L n_cols keys; the lower median of depth j is element
//              floor((n_sel - 1) / 2) of its segment.
//   curve      a lane per depth adds up the six histograms and picks the two medians.
// The (level, column) counts are a block's LDS table first where L n_cols <= SAT_LDS_TABLE words, and global atomicAdds
// otherwise; integer sums either way.  No thread walks a column, a run or a bucket beyond SAT_SMALL; every kernel loops
// grid-stride.
//
// One synchronisation, at the end, brings the control words and the curve.  Workspace, in bytes: 4 N + 52 m +
// 56 L n_cols + the two sorts' and the scan's temporaries (the larger of radix_sort_temp_bytes(m) and of (2 L n_cols),
// scan_temp_bytes(m)) + 4 KB.  It is n_cols, not n_sel, that the column tables and the median sort are sized by: the selected columns are
// not compacted (that would take a scan and a second synchronisation).
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

namespace {

constexpr int SAT_THREADS = 256;
constexpr uint32_t SAT_SMALL = 32;       // a bucket of more entries is a wave's (umihip_velocity.hip's VEL_SMALL)
constexpr uint32_t SAT_NONE = 32;        // the level of what has no read
constexpr uint32_t SAT_LDS_TABLE = 4096; // words of a block's own (level, column) table
constexpr uint64_t SAT_UNSELECTED = 1ull << 32; // the count of a column that is not selected, in a median key
constexpr int SAT_COUNT_BITS = 33;

enum SatCtl : int {
    SAT_BAD_IDS = 0,   // non-empty buckets with an id out of range
    SAT_BAD_ENTRY = 1, // the smallest read with a read_entry out of range (all ones: none)
    SAT_BAD_ROOT = 2,  // ... whose entry's root is out of range
    SAT_N_SEL = 3,     // selected columns
    SAT_CTL_COUNT = 4, // then six histograms of SAT_NONE bins, in the curve's order of columns 0..5
};
static_assert(SAT_BAD_IDS == 0, "the bucket walk counts into ctl[0]");
enum SatHist : int { H_READS = 0, H_MOLECULES = 1, H_PAIRS = 2, H_CELLS = 3, H_MOLECULES_IN = 4, H_PAIRS_IN = 5, H_COUNT = 6 };
constexpr size_t SAT_CTL_BYTES = (SAT_CTL_COUNT + H_COUNT * SAT_NONE) * 8, SAT_CURVE_WORDS = SAT_NONE * 8;

struct SatWs : PairTableWs { // (ctl: the control words, then the histograms)
    unsigned long long *curve;
    uint32_t *levels;        // [n] a word per entry: the levels of the reads of the molecule it roots
    uint32_t *blev;          // [m] a bucket's smallest level
    uint32_t *plev, *pcol;   // [m] a pair's smallest level and its column, by slot
    uint32_t *tab_m, *tab_p; // [L][n_cols] molecules and pairs of a column at a level
    uint64_t *mka, *mkb;     // [2 L n_cols] the median keys
    uint32_t *mva, *mvb;
    size_t levels_bytes, tab_bytes, total;
};
SatWs sat_carve(void *ws, uint64_t n, uint32_t m, bool has_idx, uint32_t n_cols, int n_levels)
{
    SatWs w;
    Carver c(ws);
    const size_t cells = (size_t)n_levels * n_cols;
    w.ctl = c.take<unsigned long long>(SAT_CTL_BYTES);
    w.curve = c.take<unsigned long long>(SAT_CURVE_WORDS * 8);
    w.levels_bytes = (size_t)n * 4;
    w.levels = c.take<uint32_t>(w.levels_bytes);
    w.carve_buckets(c, m, has_idx);
    w.blev = c.take<uint32_t>((size_t)m * 4);
    w.plev = c.take<uint32_t>((size_t)m * 4);
    w.pcol = c.take<uint32_t>((size_t)m * 4);
    w.tab_bytes = cells * 4;
    w.tab_m = c.take<uint32_t>(w.tab_bytes);
    w.tab_p = c.take<uint32_t>(w.tab_bytes);
    w.mka = c.take<uint64_t>(2 * cells * 8);
    w.mkb = c.take<uint64_t>(2 * cells * 8);
    w.mva = c.take<uint32_t>(2 * cells * 4);
    w.mvb = c.take<uint32_t>(2 * cells * 4);
    w.carve_temps(c, m, std::max(radix_sort_temp_bytes(m), radix_sort_temp_bytes((uint32_t)(2 * cells))));
    w.total = c.o;
    return w;
}

// the level of read i: the upper half of a splitmix64 of its number, scaled to 0..L-1 (umihip.h has the rule)
__device__ __forceinline__ uint32_t sat_level(uint64_t seed, uint64_t i, uint32_t n_levels)
{
    uint64_t z = seed + (i + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (uint32_t)(((z >> 32) * n_levels) >> 32);
}

template <bool SKIP_SET>
__global__ __launch_bounds__(SAT_THREADS) void saturation_scatter_kernel(const uint32_t *__restrict__ read_entry, uint32_t n_reads,
                                                                         const uint8_t *__restrict__ kept,
                                                                         const uint32_t *__restrict__ root, uint64_t n, uint64_t seed,
                                                                         uint32_t n_levels, uint32_t *levels, unsigned long long *ctl)
{
    __shared__ uint32_t hist[SAT_NONE];
    if (threadIdx.x < SAT_NONE) hist[threadIdx.x] = 0;
    __syncthreads();
    for (uint64_t i = (uint64_t)blockIdx.x * SAT_THREADS + threadIdx.x; i < n_reads; i += (uint64_t)gridDim.x * SAT_THREADS) {
        const uint32_t e = read_entry[i];
        if (e == UMI_READ_UNSTAGED) continue;
        if (e >= n) {
            atomicMin(ctl + SAT_BAD_ENTRY, (unsigned long long)i);
            continue;
        }
        const uint32_t r = root[e];
        if (r >= n) {
            atomicMin(ctl + SAT_BAD_ROOT, (unsigned long long)i);
            continue;
        }
        if (!kept[r]) continue; // (what the multi-gene filter removed: neither a molecule nor a counted read)
        const uint32_t lev = sat_level(seed, i, n_levels);
        atomicAdd(&hist[lev], 1u);
        const uint32_t bit = 1u << lev;
        // (the load is the device's view, as the atomics': a bit set by another CU is seen; a 0 read too early costs an
        // atomic, never a wrong bit)
        if (SKIP_SET && (__hip_atomic_load(levels + r, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) & bit)) continue;
        atomicOr(levels + r, bit);
    }
    __syncthreads();
    if (threadIdx.x < n_levels && hist[threadIdx.x]) atomicAdd(ctl + SAT_CTL_COUNT + H_READS * SAT_NONE + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
}

// A block's (level, column) counts: its LDS table where the whole table fits, the global one otherwise
struct SatTable {
    uint32_t *lds, *global;
    uint32_t n_cols;
    __device__ __forceinline__ void add(uint32_t lev, uint32_t col, uint32_t count) const
    {
        atomicAdd((lds ? lds : global) + (size_t)lev * n_cols + col, count);
    }
};
__device__ __forceinline__ void sat_table_clear(uint32_t *lds, uint32_t words)
{
    for (uint32_t t = threadIdx.x; t < words; t += SAT_THREADS) lds[t] = 0;
}
__device__ __forceinline__ void sat_table_flush(const uint32_t *lds, uint32_t words, uint32_t *global)
{
    for (uint32_t t = threadIdx.x; t < words; t += SAT_THREADS)
        if (lds[t]) atomicAdd(global + t, lds[t]);
}

struct SatArgs {
    PairTable t;
    const uint8_t *kept;
    const uint32_t *levels;
    uint32_t n_levels, lds_words; // lds_words: L n_cols where the block's table is in LDS, else 0
    uint32_t *blev, *tab_m;
};

__global__ __launch_bounds__(SAT_THREADS) void saturation_molecules_kernel(SatArgs a)
{
    __shared__ uint32_t hist[SAT_NONE];
    __shared__ uint32_t lds_table[SAT_LDS_TABLE];
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    if (tid < SAT_NONE) hist[tid] = 0;
    sat_table_clear(lds_table, a.lds_words);
    const SatTable table{a.lds_words ? lds_table : nullptr, a.tab_m, a.t.n_cols};
    pair_bucket_walk<SAT_THREADS, SAT_SMALL>( // (its first barrier is the cleared tables' too)
        a.t,
        [&](uint64_t j, uint64_t lo, uint64_t hi, uint32_t col, bool bad) {
            uint32_t least = SAT_NONE;
            for (uint64_t e = lo; e < hi; e++) {
                const uint32_t w = a.levels[e];
                if (!a.kept[e] || !w) continue;
                const uint32_t lev = (uint32_t)__ffs((int)w) - 1u;
                least = min(least, lev);
                atomicAdd(&hist[lev], 1u);
                if (!bad) table.add(lev, col, 1u);
            }
            a.blev[j] = least;
        },
        [&](uint64_t jb, uint64_t lo, uint64_t hi) {
            const uint32_t b = a.t.idx ? a.t.idx[jb] : (uint32_t)jb;
            const uint32_t col = a.t.col[b];
            const bool bad = a.t.row[b] >= a.t.n_rows || col >= a.t.n_cols;
            uint32_t mine = 0; // lane l: the bucket's molecules of level l
            for (uint64_t e0 = lo; e0 < hi; e0 += 64) {
                const uint64_t e = e0 + lane;
                uint32_t lev = SAT_NONE;
                if (e < hi) {
                    const uint32_t w = a.levels[e];
                    if (a.kept[e] && w) lev = (uint32_t)__ffs((int)w) - 1u;
                }
                for (uint32_t l = 0; l < a.n_levels; l++) {
                    const uint32_t c = (uint32_t)__popcll(__ballot(lev == l));
                    if (lane == l) mine += c;
                }
            }
            const unsigned long long have = __ballot(mine != 0);
            if (mine) {
                atomicAdd(&hist[lane], mine);
                if (!bad) table.add(lane, col, mine);
            }
            if (lane == 0) a.blev[jb] = have ? (uint32_t)__ffsll((unsigned long long)have) - 1u : SAT_NONE;
        });
    __syncthreads();
    if (tid < a.n_levels && hist[tid]) atomicAdd(a.t.ctl + SAT_CTL_COUNT + H_MOLECULES * SAT_NONE + tid, (unsigned long long)hist[tid]);
    sat_table_flush(lds_table, a.lds_words, a.tab_m);
}

// plev[] holds all ones on entry
__global__ __launch_bounds__(SAT_THREADS) void saturation_pair_min_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                          const uint64_t *__restrict__ incl,
                                                                          const uint32_t *__restrict__ blev, uint32_t m, int rb,
                                                                          uint32_t *plev, uint32_t *__restrict__ pcol)
{
    for (uint64_t base = (uint64_t)blockIdx.x * SAT_THREADS; base < m; base += (uint64_t)gridDim.x * SAT_THREADS) {
        const uint64_t i = base + threadIdx.x;
        const WaveRuns run(incl, i, m);
        uint32_t v = run.valid ? blev[val[i]] : SAT_NONE;
        run.scan([](uint32_t x, uint32_t y) { return min(x, y); }, v);
        if (run.head) pcol[run.slot()] = (uint32_t)(key[i] >> rb);
        if (run.tail()) atomicMin(plev + run.slot(), v);
    }
}

__global__ __launch_bounds__(SAT_THREADS) void saturation_pairs_kernel(const uint32_t *__restrict__ plev, const uint32_t *__restrict__ pcol,
                                                                       const uint64_t *__restrict__ nnz_at, uint32_t n_levels,
                                                                       uint32_t n_cols, uint32_t lds_words, uint32_t *tab_p,
                                                                       unsigned long long *ctl)
{
    __shared__ uint32_t hist[SAT_NONE];
    __shared__ uint32_t lds_table[SAT_LDS_TABLE];
    if (threadIdx.x < SAT_NONE) hist[threadIdx.x] = 0;
    sat_table_clear(lds_table, lds_words);
    __syncthreads();
    const SatTable table{lds_words ? lds_table : nullptr, tab_p, n_cols};
    const uint64_t nnz = *nnz_at;
    for (uint64_t i = (uint64_t)blockIdx.x * SAT_THREADS + threadIdx.x; i < nnz; i += (uint64_t)gridDim.x * SAT_THREADS) {
        const uint32_t lev = plev[i];
        if (lev >= n_levels) continue;
        const uint32_t col = pcol[i];
        atomicAdd(&hist[lev], 1u);
        if (col < n_cols) table.add(lev, col, 1u); // (a bucket out of range has key 0; the call fails, nothing is read)
    }
    __syncthreads();
    if (threadIdx.x < n_levels && hist[threadIdx.x]) atomicAdd(ctl + SAT_CTL_COUNT + H_PAIRS * SAT_NONE + threadIdx.x, (unsigned long long)hist[threadIdx.x]);
    sat_table_flush(lds_table, lds_words, tab_p);
}

__global__ __launch_bounds__(SAT_THREADS) void saturation_columns_kernel(const uint32_t *__restrict__ tab_m, const uint32_t *__restrict__ tab_p,
                                                                         const uint8_t *__restrict__ cell_mask, uint32_t n_cols,
                                                                         uint32_t n_levels, uint64_t *__restrict__ mkey,
                                                                         uint32_t *__restrict__ mval, unsigned long long *ctl)
{
    __shared__ uint32_t hist[3][SAT_NONE]; // cells, molecules in cells, pairs in cells
    __shared__ uint32_t n_sel;
    if (threadIdx.x < 3 * SAT_NONE) (&hist[0][0])[threadIdx.x] = 0;
    if (threadIdx.x == 0) n_sel = 0;
    __syncthreads();
    for (uint64_t c = (uint64_t)blockIdx.x * SAT_THREADS + threadIdx.x; c < n_cols; c += (uint64_t)gridDim.x * SAT_THREADS) {
        bool any = false;
        for (uint32_t l = 0; l < n_levels; l++) any = any || tab_m[(size_t)l * n_cols + c] != 0;
        const bool sel = cell_mask ? cell_mask[c] != 0 : any;
        if (sel) atomicAdd(&n_sel, 1u);
        uint64_t cm = 0, cp = 0;
        bool first = sel;
        for (uint32_t l = 0; l < n_levels; l++) {
            const uint32_t mols = tab_m[(size_t)l * n_cols + c], pairs = tab_p[(size_t)l * n_cols + c];
            cm += mols;
            cp += pairs;
            if (sel && mols) atomicAdd(&hist[1][l], mols);
            if (sel && pairs) atomicAdd(&hist[2][l], pairs);
            if (first && mols) {
                atomicAdd(&hist[0][l], 1u);
                first = false;
            }
            const size_t at_m = (size_t)l * n_cols + c, at_p = (size_t)(n_levels + l) * n_cols + c;
            mkey[at_m] = ((uint64_t)l << SAT_COUNT_BITS) | (sel ? cm : SAT_UNSELECTED);
            mkey[at_p] = ((uint64_t)(n_levels + l) << SAT_COUNT_BITS) | (sel ? cp : SAT_UNSELECTED);
            mval[at_m] = mval[at_p] = (uint32_t)c;
        }
    }
    __syncthreads();
    if (threadIdx.x < n_levels)
        for (int h = 0; h < 3; h++)
            if (hist[h][threadIdx.x])
                atomicAdd(ctl + SAT_CTL_COUNT + (H_CELLS + h) * SAT_NONE + threadIdx.x, (unsigned long long)hist[h][threadIdx.x]);
    if (threadIdx.x == 0 && n_sel) atomicAdd(ctl + SAT_N_SEL, (unsigned long long)n_sel);
}

__global__ __launch_bounds__(64) void saturation_curve_kernel(const unsigned long long *__restrict__ ctl, const uint64_t *__restrict__ sorted,
                                                              uint32_t n_cols, uint32_t n_levels, unsigned long long *__restrict__ curve)
{
    const unsigned long long *hist = ctl + SAT_CTL_COUNT;
    const uint64_t n_sel = ctl[SAT_N_SEL], mid = n_sel ? (n_sel - 1) / 2 : 0;
    for (uint32_t j = blockIdx.x * 64 + threadIdx.x; j < n_levels; j += gridDim.x * 64) {
        for (int h = 0; h < H_COUNT; h++) {
            unsigned long long sum = 0;
            for (uint32_t l = 0; l <= j; l++) sum += hist[h * SAT_NONE + l];
            curve[j * 8 + h] = sum;
        }
        const uint64_t count_mask = (1ull << SAT_COUNT_BITS) - 1ull;
        curve[j * 8 + 6] = n_sel ? sorted[(size_t)j * n_cols + mid] & count_mask : 0ull;
        curve[j * 8 + 7] = n_sel ? sorted[(size_t)(n_levels + j) * n_cols + mid] & count_mask : 0ull;
    }
}

} // namespace

size_t saturation_workspace_bytes(uint64_t n, uint32_t m, bool has_idx, uint32_t n_cols, int n_levels)
{
    return sat_carve(nullptr, n, m, has_idx, n_cols, n_levels).total;
}

int saturation_curve_on_device(void *workspace, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                               const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx, uint32_t m,
                               const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint64_t seed,
                               int n_levels, const uint8_t *d_cell_mask, bool skip_set, uint64_t *bad_ids, int *bad_kind,
                               uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s)
{
    const SatWs w = sat_carve(workspace, n, m, h_idx != nullptr, n_cols, n_levels);
    const int rb = bits_of(n_rows - 1), cb = bits_of(n_cols - 1);
    int r;
    const uint32_t L = (uint32_t)n_levels, cells = L * n_cols;
    const uint32_t lds_words = cells <= SAT_LDS_TABLE ? cells : 0u;
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, SAT_CTL_BYTES, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl + SAT_BAD_ENTRY, 0xFF, 2 * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.levels, 0, w.levels_bytes, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.plev, 0xFF, (size_t)m * 4, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.tab_m, 0, w.tab_bytes, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.tab_p, 0, w.tab_bytes, s));
    if ((r = pair_table_upload(w, h_off, h_idx, m, s))) return r;
    if (n_reads) {
        const uint32_t grid = std::min(blocks_for(n_reads, SAT_THREADS), n_cus * 16);
        if (skip_set)
            saturation_scatter_kernel<true><<<grid, SAT_THREADS, 0, s>>>(d_read_entry, n_reads, d_kept, d_root, n, seed, L, w.levels, w.ctl);
        else
            saturation_scatter_kernel<false><<<grid, SAT_THREADS, 0, s>>>(d_read_entry, n_reads, d_kept, d_root, n, seed, L, w.levels, w.ctl);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    const SatArgs a{{w.off, w.idx, d_row, d_col, n_rows, n_cols, m, rb, w.ka, w.va, w.ctl},
                    d_kept, w.levels, L, lds_words, w.blev, w.tab_m};
    const uint32_t per_bucket_grid = std::min(blocks_for(m, SAT_THREADS), n_cus * 4); // (a block flushes its table at its end)
    saturation_molecules_kernel<<<per_bucket_grid, SAT_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    const uint64_t *keys;
    const uint32_t *vals;
    uint64_t *incl;
    const uint32_t capped_grid = std::min(blocks_for(m, SAT_THREADS), n_cus * 8);
    if ((r = pair_table_sort_and_number<SAT_THREADS>(w, m, rb + cb, capped_grid, s, &keys, &vals, &incl))) return r;
    saturation_pair_min_kernel<<<capped_grid, SAT_THREADS, 0, s>>>(keys, vals, incl, w.blev, m, rb, w.plev, w.pcol);
    UMIHIP_TRY_NEG(hipGetLastError());
    saturation_pairs_kernel<<<per_bucket_grid, SAT_THREADS, 0, s>>>(w.plev, w.pcol, incl + (m - 1), L, n_cols, lds_words, w.tab_p, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    saturation_columns_kernel<<<std::min(blocks_for(n_cols, SAT_THREADS), n_cus * 8), SAT_THREADS, 0, s>>>(w.tab_m, w.tab_p, d_cell_mask, n_cols, L,
                                                                                                         w.mka, w.mva, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    bool med_in_b = false;
    UMIHIP_TRY_NEG(radix_sort_pairs_u64(w.mka, w.mkb, w.mva, w.mvb, 2 * cells, 0, SAT_COUNT_BITS + 6, w.radix_tmp, w.radix_bytes, &med_in_b, s));
    saturation_curve_kernel<<<1, 64, 0, s>>>(w.ctl, med_in_b ? w.mkb : w.mka, n_cols, L, w.curve);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, w.ctl, SAT_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned + SAT_CTL_COUNT, w.curve, (size_t)L * 8 * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    *bad_ids = h_pinned[SAT_BAD_IDS];
    *bad_kind = 0;
    *bad_read = ~0ull;
    for (int k = 1; k <= 2; k++)
        if (h_pinned[k] < *bad_read) {
            *bad_read = h_pinned[k];
            *bad_kind = k;
        }
    return 0;
}

} // namespace umihip
