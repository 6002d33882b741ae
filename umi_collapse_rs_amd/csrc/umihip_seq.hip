// Whole-read keys (gfx950): FASTQ mode's long-key path, reads of up to UMI_MAX_SEQ_LEN = 256 bases,
// 1..12 words of 64 bits per key, several read lengths (buckets) in one call.
//
// What it replaces in the reference (tkob-vh/umi-collapse-rs): the same lines as the other pair
// kernels -- Naive::remove_near's scans (src/data/naive.rs:26-40) over BitSet::bit_count_xor's per-word
// loop (src/utils/bitset.rs:77-91) and umi_dist (src/utils/mod.rs:24-26) -- for the keys of the fastq
// mode the reference leaves as a TODO (src/main.rs:49-50).  The arithmetic is the reference's word by
// word, the straddling-N quirk included (bases 21, 42, 85, 106, 149, 170, 213, 234).
//
// Partition.  A bucket of n entries and length L is cut into P = k + 1 parts, part j covering bases
// [jL/P, (j+1)L/P).  Every mismatched base costs at least 2 bits of bit_count_xor, so dist <= k means
// at most k differing bases and, by pigeonhole, one part that is exactly equal.  Each entry gets one
// record per part: (group, 32-bit hash of the part's bits) -> entry; one radix sort of the records
// puts the entries of equal parts next to each other (a bin = a run of equal records).  Hashing the
// whole part, rather than binning by its leading bases, keeps a shared prefix (a linker, a primer)
// from putting a whole bucket into one bin unless the whole part is shared.  Buckets that are small
// or whose parts would be shorter than SEQ_MIN_PART_BASES bases form one group of a single part
// with a constant hash: one bin, the exact all-pairs evaluation.
//
// Exactly once.  In the bin of part j a pair is decided only if part j is exactly equal (hash
// collisions share bins) and no part 0..j-1 is (the bin of that part decides it); then it is an edge
// iff its distance over all ceil(3L/64) words is <= k.
//
// Tiles.  A bin of m entries is ceil(m/64) x ceil(m/64) upper-triangular 64x64 tiles, and every tile
// is a task of its own, dealt over a persistent grid: a heavy bin (a constant half, as in amplicon
// reads) spreads over the whole chip instead of running on one wave.  One wave per task: a row per
// lane with its key in registers, the tile's 64 columns one lane each, broadcast with v_readlane; the
// distance loop stops as soon as every lane of the wave is past k (candidates share one part and
// almost always differ elsewhere).  Integer / bitwise work, no MFMA.
//
// Edges go to the same list, in the same format, as every other pair kernel's; the collapse and the
// finalisation behind it are the existing ones (EdgeCollapse, umihip_pipeline.cpp).
#include <hip/hip_runtime.h>

#include "umihip_internal.h"
#include "umihip_device.h"

namespace umihip {

namespace {

__device__ __forceinline__ uint64_t mix64(uint64_t z)
{ // splitmix64's finaliser
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// bits [lo, hi) of word w of a key (lo/hi in bit positions of the whole key string)
__device__ __forceinline__ uint64_t part_mask(int w, int lo, int hi)
{
    const int a = max(lo, 64 * w), b = min(hi, 64 * w + 64);
    if (a >= b) return 0ull;
    const int n = b - a;
    return (n == 64 ? ~0ull : ((1ull << n) - 1ull)) << (a - 64 * w);
}

__device__ __forceinline__ int part_lo(uint32_t j, uint32_t len, uint32_t parts) { return 3 * (int)(j * len / parts); }

// One record per (group, entry): key = group << 32 | hash of the group's part, value = entry.  The
// first group of every bucket also does the per-entry work of the call: threshold, and the contract
// check (freq >= 1, not rising inside the bucket, no N code where nmask is NULL).
__global__ __launch_bounds__(256) void seq_records_kernel(const SeqGroup *__restrict__ groups, uint32_t n_groups,
                                                          uint32_t n_rec, const uint64_t *__restrict__ keys,
                                                          const uint64_t *__restrict__ nmask, int stride,
                                                          const int32_t *__restrict__ freq, float percentage,
                                                          int32_t *__restrict__ thr, uint64_t *__restrict__ rkey,
                                                          uint32_t *__restrict__ rval,
                                                          unsigned long long *__restrict__ counters)
{
    unsigned int bad = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        uint32_t lo = 0, hi = n_groups; // last group with rec_off <= r
        while (hi - lo > 1) {
            const uint32_t mid = (lo + hi) / 2;
            if (groups[mid].rec_off <= r) lo = mid;
            else hi = mid;
        }
        const SeqGroup g = groups[lo];
        const uint32_t i = g.bstart + (r - g.rec_off);
        const uint64_t *key = keys + (size_t)i * stride;
        uint32_t h = 0;
        if (g.part != SEQ_ALL_PAIRS) {
            const int plo = part_lo(g.part, g.len, g.n_parts), phi = part_lo(g.part + 1, g.len, g.n_parts);
            uint64_t acc = 0x9E3779B97F4A7C15ull;
            for (int w = plo >> 6; w <= (phi - 1) >> 6; w++) acc = mix64(acc ^ (key[w] & part_mask(w, plo, phi)) ^ (uint64_t)w);
            h = (uint32_t)(acc >> 32);
        }
        rkey[r] = ((uint64_t)lo << 32) | h;
        rval[r] = i;
        if (g.part == 0 || g.part == SEQ_ALL_PAIRS) {
            const int32_t f = freq[i];
            thr[i] = threshold_of(percentage, f);
            bad += f < 1 ? 1u : 0u;
            bad += (i > g.bstart && f > freq[i - 1]) ? 1u : 0u;
            if (!nmask) { // NULL promises that no key holds the N code (100)
                for (uint32_t b = 0; b < g.len; b++) {
                    const uint32_t bit = 3 * b;
                    uint64_t c = key[bit >> 6] >> (bit & 63);
                    if ((bit & 63) > 61) c |= key[(bit >> 6) + 1] << (64 - (bit & 63));
                    bad += (c & 7u) == 4u ? 1u : 0u;
                }
            }
        }
    }
    block_count_add(bad, &counters[CNT_ERROR]);
}

// start[r] = 1 where a run of equal records begins
__global__ __launch_bounds__(256) void seq_run_flags_kernel(const uint64_t *__restrict__ rkey, uint32_t n_rec,
                                                            uint64_t *__restrict__ flag)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x)
        flag[r] = (r == 0 || rkey[r] != rkey[r - 1]) ? 1ull : 0ull;
}

// run_start[run] for every run, run_start[n_runs] = n_rec (run_id: inclusive scan of the flags)
__global__ __launch_bounds__(256) void seq_run_starts_kernel(const uint64_t *__restrict__ flag,
                                                             const uint64_t *__restrict__ run_id, uint32_t n_rec,
                                                             uint32_t *__restrict__ run_start)
{
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        if (flag[r]) run_start[run_id[r] - 1] = r;
        if (r == n_rec - 1) run_start[run_id[r]] = n_rec;
    }
}

__device__ __forceinline__ uint64_t tri(uint64_t t) { return t * (t + 1) / 2; }

// tiles of every run (0 for a single entry), and the pairs inside the runs (n_pairs_evaluated)
__global__ __launch_bounds__(256) void seq_run_tasks_kernel(const uint64_t *__restrict__ run_id,
                                                            const uint32_t *__restrict__ run_start, uint32_t n_rec,
                                                            uint64_t *__restrict__ n_tasks,
                                                            unsigned long long *__restrict__ counters)
{
    const uint64_t n_runs = run_id[n_rec - 1];
    unsigned long long pairs = 0;
    for (uint32_t r = blockIdx.x * blockDim.x + threadIdx.x; r < n_rec; r += gridDim.x * blockDim.x) {
        uint64_t t = 0;
        if (r < n_runs) {
            const uint64_t m = run_start[r + 1] - run_start[r];
            if (m >= 2) {
                t = tri((m + SEQ_TILE - 1) / SEQ_TILE);
                pairs += m * (m - 1) / 2;
            }
        }
        n_tasks[r] = t;
    }
    for (int off = 32; off > 0; off >>= 1) pairs += __shfl_down(pairs, off);
    if ((threadIdx.x & 63) == 0 && pairs) atomicAdd(&counters[CNT_SEG_PAIRS], pairs);
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// bitset.rs:85-87 for one word
__device__ __forceinline__ int word_bcx(uint64_t ka, uint64_t na, uint64_t kb, uint64_t nb)
{
    const uint64_t x = na ^ nb;
    return __builtin_popcountll(x | (ka ^ kb)) - __builtin_popcountll(x) / 3;
}

// One wave per task (a 64x64 tile of one run), tasks dealt over a persistent grid.
template <bool HAS_N>
__global__ __launch_bounds__(64) void seq_pair_kernel(SeqPairArgs a)
{
    __shared__ EdgeStage stage;
    const int lane = threadIdx.x;
    if (lane == 0) {
        stage.count = 0;
        stage.candidates = 0;
    }
    __syncthreads();
    const uint64_t n_runs = a.run_id[a.n_rec - 1];
    const uint64_t total = a.task_end[n_runs - 1];
    const int lim = 2 * a.k + 2; // dist <= k  <=>  summed bit_count_xor < 2k + 2
    unsigned int n_cand = 0;
    for (uint64_t t = blockIdx.x; t < total; t += gridDim.x) {
        uint64_t lo = 0, hi = n_runs - 1; // first run with task_end > t
        while (lo < hi) {
            const uint64_t mid = (lo + hi) / 2;
            if (a.task_end[mid] > t) hi = mid;
            else lo = mid + 1;
        }
        const uint32_t run = (uint32_t)lo;
        const uint64_t q = t - (run ? a.task_end[run - 1] : 0ull);
        const uint32_t rs = a.run_start[run], m = a.run_start[run + 1] - rs;
        const uint64_t nt = (m + SEQ_TILE - 1) / SEQ_TILE;
        // row tile rt: tasks before it = rt * nt - rt (rt - 1) / 2
        auto before = [nt](uint64_t rt) { return rt * nt - rt * (rt - 1) / 2; };
        const double bq = 2.0 * (double)nt + 1.0;
        uint64_t rt = (uint64_t)max(0.0, floor((bq - sqrt(max(0.0, bq * bq - 8.0 * (double)q))) / 2.0));
        if (rt >= nt) rt = nt - 1;
        while (rt > 0 && before(rt) > q) rt--;
        while (rt + 1 < nt && before(rt + 1) <= q) rt++;
        const uint64_t ct = rt + (q - before(rt));
        const SeqGroup g = a.groups[a.rkey[rs] >> 32];
        const int nw = (int)g.nw;
        const bool diag = rt == ct;

        const uint32_t pr = (uint32_t)rt * SEQ_TILE + (uint32_t)lane, pc = (uint32_t)ct * SEQ_TILE + (uint32_t)lane;
        const bool row_ok = pr < m, col_ok = pc < m;
        const uint32_t er = row_ok ? a.rval[rs + pr] : 0u, ec = col_ok ? a.rval[rs + pc] : 0u;
        uint64_t kr[SEQ_MAX_WORDS], nr[SEQ_MAX_WORDS], kc[SEQ_MAX_WORDS], nc[SEQ_MAX_WORDS];
#pragma unroll
        for (int w = 0; w < SEQ_MAX_WORDS; w++) {
            const bool in = w < nw;
            kr[w] = (in && row_ok) ? a.keys[(size_t)er * a.stride + w] : 0ull;
            kc[w] = (in && col_ok) ? a.keys[(size_t)ec * a.stride + w] : 0ull;
            nr[w] = (HAS_N && in && row_ok) ? a.nmask[(size_t)er * a.stride + w] : 0ull;
            nc[w] = (HAS_N && in && col_ok) ? a.nmask[(size_t)ec * a.stride + w] : 0ull;
        }
        const int32_t fr = row_ok ? a.freq[er] : 0, tr = row_ok ? a.thr[er] : 0;
        const int32_t fc = col_ok ? a.freq[ec] : 0, tc = col_ok ? a.thr[ec] : 0;
        const uint32_t ncols = min((uint32_t)SEQ_TILE, m - (uint32_t)ct * SEQ_TILE);
        for (uint32_t j = 0; j < ncols; j++) { // (wave-uniform trip count)
            // rows that take part: inside the run, and below the column on the diagonal tile
            int res = (row_ok && (!diag || (uint32_t)lane < j)) ? 0 : lim;
#pragma unroll
            for (int w = 0; w < SEQ_MAX_WORDS; w++) {
                if (w >= nw || __ballot(res < lim) == 0ull) break;
                res += word_bcx(kr[w], nr[w], readlane64(kc[w], (int)j), HAS_N ? readlane64(nc[w], (int)j) : 0ull);
            }
            const bool near = res < lim;
            if (__ballot(near) == 0ull) continue;
            // exactly once: part g.part equal, no earlier part equal (the xor words, from the column's lane)
            uint64_t d[SEQ_MAX_WORDS];
#pragma unroll
            for (int w = 0; w < SEQ_MAX_WORDS; w++) d[w] = w < nw ? kr[w] ^ readlane64(kc[w], (int)j) : 0ull;
            bool take = near;
            if (take && g.part != SEQ_ALL_PAIRS) { // (a partitioned bucket has at most 256 / 8 = 32 parts)
                uint64_t differs = 0; // bit jp: part jp is not equal
#pragma unroll
                for (int w = 0; w < SEQ_MAX_WORDS; w++) {
                    if (!d[w]) continue;
                    for (uint32_t jp = 0; jp <= g.part; jp++)
                        if (d[w] & part_mask(w, part_lo(jp, g.len, g.n_parts), part_lo(jp + 1, g.len, g.n_parts)))
                            differs |= 1ull << jp;
                }
                const uint64_t earlier = (1ull << g.part) - 1ull;
                take = !((differs >> g.part) & 1ull) && (differs & earlier) == earlier;
            }
            const uint32_t gj = (uint32_t)__builtin_amdgcn_readlane((int)ec, (int)j);
            const int32_t fj = __builtin_amdgcn_readlane(fc, (int)j), tj = __builtin_amdgcn_readlane(tc, (int)j);
            if (!take) continue;
            n_cand++;
            const int dist = res / 2;
            bool fwd, bwd;
            if (a.mode == MODE_DIRECTIONAL) { // naive.rs:31 with max_freq = threshold(start) (directional.rs:38-39)
                fwd = fj <= tr;
                bwd = fr <= tj;
            } else if (a.mode == MODE_CLUSTER) { // connected components: a union, nothing to ask of freq
                fwd = bwd = true;
            } else { // adjacency.rs:56: a root only ever sees entries of larger rank
                fwd = fj <= a.adj_max_freq;
                bwd = false;
            }
            if (fwd && bwd) emit_edge(&stage, a.edges, nullptr, a.counters, a.edge_cap, er | SYM_FLAG, gj, dist, false);
            else if (fwd) emit_edge(&stage, a.edges, nullptr, a.counters, a.edge_cap, er, gj, dist, false);
            else if (bwd) emit_edge(&stage, a.edges, nullptr, a.counters, a.edge_cap, gj, er, dist, false);
        }
        flush_edges<64>(&stage, a.edges, nullptr, a.counters, a.edge_cap, false, false);
    }
    flush_edges<64>(&stage, a.edges, nullptr, a.counters, a.edge_cap, false, true);
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off);
    if (lane == 0 && n_cand) atomicAdd(&a.counters[CNT_CANDIDATES], (unsigned long long)n_cand);
}

constexpr uint32_t grid_of(uint32_t n, uint32_t threads, uint32_t cap)
{
    return n == 0 ? 1u : ((n + threads - 1) / threads < cap ? (n + threads - 1) / threads : cap);
}

} // namespace

hipError_t launch_seq_records(const SeqGroup *groups, uint32_t n_groups, uint32_t n_rec, const uint64_t *keys,
                              const uint64_t *nmask, int stride, const int32_t *freq, float percentage, int32_t *thr,
                              uint64_t *rkey, uint32_t *rval, unsigned long long *counters, hipStream_t s)
{
    if (n_rec == 0) return hipSuccess;
    seq_records_kernel<<<grid_of(n_rec, 256, 4096), 256, 0, s>>>(groups, n_groups, n_rec, keys, nmask, stride, freq,
                                                                 percentage, thr, rkey, rval, counters);
    return hipGetLastError();
}

hipError_t launch_seq_runs(const uint64_t *rkey, uint32_t n_rec, uint64_t *flag, uint64_t *run_id,
                           uint32_t *run_start, uint64_t *task_end, void *scan_temp, size_t scan_temp_size,
                           unsigned long long *counters, hipStream_t s)
{
    if (n_rec == 0) return hipSuccess;
    const uint32_t grid = grid_of(n_rec, 256, 4096);
    seq_run_flags_kernel<<<grid, 256, 0, s>>>(rkey, n_rec, flag);
    hipError_t e = scan_inclusive_u64(flag, run_id, n_rec, scan_temp, scan_temp_size, s);
    if (e != hipSuccess) return e;
    seq_run_starts_kernel<<<grid, 256, 0, s>>>(flag, run_id, n_rec, run_start);
    seq_run_tasks_kernel<<<grid, 256, 0, s>>>(run_id, run_start, n_rec, flag, counters); // (flag: the tiles per run)
    return scan_inclusive_u64(flag, task_end, n_rec, scan_temp, scan_temp_size, s);
}

hipError_t launch_seq_pairs(const SeqPairArgs &a, uint32_t n_blocks, hipStream_t s)
{
    if (a.n_rec == 0) return hipSuccess;
    if (a.nmask) seq_pair_kernel<true><<<n_blocks, 64, 0, s>>>(a);
    else seq_pair_kernel<false><<<n_blocks, 64, 0, s>>>(a);
    return hipGetLastError();
}

} // namespace umihip
