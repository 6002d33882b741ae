// What a batched call did to its buckets, as tables (umi_dedup_stats, the program's --output-stats), gfx950:
// family sizes before and after, the mean UMI distance of every bucket before and after against a null, and
// how every UMI sequence is used.  No counterpart in the reference; the tables are umi_tools dedup
// --output-stats's, tests/stats_model.py defines them.  Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The mean pair distance of a set of m UMIs needs no pairs: per base the differing pairs are
// C(m, 2) - sum over the five letters C(count, 2), so a bucket costs one pass over its keys.
//
// The host walks the bucket table once: empty buckets are left out (m non-empty ones remain), buckets of at
// least "stats_split" entries are cut into pieces of STATS_PIECE entries for the whole grid.
//
//   entry    per entry: the key's codes are checked, freq goes to the family sizes before and, as 64 bits, to
//            the scan's input.  The low STATS_HIST_LDS bins are a block's own in LDS, added to the output at
//            the block's end; the rest are global atomics.
//   scan     scan_inclusive_u64: cum[] (umihip_radix.hip).
//   pick     per entry i the null's draw pick(i): splitmix64 of the seed and i, scaled to the reads, a binary
//            search in cum[].  4 bytes per entry; the post null is a prefix of the pre null's draws.
//   bucket   the buckets below the split, 256 per block at a time, in two kernels (one kernel for both spilled
//            scalar registers).  A bucket of up to STATS_LANE_MAX entries is its lane's: it checks root[], adds up
//            total[] (nobody else touches its bucket's words) and compares its few pairs directly.  A larger one is
//            queued in LDS and taken by one of the block's waves: root[] is checked and total[] added by atomics, the lanes of a wave that
//            share a root first summed over the wave; then 64 entries at a time, per base, six ballots (own
//            letter number's bits x 3, drawn x 3) under two masks (kept, i < s + kept entries) give twenty counts, which
//            lanes 0..19 add to the wave's [umi_len][5][4] table in LDS; the table's finish gives the four bins.
//            The bins are counted in LDS per block.
//   deep     buckets at or above the split: kept count and total[] by piece, the counts by piece into the
//            bucket's global table (atomics, from the wave's LDS table), a wave per bucket to finish.
//   post     per kept entry: total[] to the family sizes after.
//   per UMI  (optional) a stable radix_sort_pairs_u64 per key word, word 0 first, carrying the entry; heads, a
//            scan, and the runs' sums over the wave (umihip_pair_table.h: WaveRuns).
//
// One synchronisation, at the end.  Bytes moved per entry without the per-UMI table: keys 8 W read three times
// (entry, bucket, and gathered through the draw), freq 4 x 2, kept 1 x 3, root 4, cum 8 written and ~log2(N)
// cached reads of it, draw 4 + 4, total[] 8 zeroed + an atomic + 8 read: ~60 + 24 W.  The table adds 2 x 12
// bytes per sort pass, 8 passes per full key word, and 56 for heads, scan and sums.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

namespace {

constexpr int ST_THREADS = 256, ST_WAVES = ST_THREADS / 64;
constexpr int ST_CELLS = 20;   // per base: 5 letters x 4 sets (0 pre, 1 pre-null, 2 post, 3 post-null)
constexpr int ST_MAX_LEN = 85;
constexpr int ST_TAB = ST_MAX_LEN * ST_CELLS;

struct StatsWs {
    unsigned long long *ctl;   // [0] keys with a code that is no letter, [1] entries whose root[] breaks the contract
    unsigned long long *total; // [n]
    uint64_t *f64, *cum;       // [n] each; the per-UMI table's flags and their scan afterwards
    uint32_t *picked;          // [n]
    uint64_t *off;             // [m + 1]
    StatsTask *tasks;          // [n_tasks]
    uint32_t *deep_j, *deep_kept, *deep_tab; // [g], [g], [g * L * 20]
    uint64_t *ka, *kb;
    uint32_t *va, *vb;
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes, total_bytes;
};
StatsWs stats_carve(void *ws, uint32_t n, uint32_t m, uint32_t g, uint32_t n_tasks, int L, bool per_umi)
{
    StatsWs w;
    Carver c(ws);
    w.ctl = c.take<unsigned long long>(256); // (total[] right behind it: bad_roots)
    w.total = c.take<unsigned long long>((size_t)n * 8);
    w.f64 = c.take<uint64_t>((size_t)n * 8);
    w.cum = c.take<uint64_t>((size_t)n * 8);
    w.picked = c.take<uint32_t>((size_t)n * 4);
    w.off = c.take<uint64_t>(((size_t)m + 1) * 8);
    w.tasks = c.take<StatsTask>((size_t)n_tasks * sizeof(StatsTask));
    w.deep_j = c.take<uint32_t>((size_t)g * 4);
    w.deep_kept = c.take<uint32_t>((size_t)g * 4);
    w.deep_tab = c.take<uint32_t>((size_t)g * (size_t)L * ST_CELLS * 4);
    w.ka = w.kb = nullptr;
    w.va = w.vb = nullptr;
    w.radix_tmp = nullptr;
    w.radix_bytes = 0;
    if (per_umi) {
        w.ka = c.take<uint64_t>((size_t)n * 8);
        w.kb = c.take<uint64_t>((size_t)n * 8);
        w.va = c.take<uint32_t>((size_t)n * 4);
        w.vb = c.take<uint32_t>((size_t)n * 4);
        w.radix_bytes = radix_sort_temp_bytes(n);
        w.radix_tmp = c.take(w.radix_bytes);
    }
    w.scan_bytes = scan_temp_bytes(n);
    w.scan_tmp = c.take(w.scan_bytes);
    w.total_bytes = c.o;
    return w;
}

struct StatsArgs {
    const uint64_t *keys;
    const int32_t *freq;
    const uint8_t *kept;
    const uint32_t *root;
    const uint64_t *off; // [m + 1]: the non-empty buckets
    const uint32_t *picked;
    unsigned long long *total, *dist; // dist: [4][L + 2]; the control words lie 256 bytes in front of total[] (bad_roots)
    uint64_t gm[4];                         // per key word: the lowest bit of every base below L that starts in it
    uint32_t m, split;
    int L, W;
};

// where the entries whose root[] breaks the contract are counted: the workspace begins with the control words, total[]
// follows them (one pointer less in the argument block: the wave kernel is at the limit of its scalar registers)
__device__ __forceinline__ unsigned long long *bad_roots(const StatsArgs &a) { return a.total - 32 + 1; }

// the five codes' letter numbers: 000 A 0, 110 C 1, 011 G 2, 101 T 3, 100 N 4 (anything else counts as A;
// the entry kernel has counted it and the call fails)
__device__ __forceinline__ uint32_t letter_of(uint32_t code) { return (0x01342000u >> (4u * code)) & 7u; }
__device__ __forceinline__ bool is_letter(uint32_t code) { return (0x79u >> code) & 1u; } // 0, 3, 4, 5, 6

__device__ __forceinline__ void load_key(const uint64_t *__restrict__ keys, uint64_t i, int W, uint64_t (&k)[4])
{
#pragma unroll
    for (int w = 0; w < 4; w++) k[w] = w < W ? keys[i * (uint64_t)W + w] : 0ull;
}

// f(b, code) for every base b < L: the 3-bit code at bits [3b, 3b + 3) of the key as one little-endian integer
// (bases 21 and 42 straddle two words).  Word by word, so that k[] is only indexed by constants.
template <typename F> __device__ __forceinline__ void for_each_base(const uint64_t (&k)[4], int L, F f)
{
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const int b0 = (64 * w + 2) / 3, b1 = min(L, (64 * w + 63) / 3 + 1); // the bases that start in word w
        for (int b = b0; b < b1; b++) {
            const int sh = 3 * b - 64 * w;
            uint64_t c = k[w] >> sh;
            if (w < 3 && sh > 61) c |= k[w + 1] << (64 - sh);
            f(b, (uint32_t)c & 7u);
        }
    }
}

// bases below L in which two keys differ (two letters differ iff their codes differ)
__device__ __forceinline__ uint32_t letter_distance(const uint64_t (&a)[4], const uint64_t (&b)[4], const uint64_t (&gm)[4])
{
    uint32_t d = 0;
#pragma unroll
    for (int w = 0; w < 4; w++) {
        const uint64_t x = a[w] ^ b[w], xn = w < 3 ? a[w + 1] ^ b[w + 1] : 0ull;
        const uint64_t y = x | (x >> 1) | (xn << 63) | (x >> 2) | (xn << 62); // bit j: bits j, j + 1, j + 2 of the difference
        d += (uint32_t)__builtin_popcountll(y & gm[w]);
    }
    return d;
}

// total[idx] += val for the lanes with `todo`, all lanes of the wave calling together: the lanes that share the
// first pending lane's word send one atomic for their sum, twice; what is left goes one by one (one component
// of 10^6 entries would otherwise put every atomic on one word)
__device__ __forceinline__ void wave_add_u64(unsigned long long *arr, uint32_t idx, unsigned long long val, bool todo)
{
    const int lane = (int)(threadIdx.x & 63u);
    for (int pass = 0; pass < 2 && __any(todo); pass++) {
        const int leader = __ffsll((unsigned long long)__ballot(todo)) - 1;
        const uint32_t tgt = (uint32_t)__shfl((int)idx, leader);
        const bool mine = todo && idx == tgt;
        unsigned long long v = mine ? val : 0ull;
#pragma unroll
        for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
        if (lane == leader) atomicAdd(&arr[tgt], v);
        todo = todo && !mine;
    }
    if (todo) atomicAdd(&arr[idx], val);
}

// one more in bin min(v, bins - 1): a block's LDS copy for the low bins (the lanes that share the first lane's
// bin counted by one of them), a global atomic for the rest.  Every lane of the wave calls.
__device__ __forceinline__ void hist_add(uint32_t *lds, unsigned long long *glob, unsigned long long v, uint32_t bins, bool todo)
{
    const uint32_t bin = (uint32_t)min(v, (unsigned long long)(bins - 1u));
    const unsigned long long pending = __ballot(todo);
    if (pending) {
        const int leader = __ffsll(pending) - 1;
        const uint32_t tgt = (uint32_t)__shfl((int)bin, leader);
        const bool mine = todo && bin == tgt;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(__ballot(mine));
        if ((int)(threadIdx.x & 63u) == leader) {
            if (tgt < STATS_HIST_LDS) atomicAdd(&lds[tgt], cnt);
            else atomicAdd(&glob[tgt], (unsigned long long)cnt);
        }
        todo = todo && !mine;
    }
    if (todo) {
        if (bin < STATS_HIST_LDS) atomicAdd(&lds[bin], 1u);
        else atomicAdd(&glob[bin], 1ull);
    }
}
__device__ __forceinline__ void hist_flush(const uint32_t *lds, unsigned long long *glob, uint32_t bins)
{
    __syncthreads();
    for (uint32_t b = threadIdx.x; b < min(bins, STATS_HIST_LDS); b += ST_THREADS)
        if (lds[b]) atomicAdd(&glob[b], (unsigned long long)lds[b]);
}

__global__ __launch_bounds__(ST_THREADS) void stats_entry_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ freq,
                                                                 uint32_t n, int L, int W, uint32_t bins, uint64_t *__restrict__ f64,
                                                                 unsigned long long *hist_pre, unsigned long long *ctl)
{
    __shared__ uint32_t hist[STATS_HIST_LDS];
    for (uint32_t b = threadIdx.x; b < STATS_HIST_LDS; b += ST_THREADS) hist[b] = 0;
    __syncthreads();
    uint32_t bad = 0;
    const uint64_t rounds = ((uint64_t)n + ST_THREADS - 1) / ST_THREADS;
    for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) { // (whole waves go round: hist_add is a wave's call)
        const uint64_t i = r * ST_THREADS + threadIdx.x;
        const bool valid = i < n;
        unsigned long long f = 0;
        if (valid) {
            uint64_t k[4];
            load_key(keys, i, W, k);
            bool ok = true;
            for_each_base(k, L, [&](int, uint32_t code) { ok = ok && is_letter(code); });
            bad += !ok;
            f = (unsigned long long)(long long)freq[i];
            f64[i] = f;
        }
        hist_add(hist, hist_pre, f, bins, valid);
    }
    if (bad) atomicAdd(ctl, (unsigned long long)bad);
    hist_flush(hist, hist_pre, bins);
}

// pick(i): an entry drawn with probability proportional to its reads
__device__ __forceinline__ uint32_t pick_entry(const uint64_t *__restrict__ cum, uint32_t n, uint64_t R, uint64_t seed, uint64_t i)
{
    uint64_t x = seed + 0x9E3779B97F4A7C15ull * (i + 1ull);
    x ^= x >> 30;
    x *= 0xBF58476D1CE4E5B9ull;
    x ^= x >> 27;
    x *= 0x94D049BB133111EBull;
    x ^= x >> 31;
    const uint64_t t = __umul64hi(x, R);
    uint32_t lo = 0, hi = n - 1; // the smallest e with cum[e] > t; it is at most n - 1 whatever cum[] holds
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (cum[mid] > t) hi = mid;
        else lo = mid + 1;
    }
    return lo;
}
__global__ __launch_bounds__(ST_THREADS) void stats_pick_kernel(const uint64_t *__restrict__ cum, uint32_t n, uint64_t seed,
                                                                uint32_t *__restrict__ picked)
{
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i < n) picked[i] = pick_entry(cum, n, cum[n - 1], seed, i);
}

__global__ __launch_bounds__(ST_THREADS) void stats_post_kernel(const uint8_t *__restrict__ kept, const unsigned long long *__restrict__ total,
                                                                uint32_t n, uint32_t bins, unsigned long long *hist_post)
{
    __shared__ uint32_t hist[STATS_HIST_LDS];
    for (uint32_t b = threadIdx.x; b < STATS_HIST_LDS; b += ST_THREADS) hist[b] = 0;
    __syncthreads();
    const uint64_t rounds = ((uint64_t)n + ST_THREADS - 1) / ST_THREADS;
    for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) {
        const uint64_t i = r * ST_THREADS + threadIdx.x;
        const bool todo = i < n && kept[i] != 0;
        hist_add(hist, hist_post, todo ? total[i] : 0ull, bins, todo);
    }
    hist_flush(hist, hist_post, bins);
}

// root[] of the entries [lo, hi) of bucket [s, e) checked, their reads added to total[]; returns the kept ones
// among them (wave-uniform).  A wave's call.
__device__ __forceinline__ uint32_t wave_roots(const StatsArgs &a, uint32_t s, uint32_t e, uint32_t lo, uint32_t hi)
{
    const uint32_t lane = threadIdx.x & 63u;
    uint32_t mk = 0, bad = 0;
    for (uint32_t base = lo; base < hi; base += 64) { // (entries stay below 2^31)
        const uint32_t i = base + lane;
        const bool valid = i < hi;
        uint32_t r = 0;
        unsigned long long f = 0;
        bool kp = false, ok = false;
        if (valid) {
            r = a.root[i];
            kp = a.kept[i] != 0;
            ok = r >= s && r < e && (kp ? r == i : a.kept[r] != 0);
            f = (unsigned long long)(long long)a.freq[i];
        }
        mk += (uint32_t)__builtin_popcountll(__ballot(kp));
        bad += valid && !ok;
        wave_add_u64(a.total, r, f, ok);
    }
    for (int o = 32; o > 0; o >>= 1) bad += __shfl_xor(bad, o);
    if (lane == 0 && bad) atomicAdd(bad_roots(a), (unsigned long long)bad);
    return mk;
}

// the letters of the entries [lo, hi) counted into the wave's table tab[L][5][4]; post_end: the entries below
// it draw for the post null.  A wave's call; lanes 0..19 own a (letter, set) each.
__device__ __forceinline__ void wave_count(const StatsArgs &a, uint32_t *tab, uint32_t lo, uint32_t hi, uint32_t post_end)
{
    const uint32_t lane = threadIdx.x & 63u;
    const uint32_t my_letter = (lane >> 2) % 5u, my_set = lane & 3u;
    const bool from_drawn = (my_set & 1u) != 0;
    const unsigned long long flip[3] = {(my_letter & 1u) ? 0ull : ~0ull, (my_letter & 2u) ? 0ull : ~0ull, (my_letter & 4u) ? 0ull : ~0ull};
    for (uint32_t base = lo; base < hi; base += 64) {
        const uint32_t i = base + lane;
        const bool valid = i < hi;
        uint64_t k[4] = {0, 0, 0, 0}, q[4] = {0, 0, 0, 0};
        bool kp = false;
        if (valid) {
            load_key(a.keys, i, a.W, k);
            load_key(a.keys, a.picked[i], a.W, q);
            kp = a.kept[i] != 0;
        }
        const unsigned long long in_all = __ballot(valid), in_kept = __ballot(kp), in_post = __ballot(valid && i < post_end);
        const unsigned long long my_mask = my_set == 2 ? in_kept : my_set == 3 ? in_post : in_all;
#pragma unroll
        for (int w = 0; w < 4; w++) {
            const int b0 = (64 * w + 2) / 3, b1 = min(a.L, (64 * w + 63) / 3 + 1);
#pragma unroll 1
            for (int b = b0; b < b1; b++) { // (not unrolled: ten ballots a base are twenty scalar registers)
                const int sh = 3 * b - 64 * w;
                uint64_t c = k[w] >> sh, d = q[w] >> sh;
                if (w < 3 && sh > 61) {
                    c |= k[w + 1] << (64 - sh);
                    d |= q[w + 1] << (64 - sh);
                }
                const uint32_t own = letter_of((uint32_t)c & 7u), drawn = letter_of((uint32_t)d & 7u);
                // the lanes that hold the lane's letter: the letter numbers' three bits by ballot, own and drawn, and
                // bit by bit the side that agrees with the lane's letter (six ballots live, not ten)
                unsigned long long mine = my_mask;
#pragma unroll
                for (uint32_t bit = 0; bit < 3; bit++) {
                    const unsigned long long bo = __ballot((own >> bit) & 1u), bd = __ballot((drawn >> bit) & 1u);
                    mine &= (from_drawn ? bd : bo) ^ flip[bit];
                }
                if (lane < ST_CELLS) tab[b * ST_CELLS + lane] += (uint32_t)__builtin_popcountll(mine);
            }
        }
    }
}

// the four bins of a bucket of n_all entries, n_kept of them kept, from its table: one more in each.  A wave's call.
template <typename Count>
__device__ __forceinline__ void wave_finish(const uint32_t *tab, int L, uint64_t n_all, uint64_t n_kept, Count *dist)
{
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long same[4] = {0, 0, 0, 0}; // per set: the pairs that agree, summed over the bases
    for (int b = (int)lane; b < L; b += 64)
#pragma unroll
        for (int c = 0; c < ST_CELLS; c++) {
            const unsigned long long v = tab[b * ST_CELLS + c];
            same[c & 3] += v * (v - 1ull) / 2ull; // (v = 0: the product is 0)
        }
#pragma unroll
    for (int s = 0; s < 4; s++)
        for (int o = 32; o > 0; o >>= 1) same[s] += __shfl_xor(same[s], o);
    if (lane < 4) {
        const unsigned long long mset = lane < 2 ? n_all : n_kept;
        const unsigned long long sm = lane == 0 ? same[0] : lane == 1 ? same[1] : lane == 2 ? same[2] : same[3];
        if (mset == 1) {
            atomicAdd(&dist[lane * (uint32_t)(L + 2) + (uint32_t)(L + 1)], (Count)1);
        } else if (mset > 1) {
            const unsigned long long P = mset * (mset - 1ull) / 2ull, S = (unsigned long long)L * P - sm;
            const unsigned long long bin = min((S + P - 1ull) / P, (unsigned long long)L); // (S <= L P: the clamp only guards the table)
            atomicAdd(&dist[lane * (uint32_t)(L + 2) + (uint32_t)bin], (Count)1);
        }
    }
}

// the buckets of up to STATS_LANE_MAX entries, a lane each
__global__ __launch_bounds__(ST_THREADS) void stats_lane_kernel(StatsArgs a)
{
    __shared__ uint32_t dist[4 * (ST_MAX_LEN + 2)];
    const uint32_t tid = threadIdx.x;
    const uint32_t L = (uint32_t)a.L, row = L + 2;
    for (uint32_t t = tid; t < 4 * row; t += ST_THREADS) dist[t] = 0;
    __syncthreads();
    for (uint64_t base = (uint64_t)blockIdx.x * ST_THREADS; base < a.m; base += (uint64_t)gridDim.x * ST_THREADS) {
        const uint64_t j = base + tid;
        if (j < a.m) {
            const uint64_t lo = a.off[j], hi = a.off[j + 1], n = hi - lo;
            if (n <= STATS_LANE_MAX) {
                // the lane's own bucket: root[] and total[] (its words are nobody else's), then its few pairs
                uint32_t mk = 0, bad = 0;
                for (uint64_t i = lo; i < hi; i++) {
                    const uint32_t r = a.root[i];
                    const bool kp = a.kept[i] != 0;
                    const bool ok = r >= lo && r < hi && (kp ? r == i : a.kept[r] != 0);
                    mk += kp;
                    bad += !ok;
                    if (ok) a.total[r] += (unsigned long long)(long long)a.freq[i];
                }
                if (bad) atomicAdd(bad_roots(a), (unsigned long long)bad);
                if (n == 1) {
                    atomicAdd(&dist[0 * row + L + 1], 1u);
                    atomicAdd(&dist[1 * row + L + 1], 1u);
                    if (mk == 1) {
                        atomicAdd(&dist[2 * row + L + 1], 1u);
                        atomicAdd(&dist[3 * row + L + 1], 1u);
                    }
                } else {
                    uint32_t S[4] = {0, 0, 0, 0};
                    const uint64_t post_end = lo + mk;
                    for (uint64_t i = lo; i + 1 < hi; i++) {
                        uint64_t ki[4], qi[4];
                        load_key(a.keys, i, a.W, ki);
                        load_key(a.keys, a.picked[i], a.W, qi);
                        const bool kpi = a.kept[i] != 0;
                        for (uint64_t u = i + 1; u < hi; u++) {
                            uint64_t ku[4], qu[4];
                            load_key(a.keys, u, a.W, ku);
                            load_key(a.keys, a.picked[u], a.W, qu);
                            const uint32_t d = letter_distance(ki, ku, a.gm), dn = letter_distance(qi, qu, a.gm);
                            S[0] += d;
                            S[1] += dn;
                            if (kpi && a.kept[u] != 0) S[2] += d;
                            if (u < post_end) S[3] += dn; // (i < u)
                        }
                    }
                    const uint32_t P_all = (uint32_t)(n * (n - 1) / 2), P_kept = mk * (mk - 1u) / 2u;
                    atomicAdd(&dist[0 * row + min((S[0] + P_all - 1u) / P_all, L)], 1u);
                    atomicAdd(&dist[1 * row + min((S[1] + P_all - 1u) / P_all, L)], 1u);
                    if (mk == 1) {
                        atomicAdd(&dist[2 * row + L + 1], 1u);
                        atomicAdd(&dist[3 * row + L + 1], 1u);
                    } else if (mk > 1) {
                        atomicAdd(&dist[2 * row + min((S[2] + P_kept - 1u) / P_kept, L)], 1u);
                        atomicAdd(&dist[3 * row + min((S[3] + P_kept - 1u) / P_kept, L)], 1u);
                    }
                }
            }
        }
    }
    __syncthreads();
    for (uint32_t t = tid; t < 4 * row; t += ST_THREADS)
        if (dist[t]) atomicAdd(&a.dist[t], (unsigned long long)dist[t]);
}

// the buckets above that and below the split: queued in LDS, 256 buckets at a time, and taken by the block's waves
__global__ __launch_bounds__(ST_THREADS) void stats_wave_kernel(StatsArgs a)
{
    __shared__ uint32_t queue[ST_THREADS];
    __shared__ uint32_t queued;
    __shared__ uint32_t dist[4 * (ST_MAX_LEN + 2)];
    __shared__ uint32_t tabs[ST_WAVES][ST_TAB];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, wave = tid >> 6;
    const uint32_t L = (uint32_t)a.L, row = L + 2;
    for (uint32_t t = tid; t < 4 * row; t += ST_THREADS) dist[t] = 0;
    for (uint32_t base = blockIdx.x * ST_THREADS; base < a.m; base += gridDim.x * ST_THREADS) { // (m < 2^31, the grid small)
        if (tid == 0) queued = 0;
        __syncthreads();
        const uint32_t j = base + tid;
        if (j < a.m) {
            const uint64_t n = a.off[j + 1] - a.off[j];
            if (n > STATS_LANE_MAX && n < a.split) queue[atomicAdd(&queued, 1u)] = tid; // (the others are the deep kernels')
        }
        __syncthreads();
        const uint32_t nq = queued;
        uint32_t *tab = tabs[wave];
        for (uint32_t t = wave; t < nq; t += ST_WAVES) {
            const uint32_t jb = base + queue[t];
            const uint32_t lo = (uint32_t)a.off[jb], hi = (uint32_t)a.off[jb + 1];
            for (uint32_t c = lane; c < L * ST_CELLS; c += 64) tab[c] = 0;
            const uint32_t mk = wave_roots(a, lo, hi, lo, hi);
            wave_count(a, tab, lo, hi, lo + mk);
            wave_finish(tab, a.L, hi - lo, mk, dist);
        }
        __syncthreads(); // (the queue is the next round's as well)
    }
    __syncthreads();
    for (uint32_t t = tid; t < 4 * row; t += ST_THREADS)
        if (dist[t]) atomicAdd(&a.dist[t], (unsigned long long)dist[t]);
}

// ---- buckets at or above the split: a wave per piece, twice, then a wave per bucket
__global__ __launch_bounds__(ST_THREADS) void stats_deep_roots_kernel(StatsArgs a, const StatsTask *__restrict__ tasks, uint32_t n_tasks,
                                                                      const uint32_t *__restrict__ deep_j, uint32_t *deep_kept)
{
    const uint32_t lane = threadIdx.x & 63u;
    for (uint32_t t = blockIdx.x * ST_WAVES + (threadIdx.x >> 6); t < n_tasks; t += gridDim.x * ST_WAVES) {
        const StatsTask k = tasks[t];
        const uint32_t j = deep_j[k.deep];
        const uint32_t mk = wave_roots(a, (uint32_t)a.off[j], (uint32_t)a.off[j + 1], (uint32_t)k.lo, (uint32_t)k.hi);
        if (lane == 0 && mk) atomicAdd(&deep_kept[k.deep], mk);
    }
}
__global__ __launch_bounds__(ST_THREADS) void stats_deep_count_kernel(StatsArgs a, const StatsTask *__restrict__ tasks, uint32_t n_tasks,
                                                                      const uint32_t *__restrict__ deep_j,
                                                                      const uint32_t *__restrict__ deep_kept, uint32_t *deep_tab)
{
    __shared__ uint32_t tabs[ST_WAVES][ST_TAB];
    const uint32_t lane = threadIdx.x & 63u, cells = (uint32_t)a.L * ST_CELLS;
    uint32_t *tab = tabs[threadIdx.x >> 6];
    for (uint32_t t = blockIdx.x * ST_WAVES + (threadIdx.x >> 6); t < n_tasks; t += gridDim.x * ST_WAVES) {
        const StatsTask k = tasks[t];
        for (uint32_t c = lane; c < cells; c += 64) tab[c] = 0;
        wave_count(a, tab, (uint32_t)k.lo, (uint32_t)k.hi, (uint32_t)a.off[deep_j[k.deep]] + deep_kept[k.deep]);
        for (uint32_t c = lane; c < cells; c += 64)
            if (tab[c]) atomicAdd(&deep_tab[(size_t)k.deep * cells + c], tab[c]);
    }
}
__global__ __launch_bounds__(64) void stats_deep_finish_kernel(StatsArgs a, const uint32_t *__restrict__ deep_j,
                                                               const uint32_t *__restrict__ deep_kept,
                                                               const uint32_t *__restrict__ deep_tab, uint32_t n_deep)
{
    const uint32_t g = blockIdx.x;
    if (g >= n_deep) return;
    const uint32_t j = deep_j[g];
    wave_finish(deep_tab + (size_t)g * (size_t)a.L * ST_CELLS, a.L, a.off[j + 1] - a.off[j], deep_kept[g], a.dist);
}

// ---- the per-UMI table
struct UmiMasks {
    uint64_t wm[4]; // per key word: the bits below 3 L
};
__global__ __launch_bounds__(ST_THREADS) void stats_word_kernel(const uint64_t *__restrict__ keys, int W, int w, uint64_t mask,
                                                                const uint32_t *__restrict__ order, uint32_t n,
                                                                uint64_t *__restrict__ out_key, uint32_t *__restrict__ out_val)
{
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = order ? order[i] : (uint32_t)i;
    out_key[i] = keys[(uint64_t)e * (uint64_t)W + (uint64_t)w] & mask;
    if (!order) out_val[i] = e;
}
__global__ __launch_bounds__(ST_THREADS) void stats_heads_kernel(const uint64_t *__restrict__ keys, int W, UmiMasks um,
                                                                 const uint32_t *__restrict__ order, uint32_t n,
                                                                 uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    if (i >= n) return;
    bool head = i == 0;
    if (!head) {
        const uint64_t x = order[i], y = order[i - 1];
        for (int w = 0; w < W; w++) head = head || ((keys[x * (uint64_t)W + w] ^ keys[y * (uint64_t)W + w]) & um.wm[w]) != 0;
    }
    flag[i] = head ? 1ull : 0ull;
}
// a lane per sorted entry: a run's sums are stored where the run begins and ends inside the wave, added by atomics
// where it crosses an edge
__global__ __launch_bounds__(ST_THREADS) void stats_umi_sum_kernel(const uint32_t *__restrict__ order, const uint64_t *__restrict__ incl,
                                                                   const int32_t *__restrict__ freq, const uint8_t *__restrict__ kept,
                                                                   const unsigned long long *__restrict__ total, uint32_t n,
                                                                   uint32_t *__restrict__ umi_entry, uint32_t *times_pre,
                                                                   unsigned long long *reads_pre, uint32_t *times_post,
                                                                   unsigned long long *reads_post)
{
    const uint64_t i = (uint64_t)blockIdx.x * ST_THREADS + threadIdx.x;
    const WaveRuns run(incl, i, n);
    uint32_t e = 0, tpre = 0, tpost = 0;
    unsigned long long rpre = 0, rpost = 0;
    if (run.valid) {
        e = order[i];
        tpre = 1;
        rpre = (unsigned long long)(long long)freq[e];
        if (kept[e] != 0) {
            tpost = 1;
            rpost = total[e];
        }
    }
    run.scan([](auto x, auto y) { return x + y; }, tpre, rpre, tpost, rpost);
    if (run.head) umi_entry[run.slot()] = e; // (the sorts are stable: the run's first is its smallest entry)
    if (run.tail()) {
        if (run.whole()) {
            times_pre[run.slot()] = tpre;
            reads_pre[run.slot()] = rpre;
            times_post[run.slot()] = tpost;
            reads_post[run.slot()] = rpost;
        } else {
            atomicAdd(times_pre + run.slot(), tpre);
            atomicAdd(reads_pre + run.slot(), rpre);
            atomicAdd(times_post + run.slot(), tpost);
            atomicAdd(reads_post + run.slot(), rpost);
        }
    }
}

} // namespace

void stats_plan(const uint64_t *h_off, uint32_t m, uint32_t split, int umi_len, uint32_t *split_used, uint32_t *n_deep,
                uint32_t *n_tasks)
{
    // (the deep buckets' tables, 80 bytes per base each, stay below 512 MB: the split rises by itself)
    uint64_t sp = split;
    for (;;) {
        uint64_t g = 0, t = 0;
        for (uint32_t j = 0; j < m; j++) {
            const uint64_t n = h_off[j + 1] - h_off[j];
            if (n >= sp) {
                g++;
                t += (n + STATS_PIECE - 1) / STATS_PIECE;
            }
        }
        if (g * (uint64_t)umi_len * ST_CELLS * 4 <= (512ull << 20) || sp >= (1ull << 30)) {
            *split_used = (uint32_t)sp;
            *n_deep = (uint32_t)g;
            *n_tasks = (uint32_t)t;
            return;
        }
        sp *= 2;
    }
}

size_t stats_workspace_bytes(uint32_t n, uint32_t m, uint32_t n_deep, uint32_t n_tasks, int umi_len, bool per_umi)
{
    return stats_carve(nullptr, n, m, n_deep, n_tasks, umi_len, per_umi).total_bytes;
}

int stats_on_device(void *workspace, const StatsCall &c, hipStream_t s)
{
    const uint32_t n = c.n, m = c.m;
    const int L = c.umi_len, W = c.n_words;
    const bool per_umi = c.d_umi_entry != nullptr;
    const StatsWs w = stats_carve(workspace, n, m, c.n_deep, c.n_tasks, L, per_umi);
    const size_t dist_words = 4 * ((size_t)L + 2);
    // the deep buckets and their pieces, into the caller's pinned block
    uint32_t *h_deep_j = c.h_deep_j;
    StatsTask *h_tasks = c.h_tasks;
    {
        uint32_t g = 0, t = 0;
        for (uint32_t j = 0; j < m; j++) {
            const uint64_t lo = c.h_off[j], hi = c.h_off[j + 1];
            if (hi - lo < c.split) continue;
            for (uint64_t p = lo; p < hi; p += STATS_PIECE) h_tasks[t++] = StatsTask{p, std::min<uint64_t>(hi, p + STATS_PIECE), g, 0u};
            h_deep_j[g++] = j;
        }
    }
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, 256, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.total, 0, (size_t)n * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(c.d_count_pre, 0, (size_t)c.hist_bins * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(c.d_count_post, 0, (size_t)c.hist_bins * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(c.d_dist, 0, dist_words * 8, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(w.off, c.h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (c.n_deep) {
        UMIHIP_TRY_NEG(hipMemcpyAsync(w.deep_j, h_deep_j, (size_t)c.n_deep * 4, hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemcpyAsync(w.tasks, h_tasks, (size_t)c.n_tasks * sizeof(StatsTask), hipMemcpyHostToDevice, s));
        UMIHIP_TRY_NEG(hipMemsetAsync(w.deep_kept, 0, (size_t)c.n_deep * 4, s));
        UMIHIP_TRY_NEG(hipMemsetAsync(w.deep_tab, 0, (size_t)c.n_deep * (size_t)L * ST_CELLS * 4, s));
    }
    const uint32_t grid_cap = c.n_cus * 8;
    stats_entry_kernel<<<std::min(blocks_for(n, ST_THREADS), grid_cap), ST_THREADS, 0, s>>>(
        c.d_keys, c.d_freq, n, L, W, c.hist_bins, w.f64, (unsigned long long *)c.d_count_pre, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(scan_inclusive_u64(w.f64, w.cum, n, w.scan_tmp, w.scan_bytes, s));
    stats_pick_kernel<<<blocks_for(n, ST_THREADS), ST_THREADS, 0, s>>>(w.cum, n, c.seed, w.picked);
    UMIHIP_TRY_NEG(hipGetLastError());
    StatsArgs a;
    a.keys = c.d_keys;
    a.freq = c.d_freq;
    a.kept = c.d_kept;
    a.root = c.d_root;
    a.off = w.off;
    a.picked = w.picked;
    a.total = w.total;
    a.dist = (unsigned long long *)c.d_dist;
    for (int wd = 0; wd < 4; wd++) {
        uint64_t g = 0;
        for (int b = 0; b < L; b++)
            if ((3 * b) / 64 == wd) g |= 1ull << ((3 * b) % 64);
        a.gm[wd] = g;
    }
    a.m = m;
    a.split = c.split;
    a.L = L;
    a.W = W;
    uint32_t n_lane = 0, n_wave = 0;
    for (uint32_t j = 0; j < m; j++) {
        const uint64_t sz = c.h_off[j + 1] - c.h_off[j];
        n_lane += sz <= STATS_LANE_MAX;
        n_wave += sz > STATS_LANE_MAX && sz < c.split;
    }
    if (n_lane) {
        stats_lane_kernel<<<std::min(blocks_for(m, ST_THREADS), grid_cap), ST_THREADS, 0, s>>>(a);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    if (n_wave) {
        stats_wave_kernel<<<std::min(blocks_for(m, ST_THREADS), grid_cap), ST_THREADS, 0, s>>>(a);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    if (c.n_deep) {
        const uint32_t blocks = std::min(blocks_for(c.n_tasks, ST_WAVES), grid_cap);
        stats_deep_roots_kernel<<<blocks, ST_THREADS, 0, s>>>(a, w.tasks, c.n_tasks, w.deep_j, w.deep_kept);
        UMIHIP_TRY_NEG(hipGetLastError());
        stats_deep_count_kernel<<<blocks, ST_THREADS, 0, s>>>(a, w.tasks, c.n_tasks, w.deep_j, w.deep_kept, w.deep_tab);
        UMIHIP_TRY_NEG(hipGetLastError());
        stats_deep_finish_kernel<<<c.n_deep, 64, 0, s>>>(a, w.deep_j, w.deep_kept, w.deep_tab, c.n_deep);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    stats_post_kernel<<<std::min(blocks_for(n, ST_THREADS), grid_cap), ST_THREADS, 0, s>>>(c.d_kept, w.total, n, c.hist_bins,
                                                                                          (unsigned long long *)c.d_count_post);
    UMIHIP_TRY_NEG(hipGetLastError());
    if (per_umi) {
        UmiMasks um;
        for (int wd = 0; wd < 4; wd++) {
            const int bits = std::min(64, std::max(0, 3 * L - 64 * wd));
            um.wm[wd] = bits == 64 ? ~0ull : (1ull << bits) - 1ull;
        }
        uint64_t *ka = w.ka, *kb = w.kb;
        uint32_t *va = w.va, *vb = w.vb;
        for (int wd = 0; wd < W; wd++) {
            const int bits = std::min(64, 3 * L - 64 * wd);
            stats_word_kernel<<<blocks_for(n, ST_THREADS), ST_THREADS, 0, s>>>(c.d_keys, W, wd, um.wm[wd], wd ? va : nullptr, n, ka, va);
            UMIHIP_TRY_NEG(hipGetLastError());
            bool in_b = false;
            UMIHIP_TRY_NEG(radix_sort_pairs_u64(ka, kb, va, vb, n, 0, bits, w.radix_tmp, w.radix_bytes, &in_b, s));
            if (in_b) {
                std::swap(ka, kb);
                std::swap(va, vb);
            }
        }
        uint64_t *flag = w.f64, *incl = w.cum; // (the draws have been made)
        stats_heads_kernel<<<blocks_for(n, ST_THREADS), ST_THREADS, 0, s>>>(c.d_keys, W, um, va, n, flag);
        UMIHIP_TRY_NEG(hipGetLastError());
        UMIHIP_TRY_NEG(scan_inclusive_u64(flag, incl, n, w.scan_tmp, w.scan_bytes, s));
        UMIHIP_TRY_NEG(hipMemsetAsync(c.d_times_pre, 0, (size_t)n * 4, s)); // (a run that crosses a wave is added up in place)
        UMIHIP_TRY_NEG(hipMemsetAsync(c.d_reads_pre, 0, (size_t)n * 8, s));
        UMIHIP_TRY_NEG(hipMemsetAsync(c.d_times_post, 0, (size_t)n * 4, s));
        UMIHIP_TRY_NEG(hipMemsetAsync(c.d_reads_post, 0, (size_t)n * 8, s));
        stats_umi_sum_kernel<<<blocks_for(n, ST_THREADS), ST_THREADS, 0, s>>>(
            va, incl, c.d_freq, c.d_kept, w.total, n, c.d_umi_entry, c.d_times_pre, (unsigned long long *)c.d_reads_pre,
            c.d_times_post, (unsigned long long *)c.d_reads_post);
        UMIHIP_TRY_NEG(hipGetLastError());
        UMIHIP_TRY_NEG(hipMemcpyAsync(c.h_pinned + 2, incl + (n - 1), 8, hipMemcpyDeviceToHost, s));
    }
    UMIHIP_TRY_NEG(hipMemcpyAsync(c.h_pinned, w.ctl, 16, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    return 0;
}

} // namespace umihip
