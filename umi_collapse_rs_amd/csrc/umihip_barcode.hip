// Correction of cell barcodes to a kit's list (umi_correct_barcodes, the program's --cell-whitelist), gfx950.
//
// The function (STARsolo's 1MM rule): a read is exact (its barcode is listed), corrected (not exact, and
// exactly one listed barcode differs from it in exactly one position; an N differs from every listed base),
// ambiguous (two or more such barcodes) or none.  It is what umi_correct_umis(max_mismatches, 1) gives for
// `match` on a list without duplicates, but that call compares every read with every entry, and a kit's
// list has 10^5 to 10^7 of them.  Here the list is indexed and a read costs one probe when it is exact and
// 3 L (one N: 4) when it is not.
//
// Packing: 2 bits per base (A 0, C 1, G 2, T 3), base b at bits 2b, 2b+1 of one 64-bit word: L <= 32, L = 32
// fills the word, the largest shift is 62.  A read carries the count of its N bases and the position of
// the last one beside the word (an N's code is 0).
//
// Index: an open-addressing table, linear probing, a power of two of at least 2 n_wl slots, built on the
// device in every call.  A slot is one 64-bit word, tag << 32 | entry index; the index field all ones
// marks an empty slot, so no key value stands for "empty" (all-A is 0, all-T of 32 bases all ones: both
// are ordinary keys).  m = mix(key) is a bijection of the 64-bit words (two xor-shift-multiply rounds);
// the slot is m's low bits.  The tag is the key itself where L <= 16 -- tag and index are then the whole
// entry, and a probe is one 8-byte load -- and m's high word beyond: a slot whose tag agrees is checked
// against the packed list (a second load, for the hit and for one probe in 2^32 otherwise).
// Fill: one 64-bit atomicCAS per slot tried, empty -> (tag, e).  An entry that finds its own key in a slot
// is a duplicate: atomicMin on the slot's word (the tags agree, so the smaller index wins), and a flag.
// Every member of a group of equal entries ends at the same slot, whatever the order, and the slot ends
// with the group's smallest index.  Only where the flag is set a second pass looks every entry up and
// takes atomicMin over those that find another index than their own: the smallest entry that equals an
// earlier one, independent of scheduling.
//
// Lookup, a wave at a time over 64 reads:
//   1. a read per lane (neighbouring lanes load neighbouring barcodes), packed, and one probe for the
//      reads without N;
//   2. the lanes that missed (and those with one N) go to the wave's LDS queue behind a ballot and its
//      prefix count;
//   3. the queue is worked off a read at a time, a variant per lane: the 3 L single substitutions in
//      passes of 64 (one N: the four letters at its position).  A ballot of the lanes that hit gives the
//      count; one hit in all is a correction, and the index comes from the lane that hit.
// A read with two or more N is "none" without a probe; with max_mismatches 0 so is every miss.
// The four status counts go out with one atomic per block each.  Integer and bitwise work only; the table's
// layout depends on the order of the atomics, what a probe returns does not.
//
// A pass of its own looks at every read byte first (the smallest read with a byte outside ACGTN is
// reported and nothing is written); the host looks once, after it and the build.
//
// umi_correct_barcodes_multi (the program's --cell-whitelist-multi; after STARsolo's 1MM_multi, tests/
// barcode_multi_model.py defines it): the ambiguous reads are weighed, not dropped.  Two passes:
//   1. the lookup above, instantiated with MULTI: an exact read also adds 1 to exact_reads[match] (one
//      atomic per distinct match of a wave: the lanes that share a match elect a leader, so the reads of a
//      deep cell cost their wave one atomic and not 64 on one address), and the reads that come out
//      ambiguous go to a global queue, one atomic per wave trip for the queue's tail;
//   2. barcode_resolve_kernel, a queued read per wave trip, probes the variants again; a lane that hits
//      forms w = (exact_reads[idx] + pseudocount) * T[min(q, 40)] from the quality at its position, wave
//      reductions give W = sum w (64 bits; below 2^57) and the greatest (w, smallest idx), and lane 0
//      accepts the winner where 1000 w >= permille W, both products in 128 bits.
// The queue's order depends on scheduling; a read's verdict depends on exact_reads and its own bytes only.
// The qualities are looked at beside the barcodes, before anything is written (bytes 33..126).
#include <hip/hip_runtime.h>
#include <algorithm>
#include <thread>
#include <vector>

#include "../../include/umihip.h"
#include "umihip_device.h"
#include "umihip_internal.h"

namespace umihip {

namespace {

#define BC_TRY(expr)                             \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

constexpr int BC_THREADS = 256;
constexpr int BC_WAVES = BC_THREADS / 64;
constexpr uint32_t BC_EMPTY = 0xFFFFFFFFu; // the index field of an empty slot

enum BcCtl : int {
    BC_BAD = 0,  // smallest read with a byte outside ACGTN (all ones: none)
    BC_DUP = 1,  // smallest entry that equals an earlier one (all ones: none)
    BC_SEEN = 2, // the build met a duplicate
    BC_STATUS0 = 3, // four words: reads exact, corrected, none, ambiguous
    BC_COUNT = 7,
    // umi_correct_barcodes_multi only
    BC_QUEUED = 7,   // the length of the queue of ambiguous reads
    BC_RESOLVED = 8, // reads the second pass resolved
    BC_BAD_QUAL = 9, // smallest read with a quality byte outside 33..126 (all ones: none)
    BC_COUNT_MULTI = 10,
};

// T[q] = round(2^26 * 10^(-q / 10)): the chance of an error at Phred quality q, in units of 2^-26
__constant__ uint32_t BC_ERR_WEIGHT[41] = {
    67108864, 53306465, 42342831, 33634106, 26716520, 21221686, 16856984, 13389979, 10636038, 8448505, 6710886,
    5330647,  4234283,  3363411,  2671652,  2122169,  1685698,  1338998,  1063604,  844851,   671089,  533065,
    423428,   336341,   267165,   212217,   168570,   133900,   106360,   84485,    67109,    53306,   42343,
    33634,    26717,    21222,    16857,    13390,    10636,    8449,     6711};

// 0..3 for ACGT, 4 for N, 5 for anything else
__device__ __forceinline__ uint32_t bc_base_code(uint8_t c)
{
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u;
}

__device__ __forceinline__ uint64_t bc_mix(uint64_t x)
{
    x ^= x >> 33;
    x *= 0xFF51AFD7ED558CCDull;
    x ^= x >> 33;
    x *= 0xC4CEB9FE1A85EC53ull;
    x ^= x >> 33;
    return x;
}

struct BcTable {
    unsigned long long *slot; // [mask + 1]
    const uint64_t *keys;     // [n_wl] the packed list
    uint32_t mask;
    int short_keys; // L <= 16: the tag is the key
};

__device__ __forceinline__ uint32_t bc_tag(const BcTable &t, uint64_t key, uint64_t m)
{
    return t.short_keys ? (uint32_t)key : (uint32_t)(m >> 32);
}

// the entry whose key this is, or BC_EMPTY (the load factor is at most one half: an empty slot ends the walk)
__device__ __forceinline__ uint32_t bc_probe(const BcTable &t, uint64_t key)
{
    const uint64_t m = bc_mix(key);
    const uint32_t tag = bc_tag(t, key, m);
    for (uint32_t s = (uint32_t)m & t.mask;; s = (s + 1) & t.mask) {
        const unsigned long long w = t.slot[s];
        const uint32_t idx = (uint32_t)w;
        if (idx == BC_EMPTY) return BC_EMPTY;
        if ((uint32_t)(w >> 32) == tag && (t.short_keys || t.keys[idx] == key)) return idx;
    }
}

__global__ void __launch_bounds__(BC_THREADS) barcode_build_kernel(const BcTable t, uint32_t n_wl, unsigned long long *ctl)
{
    for (uint32_t e = blockIdx.x * BC_THREADS + threadIdx.x; e < n_wl; e += gridDim.x * BC_THREADS) {
        const uint64_t key = t.keys[e];
        const uint64_t m = bc_mix(key);
        const unsigned long long mine = (unsigned long long)bc_tag(t, key, m) << 32 | e;
        for (uint32_t s = (uint32_t)m & t.mask;; s = (s + 1) & t.mask) {
            unsigned long long w = __hip_atomic_load(&t.slot[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if ((uint32_t)w == BC_EMPTY) {
                const unsigned long long seen = atomicCAS(&t.slot[s], w, mine);
                if (seen == w) break;
                w = seen; // (taken meanwhile: by whom?)
            }
            // (the slot's index may be lowered by others of its group while this looks: its key stays)
            if ((w >> 32) == (mine >> 32) && (t.short_keys || t.keys[(uint32_t)w] == key)) {
                atomicMin(&t.slot[s], mine);
                ctl[BC_SEEN] = 1;
                break;
            }
        }
    }
}

// (only after a build that met a duplicate) every slot holds the smallest index of its key by now
__global__ void __launch_bounds__(BC_THREADS) barcode_dup_kernel(const BcTable t, uint32_t n_wl, unsigned long long *ctl)
{
    for (uint32_t e = blockIdx.x * BC_THREADS + threadIdx.x; e < n_wl; e += gridDim.x * BC_THREADS)
        if (bc_probe(t, t.keys[e]) != e) atomicMin(&ctl[BC_DUP], (unsigned long long)e);
}

__global__ void __launch_bounds__(BC_THREADS) barcode_check_kernel(const uint8_t *__restrict__ bc, uint32_t n, int bc_len,
                                                                   unsigned long long *ctl)
{
    __shared__ unsigned int first[BC_WAVES];
    unsigned int mine = 0xFFFFFFFFu;
    for (uint64_t i = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BC_THREADS) {
        const uint8_t *u = bc + (size_t)i * bc_len;
        uint32_t worst = 0;
        for (int b = 0; b < bc_len; b++) worst = max(worst, bc_base_code(u[b]));
        if (worst > 4u) mine = min(mine, (unsigned int)i);
    }
    for (int off = 32; off > 0; off >>= 1) mine = min(mine, (unsigned int)__shfl_down((int)mine, off));
    if ((threadIdx.x & 63) == 0) first[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int m = first[0];
        for (int w = 1; w < BC_WAVES; w++) m = min(m, first[w]);
        if (m != 0xFFFFFFFFu) atomicMin(&ctl[BC_BAD], (unsigned long long)m);
    }
}

// the same over the qualities: the smallest read with a byte outside 33..126
__global__ void __launch_bounds__(BC_THREADS) barcode_qual_check_kernel(const uint8_t *__restrict__ qual, uint32_t n, int bc_len,
                                                                        unsigned long long *ctl)
{
    __shared__ unsigned int first[BC_WAVES];
    unsigned int mine = 0xFFFFFFFFu;
    for (uint64_t i = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * BC_THREADS) {
        const uint8_t *u = qual + (size_t)i * bc_len;
        bool bad = false;
        for (int b = 0; b < bc_len; b++) bad = bad || u[b] < 33 || u[b] > 126;
        if (bad) mine = min(mine, (unsigned int)i);
    }
    for (int off = 32; off > 0; off >>= 1) mine = min(mine, (unsigned int)__shfl_down((int)mine, off));
    if ((threadIdx.x & 63) == 0) first[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int m = first[0];
        for (int w = 1; w < BC_WAVES; w++) m = min(m, first[w]);
        if (m != 0xFFFFFFFFu) atomicMin(&ctl[BC_BAD_QUAL], (unsigned long long)m);
    }
}

struct BcArgs {
    const uint8_t *bc;
    int32_t *match;
    uint8_t *status; // may be null
    unsigned long long *ctl;
    uint32_t n;
    int bc_len, max_mismatches;
    // MULTI only
    uint32_t *exact_reads; // [n_wl], zero at the start
    uint32_t *queue;       // [n] the ambiguous reads, in any order; its length is ctl[BC_QUEUED]
};

// MULTI: the first pass of umi_correct_barcodes_multi; without it the code is umi_correct_barcodes' as it was
template <bool MULTI>
__global__ void __launch_bounds__(BC_THREADS) barcode_lookup_kernel(const BcTable t, const BcArgs a)
{
    // per wave: the reads that go on to the variants, as (key, read << 8 | position of the N or 0xFF)
    __shared__ uint64_t q_key[BC_WAVES][64];
    __shared__ uint64_t q_read[BC_WAVES][64];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    unsigned int cnt[4] = {0, 0, 0, 0};
    const uint64_t n64 = ((uint64_t)a.n + 63) & ~63ull; // (whole waves make the trips: ballots and LDS inside)
    for (uint64_t i = (uint64_t)blockIdx.x * BC_THREADS + threadIdx.x; i < n64; i += (uint64_t)gridDim.x * BC_THREADS) {
        // 1. pack and probe
        uint64_t key = 0;
        uint32_t n_count = 0, n_pos = 0xFFu;
        bool queued = false;
        if (i < a.n) {
            const uint8_t *u = a.bc + (size_t)i * a.bc_len;
            for (int b = 0; b < a.bc_len; b++) {
                const uint32_t c = bc_base_code(u[b]);
                key |= (uint64_t)(c & 3u) << (2 * b);
                if (c >> 2) {
                    n_count++;
                    n_pos = (uint32_t)b;
                }
            }
            uint32_t hit = BC_EMPTY;
            if (n_count == 0) hit = bc_probe(t, key);
            if (hit != BC_EMPTY) {
                a.match[i] = (int32_t)hit;
                if (a.status) a.status[i] = UMI_BARCODE_EXACT;
                cnt[UMI_BARCODE_EXACT]++;
            } else if (a.max_mismatches == 0 || n_count > 1) {
                a.match[i] = -1;
                if (a.status) a.status[i] = UMI_BARCODE_NONE;
                cnt[UMI_BARCODE_NONE]++;
            } else {
                queued = true;
            }
            if constexpr (MULTI) {
                // the lanes of one match add their number with one atomic (a wave of a deep cell's reads: one in all)
                unsigned long long todo = __ballot(hit != BC_EMPTY);
                while (todo) { // (wave-uniform; the lanes beyond a.n sit this block out, below)
                    const uint32_t lead = (uint32_t)__builtin_amdgcn_readlane((int)hit, __ffsll(todo) - 1);
                    const unsigned long long same = __ballot(hit == lead);
                    if (lane == __ffsll(todo) - 1) atomicAdd(&a.exact_reads[lead], (uint32_t)__builtin_popcountll(same));
                    todo &= ~same;
                }
            }
        }
        // 2. the others to the wave's queue
        const unsigned long long qmask = __ballot(queued);
        if (qmask == 0) continue; // (wave-uniform)
        if (queued) {
            const uint32_t before =
                __builtin_amdgcn_mbcnt_hi((uint32_t)(qmask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)qmask, 0u));
            q_key[wave][before] = key;
            q_read[wave][before] = i << 8 | n_pos;
        }
        __builtin_amdgcn_wave_barrier(); // (one wave, in lockstep; LDS accesses stay in program order)
        // 3. a queued read at a time, a variant per lane
        const int qn = __builtin_popcountll(qmask);
        uint32_t amb_n = 0, amb_read = 0; // MULTI: the trip's ambiguous reads, the j-th in lane j
        for (int q = 0; q < qn; q++) {
            const uint64_t k0 = q_key[wave][q], rd = q_read[wave][q]; // (one address for the wave: a broadcast)
            const uint32_t npos = (uint32_t)rd & 0xFFu;
            const int n_var = npos != 0xFFu ? 4 : 3 * a.bc_len;
            uint32_t hits = 0, idx = 0;
            for (int v0 = 0; v0 < n_var; v0 += 64) {
                const int v = v0 + lane;
                uint32_t found = BC_EMPTY;
                if (v < n_var) {
                    // one N: letter v at its position (the code there is 0); else letter (own + 1 + v % 3) % 4 at v / 3
                    const uint64_t var = npos != 0xFFu ? k0 | (uint64_t)v << (2 * npos) : k0 ^ (uint64_t)(1 + v % 3) << (2 * (v / 3));
                    found = bc_probe(t, var);
                }
                const unsigned long long hmask = __ballot(found != BC_EMPTY);
                if (hmask) {
                    hits += (uint32_t)__builtin_popcountll(hmask);
                    idx = (uint32_t)__builtin_amdgcn_readlane((int)found, __ffsll(hmask) - 1);
                }
            }
            if (lane == 0) {
                const uint64_t r = rd >> 8;
                const uint32_t st = hits == 1 ? UMI_BARCODE_CORRECTED : hits == 0 ? UMI_BARCODE_NONE : UMI_BARCODE_AMBIGUOUS;
                a.match[r] = hits == 1 ? (int32_t)idx : -1;
                if (a.status) a.status[r] = (uint8_t)st;
                cnt[UMI_BARCODE_CORRECTED] += hits == 1;
                cnt[UMI_BARCODE_NONE] += hits == 0;
                cnt[UMI_BARCODE_AMBIGUOUS] += hits > 1;
            }
            if constexpr (MULTI) {
                if (hits > 1) { // (wave-uniform)
                    if (lane == (int)amb_n) amb_read = (uint32_t)(rd >> 8);
                    amb_n++;
                }
            }
        }
        if constexpr (MULTI) {
            if (amb_n) { // one atomic for the trip's stretch of the global queue
                unsigned long long base = 0;
                if (lane == 0) base = atomicAdd(&a.ctl[BC_QUEUED], (unsigned long long)amb_n);
                const uint32_t at = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)base);
                if (lane < (int)amb_n) a.queue[at + lane] = amb_read; // (at most n reads are queued in all)
            }
        }
        __builtin_amdgcn_wave_barrier(); // (the queue is read before the next trip writes it)
    }
    for (int s = 0; s < 4; s++) block_count_add(cnt[s], &a.ctl[BC_STATUS0 + s]);
}

struct BcResolveArgs {
    const uint8_t *bc, *qual;
    const uint32_t *exact_reads, *queue;
    int32_t *match;
    uint8_t *status; // may be null
    unsigned long long *ctl;
    int bc_len;
    uint32_t permille, pseudocount;
};

// The second pass of umi_correct_barcodes_multi: a queued (ambiguous) read per wave trip, a variant per lane.
__global__ void __launch_bounds__(BC_THREADS) barcode_resolve_kernel(const BcTable t, const BcResolveArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint32_t qn = (uint32_t)a.ctl[BC_QUEUED];
    unsigned int resolved = 0;
    for (uint32_t q = blockIdx.x * BC_WAVES + (threadIdx.x >> 6); q < qn; q += gridDim.x * BC_WAVES) {
        const uint32_t r = a.queue[q];
        // (every lane packs the read: one address per load for the wave)
        const uint8_t *u = a.bc + (size_t)r * a.bc_len;
        uint64_t k0 = 0;
        uint32_t npos = 0xFFu;
        for (int b = 0; b < a.bc_len; b++) {
            const uint32_t c = bc_base_code(u[b]);
            k0 |= (uint64_t)(c & 3u) << (2 * b);
            if (c >> 2) npos = (uint32_t)b;
        }
        const int n_var = npos != 0xFFu ? 4 : 3 * a.bc_len;
        uint64_t w_sum = 0, w_best = 0; // this lane's candidates: at most two (3 L <= 96)
        uint32_t i_best = BC_EMPTY;
        for (int v0 = 0; v0 < n_var; v0 += 64) {
            const int v = v0 + lane;
            if (v < n_var) {
                const uint32_t p = npos != 0xFFu ? npos : (uint32_t)(v / 3);
                const uint64_t var = npos != 0xFFu ? k0 | (uint64_t)v << (2 * npos) : k0 ^ (uint64_t)(1 + v % 3) << (2 * (v / 3));
                const uint32_t found = bc_probe(t, var);
                if (found != BC_EMPTY) {
                    const uint32_t ql = min((uint32_t)a.qual[(size_t)r * a.bc_len + p] - 33u, 40u);
                    const uint64_t w = (uint64_t)(a.exact_reads[found] + a.pseudocount) * BC_ERR_WEIGHT[ql];
                    w_sum += w;
                    if (w > w_best || (w == w_best && found < i_best)) {
                        w_best = w;
                        i_best = found;
                    }
                }
            }
        }
        // the wave's sum, and its greatest weight with the smallest index among equals
        for (int off = 32; off > 0; off >>= 1) {
            w_sum += (uint64_t)__shfl_xor((unsigned long long)w_sum, off);
            const uint64_t w_o = (uint64_t)__shfl_xor((unsigned long long)w_best, off);
            const uint32_t i_o = (uint32_t)__shfl_xor((int)i_best, off);
            if (w_o > w_best || (w_o == w_best && i_o < i_best)) {
                w_best = w_o;
                i_best = i_o;
            }
        }
        if (lane == 0) {
            // 1000 w >= permille W, in 128 bits (W < 2^57, but 1000 W may pass 2^64)
            const uint64_t l_hi = __umul64hi(1000ull, w_best), l_lo = 1000ull * w_best;
            const uint64_t r_hi = __umul64hi((uint64_t)a.permille, w_sum), r_lo = (uint64_t)a.permille * w_sum;
            if (w_sum > 0 && (l_hi > r_hi || (l_hi == r_hi && l_lo >= r_lo))) {
                a.match[r] = (int32_t)i_best;
                if (a.status) a.status[r] = UMI_BARCODE_RESOLVED;
                resolved++;
            }
        }
    }
    block_count_add(resolved, &a.ctl[BC_RESOLVED]);
}

inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace

// (no branch per base: on a kit's list -- random letters -- a switch mispredicts three times in four, ~100 ns
// per 16-base entry, 0.67 s for the 6.8 M entries of a 10x list; a table and a few threads: ~10 ms)
int barcode_pack_list(const uint8_t *ascii, uint32_t n_wl, int bc_len, uint64_t *packed, uint64_t *bad_entry)
{
    uint8_t code[256];
    for (int c = 0; c < 256; c++) code[c] = 4;
    code['A'] = 0, code['C'] = 1, code['G'] = 2, code['T'] = 3;
    const uint32_t n_threads = n_wl < (1u << 16) ? 1u : std::min(8u, std::max(1u, std::thread::hardware_concurrency()));
    const uint32_t per = (n_wl + n_threads - 1) / n_threads;
    std::vector<uint64_t> first_bad(n_threads, ~0ull);
    auto work = [&](uint32_t t) {
        for (uint32_t e = t * per; e < std::min(n_wl, (t + 1) * per); e++) {
            const uint8_t *a = ascii + (size_t)e * bc_len;
            uint64_t k = 0;
            uint32_t worst = 0;
            for (int b = 0; b < bc_len; b++) {
                const uint32_t c = code[a[b]];
                worst |= c;
                k |= (uint64_t)(c & 3u) << (2 * b);
            }
            packed[e] = k;
            if (worst > 3u && first_bad[t] == ~0ull) first_bad[t] = e;
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < n_threads; t++) pool.emplace_back(work, t);
    work(0);
    for (std::thread &th : pool) th.join();
    for (uint32_t t = 0; t < n_threads; t++)
        if (first_bad[t] != ~0ull) {
            *bad_entry = first_bad[t];
            return 1;
        }
    return 0;
}

uint32_t barcode_table_slots(uint32_t n_wl)
{
    uint32_t s = 64;
    while (s < 2 * n_wl) s <<= 1; // (n_wl <= 2^24: at most 2^25)
    return s;
}

size_t barcode_workspace_bytes(uint32_t n_wl)
{
    return 256 + align256((size_t)n_wl * 8) + (size_t)barcode_table_slots(n_wl) * 8;
}

// ... and behind it exact_reads [n_wl] and the queue of ambiguous reads [n_reads]
size_t barcode_multi_workspace_bytes(uint32_t n_wl, uint32_t n_reads)
{
    return barcode_workspace_bytes(n_wl) + align256((size_t)n_wl * 4) + align256((size_t)n_reads * 4);
}

int barcode_on_device(void *workspace, const uint8_t *d_bc, uint32_t n_reads, int bc_len, const uint64_t *h_packed, uint32_t n_wl,
                      int max_mismatches, int32_t *d_match, uint8_t *d_status, uint64_t counts[4], uint64_t *bad, uint32_t n_cus,
                      unsigned long long *h_pinned, hipStream_t s)
{
    return barcode_multi_on_device(workspace, d_bc, nullptr, n_reads, bc_len, h_packed, n_wl, max_mismatches, 0, 0, d_match,
                                   d_status, nullptr, counts, bad, n_cus, h_pinned, s);
}

int barcode_multi_on_device(void *workspace, const uint8_t *d_bc, const uint8_t *d_qual, uint32_t n_reads, int bc_len,
                            const uint64_t *h_packed, uint32_t n_wl, int max_mismatches, uint32_t permille, uint32_t pseudocount,
                            int32_t *d_match, uint8_t *d_status, uint32_t *d_exact_reads, uint64_t *counts, uint64_t *bad,
                            uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s)
{
    const bool multi = d_qual != nullptr;
    unsigned long long *ctl = (unsigned long long *)workspace;
    uint64_t *d_keys = (uint64_t *)((char *)workspace + 256);
    const uint32_t slots = barcode_table_slots(n_wl);
    BcTable t;
    t.slot = (unsigned long long *)((char *)workspace + 256 + align256((size_t)n_wl * 8));
    t.keys = d_keys;
    t.mask = slots - 1;
    t.short_keys = bc_len <= 16;
    uint32_t *exact_reads = multi ? (uint32_t *)((char *)workspace + barcode_workspace_bytes(n_wl)) : nullptr;
    uint32_t *queue = multi ? (uint32_t *)((char *)exact_reads + align256((size_t)n_wl * 4)) : nullptr;
    BC_TRY(hipMemsetAsync(ctl, 0xFF, 16, s));
    BC_TRY(hipMemsetAsync(ctl + BC_SEEN, 0, (BC_COUNT - BC_SEEN) * 8, s));
    if (multi) {
        BC_TRY(hipMemsetAsync(ctl + BC_QUEUED, 0, 16, s));
        BC_TRY(hipMemsetAsync(ctl + BC_BAD_QUAL, 0xFF, 8, s));
        BC_TRY(hipMemsetAsync(exact_reads, 0, (size_t)n_wl * 4, s));
    }
    BC_TRY(hipMemsetAsync(t.slot, 0xFF, (size_t)slots * 8, s));
    BC_TRY(hipMemcpyAsync(d_keys, h_packed, (size_t)n_wl * 8, hipMemcpyHostToDevice, s));
    const uint32_t wl_grid = std::max(1u, std::min(blocks_for(n_wl, BC_THREADS), n_cus * 8));
    barcode_build_kernel<<<wl_grid, BC_THREADS, 0, s>>>(t, n_wl, ctl);
    BC_TRY(hipGetLastError());
    barcode_check_kernel<<<std::max(1u, std::min(blocks_for(n_reads, BC_THREADS), n_cus * 8)), BC_THREADS, 0, s>>>(d_bc, n_reads,
                                                                                                                  bc_len, ctl);
    BC_TRY(hipGetLastError());
    if (multi) {
        barcode_qual_check_kernel<<<std::max(1u, std::min(blocks_for(n_reads, BC_THREADS), n_cus * 8)), BC_THREADS, 0, s>>>(
            d_qual, n_reads, bc_len, ctl);
        BC_TRY(hipGetLastError());
    }
    BC_TRY(hipMemcpyAsync(h_pinned, ctl, multi ? BC_COUNT_MULTI * 8 : 24, hipMemcpyDeviceToHost, s));
    BC_TRY(hipStreamSynchronize(s));
    if (h_pinned[BC_SEEN]) { // (the list first, as its bytes come before the reads')
        barcode_dup_kernel<<<wl_grid, BC_THREADS, 0, s>>>(t, n_wl, ctl);
        BC_TRY(hipGetLastError());
        BC_TRY(hipMemcpyAsync(h_pinned, ctl, 16, hipMemcpyDeviceToHost, s));
        BC_TRY(hipStreamSynchronize(s));
        *bad = h_pinned[BC_DUP];
        return 2;
    }
    // (a bad barcode byte is reported before a bad quality byte of the same or a later read)
    if (h_pinned[BC_BAD] != ~0ull && (!multi || h_pinned[BC_BAD] <= h_pinned[BC_BAD_QUAL])) {
        *bad = h_pinned[BC_BAD];
        return 1;
    }
    if (multi && h_pinned[BC_BAD_QUAL] != ~0ull) {
        *bad = h_pinned[BC_BAD_QUAL];
        return 3;
    }
    BcArgs a;
    a.bc = d_bc;
    a.match = d_match;
    a.status = d_status;
    a.ctl = ctl;
    a.n = n_reads;
    a.bc_len = bc_len;
    a.max_mismatches = max_mismatches;
    a.exact_reads = exact_reads;
    a.queue = queue;
    // every block resident at once where there are that many reads (8 blocks of 4 waves per CU)
    const uint32_t grid = std::max(1u, std::min(blocks_for(n_reads, BC_THREADS), n_cus * 8));
    if (!multi) {
        barcode_lookup_kernel<false><<<grid, BC_THREADS, 0, s>>>(t, a);
        BC_TRY(hipGetLastError());
        BC_TRY(hipMemcpyAsync(h_pinned, ctl, BC_COUNT * 8, hipMemcpyDeviceToHost, s));
        BC_TRY(hipStreamSynchronize(s));
        for (int c = 0; c < 4; c++) counts[c] = h_pinned[BC_STATUS0 + c];
        return 0;
    }
    barcode_lookup_kernel<true><<<grid, BC_THREADS, 0, s>>>(t, a);
    BC_TRY(hipGetLastError());
    BcResolveArgs ra;
    ra.bc = d_bc;
    ra.qual = d_qual;
    ra.exact_reads = exact_reads;
    ra.queue = queue;
    ra.match = d_match;
    ra.status = d_status;
    ra.ctl = ctl;
    ra.bc_len = bc_len;
    ra.permille = permille;
    ra.pseudocount = pseudocount;
    // (the queue's length is known on the device only: the grid is sized for every read, a wave per read, and
    // capped as above; a block without a read leaves at once)
    barcode_resolve_kernel<<<std::max(1u, std::min(blocks_for(n_reads, BC_WAVES), n_cus * 8)), BC_THREADS, 0, s>>>(t, ra);
    BC_TRY(hipGetLastError());
    if (d_exact_reads) BC_TRY(hipMemcpyAsync(d_exact_reads, exact_reads, (size_t)n_wl * 4, hipMemcpyDeviceToDevice, s));
    BC_TRY(hipMemcpyAsync(h_pinned, ctl, BC_COUNT_MULTI * 8, hipMemcpyDeviceToHost, s));
    BC_TRY(hipStreamSynchronize(s));
    for (int c = 0; c < 4; c++) counts[c] = h_pinned[BC_STATUS0 + c];
    counts[UMI_BARCODE_AMBIGUOUS] -= h_pinned[BC_RESOLVED];
    counts[UMI_BARCODE_RESOLVED] = h_pinned[BC_RESOLVED];
    return 0;
}

#undef BC_TRY

} // namespace umihip
