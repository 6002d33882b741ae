// Correction of UMIs to a fixed list (umi_correct_umis, the program's --umi-whitelist), gfx950.
//
// Every read's UMI is compared with every listed UMI: d(u, w) = positions whose bytes differ (the list
// holds ACGT only, so an N of the read differs from every listed base -- the reference's umi_dist on
// the encoded keys, src/utils/bitset.rs:77-91).  Per read: best = the smallest distance, idx = the
// smallest index that reaches it, second = the smallest distance over every other entry (umi_len + 1
// where there is none).  Matched iff best <= max_mismatches and second - best >= min_distance.
//
// Packing: 2 bits per base (A 0, C 1, G 2, T 3), 16 bases per 32-bit word, so no base lies across two
// words; a read carries a second plane with the odd bit of every N base set (its code is 0).  Per word
// of a (read, entry) pair:
//     x = r ^ w;  t = x | x << 1;  m = (t & 0xAAAAAAAA) | n;  d += popcount(m)       4 VALU operations
// and per pair, with key = d << 24 | entry index (keys of one read are all different):
//     second = min(second, max(best, key));  best = min(best, key)                  4 with the key's making
// The walk is in ascending index order and the index is the low part of the key, so a tie goes to the
// lower index by the comparison itself.
//
// Shape: a block of 256 lanes takes CORR_READS reads per lane into registers (read i of the chunk at
// lane i % 256: neighbouring lanes load neighbouring UMIs) and walks the list in tiles of CORR_TILE
// entries staged in LDS, entry-major: every lane of a wave reads the same entry at the same time, one
// broadcast read per entry that serves the lane's CORR_READS reads.  A list of one tile is staged once
// per block, a longer one once per chunk and tile (one load per CORR_READS * CORR_TILE comparisons).
// The grid strides over the chunks.  Three counters -- exact, corrected, unmatched -- go out with one
// atomic per block each.
//
// A pass of its own looks at every read byte first (the smallest read with a byte outside ATCGN is
// reported and nothing is written); the host looks once, between the two.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_device.h"
#include "umihip_internal.h"

namespace umihip {

namespace {

#define CORR_TRY(expr)                           \
    do {                                         \
        const hipError_t e__ = (expr);           \
        if (e__ != hipSuccess) return -(int)e__; \
    } while (0)

constexpr int CORR_THREADS = 256;
constexpr int CORR_READS = 2; // reads per lane
constexpr uint32_t CORR_CHUNK = CORR_THREADS * CORR_READS;
constexpr uint32_t CORR_NO_KEY = 0xFFFFFFFFu;
constexpr int CORR_IDX_BITS = 24;
static_assert(CORR_MAX_LIST <= (1u << CORR_IDX_BITS), "an entry index must fit the low part of a key");
static_assert(UMI_MAX_WIDE_UMI_LEN < (1 << (32 - CORR_IDX_BITS)) - 1, "a distance must fit the high part of a key");

enum CorrCtl : int {
    RC_BAD = 0, // smallest read with a byte outside ATCGN (all ones: none)
    RC_EXACT = 1,
    RC_CORRECTED = 2,
    RC_UNMATCHED = 3,
    RC_COUNT = 4,
};

// 0..3 for ACGT, 4 for N, 5 for anything else
__device__ __forceinline__ uint32_t base_code(uint8_t c)
{
    return c == 'A' ? 0u : c == 'C' ? 1u : c == 'G' ? 2u : c == 'T' ? 3u : c == 'N' ? 4u : 5u;
}

__global__ void __launch_bounds__(CORR_THREADS) correct_check_kernel(const uint8_t *__restrict__ umi, uint32_t n, int umi_len,
                                                                     unsigned long long *ctl)
{
    __shared__ unsigned int first[CORR_THREADS / 64];
    unsigned int mine = 0xFFFFFFFFu;
    for (uint64_t i = (uint64_t)blockIdx.x * CORR_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * CORR_THREADS) {
        const uint8_t *u = umi + (size_t)i * umi_len;
        uint32_t worst = 0;
        for (int b = 0; b < umi_len; b++) worst = max(worst, base_code(u[b]));
        if (worst > 4u) mine = min(mine, (unsigned int)i);
    }
    for (int off = 32; off > 0; off >>= 1) mine = min(mine, (unsigned int)__shfl_down((int)mine, off));
    if ((threadIdx.x & 63) == 0) first[threadIdx.x >> 6] = mine;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned int m = first[0];
        for (int w = 1; w < CORR_THREADS / 64; w++) m = min(m, first[w]);
        if (m != 0xFFFFFFFFu) atomicMin(&ctl[RC_BAD], (unsigned long long)m);
    }
}

struct CorrArgs {
    const uint8_t *umi;
    const uint32_t *wl; // [n_wl * W] packed entries
    uint8_t *out;       // may be null, may be umi
    int32_t *match;
    uint8_t *best, *second; // may be null
    unsigned long long *ctl;
    uint32_t n, n_wl;
    int umi_len, max_mismatches, min_distance;
};

// W: 32-bit words per packed UMI, ceil(umi_len / 16)
template <int W> __global__ void __launch_bounds__(CORR_THREADS) correct_kernel(const CorrArgs a)
{
    __shared__ uint32_t tile[CORR_TILE * W];
    const bool one_tile = a.n_wl <= CORR_TILE;
    bool staged = false;
    unsigned int n_exact = 0, n_corrected = 0, n_unmatched = 0;
    // (every lane of the block makes the same trips: the barriers of the tile loop are inside)
    for (uint64_t base = (uint64_t)blockIdx.x * CORR_CHUNK; base < a.n; base += (uint64_t)gridDim.x * CORR_CHUNK) {
        uint32_t rk[CORR_READS][W], rn[CORR_READS][W], bk[CORR_READS], sk[CORR_READS];
#pragma unroll
        for (int r = 0; r < CORR_READS; r++) {
            const uint64_t i = base + (uint64_t)r * CORR_THREADS + threadIdx.x;
#pragma unroll
            for (int w = 0; w < W; w++) rk[r][w] = rn[r][w] = 0;
            bk[r] = sk[r] = CORR_NO_KEY;
            if (i < a.n) {
                const uint8_t *u = a.umi + (size_t)i * a.umi_len;
#pragma unroll
                for (int w = 0; w < W; w++)
                    for (int b = 16 * w; b < min(16 * w + 16, a.umi_len); b++) {
                        const uint32_t c = base_code(u[b]);
                        rk[r][w] |= (c & 3u) << (2 * (b & 15));
                        rn[r][w] |= (c >> 2 ? 2u : 0u) << (2 * (b & 15));
                    }
#pragma unroll
                for (int w = 0; w < W; w++) rk[r][w] &= ~(rn[r][w] | rn[r][w] >> 1); // an N's code is 0
            }
        }
        for (uint32_t t0 = 0; t0 < a.n_wl; t0 += CORR_TILE) {
            const uint32_t nt = min(CORR_TILE, a.n_wl - t0);
            if (!(one_tile && staged)) {
                __syncthreads(); // (the tile before this one has been walked by every wave)
                for (uint32_t q = threadIdx.x; q < nt * W; q += CORR_THREADS) tile[q] = a.wl[(size_t)t0 * W + q];
                __syncthreads();
                staged = true;
            }
#pragma unroll 4
            for (uint32_t j = 0; j < nt; j++) {
                uint32_t wv[W];
#pragma unroll
                for (int w = 0; w < W; w++) wv[w] = tile[j * W + w]; // (one address for the wave: a broadcast)
#pragma unroll
                for (int r = 0; r < CORR_READS; r++) {
                    uint32_t d = 0;
#pragma unroll
                    for (int w = 0; w < W; w++) {
                        const uint32_t x = rk[r][w] ^ wv[w];
                        d += (uint32_t)popc((uint32_t)(((x | x << 1) & 0xAAAAAAAAu) | rn[r][w]));
                    }
                    const uint32_t key = d << CORR_IDX_BITS | (t0 + j);
                    sk[r] = min(sk[r], max(bk[r], key)); // (best <= second: the middle one of the three)
                    bk[r] = min(bk[r], key);
                }
            }
        }
#pragma unroll
        for (int r = 0; r < CORR_READS; r++) {
            const uint64_t i = base + (uint64_t)r * CORR_THREADS + threadIdx.x;
            if (i >= a.n) continue;
            const int best = (int)(bk[r] >> CORR_IDX_BITS);
            const uint32_t idx = bk[r] & ((1u << CORR_IDX_BITS) - 1u);
            const int second = sk[r] == CORR_NO_KEY ? a.umi_len + 1 : (int)(sk[r] >> CORR_IDX_BITS);
            const bool matched = best <= a.max_mismatches && second - best >= a.min_distance;
            a.match[i] = matched ? (int32_t)idx : -1;
            if (a.best) a.best[i] = (uint8_t)best;
            if (a.second) a.second[i] = (uint8_t)second;
            n_exact += matched && best == 0;
            n_corrected += matched && best != 0;
            n_unmatched += !matched;
            if (a.out) {
                uint8_t *o = a.out + (size_t)i * a.umi_len;
                if (matched) {
                    const uint32_t *e = a.wl + (size_t)idx * W;
                    for (int b = 0; b < a.umi_len; b++) {
                        const uint32_t c = (e[b >> 4] >> (2 * (b & 15))) & 3u;
                        o[b] = c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T';
                    }
                } else if (a.out != a.umi) { // (in place: the bytes are there already)
                    const uint8_t *u = a.umi + (size_t)i * a.umi_len;
                    for (int b = 0; b < a.umi_len; b++) o[b] = u[b];
                }
            }
        }
    }
    block_count_add(n_exact, &a.ctl[RC_EXACT]);
    block_count_add(n_corrected, &a.ctl[RC_CORRECTED]);
    block_count_add(n_unmatched, &a.ctl[RC_UNMATCHED]);
}

inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }
inline size_t align256(size_t v) { return (v + 255) & ~(size_t)255; }

} // namespace

int correct_words(int umi_len) { return (umi_len + 15) / 16; }

int correct_pack_list(const uint8_t *ascii, uint32_t n_wl, int umi_len, uint32_t *packed, uint64_t *bad_entry)
{
    const int W = correct_words(umi_len);
    for (uint32_t e = 0; e < n_wl; e++) {
        uint32_t *p = packed + (size_t)e * W;
        for (int w = 0; w < W; w++) p[w] = 0;
        for (int b = 0; b < umi_len; b++) {
            uint32_t c;
            switch (ascii[(size_t)e * umi_len + b]) {
            case 'A': c = 0; break;
            case 'C': c = 1; break;
            case 'G': c = 2; break;
            case 'T': c = 3; break;
            default: *bad_entry = e; return 1;
            }
            p[b >> 4] |= c << (2 * (b & 15));
        }
    }
    return 0;
}

size_t correct_workspace_bytes(uint32_t n_wl, int umi_len)
{
    return 256 + align256((size_t)n_wl * correct_words(umi_len) * 4);
}

int correct_on_device(void *workspace, const uint8_t *d_umi, uint32_t n_reads, int umi_len, const uint32_t *h_packed,
                      uint32_t n_wl, int max_mismatches, int min_distance, uint8_t *d_out, int32_t *d_match, uint8_t *d_best,
                      uint8_t *d_second, uint64_t counts[3], uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned,
                      hipStream_t s)
{
    const int W = correct_words(umi_len);
    unsigned long long *ctl = (unsigned long long *)workspace;
    uint32_t *d_wl = (uint32_t *)((char *)workspace + 256);
    CORR_TRY(hipMemsetAsync(ctl, 0xFF, 8, s));
    CORR_TRY(hipMemsetAsync(ctl + 1, 0, (RC_COUNT - 1) * 8, s));
    CORR_TRY(hipMemcpyAsync(d_wl, h_packed, (size_t)n_wl * W * 4, hipMemcpyHostToDevice, s));
    correct_check_kernel<<<std::max(1u, std::min(blocks_for(n_reads, CORR_THREADS), n_cus * 8)), CORR_THREADS, 0, s>>>(
        d_umi, n_reads, umi_len, ctl);
    CORR_TRY(hipGetLastError());
    CORR_TRY(hipMemcpyAsync(h_pinned, ctl, 8, hipMemcpyDeviceToHost, s));
    CORR_TRY(hipStreamSynchronize(s));
    if (h_pinned[RC_BAD] != ~0ull) {
        *bad_read = h_pinned[RC_BAD];
        return 1;
    }
    CorrArgs a;
    a.umi = d_umi;
    a.wl = d_wl;
    a.out = d_out;
    a.match = d_match;
    a.best = d_best;
    a.second = d_second;
    a.ctl = ctl;
    a.n = n_reads;
    a.n_wl = n_wl;
    a.umi_len = umi_len;
    a.max_mismatches = max_mismatches;
    a.min_distance = min_distance;
    // every block resident at once where there are that many chunks (8 blocks of 4 waves per CU)
    const uint32_t grid = std::max(1u, std::min(blocks_for(n_reads, CORR_CHUNK), n_cus * 8));
    switch (W) {
    case 1: correct_kernel<1><<<grid, CORR_THREADS, 0, s>>>(a); break;
    case 2: correct_kernel<2><<<grid, CORR_THREADS, 0, s>>>(a); break;
    case 3: correct_kernel<3><<<grid, CORR_THREADS, 0, s>>>(a); break;
    case 4: correct_kernel<4><<<grid, CORR_THREADS, 0, s>>>(a); break;
    case 5: correct_kernel<5><<<grid, CORR_THREADS, 0, s>>>(a); break;
    case 6: correct_kernel<6><<<grid, CORR_THREADS, 0, s>>>(a); break;
    default: return -(int)hipErrorInvalidValue;
    }
    CORR_TRY(hipGetLastError());
    CORR_TRY(hipMemcpyAsync(h_pinned, ctl, RC_COUNT * 8, hipMemcpyDeviceToHost, s));
    CORR_TRY(hipStreamSynchronize(s));
    counts[0] = h_pinned[RC_EXACT];
    counts[1] = h_pinned[RC_CORRECTED];
    counts[2] = h_pinned[RC_UNMATCHED];
    return 0;
}

#undef CORR_TRY

} // namespace umihip
