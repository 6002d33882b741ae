// One-mismatch UMI correction after Cell Ranger's correct_umi / STARsolo's 1MM_CR (gfx950): umi_dedup_batch_cr.
//
// No counterpart in the reference (tkob-vh/umi-collapse-rs has the directional and the adjacency collapse only,
// src/algo/mod.rs).  The rule, per bucket of distinct UMIs (include/umihip.h has it in full): t is a candidate
// for s when the two differ at exactly one base and t's letter there is one of A C G T; target(s) is the largest
// of s and its candidates by (freq, then the UMI as a byte string, A < C < G < N < T); an entry is kept iff it is
// some entry's target.  Nothing is transitive: a -> b -> c keeps b and c, so no union-find and no rounds -- an
// arg-max per entry.
//
// Two paths, by bucket size:
//   small   one lane per entry walks the other entries of its bucket (contiguous: the lanes of a bucket load the
//           same words, the loads of a wave broadcast), keeps its best (freq, key, index) in registers and stores
//           target[i] and kept[target[i]] = 1 -- a plain byte store, several lanes storing the same 1 is the
//           intended race.  A lane finds its bucket through one word, span[i] = (i - start) | size << 10, that a
//           pass over the bucket table has stored: runs of one- to three-entry buckets fill waves whole.
//   list    the pipeline's MODE_NEIGHBOURS at k = 1 leaves every pair within one substitution (and a few more:
//           N is half a wildcard to umi_dist) in one (i, j) list.  Three passes over it, none of which depends on
//           the list's order: atomicMax of the best count, 64-bit atomicMax of the best string among the
//           candidates at that count, a store of the one index whose string is that one (strings are distinct
//           inside a bucket: one writer per entry).
// Two strings are compared at the lowest 3-bit group in which their keys differ (base 0 is the most significant
// letter and sits in the lowest bits): no recoded key is carried in the small path.  The list path needs a number
// to take a maximum of: the order-preserving recoding, base 0 on top, 3 bits a base, 63 bits at most.
// Integer / bitwise work, 64-lane waves, no MFMA, no LDS beyond the block sums.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "umihip_internal.h"
#include "umihip_device.h"

namespace umihip {

namespace {

constexpr uint64_t CR_GROUP_LSB = 0x1249249249249249ull; // bit 0 of every 3-bit group

__device__ __forceinline__ uint64_t cr_key_mask(int umi_len)
{
    return umi_len >= 21 ? 0x7FFFFFFFFFFFFFFFull : ((1ull << (3 * umi_len)) - 1ull);
}
// place of a letter in A < C < G < N < T from its code (A 000, C 110, G 011, N 100, T 101): a nibble per code
__device__ __forceinline__ uint32_t cr_rank(uint32_t code) { return (0x01432000u >> (4u * code)) & 7u; }
// x = a ^ b of two masked keys: they differ in exactly one base
__device__ __forceinline__ bool cr_one_base(uint64_t x)
{
    const uint64_t g = (x | (x >> 1) | (x >> 2)) & CR_GROUP_LSB;
    return g != 0 && (g & (g - 1)) == 0;
}
// first bit of the lowest group in which x is set (x != 0)
__device__ __forceinline__ int cr_group_of(uint64_t x) { return (__builtin_ctzll(x) / 3) * 3; }
// a > b as byte strings (masked keys)
__device__ __forceinline__ bool cr_string_above(uint64_t a, uint64_t b)
{
    const uint64_t x = a ^ b;
    if (x == 0) return false;
    const int p = cr_group_of(x);
    return cr_rank((uint32_t)(a >> p) & 7u) > cr_rank((uint32_t)(b >> p) & 7u);
}
// the string as a number: base 0 most significant
__device__ __forceinline__ unsigned long long cr_string_key(uint64_t key, int umi_len)
{
    unsigned long long sk = 0;
    for (int b = 0; b < umi_len; b++) sk = (sk << 3) | cr_rank((uint32_t)(key >> (3 * b)) & 7u);
    return sk;
}

uint32_t cr_grid(uint64_t n, uint32_t n_cus)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + 255) / 256, (uint64_t)n_cus * 8));
}

__global__ __launch_bounds__(256) void cr_check_kernel(const uint64_t *__restrict__ keys, const uint64_t *__restrict__ nmask,
                                                       const int32_t *__restrict__ freq, uint32_t n, int umi_len,
                                                       unsigned long long *__restrict__ counters)
{
    const uint64_t km = cr_key_mask(umi_len);
    unsigned int bad = 0, rises = 0, has_n = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t key = keys[i] & km;
        const int32_t f = freq[i];
        bad += f < 1 ? 1u : 0u;
        rises += (i > 0 && f > freq[i - 1]) ? 1u : 0u;
        // groups that hold 100
        const uint64_t nn = (key >> 2) & ~(key >> 1) & ~key & CR_GROUP_LSB;
        has_n += nn != 0 ? 1u : 0u;
        if (nmask) bad += ((nn * 7ull) & ~nmask[i]) != 0 ? 1u : 0u; // (a given nmask covers every N code, as in prep_kernel)
    }
    block_count_add(bad, &counters[CR_BAD]);
    block_count_add(rises, &counters[CR_RISES]);
    block_count_add(has_n, &counters[CR_HAS_N]);
}

__global__ __launch_bounds__(256) void cr_span_kernel(const uint64_t *__restrict__ bucket_off, uint64_t n_buckets, uint32_t n,
                                                      uint32_t small_max, const int32_t *__restrict__ freq,
                                                      uint32_t *__restrict__ span, unsigned long long *__restrict__ counters)
{
    unsigned int rises = 0, bad = 0;
    const uint32_t lane = threadIdx.x & 63u;
    // (block-uniform trip count: the ballot below is every lane's)
    for (uint64_t b0 = (uint64_t)blockIdx.x * blockDim.x; b0 < n_buckets; b0 += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t b = b0 + threadIdx.x;
        uint64_t s = 0, e = 0;
        if (b < n_buckets) {
            s = bucket_off[b];
            e = bucket_off[b + 1];
        }
        const bool inside = s <= e && e <= (uint64_t)n;
        bad += inside ? 0u : 1u;
        const uint32_t sz = inside ? (uint32_t)(e - s) : 0u, s32 = (uint32_t)s;
        if (sz && s32 > 0) rises += freq[s32] > freq[s32 - 1] ? 1u : 0u;
        const bool small = sz >= 1 && sz <= small_max;
        if (small && sz <= 4)
            for (uint32_t j = 0; j < sz; j++) span[s32 + j] = j | (sz << 10);
        // a longer one: the wave stores its words together
        unsigned long long todo = __ballot(small && sz > 4);
        while (todo) {
            const int l = __ffsll(todo) - 1;
            todo &= todo - 1;
            const uint32_t ss = (uint32_t)__shfl((int)s32, l), zz = (uint32_t)__shfl((int)sz, l);
            for (uint32_t j = lane; j < zz; j += 64) span[ss + j] = j | (zz << 10);
        }
    }
    block_count_add(rises, &counters[CR_START_RISES]);
    block_count_add(bad, &counters[CR_BAD]);
}

__global__ __launch_bounds__(256) void cr_small_kernel(const uint64_t *__restrict__ keys, const int32_t *__restrict__ freq,
                                                       const uint32_t *__restrict__ span, uint32_t n, int umi_len,
                                                       uint32_t *__restrict__ target, uint8_t *__restrict__ kept,
                                                       unsigned long long *__restrict__ counters)
{
    const uint64_t km = cr_key_mask(umi_len);
    unsigned int pairs = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint32_t code = span[i];
        if (!code) continue; // an entry of a larger bucket
        const uint32_t s = i - (code & 1023u), e = s + (code >> 10); // (inside [0, n]: cr_span_kernel)
        const uint64_t ki = keys[i] & km;
        int32_t best_f = freq[i];
        uint64_t best_k = ki;
        uint32_t best = i;
        for (uint32_t j = s; j < e; j++) {
            const uint64_t kj = keys[j] & km, x = ki ^ kj;
            if (!cr_one_base(x)) continue; // (j == i: x == 0)
            pairs += j > i ? 1u : 0u;
            if (((uint32_t)(kj >> cr_group_of(x)) & 7u) == 4u) continue; // an N is never substituted in
            const int32_t fj = freq[j];
            if (fj > best_f || (fj == best_f && cr_string_above(kj, best_k))) {
                best_f = fj;
                best_k = kj;
                best = j;
            }
        }
        target[i] = best;
        kept[best] = 1;
    }
    block_count_add(pairs, &counters[CR_PAIRS]);
}

// one task per block: a stretch of a larger bucket
__global__ __launch_bounds__(256) void cr_gather_kernel(const CrGatherTask *__restrict__ tasks, const uint64_t *__restrict__ keys,
                                                        const int32_t *__restrict__ freq, uint64_t *__restrict__ ckeys,
                                                        int32_t *__restrict__ cfreq, uint32_t *__restrict__ gidx)
{
    const CrGatherTask t = tasks[blockIdx.x];
    for (uint32_t j = threadIdx.x; j < t.len; j += blockDim.x) {
        ckeys[t.dst + j] = keys[t.src + j];
        cfreq[t.dst + j] = freq[t.src + j];
        gidx[t.dst + j] = t.src + j;
    }
}

__global__ __launch_bounds__(256) void cr_nmask_kernel(const uint64_t *__restrict__ ckeys, uint32_t nl, int umi_len,
                                                       uint64_t *__restrict__ nmask)
{
    const uint64_t km = cr_key_mask(umi_len);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x) {
        const uint64_t key = ckeys[i] & km;
        nmask[i] = ((key >> 2) & ~(key >> 1) & ~key & CR_GROUP_LSB) * 7ull;
    }
}

__global__ __launch_bounds__(256) void cr_init_kernel(const uint64_t *__restrict__ ckeys, const int32_t *__restrict__ cfreq, uint32_t nl,
                                                      int umi_len, const uint32_t *__restrict__ gidx, int32_t *__restrict__ best_f,
                                                      unsigned long long *__restrict__ best_k, uint32_t *__restrict__ target)
{
    const uint64_t km = cr_key_mask(umi_len);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x) {
        best_f[i] = cfreq[i];
        best_k[i] = cr_string_key(ckeys[i] & km, umi_len);
        const uint32_t g = gidx ? gidx[i] : i;
        target[g] = g;
    }
}

// What a listed pair means to the rule: whether its keys differ at exactly one base, and which of the two may take the
// other (the other's letter at that base is no N).  A direction matters only where the candidate's count is not
// below the entry's own: target(s) beats s itself or is s.
struct CrPair {
    uint32_t a, b;
    uint64_t ka, kb;
    int32_t fa, fb;
    bool one, a_takes_b, b_takes_a;
};
__device__ __forceinline__ CrPair cr_pair_of(uint2 e, const uint64_t *__restrict__ ckeys, const int32_t *__restrict__ cfreq,
                                             uint32_t nl, uint64_t km)
{
    CrPair p;
    p.a = e.x & 0x7FFFFFFFu;
    p.b = e.y & 0x7FFFFFFFu;
    p.one = p.a_takes_b = p.b_takes_a = false;
    if (p.a >= nl || p.b >= nl) return p; // (nothing in the list lies outside: a guard, not a case)
    p.ka = ckeys[p.a] & km;
    p.kb = ckeys[p.b] & km;
    const uint64_t x = p.ka ^ p.kb;
    if (!cr_one_base(x)) return p;
    p.one = true;
    p.fa = cfreq[p.a];
    p.fb = cfreq[p.b];
    const int g = cr_group_of(x);
    p.a_takes_b = ((uint32_t)(p.kb >> g) & 7u) != 4u && p.fb >= p.fa;
    p.b_takes_a = ((uint32_t)(p.ka >> g) & 7u) != 4u && p.fa >= p.fb;
    return p;
}
// the 64-bit word of pass 2: a candidate above the entry's own count outranks the entry's own string (the start value)
__device__ __forceinline__ unsigned long long cr_word(uint64_t key, int umi_len, bool above)
{
    return cr_string_key(key, umi_len) | (above ? 1ull << 63 : 0ull);
}

__global__ __launch_bounds__(256) void cr_best_count_kernel(const uint2 *__restrict__ edges, uint32_t n_edges,
                                                            const uint64_t *__restrict__ ckeys, const int32_t *__restrict__ cfreq,
                                                            uint32_t nl, int umi_len, int32_t *__restrict__ best_f,
                                                            unsigned long long *__restrict__ counters)
{
    const uint64_t km = cr_key_mask(umi_len);
    unsigned int pairs = 0;
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_edges; t += gridDim.x * blockDim.x) {
        const CrPair p = cr_pair_of(edges[t], ckeys, cfreq, nl, km);
        pairs += p.one ? 1u : 0u;
        if (p.a_takes_b && p.fb > p.fa) atomicMax(&best_f[p.a], p.fb);
        if (p.b_takes_a && p.fa > p.fb) atomicMax(&best_f[p.b], p.fa);
    }
    block_count_add(pairs, &counters[CR_PAIRS]);
}

__global__ __launch_bounds__(256) void cr_best_string_kernel(const uint2 *__restrict__ edges, uint32_t n_edges,
                                                             const uint64_t *__restrict__ ckeys, const int32_t *__restrict__ cfreq,
                                                             uint32_t nl, int umi_len, const int32_t *__restrict__ best_f,
                                                             unsigned long long *__restrict__ best_k)
{
    const uint64_t km = cr_key_mask(umi_len);
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_edges; t += gridDim.x * blockDim.x) {
        const CrPair p = cr_pair_of(edges[t], ckeys, cfreq, nl, km);
        if (p.a_takes_b && p.fb == best_f[p.a]) atomicMax(&best_k[p.a], cr_word(p.kb, umi_len, p.fb > p.fa));
        if (p.b_takes_a && p.fa == best_f[p.b]) atomicMax(&best_k[p.b], cr_word(p.ka, umi_len, p.fa > p.fb));
    }
}

__global__ __launch_bounds__(256) void cr_pick_kernel(const uint2 *__restrict__ edges, uint32_t n_edges,
                                                      const uint64_t *__restrict__ ckeys, const int32_t *__restrict__ cfreq, uint32_t nl,
                                                      int umi_len, const uint32_t *__restrict__ gidx, const int32_t *__restrict__ best_f,
                                                      const unsigned long long *__restrict__ best_k, uint32_t *__restrict__ target)
{
    const uint64_t km = cr_key_mask(umi_len);
    for (uint32_t t = blockIdx.x * blockDim.x + threadIdx.x; t < n_edges; t += gridDim.x * blockDim.x) {
        const CrPair p = cr_pair_of(edges[t], ckeys, cfreq, nl, km);
        if (p.a_takes_b && p.fb == best_f[p.a] && cr_word(p.kb, umi_len, p.fb > p.fa) == best_k[p.a])
            target[gidx ? gidx[p.a] : p.a] = gidx ? gidx[p.b] : p.b;
        if (p.b_takes_a && p.fa == best_f[p.b] && cr_word(p.ka, umi_len, p.fa > p.fb) == best_k[p.b])
            target[gidx ? gidx[p.b] : p.b] = gidx ? gidx[p.a] : p.a;
    }
}

__global__ __launch_bounds__(256) void cr_mark_kernel(uint32_t nl, const uint32_t *__restrict__ gidx,
                                                      const uint32_t *__restrict__ target, uint8_t *__restrict__ kept)
{
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < nl; i += gridDim.x * blockDim.x)
        kept[target[gidx ? gidx[i] : i]] = 1;
}

__global__ __launch_bounds__(256) void cr_finish_kernel(const uint8_t *__restrict__ kept, const uint32_t *__restrict__ target,
                                                        uint32_t n, uint32_t *__restrict__ root,
                                                        unsigned long long *__restrict__ counters)
{
    unsigned int n_kept = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const bool k = kept[i] != 0;
        n_kept += k ? 1u : 0u;
        if (root) root[i] = k ? i : target[i]; // (a target is kept by construction)
    }
    block_count_add(n_kept, &counters[CR_KEPT]);
}

} // namespace

hipError_t launch_cr_check(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq, uint32_t n, int umi_len,
                           unsigned long long *counters, uint32_t n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    cr_check_kernel<<<cr_grid(n, n_cus), 256, 0, s>>>(keys, nmask, freq, n, umi_len, counters);
    return hipGetLastError();
}

hipError_t launch_cr_spans(const uint64_t *d_bucket_off, uint64_t n_buckets, uint32_t n, uint32_t small_max,
                           const int32_t *freq, uint32_t *span, unsigned long long *counters, uint32_t n_cus, hipStream_t s)
{
    if (n_buckets == 0) return hipSuccess;
    if (small_max > CR_SMALL_MAX_CAP) return hipErrorInvalidValue;
    cr_span_kernel<<<cr_grid(n_buckets, n_cus), 256, 0, s>>>(d_bucket_off, n_buckets, n, small_max, freq, span, counters);
    return hipGetLastError();
}

hipError_t launch_cr_small(const uint64_t *keys, const int32_t *freq, const uint32_t *span, uint32_t n, int umi_len,
                           uint32_t *target, uint8_t *kept, unsigned long long *counters, uint32_t n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    cr_small_kernel<<<cr_grid(n, n_cus), 256, 0, s>>>(keys, freq, span, n, umi_len, target, kept, counters);
    return hipGetLastError();
}

hipError_t launch_cr_gather(const CrGatherTask *tasks, uint32_t n_tasks, const uint64_t *keys, const int32_t *freq,
                            uint64_t *ckeys, int32_t *cfreq, uint32_t *gidx, hipStream_t s)
{
    if (n_tasks == 0) return hipSuccess;
    cr_gather_kernel<<<n_tasks, 256, 0, s>>>(tasks, keys, freq, ckeys, cfreq, gidx);
    return hipGetLastError();
}

hipError_t launch_cr_nmask(const uint64_t *ckeys, uint32_t nl, int umi_len, uint64_t *nmask, uint32_t n_cus, hipStream_t s)
{
    if (nl == 0) return hipSuccess;
    cr_nmask_kernel<<<cr_grid(nl, n_cus), 256, 0, s>>>(ckeys, nl, umi_len, nmask);
    return hipGetLastError();
}

hipError_t launch_cr_resolve(const uint2 *edges, uint32_t n_edges, const uint64_t *ckeys, const int32_t *cfreq, uint32_t nl,
                             int umi_len, const uint32_t *gidx, int32_t *best_f, unsigned long long *best_k, uint32_t *target,
                             uint8_t *kept, unsigned long long *counters, uint32_t n_cus, hipStream_t s)
{
    if (nl == 0) return hipSuccess;
    cr_init_kernel<<<cr_grid(nl, n_cus), 256, 0, s>>>(ckeys, cfreq, nl, umi_len, gidx, best_f, best_k, target);
    if (n_edges) {
        const uint32_t grid = cr_grid(n_edges, n_cus);
        cr_best_count_kernel<<<grid, 256, 0, s>>>(edges, n_edges, ckeys, cfreq, nl, umi_len, best_f, counters);
        cr_best_string_kernel<<<grid, 256, 0, s>>>(edges, n_edges, ckeys, cfreq, nl, umi_len, best_f, best_k);
        cr_pick_kernel<<<grid, 256, 0, s>>>(edges, n_edges, ckeys, cfreq, nl, umi_len, gidx, best_f, best_k, target);
    }
    cr_mark_kernel<<<cr_grid(nl, n_cus), 256, 0, s>>>(nl, gidx, target, kept);
    return hipGetLastError();
}

hipError_t launch_cr_finish(const uint8_t *kept, const uint32_t *target, uint32_t n, uint32_t *root,
                            unsigned long long *counters, uint32_t n_cus, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    cr_finish_kernel<<<cr_grid(n, n_cus), 256, 0, s>>>(kept, target, n, root, counters);
    return hipGetLastError();
}

} // namespace umihip
