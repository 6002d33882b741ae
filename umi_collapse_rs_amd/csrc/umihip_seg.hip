// Segment index of the large buckets (gfx950): the n-gram partition and the all-pairs evaluation
// inside its sub-buckets.
//
// What it replaces in the reference (tkob-vh/umi-collapse-rs): the same rows of the scope table as
// the tile kernels of umihip_kernels.hip -- Naive::remove_near's linear scans
// (src/data/naive.rs:26-40) with BitSet::bit_count_xor / umi_dist (src/utils/bitset.rs:77-91,
// src/utils/mod.rs:24-26) -- for buckets large enough that evaluating every pair is the cost.
// Two UMIs within k substitutions agree exactly on at least one of k+1 disjoint base ranges, so a
// bucket is cut k+1 times into sub-buckets by the value of one range (a counting sort on the
// device: histogram in prep_kernel, scan, scatter) and only the pairs inside a sub-buckets are
// evaluated, with the same arithmetic; a pair that shares several ranges is reported by the first.
// Result = Naive's, pair for pair.  Integer/bitwise work, 64-lane waves, no MFMA.
#include <hip/hip_runtime.h>

#include "umihip_internal.h"
#include "umihip_device.h"

namespace umihip {

namespace {

constexpr int SCAN_THREADS = 256;
constexpr int SCAN_PER_THREAD = SEG_SCAN_CHUNK / SCAN_THREADS; // one bin per thread

// a part whose bins are indexed by nb bases has its sub-buckets decided by lookups (seg_local_kernel)
__device__ __forceinline__ bool probe_part(const SegArgs &g, uint32_t nb)
{
    return g.probe_rest != 0u && g.umi_len - (int)nb <= (int)g.probe_rest;
}
// (a part-0 sub-bucket the local kernel takes has no tile tasks)
__device__ __forceinline__ bool local_bin(const SegArgs &g, uint32_t part, uint32_t c) { return part == 0 && c <= g.local_cap; }
// a super-bin of n entries is seg_super_kernel's: its bins have no tile tasks either
__device__ __forceinline__ bool super_taken(const SegArgs &g, uint32_t n) { return n >= 2u && n <= g.super_cap; }
// super-bin exponent of a segment in this call (wave-uniform)
__device__ __forceinline__ uint32_t super_bases(const SegArgs &g, uint32_t seg) { return g.super_cap ? g.segs[seg].sup_g : 0u; }
// ... if its part 0 is filed by super-bin (SegArgs::super_coarse), else 0: the bases a run's bins differ in
__device__ __forceinline__ uint32_t coarse_bases(const SegArgs &g, uint32_t seg) { return g.super_coarse ? super_bases(g, seg) : 0u; }

// Exclusive scan of the bin counts -> bin_start, the task list, the pair count: ONE launch, the
// chunks chained by a decoupled look-back.  A block draws its chunk from a ticket counter (so that
// every chunk before it has a block that is already running), sums its 256 bins' (entries, tasks),
// publishes the sums, adds up what the chunks before it have published -- stopping at the first
// that already knows its own prefix -- publishes its prefix and writes its bins.
// Status word of a chunk: bit 63 = sums there, bit 31 = they include all chunks before; entries in
// bits 32..62, tasks in bits 0..30 (both stay below 2^31: checked on the host); one 64-bit access.
constexpr unsigned long long SCAN_HAVE = 1ull << 63, SCAN_PREFIX = 1ull << 31;
__device__ __forceinline__ unsigned long long scan_pack(uint32_t e, uint32_t t) { return ((unsigned long long)e << 32) | t; }
__global__ __launch_bounds__(SCAN_THREADS) void seg_scan_kernel(SegArgs g, unsigned long long *counters)
{
    __shared__ uint2 wsum[SCAN_THREADS / 64];
    __shared__ uint32_t my_chunk;
    __shared__ uint2 prefix;
    unsigned long long *ticket = g.scan_state, *status = g.scan_state + 1;
    if (threadIdx.x == 0) my_chunk = (uint32_t)atomicAdd(ticket, 1ull);
    __syncthreads();
    const uint32_t ci = my_chunk;
    const SegScanChunk ch = g.chunks[ci];
    // a thread owns SCAN_PER_THREAD consecutive bins
    uint32_t c[SCAN_PER_THREAD];
    uint2 mine = make_uint2(0u, 0u);
    const uint32_t b_first = threadIdx.x * SCAN_PER_THREAD;
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; q++) {
        const uint32_t b = b_first + q;
        c[q] = b < ch.nbins ? g.bin_cnt[ch.bin0 + b] : 0u;
        mine.x += c[q];
    }
    // bit q: bin q of this thread has no tile tasks -- the local kernel's, or inside a taken super-bin.  A super-bin
    // is 4^sg adjacent bins, the bins of 4^sg / SCAN_PER_THREAD adjacent threads (one chunk at most)
    uint32_t no_tasks = 0;
    const uint32_t sg = ch.part == 0 ? super_bases(g, ch.seg) : 0u; // (block-uniform)
    if (sg) {
        static_assert(SCAN_PER_THREAD == 1 || SCAN_PER_THREAD == 4, "a super-bin is whole threads' bins");
        __shared__ uint32_t tcnt[SCAN_THREADS];
        tcnt[threadIdx.x] = mine.x;
        __syncthreads();
        const uint32_t nthr = (1u << (2 * sg)) / SCAN_PER_THREAD, t0 = threadIdx.x & ~(nthr - 1u);
        uint32_t n_super = 0;
        for (uint32_t i = 0; i < nthr; i++) n_super += tcnt[t0 + i];
        if (super_taken(g, n_super)) no_tasks = (1u << SCAN_PER_THREAD) - 1u;
        // a super-bin above the cap goes to the tiles: the segment's word says that not all of its super-bins are
        // taken (the blocks that find one all store the same value; an empty or single entry holds no pair)
        if (n_super > g.super_cap && threadIdx.x == t0) g.scan_state[seg_scan_flag_word(g.n_chunks, ch.seg)] = 1ull;
    } else {
#pragma unroll
        for (int q = 0; q < SCAN_PER_THREAD; q++)
            if (local_bin(g, ch.part, c[q])) no_tasks |= 1u << q;
    }
    // a cross segment has no tile tasks at all: seg_super_kernel and seg_cross_kernel decide its pairs between them (a
    // super-bin they cannot serve sends the whole call back through the index: CNT_SEG_CROSS_ABANDONED)
    if (g.segs[ch.seg].cross) no_tasks = (1u << SCAN_PER_THREAD) - 1u; // (block-uniform)
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; q++) mine.y += (no_tasks >> q) & 1u ? 0u : seg_tasks_of_bin(c[q]);
    uint2 incl = mine;
    for (int d = 1; d < 64; d <<= 1) {
        const uint32_t ux = __shfl_up(incl.x, d), uy = __shfl_up(incl.y, d);
        if ((int)(threadIdx.x & 63) >= d) {
            incl.x += ux;
            incl.y += uy;
        }
    }
    if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
    __syncthreads();
    if (threadIdx.x < 64) { // the first wave: the block's sums out, the look-back
        uint2 tot = make_uint2(0u, 0u);
        for (int w = 0; w < SCAN_THREADS / 64; w++) {
            tot.x += wsum[w].x;
            tot.y += wsum[w].y;
        }
        const int lane = threadIdx.x;
        if (lane == 0)
            __hip_atomic_store(&status[ci], SCAN_HAVE | (ci == 0 ? SCAN_PREFIX : 0ull) | scan_pack(tot.x, tot.y),
                               __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
        uint2 before = make_uint2(0u, 0u);
        int64_t j0 = (int64_t)ci - 1; // lane l looks at chunk j0 - l
        while (j0 >= 0) {
            const int64_t j = j0 - lane;
            unsigned long long st = SCAN_HAVE | SCAN_PREFIX; // (before the first chunk: an empty prefix)
            if (j >= 0)
                do st = __hip_atomic_load(&status[j], __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT);
                while (!(st & SCAN_HAVE)); // (chunk j's block drew its ticket before this one: it is running)
            const unsigned long long stops = __ballot((st & SCAN_PREFIX) != 0);
            const int first = __ffsll(stops) - 1; // nearest chunk whose sums include everything before it
            const bool take = first < 0 || lane <= first;
            uint32_t e = take && j >= 0 ? (uint32_t)(st >> 32) & 0x7FFFFFFFu : 0u;
            uint32_t t = take && j >= 0 ? (uint32_t)st & 0x7FFFFFFFu : 0u;
            for (int off = 32; off > 0; off >>= 1) {
                e += __shfl_xor(e, off);
                t += __shfl_xor(t, off);
            }
            before.x += e;
            before.y += t;
            if (first >= 0) break;
            j0 -= 64;
        }
        if (lane == 0) {
            if (ci != 0)
                __hip_atomic_store(&status[ci], SCAN_HAVE | SCAN_PREFIX | scan_pack(before.x + tot.x, before.y + tot.y),
                                   __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            prefix = before;
            if (ci + 1 == g.n_chunks) counters[CNT_SEG_TASKS] = before.y + tot.y;
        }
    }
    __syncthreads();
    const uint2 base = prefix;
    uint2 off = make_uint2(base.x + incl.x - mine.x, base.y + incl.y - mine.y);
    for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) {
        off.x += wsum[w].x;
        off.y += wsum[w].y;
    }
    // bin_start, the bins' tasks; bin_cnt is cleared for its second use as the scatter cursor
    unsigned long long pairs = 0;
#pragma unroll
    for (int q = 0; q < SCAN_PER_THREAD; q++) {
        const uint32_t b = b_first + q;
        if (b < ch.nbins) {
            g.bin_start[ch.bin0 + b] = off.x;
            g.bin_cnt[ch.bin0 + b] = 0;
            const uint32_t nt = (no_tasks >> q) & 1u ? 0u : seg_chunks_of(c[q]), e = seg_span_log2(nt), span = 1u << e;
            const uint32_t where = ch.seg | (ch.part << 24) | (e << 28);
            uint32_t ti = off.y;
            for (uint32_t t = 0; t < nt; t++) {
                const uint32_t row0 = off.x + 64u * t;
                for (uint32_t sp = 0; sp < nt - t; sp += span, ti++)
                    if (ti < g.task_cap) g.tasks[ti] = SegTask{row0, off.x + c[q], row0 + 1u + 64u * sp, where};
            }
            const uint32_t n_bin_tasks = ti - off.y;
            // (filed by super-bin: a bin's count is its whole run's, the pairs inside the fine bins are seg_super_kernel's to count)
            if (!(sg && g.super_coarse)) pairs += (unsigned long long)c[q] * (c[q] ? c[q] - 1 : 0) / 2;
            off.x += c[q];
            off.y += n_bin_tasks;
        }
    }
    // (64-bit sum over the block, one atomic)
    __shared__ unsigned long long psum[SCAN_THREADS / 64];
    for (int o = 32; o > 0; o >>= 1) pairs += __shfl_down(pairs, o);
    if ((threadIdx.x & 63) == 0) psum[threadIdx.x >> 6] = pairs;
    __syncthreads();
    if (threadIdx.x == 0) {
        unsigned long long t = 0;
        for (int w = 0; w < SCAN_THREADS / 64; w++) t += psum[w];
        if (t) atomicAdd(&counters[CNT_SEG_PAIRS], t);
    }
}

template <typename KeyT> struct SegRecOf;
template <> struct SegRecOf<uint32_t> { using type = SegRec32; };
template <> struct SegRecOf<uint64_t> { using type = SegRec64; };
// The 3-bit code of every base of a 2-bit filter key (A 000, T 101, C 110, G 011 as in
// src/utils/read.rs:23-31; the filter key holds the low two bits, the third is their xor): any two
// different bases differ in exactly two bits.  umi_len <= 16: 48 bits.
__device__ __forceinline__ uint64_t expand3(uint32_t fkey, int umi_len)
{
    uint64_t e = 0;
    for (int b = 0; b < umi_len; b++) {
        const uint32_t c = (fkey >> (2 * b)) & 3u;
        e |= (uint64_t)(c | (((c >> 1) ^ c) & 1u) << 2) << (3 * b);
    }
    return e;
}
// ... without the nb bases from b0 on (the bin's own); 0 if more than 10 bases are left
__device__ __forceinline__ uint32_t compare_key(uint64_t e3, int b0, int nb, int umi_len)
{
    if (umi_len - nb > 10) return 0u;
    const uint64_t lo = e3 & ((1ull << (3 * b0)) - 1ull);
    const uint64_t hi = e3 >> (3 * (b0 + nb));
    return (uint32_t)(lo | (hi << (3 * b0)));
}
__device__ __forceinline__ SegRec32 make_rec(uint32_t key, uint32_t idx, int32_t freq, uint32_t ckey) { return SegRec32{key, idx, freq, ckey}; }
__device__ __forceinline__ SegRec64 make_rec(uint64_t key, uint32_t idx, int32_t freq, uint32_t) { return SegRec64{key, idx, freq}; }
__device__ __forceinline__ uint64_t expand3(uint64_t, int) { return 0ull; }

// every entry of a segment to its position in each part's sub-bucket order (the order inside a
// sub-bucket is arbitrary: all its pairs are evaluated, and a pair is reported with its entry
// indices in rank order whatever the positions)
template <typename KeyT>
__global__ __launch_bounds__(256) void seg_scatter_kernel(SegArgs g, const KeyT *__restrict__ fkey,
                                                          const int32_t *__restrict__ freq)
{
    using Rec = typename SegRecOf<KeyT>::type;
    const RangeTask r = g.ranges[blockIdx.x];
    if (r.seg == SEG_NONE) return;
    const SegDesc *__restrict__ sd = g.segs + r.seg;
    Rec *__restrict__ sub = (Rec *)g.sub_rec;
    for (uint32_t i = r.start + threadIdx.x; i < r.end; i += blockDim.x) {
        const KeyT key = fkey[i];
        const int32_t f = freq[i];
        const uint64_t e3 = g.use_ckey ? expand3(key, g.umi_len) : 0ull;
        for (int j = 0; j < g.n_parts; j++) {
            const uint32_t b = sd->bin_off[j] + seg_part_bits(key, sd->b0[j], sd->nb[j]);
            const uint32_t pos = g.bin_start[b] + atomicAdd(&g.bin_cnt[b], 1u);
            sub[pos] = make_rec(key, i, f, g.use_ckey ? compare_key(e3, sd->b0[j], sd->nb[j], g.umi_len) : 0u);
        }
    }
}

// ---- the counting sort's LDS path --------------------------------------------------------------
// A block of 1024 threads owns up to SEG_BLOCK_ENTRIES consecutive entries of one segment (their
// filter keys stay in L2 between the passes) and takes the segment's parts one after the other:
// the block's entries are counted per bin in LDS, and a bin's global word is touched once per
// block.  Count pass: one add of the block's count.  Scatter pass (after the scan has turned the
// totals into bin_start and cleared the words): one returning add that reserves the block's run
// inside the bin; the position of an entry is then bin_start + run start + an LDS counter.
// A (block, bin) run is contiguous in the sub-bucket arrays, so the 16-byte records of a block
// fill whole lines instead of landing one by one.
// The parts of one pass: as many as fit the LDS counters side by side (both parts of a 12-base
// UMI at k = 1: the keys are read once per pass).
constexpr int SEG_PASS_PARTS = 4;
struct SegPass {
    int np;                        // parts in this pass
    int b0[SEG_PASS_PARTS], nb[SEG_PASS_PARTS];
    uint32_t nbins[SEG_PASS_PARTS], bin_off[SEG_PASS_PARTS];
    uint32_t lds_off[SEG_PASS_PARTS]; // first counter of the part in hist[]
    uint32_t sh[SEG_PASS_PARTS];   // low bits of the bin code a counter leaves out: 2 * cg for part 0, else 0
    uint32_t total;                // counters of the pass
};
// cg (coarse_bases): part 0 is filed by runs of 4^cg bins -- its counters are the runs, dense in LDS (4^cg words
// apart they would share a handful of banks), and stand for the first bin of their run
__device__ __forceinline__ SegPass seg_pass_of(const SegDesc *__restrict__ sd, int j0, int n_parts, int per_pass, uint32_t cg)
{
    SegPass ps;
    ps.np = min(per_pass, n_parts - j0);
    ps.total = 0;
#pragma unroll
    for (int q = 0; q < SEG_PASS_PARTS; q++) {
        const bool on = q < ps.np;
        ps.b0[q] = on ? sd->b0[j0 + q] : 0;
        ps.nb[q] = on ? sd->nb[j0 + q] : 0;
        ps.sh[q] = on && j0 + q == 0 ? 2u * cg : 0u;
        ps.nbins[q] = on ? (1u << (2 * ps.nb[q])) >> ps.sh[q] : 0u;
        ps.bin_off[q] = on ? sd->bin_off[j0 + q] : 0u;
        ps.lds_off[q] = ps.total;
        ps.total += ps.nbins[q];
    }
    return ps;
}
// part and bin of counter c of the pass (c < ps.total)
__device__ __forceinline__ uint32_t seg_pass_global_bin(const SegPass &ps, uint32_t c)
{
    uint32_t gb = 0;
#pragma unroll
    for (int q = 0; q < SEG_PASS_PARTS; q++)
        if (q < ps.np && c >= ps.lds_off[q] && c < ps.lds_off[q] + ps.nbins[q]) gb = ps.bin_off[q] + ((c - ps.lds_off[q]) << ps.sh[q]);
    return gb;
}

// count the block's entries per bin of the pass's parts into hist[] (LDS, cleared first)
template <typename KeyT>
__device__ __forceinline__ void seg_block_histogram(const SegBlock &blk, const KeyT *__restrict__ fkey,
                                                    const SegPass &ps, uint32_t *hist)
{
    for (uint32_t b = threadIdx.x; b < ps.total; b += SEG_BLOCK_THREADS) hist[b] = 0;
    __syncthreads();
    constexpr int B = 8; // loads in flight per thread
    for (uint32_t i0 = blk.start + threadIdx.x; i0 < blk.end; i0 += B * SEG_BLOCK_THREADS) {
        KeyT key[B];
#pragma unroll
        for (int q = 0; q < B; q++) {
            const uint32_t i = i0 + (uint32_t)q * SEG_BLOCK_THREADS;
            key[q] = i < blk.end ? fkey[i] : KeyT(0);
        }
#pragma unroll
        for (int q = 0; q < B; q++)
            if (i0 + (uint32_t)q * SEG_BLOCK_THREADS < blk.end) {
#pragma unroll
                for (int j = 0; j < SEG_PASS_PARTS; j++)
                    if (j < ps.np) atomicAdd(&hist[ps.lds_off[j] + (seg_part_bits(key[q], ps.b0[j], ps.nb[j]) >> ps.sh[j])], 1u);
            }
    }
    __syncthreads();
}

// the filter key of an entry (umihip_kernels.hip's prep_kernel): 2 bits per base in 32 bits, or the
// 3-bit key itself in 64, N (masked by n_bits) folded onto A
__device__ __forceinline__ void store_filter_key(uint32_t *fkey, uint32_t i, uint64_t k3, int umi_len)
{
    uint32_t fk = 0;
    for (int b = 0; b < umi_len; b++) fk |= (uint32_t)((k3 >> (3 * b)) & 3ull) << (2 * b);
    fkey[i] = fk;
}
__device__ __forceinline__ void store_filter_key(uint64_t *fkey, uint32_t i, uint64_t k3, int) { fkey[i] = k3; }

template <typename KeyT>
__global__ __launch_bounds__(SEG_BLOCK_THREADS) void seg_count_lds_kernel(SegArgs g, KeyT *fkey)
{
    extern __shared__ uint32_t hist[];
    const SegBlock blk = g.blocks[blockIdx.x];
    const SegDesc *__restrict__ sd = g.segs + blk.seg;
    const uint32_t cg = coarse_bases(g, blk.seg); // (block-uniform)
    if (g.prep_keys) {
        // the entry kernel's work for this block's entries (prep_kernel, umihip_kernels.hip): filter
        // key, threshold (directional.rs:38), label, and the contract check -- freq >= 1, no N code
        // without nmask, no rise of freq inside the bucket (a segment is one bucket: its first entry
        // is the one place where freq may rise; the host wants CNT_RISES == CNT_START_RISES, and
        // this kernel adds to neither for that entry)
        unsigned int bad = 0, rises = 0;
        for (uint32_t i = blk.start + threadIdx.x; i < blk.end; i += SEG_BLOCK_THREADS) {
            const uint64_t key = g.prep_keys[(size_t)i * g.key_words];
            const uint64_t nm = g.prep_nmask ? g.prep_nmask[(size_t)i * g.key_words] : 0ull;
            const int32_t f = g.prep_freq[i];
            g.prep_thr[i] = threshold_of(g.prep_percentage, f);
            g.prep_label[i] = i;
            if (g.prep_lab) g.prep_lab[i] = i; // (the mask-only collapse starts from it: its round 0 has no entry pass)
            const uint64_t k3 = key & ~nm & (g.umi_len >= 21 ? 0x7FFFFFFFFFFFFFFFull : ((1ull << (3 * g.umi_len)) - 1ull));
            store_filter_key(fkey, i, k3, g.umi_len);
            bad += f < 1 ? 1u : 0u;
            const uint64_t b2 = k3 & 0x4924924924924924ull;
            bad += (b2 & ~((k3 << 1) | (k3 << 2))) != 0 ? 1u : 0u;
            if (g.key_words > 1 && !g.prep_nmask)
                bad += wide_n_codes(g.prep_keys + (size_t)i * g.key_words, g.key_words, g.full_umi_len);
            rises += (i > sd->start && f > g.prep_freq[i - 1]) ? 1u : 0u;
        }
        if (__any(bad != 0u)) { // (rare: no reduction tree for it)
            if (bad) atomicAdd(&g.prep_counters[CNT_ERROR], (unsigned long long)bad);
        }
        for (int off = 32; off > 0; off >>= 1) rises += __shfl_down(rises, off);
        if ((threadIdx.x & 63) == 0 && rises) atomicAdd(&g.prep_counters[CNT_RISES], (unsigned long long)rises);
        __syncthreads(); // the block's filter keys are read back below
    }
    for (int j0 = 0; j0 < g.n_parts; j0 += (int)g.parts_per_pass) {
        const SegPass ps = seg_pass_of(sd, j0, g.n_parts, (int)g.parts_per_pass, cg);
        seg_block_histogram(blk, fkey, ps, hist);
        for (uint32_t c = threadIdx.x; c < ps.total; c += SEG_BLOCK_THREADS) {
            const uint32_t cnt = hist[c];
            if (cnt) atomicAdd(&g.bin_cnt[seg_pass_global_bin(ps, c)], cnt);
        }
        __syncthreads();
    }
}

template <typename KeyT>
__global__ __launch_bounds__(SEG_BLOCK_THREADS) void seg_scatter_lds_kernel(SegArgs g, const KeyT *__restrict__ fkey,
                                                                            const int32_t *__restrict__ freq)
{
    using Rec = typename SegRecOf<KeyT>::type;
    extern __shared__ uint32_t hist[];
    const SegBlock blk = g.blocks[blockIdx.x];
    const SegDesc *__restrict__ sd = g.segs + blk.seg;
    const uint32_t cg = coarse_bases(g, blk.seg); // (block-uniform)
    Rec *__restrict__ sub = (Rec *)g.sub_rec;
    // (a cross segment files part 0 alone: nobody reads its part 1, whose positions hold seg_super_kernel's ranks)
    const int n_parts = sd->cross ? 1 : g.n_parts; // (block-uniform)
    for (int j0 = 0; j0 < n_parts; j0 += (int)g.parts_per_pass) {
        const SegPass ps = seg_pass_of(sd, j0, n_parts, (int)g.parts_per_pass, cg);
        seg_block_histogram(blk, fkey, ps, hist);
        // the block's run inside every bin it has entries for: the counter becomes its first position
        for (uint32_t c = threadIdx.x; c < ps.total; c += SEG_BLOCK_THREADS) {
            const uint32_t cnt = hist[c];
            if (cnt) {
                const uint32_t gb = seg_pass_global_bin(ps, c);
                hist[c] = g.bin_start[gb] + atomicAdd(&g.bin_cnt[gb], cnt);
            }
        }
        __syncthreads();
        constexpr int B = 4;
        for (uint32_t i0 = blk.start + threadIdx.x; i0 < blk.end; i0 += B * SEG_BLOCK_THREADS) {
            KeyT key[B];
            int32_t f[B];
#pragma unroll
            for (int q = 0; q < B; q++) {
                const uint32_t i = i0 + (uint32_t)q * SEG_BLOCK_THREADS;
                key[q] = i < blk.end ? fkey[i] : KeyT(0);
                f[q] = i < blk.end ? freq[i] : 0;
            }
            uint64_t e3[B];
#pragma unroll
            for (int q = 0; q < B; q++) e3[q] = g.use_ckey ? expand3(key[q], g.umi_len) : 0ull;
#pragma unroll
            for (int j = 0; j < SEG_PASS_PARTS; j++) {
                if (j < ps.np) {
                    uint32_t pos[B];
#pragma unroll
                    for (int q = 0; q < B; q++)
                        pos[q] = i0 + (uint32_t)q * SEG_BLOCK_THREADS < blk.end
                                     ? atomicAdd(&hist[ps.lds_off[j] + (seg_part_bits(key[q], ps.b0[j], ps.nb[j]) >> ps.sh[j])], 1u)
                                     : 0u;
#pragma unroll
                    for (int q = 0; q < B; q++) {
                        const uint32_t i = i0 + (uint32_t)q * SEG_BLOCK_THREADS;
                        if (i < blk.end)
                            sub[pos[q]] = make_rec(key[q], i, f[q],
                                                   g.use_ckey ? compare_key(e3[q], ps.b0[j], ps.nb[j], g.umi_len) : 0u);
                    }
                }
            }
        }
        __syncthreads();
    }
}

__device__ __forceinline__ uint32_t readlane_key(uint32_t v, int lane)
{
    return (uint32_t)__builtin_amdgcn_readlane((int)v, lane);
}
__device__ __forceinline__ uint64_t readlane_key(uint64_t v, int lane)
{
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)v, lane);
    const uint32_t hi = (uint32_t)__builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), lane);
    return ((uint64_t)hi << 32) | lo;
}

// base-level filter test of the inner loop: at most k bases of the two filter keys differ
// (exact on N-free keys: the filter key is the key there)
__device__ __forceinline__ bool within_k(uint32_t z, int k)
{
    return __builtin_popcount((z | (z >> 1)) & 0x55555555u) <= k;
}
__device__ __forceinline__ bool within_k(uint64_t z, int k)
{ // 3-bit codes with the third bit clear: two codes differ in exactly two bits or in none
    return __builtin_popcountll(z) <= 2 * k;
}

// All pairs inside the sub-buckets.  One wave per block, persistent over the task list.  A task
// is 64 rows of a sub-bucket (one per lane, the filter key in a register) against the later
// entries of the same sub-bucket, 64 columns at a time, one per lane as well: column j of the tile
// is broadcast with v_readlane (j is a constant of the unrolled loop), and every lane keeps the
// outcome for its own row as bit j of a 64-bit mask -- eight VALU instructions per column and 64
// pairs (readlane, xor, shift, and-or, popcount, compare, select, or), no branch, no scalar
// dependency, no LDS.  Sub-buckets are dense in neighbours by construction (about one pair in 200
// at config 2: some twenty hits per 64 x 64 tile), so a hit must be cheap where it is found: after
// the tile the lanes with a set bit note (row position, column position) in a queue in LDS, one
// hit per lane and round.  When 64 are queued the wave works them off one per lane: both records
// again (L2), the dedupe rule (a pair that shares an earlier part's bin was reported there), the
// exact distance with the reference's arithmetic where keys carry N, the freq predicate of the
// mode, and the edge goes to the block's LDS stage.
// the key the column loop compares: the record's filter key, or (CK) its compare key
template <bool CK> __device__ __forceinline__ uint32_t loop_key(const SegRec32 &r) { return CK ? r.ckey : r.key; }
template <bool CK> __device__ __forceinline__ uint64_t loop_key(const SegRec64 &r) { return r.key; }
// at most k bases differ
template <bool CK> __device__ __forceinline__ bool loop_within_k(uint32_t z, int k)
{
    return CK ? __builtin_popcount(z) <= 2 * k : within_k(z, k);
}
template <bool CK> __device__ __forceinline__ bool loop_within_k(uint64_t z, int k) { return within_k(z, k); }

// Columns J, J-1, J-2, J-3 of the tile (keys in the lanes of ky) against this lane's row x: the
// outcome "at most k bases differ" of each is shifted into h from below, highest column first.
// Compare keys (CK; lim2 = 2 k, wave-uniform): five instructions per column -- broadcast, xor,
// popcount, compare, add-with-carry -- written out, four columns interleaved so that no broadcast
// or compare mask is read within two instructions of the VALU instruction that wrote it (gfx950:
// two wait states between a VALU write of an SGPR or VCC and a VALU read of it -- the compiler
// covers them with s_nop, inline asm has to keep the distance itself; the compiler's own
// select-and-or accumulation takes two to three instructions instead of the add).
template <bool CK, int J> __device__ __forceinline__ uint32_t four_columns(uint32_t h, uint32_t x, uint32_t ky, int k, uint32_t lim2)
{
    if (CK) {
        uint32_t s0, s1, s2, s3, t0, t1, t2, t3;
        unsigned long long p0, p1, p2, p3; // the compares' lane masks, each its own SGPR pair
        asm("v_readlane_b32 %1, %14, %16\n\t"
            "v_readlane_b32 %2, %14, %17\n\t"
            "v_readlane_b32 %3, %14, %18\n\t"
            "v_readlane_b32 %4, %14, %19\n\t"
            "v_xor_b32_e32 %5, %1, %13\n\t"
            "v_xor_b32_e32 %6, %2, %13\n\t"
            "v_xor_b32_e32 %7, %3, %13\n\t"
            "v_xor_b32_e32 %8, %4, %13\n\t"
            "v_bcnt_u32_b32 %5, %5, 0\n\t"
            "v_bcnt_u32_b32 %6, %6, 0\n\t"
            "v_bcnt_u32_b32 %7, %7, 0\n\t"
            "v_bcnt_u32_b32 %8, %8, 0\n\t"
            "v_cmp_ge_u32_e64 %9, %15, %5\n\t"
            "v_cmp_ge_u32_e64 %10, %15, %6\n\t"
            "v_cmp_ge_u32_e64 %11, %15, %7\n\t"
            "v_cmp_ge_u32_e64 %12, %15, %8\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %9\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %10\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %11\n\t"
            "v_addc_co_u32_e64 %0, vcc, %0, %0, %12"
            : "+v"(h), "=&s"(s0), "=&s"(s1), "=&s"(s2), "=&s"(s3), "=&v"(t0), "=&v"(t1), "=&v"(t2), "=&v"(t3),
              "=&s"(p0), "=&s"(p1), "=&s"(p2), "=&s"(p3)
            : "v"(x), "v"(ky), "s"(lim2), "n"(J), "n"(J - 1), "n"(J - 2), "n"(J - 3)
            : "vcc");
        return h;
    }
#pragma unroll
    for (int j = J; j > J - 4; j--) h = h + h + (within_k(x ^ readlane_key(ky, j), k) ? 1u : 0u);
    return h;
}
template <bool CK, int J> __device__ __forceinline__ uint32_t four_columns(uint32_t h, uint64_t x, uint64_t ky, int k, uint32_t)
{
#pragma unroll
    for (int j = J; j > J - 4; j--) h = h + h + (within_k(x ^ readlane_key(ky, j), k) ? 1u : 0u);
    return h;
}
// columns BASE + 31 .. BASE of the tile
template <bool CK, int BASE, typename KeyT>
__device__ __forceinline__ uint32_t columns32(KeyT x, KeyT ky, int k, uint32_t lim2)
{
    uint32_t h = 0;
    h = four_columns<CK, BASE + 31>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 27>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 23>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 19>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 15>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 11>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 7>(h, x, ky, k, lim2);
    h = four_columns<CK, BASE + 3>(h, x, ky, k, lim2);
    return h;
}

// The same 64 columns against this lane's row, bit-sliced (compare keys, k <= 3): per base of the
// compare key the two low bits of the columns' codes become two wave ballots (bit j = column j), the
// lane XORs them with its own row's bits (as 0 / ~0 masks) -- a mismatch of the base where either
// differs (the third code bit is the xor of the two: src/utils/read.rs:23-31) -- and feeds sticky
// counters "more than l bases differ so far" through v_bitop3: fourteen instructions per base and
// 64 pairs at k = 1, 84 for the six compared bases of a 12-bp position, where the broadcast loop
// above takes 320.  Bit j of the result: at most K bases of column j differ from the row.
// SUP: ... and one of the bases in sup_bases (bit b: base b of the compare key, wave-uniform) is among them -- part 1
// of a segment whose super-bins are all taken: a pair that agrees on the bases a super-bin shares is not this tile's
template <int K, int NB, bool SUP = false>
__device__ __forceinline__ unsigned long long columns64_sliced(uint32_t x, uint32_t ky, uint32_t sup_bases = 0)
{
    uint32_t cl[K + 1], ch[K + 1], sl = 0, sh = 0;
#pragma unroll
    for (int l = 0; l <= K; l++) cl[l] = ch[l] = 0u;
#pragma unroll
    for (int b = 0; b < NB; b++) {
        const unsigned long long p0 = __ballot((ky & (1u << (3 * b))) != 0u), p1 = __ballot((ky & (2u << (3 * b))) != 0u);
        const uint32_t r0 = (uint32_t)((int32_t)(x << (31 - 3 * b)) >> 31), r1 = (uint32_t)((int32_t)(x << (30 - 3 * b)) >> 31);
        const uint32_t dl = BITOP3((uint32_t)p0 ^ r0, (uint32_t)p1, r1, TT_A | (TT_B ^ TT_C));
        const uint32_t dh = BITOP3((uint32_t)(p0 >> 32) ^ r0, (uint32_t)(p1 >> 32), r1, TT_A | (TT_B ^ TT_C));
#pragma unroll
        for (int l = K; l >= 1; l--) {
            cl[l] = BITOP3(cl[l], cl[l - 1], dl, TT_A | (TT_B & TT_C));
            ch[l] = BITOP3(ch[l], ch[l - 1], dh, TT_A | (TT_B & TT_C));
        }
        cl[0] |= dl;
        ch[0] |= dh;
        if (SUP && (sup_bases >> b) & 1u) {
            sl |= dl;
            sh |= dh;
        }
    }
    if (SUP) return (((unsigned long long)(sh & ~ch[K]) << 32) | (sl & ~cl[K]));
    return ~(((unsigned long long)ch[K] << 32) | cl[K]);
}
template <int K> __device__ __forceinline__ unsigned long long columns64_sliced_nb(uint32_t x, uint32_t ky, int nb, uint32_t sup_bases)
{
    if (K == 1 && sup_bases)
        switch (nb) {
        case 1: return columns64_sliced<1, 1, true>(x, ky, sup_bases);
        case 2: return columns64_sliced<1, 2, true>(x, ky, sup_bases);
        case 3: return columns64_sliced<1, 3, true>(x, ky, sup_bases);
        case 4: return columns64_sliced<1, 4, true>(x, ky, sup_bases);
        case 5: return columns64_sliced<1, 5, true>(x, ky, sup_bases);
        case 6: return columns64_sliced<1, 6, true>(x, ky, sup_bases);
        case 7: return columns64_sliced<1, 7, true>(x, ky, sup_bases);
        case 8: return columns64_sliced<1, 8, true>(x, ky, sup_bases);
        case 9: return columns64_sliced<1, 9, true>(x, ky, sup_bases);
        default: return columns64_sliced<1, 10, true>(x, ky, sup_bases);
        }
    switch (nb) { // (wave-uniform: the bases a compare key holds)
    case 1: return columns64_sliced<K, 1>(x, ky);
    case 2: return columns64_sliced<K, 2>(x, ky);
    case 3: return columns64_sliced<K, 3>(x, ky);
    case 4: return columns64_sliced<K, 4>(x, ky);
    case 5: return columns64_sliced<K, 5>(x, ky);
    case 6: return columns64_sliced<K, 6>(x, ky);
    case 7: return columns64_sliced<K, 7>(x, ky);
    case 8: return columns64_sliced<K, 8>(x, ky);
    case 9: return columns64_sliced<K, 9>(x, ky);
    default: return columns64_sliced<K, 10>(x, ky);
    }
}
// (sup_bases: only ever set at k = 1)
__device__ __forceinline__ unsigned long long columns64_sliced_k(uint32_t x, uint32_t ky, int k, int nb, uint32_t sup_bases = 0)
{
    switch (k) {
    case 0: return columns64_sliced_nb<0>(x, ky, nb, 0u);
    case 1: return columns64_sliced_nb<1>(x, ky, nb, sup_bases);
    case 2: return columns64_sliced_nb<2>(x, ky, nb, 0u);
    default: return columns64_sliced_nb<3>(x, ky, nb, 0u);
    }
}
__device__ __forceinline__ unsigned long long columns64_sliced_k(uint64_t, uint64_t, int, int, uint32_t = 0) { return 0ull; } // (never: CK is 32-bit)

// ILP unions per lane, their steps interleaved: a union is a chain of dependent scattered accesses
// (a load or a compare-and-swap per step, each a trip to the memory side), and a wave waits for
// the longest chain among its lanes; with ILP chains per lane in flight the trips of the others
// ride along.  Same algorithm as uf_union, step for step.
template <int ILP>
__device__ __forceinline__ void uf_union_multi(uint32_t *parent, uint32_t (&u)[ILP], uint32_t (&v)[ILP], bool (&act)[ILP])
{
    uint32_t pu[ILP], pv[ILP];
    // (u < v.)  First a direct try, as in uf_union: v, if it is still the root it started as, goes
    // under u with one access; otherwise the swap has returned v's parent and the walk starts with it.
    // (Behind seg_local_kernel about half the entries are children of depth-1 trees, and the try fails
    // more often; loading u's parent in the same trip as the swap was measured there: 0.305 ms per
    // config-2 step against 0.300 -- the extra load costs more than the trip it saves.)
    uint32_t seen[ILP];
#pragma unroll
    for (int s = 0; s < ILP; s++) seen[s] = act[s] ? atomicCAS(&parent[v[s]], v[s], u[s]) : 0u;
#pragma unroll
    for (int s = 0; s < ILP; s++) act[s] = act[s] && seen[s] != v[s] && seen[s] != u[s];
#pragma unroll
    for (int s = 0; s < ILP; s++) {
        pu[s] = act[s] ? ld_parent(&parent[u[s]]) : 0u;
        pv[s] = seen[s]; // (v's parent is known now)
    }
    for (;;) {
        bool cas[ILP], any = false;
#pragma unroll
        for (int s = 0; s < ILP; s++) {
            act[s] = act[s] && pu[s] != pv[s];
            if (act[s] && pu[s] < pv[s]) { // u is the side whose parent is the larger
                uint32_t t = u[s]; u[s] = v[s]; v[s] = t;
                t = pu[s]; pu[s] = pv[s]; pv[s] = t;
            }
            cas[s] = act[s] && u[s] == pu[s]; // a root, as far as was seen: under the other side's parent
            any = any || act[s];
        }
        if (!any) break;
        uint32_t r[ILP];
#pragma unroll
        for (int s = 0; s < ILP; s++) // (all of the step's accesses go out before any is waited for)
            r[s] = !act[s] ? 0u : cas[s] ? atomicCAS(&parent[u[s]], u[s], pv[s]) : ld_parent(&parent[pu[s]]);
#pragma unroll
        for (int s = 0; s < ILP; s++) {
            if (!act[s]) continue;
            if (cas[s]) {
                if (r[s] == u[s]) act[s] = false; // hooked
                else pu[s] = r[s];                // hooked by somebody else meanwhile: that is where it points now
            } else { // climbed
                u[s] = pu[s];
                pu[s] = r[s];
            }
        }
    }
}

// W > 1: keys of W words -- the filter keys hold the first word's 21 bases, every filter hit is decided
// by the distance over all words (src/utils/bitset.rs:77-91, word by word)
template <typename KeyT, bool HAS_N, bool CK, int W = 1>
__global__ __launch_bounds__(64) void seg_pair_kernel(PairArgs a, SegArgs g, float percentage,
                                                      uint32_t part, uint32_t n_parts)
{
    using Rec = typename SegRecOf<KeyT>::type;
    constexpr int ILP = 1;                      // queued hits a lane works off together (more: fewer, longer
                                                // drains, and a wave of config 2 queues under 200 hits in all --
                                                // the unions would all wait for the end of the kernel)
    constexpr uint32_t DRAIN_AT = 64 * ILP;     // a drain starts at this many queued hits ...
    constexpr uint32_t HITQ = DRAIN_AT + 64;    // ... and one round adds at most 64
    __shared__ EdgeStage stage;
    __shared__ uint2 hitq[HITQ]; // (row position, column position) in the sub-bucket arrays
    const int lane = threadIdx.x;
    const Rec *__restrict__ sub = (const Rec *)g.sub_rec;
    const uint4 *__restrict__ task_words = (const uint4 *)g.tasks;
    const bool with_dist = a.mode == MODE_NEIGHBOURS;
    if (lane == 0) {
        stage.count = 0;
        stage.candidates = 0;
    }
    __syncthreads();
    const uint32_t n_tasks = (uint32_t)min((unsigned long long)g.task_cap, a.counters[CNT_SEG_TASKS]);
    unsigned int n_cand = 0, n_direct = 0;
    const uint32_t lim2 = (uint32_t)__builtin_amdgcn_readfirstlane(2 * a.k);
    // masks of the bins of the parts before the task's own: a pair that shares one of them was
    // reported there.  Kept while the tasks stay in one (segment, part): nearly always.
    KeyT dup_mask[SEG_MAX_PARTS - 1];
#pragma unroll
    for (int j = 0; j < SEG_MAX_PARTS - 1; j++) dup_mask[j] = KeyT(0);
    uint32_t have_seg = SEG_NONE, have_part = 0;
    int ck_bases = 0;
    // a segment with super-bins, tasks of part 1: the filter-key bits of the bases a super-bin shares (as a part-0
    // bin code they are the super-bin's first bin), the bins of a super-bin, the segment's first part-0 bin
    // sup_tile: every super-bin of the segment is taken (the scan's word) and the tiles are bit-sliced -- the tile itself
    // leaves out the pairs that agree on these bases of the compare key, and the drain has nothing to ask (sup_bins 0)
    uint32_t sup_mask = 0, sup_bins = 0, sup_bin0 = 0, sup_tile = 0;
    // tasks of part 0 of a segment filed by super-bin (a run above the cap, one sub-bucket of 4^g fine bins whose
    // compare keys leave out all of the bin's bases): the part's own mask -- a hit is one only inside a fine bin
    KeyT coarse_mask = KeyT(0);
    const bool sliced = a.k <= 3 && g.col_sliced != 0;
    uint32_t nq = 0; // queued hits (wave-uniform); the queue outlives a task

    // The queued hits, ILP per lane at a time: both records again (L2), the dedupe rule (a pair
    // that shares an earlier part's bin was reported there), the exact distance with the
    // reference's arithmetic where keys carry N, the freq predicate of the mode; a one-way pair
    // goes to the block's LDS stage, a symmetric one is united on the spot (batched directional
    // path) or staged as well.
    auto drain = [&]() {
        __builtin_amdgcn_wave_barrier();
        for (uint32_t q0 = 0; q0 < nq; q0 += 64 * ILP) {
            Rec ra[ILP], cb[ILP];
            bool live[ILP];
#pragma unroll
            for (int s = 0; s < ILP; s++) {
                const uint32_t q = q0 + (uint32_t)s * 64u + (uint32_t)lane;
                live[s] = q < nq;
                const uint2 h = live[s] ? hitq[q] : make_uint2(0u, 0u);
                ra[s] = sub[live[s] ? h.x : 0u]; // (position 0 exists: the call has a segment)
                cb[s] = sub[live[s] ? h.y : 0u];
            }
            uint32_t uu[ILP], uv[ILP];
            bool unite[ILP];
#pragma unroll
            for (int s = 0; s < ILP; s++) {
                unite[s] = false;
                uu[s] = uv[s] = 0;
                if (!live[s]) continue;
                const KeyT z = ra[s].key ^ cb[s].key;
                bool ok = (z & coarse_mask) == KeyT(0); // (two fine bins of one run: no pair of this part)
#pragma unroll
                for (int p = 0; p < SEG_MAX_PARTS - 1; p++)
                    ok = ok && (dup_mask[p] == KeyT(0) || (z & dup_mask[p]) != KeyT(0));
                if (!ok) continue;
                // ... and a pair inside a taken super-bin by seg_super_kernel
                if (sup_bins && ((uint32_t)z & sup_mask) == 0u) {
                    const uint32_t b = sup_bin0 + ((uint32_t)ra[s].key & sup_mask);
                    if (super_taken(g, g.bin_start[b + sup_bins] - g.bin_start[b])) continue;
                }
                // entry indices in rank order (src/algo/directional.rs:67-72)
                const bool sw = cb[s].idx < ra[s].idx;
                const uint32_t gi = sw ? cb[s].idx : ra[s].idx, gj = sw ? ra[s].idx : cb[s].idx;
                const int32_t fi = sw ? cb[s].freq : ra[s].freq, fj = sw ? ra[s].freq : cb[s].freq;
                int dist;
                if (W > 1) { // bitset.rs:77-91, word by word, and utils/mod.rs:25
                    int res = 0;
#pragma unroll
                    for (int w = 0; w < W; w++) {
                        const uint64_t ka = a.keys[(size_t)gi * W + w], kb = a.keys[(size_t)gj * W + w];
                        const uint64_t xn = HAS_N ? a.nmask[(size_t)gi * W + w] ^ a.nmask[(size_t)gj * W + w] : 0ull;
                        res += __builtin_popcountll(xn | (ka ^ kb)) - __builtin_popcountll(xn) / 3;
                    }
                    dist = res / 2;
                } else if (HAS_N) { // bitset.rs:85-87 (one word) and utils/mod.rs:25
                    const uint64_t ka = a.keys[gi], kb = a.keys[gj];
                    const uint64_t xn = a.nmask[gi] ^ a.nmask[gj];
                    dist = (__builtin_popcountll(xn | (ka ^ kb)) - __builtin_popcountll(xn) / 3) / 2;
                } else { // no N in the call: the filter key is the key
                    dist = filter_key_distance(ra[s].key, cb[s].key);
                }
                n_cand++;
                if (dist > a.k) continue;
                if (a.mode == MODE_NEIGHBOURS) {
                    emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gi, gj, dist, true);
                    continue;
                }
                bool fwd, bwd;
                if (a.mode == MODE_DIRECTIONAL) { // naive.rs:31 under directional.rs:38-39
                    fwd = fj <= threshold_of(percentage, fi);
                    bwd = fi <= threshold_of(percentage, fj);
                } else if (a.mode == MODE_CLUSTER) { // connected components: a union, nothing to ask of freq
                    fwd = bwd = true;
                } else { // adjacency.rs:56: a root only ever sees entries of larger rank
                    fwd = fj <= a.adj_max_freq;
                    bwd = false;
                }
                if (fwd && bwd) {
                    if (g.uf_parent) { // reachability inside such a set is symmetric: one set
                        unite[s] = true;
                        uu[s] = gi;
                        uv[s] = gj;
                        n_direct++;
                    } else {
                        emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gi | SYM_FLAG, gj, dist, false);
                    }
                } else if (fwd) {
                    emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gi, gj, dist, false);
                } else if (bwd) {
                    emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gj, gi, dist, false);
                }
            }
            if (g.uf_parent) uf_union_multi<ILP>(g.uf_parent, uu, uv, unite);
            __builtin_amdgcn_wave_barrier();
            // (the stage is this wave's alone: its fill level is wave-uniform; a pass adds at most 64 * ILP)
            static_assert(64 * ILP <= EDGE_BUF / 4, "a pass must fit the stage's last quarter");
            if ((unsigned int)__builtin_amdgcn_readfirstlane((int)*(volatile unsigned int *)&stage.count) >= (unsigned int)EDGE_BUF * 3u / 4u)
                flush_edges<64>(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, with_dist, false);
        }
        nq = 0;
        __builtin_amdgcn_wave_barrier();
    };

    // Tasks are dealt statically, task t to block t mod the grid, and two stages run ahead of the
    // task in hand: the record of the task after next and the row and column keys of the next one
    // are under way while this one's columns are walked (a task is one 64 x 64 tile: a few hundred
    // instructions, less than one trip to memory).
    const uint32_t stride = gridDim.x;
    const uint4 none = make_uint4(0u, 0u, 0u, 0u);
    auto task_keys = [&](const uint4 &w, bool valid, KeyT &xk, KeyT &ck) {
        const uint32_t row0 = __builtin_amdgcn_readfirstlane(w.x), end = __builtin_amdgcn_readfirstlane(w.y);
        const uint32_t col0 = __builtin_amdgcn_readfirstlane(w.z);
        xk = pad_row<KeyT>();
        ck = pad_col<KeyT>();
        if (valid && row0 + (uint32_t)lane < end && lane < 64) xk = loop_key<CK>(sub[row0 + (uint32_t)lane]);
        if (valid && col0 + (uint32_t)lane < end) ck = loop_key<CK>(sub[col0 + (uint32_t)lane]);
    };
    uint32_t t = blockIdx.x;
    uint4 tw = t < n_tasks ? task_words[t] : none;
    uint4 tw1 = t + stride < n_tasks && t + stride > t ? task_words[t + stride] : none;
    KeyT x, ky;
    task_keys(tw, t < n_tasks, x, ky);
    while (t < n_tasks) {
        const uint32_t t1 = t + stride, t2 = t1 + stride;
        const bool has1 = t1 < n_tasks && t1 > t, has2 = has1 && t2 < n_tasks && t2 > t1;
        const uint4 tw2 = has2 ? task_words[t2] : none;
        KeyT x1, ky1;
        task_keys(tw1, has1, x1, ky1);
        const uint32_t row0 = __builtin_amdgcn_readfirstlane(tw.x);
        const uint32_t end = __builtin_amdgcn_readfirstlane(tw.y);
        const uint32_t col0 = __builtin_amdgcn_readfirstlane(tw.z);
        const uint32_t where = __builtin_amdgcn_readfirstlane(tw.w);
        const uint32_t seg = where & 0xFFFFFFu, my_part = (where >> 24) & 15u;
        const uint32_t col1 = (uint32_t)min((unsigned long long)end, (unsigned long long)col0 + (64ull << (where >> 28)));
        // A multi-GPU split hands out whole sub-buckets: the order inside one differs from rank to
        // rank (the scatter's atomics), its extent does not -- `end` names the sub-bucket.
        const bool mine = !(n_parts > 1 && (((end ^ (end >> 7)) * 0x9E3779B1u) >> 8) % n_parts != part);
        if (mine) {
            const uint32_t n_rows = min(64u, end - row0);
            const uint32_t r = row0 + (uint32_t)lane;
            if (seg != have_seg || my_part != have_part) { // (wave-uniform)
                if (nq) drain(); // the queued hits belong to the masks in hand
                const SegDesc *__restrict__ sd = g.segs + seg;
#pragma unroll
                for (int j = 0; j < SEG_MAX_PARTS - 1; j++)
                    dup_mask[j] = (uint32_t)j < my_part ? (KeyT)sd->mask[j] : KeyT(0);
                have_seg = seg;
                have_part = my_part;
                ck_bases = __builtin_amdgcn_readfirstlane(g.umi_len - (int)sd->nb[my_part]); // bases a compare key holds
                coarse_mask = my_part == 0 && coarse_bases(g, seg) ? (KeyT)sd->mask[0] : KeyT(0);
                const uint32_t sg = my_part != 0 ? super_bases(g, seg) : 0u;
                sup_mask = sg ? ((1u << (2 * (sd->nb[0] - sg))) - 1u) << (2 * sg) : 0u;
                sup_bins = sg ? 1u << (2 * sg) : 0u; // (0: no super-bins here)
                sup_bin0 = sd->bin_off[0];
                // (k = 1: part 1's compare key holds all of part 0's bases, base b at place b; a segment that is one
                // super-bin shares no base: the drain drops every hit of its part 1, as before)
                sup_tile = 0u;
                if (CK && sliced && sg && sg < sd->nb[0] && __builtin_amdgcn_readfirstlane((uint32_t)g.scan_state[seg_scan_flag_word(g.n_chunks, seg)]) == 0u) {
                    sup_tile = ((1u << sd->nb[0]) - 1u) & ~((1u << sg) - 1u);
                    sup_bins = 0u;
                }
            }
            for (uint32_t c0 = col0; c0 < col1; c0 += 64) {
                // (a task of several tiles -- a sub-bucket beyond 1025 entries: the next 64 columns
                // under way while these are walked)
                const uint32_t cn_pos = c0 + 64u + (uint32_t)lane;
                KeyT kn = pad_col<KeyT>();
                if (c0 + 64u < col1 && cn_pos < end) kn = loop_key<CK>(sub[cn_pos]);
                const uint32_t nc = min(64u, end - c0);
                unsigned long long h; // bit j: this lane's row is within k of column j of the tile
                if (CK && sliced) {
                    h = columns64_sliced_k(x, ky, a.k, ck_bases, sup_tile);
                } else {
                    uint32_t hlo = 0, hhi = 0;
                    hlo = columns32<CK, 0>(x, ky, a.k, lim2);
                    if (nc > 32) hhi = columns32<CK, 32>(x, ky, a.k, lim2);
                    h = ((unsigned long long)hhi << 32) | hlo;
                }
                // the columns this lane's row may pair with: inside the tile, and behind the row
                // (position c0 + j > r, i.e. j > lane - (c0 - row0))
                const int j_min = lane + 1 - (int)(c0 - row0);
                if (nc < 64) h &= (1ull << nc) - 1ull;
                if (j_min > 0) h = j_min >= 64 ? 0ull : h & ~((1ull << j_min) - 1ull);
                if ((uint32_t)lane >= n_rows) h = 0ull;
                while (__any(h != 0ull)) { // one hit per lane and round
                    const unsigned long long bal = __ballot(h != 0ull);
                    if (h) {
                        const int j = __builtin_ctzll(h);
                        h &= h - 1ull;
                        hitq[nq + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] =
                            make_uint2(r, c0 + (uint32_t)j);
                    }
                    nq += (uint32_t)__builtin_popcountll(bal);
                    if (nq >= DRAIN_AT) drain();
                }
                ky = kn;
            }
        }
        if (!has1) break;
        t = t1;
        tw = tw1;
        tw1 = tw2;
        x = x1;
        ky = ky1;
    }
    if (nq) drain();
    { // what the stage still holds goes to this block's own slot (seg_edge_append_kernel moves it)
        __builtin_amdgcn_wave_barrier();
        const unsigned int left = min(*(volatile unsigned int *)&stage.count, (unsigned int)EDGE_BUF);
        for (unsigned int i = lane; i < left; i += 64) {
            g.priv_edges[(size_t)blockIdx.x * SEG_PRIV_CAP + i] = stage.e[i];
            if (with_dist) g.priv_dist[(size_t)blockIdx.x * SEG_PRIV_CAP + i] = stage.d[i];
        }
        if (lane == 0) g.priv_cnt[blockIdx.x] = left;
    }
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off);
    for (int off = 32; off > 0; off >>= 1) n_direct += __shfl_down(n_direct, off);
    if (g.priv_stat) {
        if (lane == 0) g.priv_stat[blockIdx.x] = make_uint2(n_cand, n_direct);
    } else {
        if (lane == 0 && n_cand) atomicAdd(&a.counters[CNT_CANDIDATES], (unsigned long long)n_cand);
        if (lane == 0 && n_direct) atomicAdd(&a.counters[CNT_UF_DIRECT], (unsigned long long)n_direct);
    }
}

// ---- part 0 in LDS ------------------------------------------------------------------------------
// The k + 1 parts each partition a segment's entries, so every pair found in a part-0 sub-bucket joins
// two entries of that sub-bucket: its symmetric pairs can be united in a forest local to the bin,
// without a global atomic.  One wave per block, persistent, dealt whole part-0 bins statically (bin
// ids in scan-chunk order: those of part 0 come first in a segment).  A bin's records go to LDS once
// (structure of arrays: compare key, entry index, freq; the filter key is not needed -- part 0 has no
// dedupe rule, and without N the compare keys give the distance); its upper triangle is walked with
// the pair kernel's 64 x 64 tiles and hit queue; a symmetric pair is united in the LDS forest over
// positions in the bin, a one-way pair goes to the block's private slot.  The bin's forest is then
// written out canonically: label[idx] = the smallest entry index of idx's set, for every entry of the
// bin, with plain stores -- depth <= 1, every root the minimum of its set, which is what the global
// union keeps as well.  (The smallest position would not do: positions come from the scatter's atomics.)
// Plain stores would race the pair kernel's compare-and-swaps on the same words: this kernel is a
// launch of its own, and stream order puts all of it ahead of every global union.
constexpr uint32_t LOCAL_DRAIN_AT = 64;
constexpr uint32_t LOCAL_HITQ = LOCAL_DRAIN_AT + 64;

__device__ __forceinline__ uint32_t lds_ld(const uint32_t *p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP); }
// uf_union over positions in LDS (u < v; par[p] <= p)
__device__ __forceinline__ void lds_union(uint32_t *par, uint32_t u, uint32_t v)
{
    const uint32_t seen = atomicCAS(&par[v], v, u);
    if (seen == v || seen == u) return;
    uint32_t pu = lds_ld(&par[u]), pv = seen;
    while (pu != pv) {
        if (pu < pv) {
            uint32_t t = u; u = v; v = t;
            t = pu; pu = pv; pv = t;
        }
        if (u == pu) {
            const uint32_t old = atomicCAS(&par[u], u, pv);
            if (old == u) return;
            pu = old;
        } else {
            u = pu;
            pu = lds_ld(&par[u]);
        }
    }
}

// ... by many waves on forests of thousands of positions (seg_super_kernel): a climb also moves the position it
// leaves under its grandparent (path halving).  Every value a position's word ever holds is an ancestor of it --
// a root's word only changes by its own compare-and-swap, the halving stores only touch words that have a parent
// already -- so a stale store costs a step, never a set.
__device__ __forceinline__ void lds_union_halving(uint32_t *par, uint32_t u, uint32_t v)
{
    const uint32_t seen = atomicCAS(&par[v], v, u);
    if (seen == v || seen == u) return;
    uint32_t pu = lds_ld(&par[u]), pv = seen;
    while (pu != pv) {
        if (pu < pv) {
            uint32_t t = u; u = v; v = t;
            t = pu; pu = pv; pv = t;
        }
        if (u == pu) {
            const uint32_t old = atomicCAS(&par[u], u, pv);
            if (old == u) return;
            pu = old;
        } else {
            const uint32_t up = lds_ld(&par[pu]);
            if (up != pu) __hip_atomic_store(&par[u], up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
            u = pu;
            pu = up;
        }
    }
}

// ---- lookups instead of pairs (k = 1, no N in the call) ------------------------------------------------
// A part that leaves rest <= SEG_PROBE_MAX_REST bases outside its bins: inside a sub-bucket an entry is the
// 2 * rest bits of those bases (its rest-code s, the low two bits of every 3-bit group of the compare key,
// in base order), two entries are within one substitution exactly when their rest-codes differ in one
// base, and so an entry has 3 * rest possible partners, s ^ (d << 2 b) for b < rest, d = 1..3, each one bit
// of a 4^rest-bit map of the sub-bucket.  The bin's records are put in the order of their rest-codes (the
// rank of a code in the bitmap: a prefix of the words' popcounts plus the popcount of the bits below it),
// so that the position of a partner follows from its code and a pair is found once, at its smaller
// position.  The hits go through the same queue and drain as those of the tile walk.  Two entries with one
// rest-code -- a key twice in the input -- show when the map is built (a returning OR): that bin is walked
// by tiles, where such a pair is a hit of distance 0.
__device__ __forceinline__ uint32_t rest_code(uint32_t ck)
{
    uint32_t s = 0;
#pragma unroll
    for (int b = 0; b < SEG_PROBE_MAX_REST; b++) s |= ((ck >> (3 * b)) & 3u) << (2 * b);
    return s;
}

// CLUSTER: connected components -- every pair within k is united, nothing is asked of freq and no one-way
// pair exists (the private slots stay empty)
template <bool HAS_N, bool CLUSTER = false>
__global__ __launch_bounds__(64) void seg_local_kernel(PairArgs a, SegArgs g, float percentage)
{
    extern __shared__ uint32_t lds[];
    const uint32_t cap = g.local_cap;
    uint32_t *ck = lds, *ix = lds + cap, *fr = lds + 2 * cap, *par = lds + 3 * cap;
    uint32_t *hitq = lds + 4 * cap; // row position | column position << 16
    uint32_t *bm = hitq + LOCAL_HITQ, *pre = bm + SEG_PROBE_WORDS; // the bin's bitmap, set bits before each word
    const int lane = threadIdx.x;
    const SegRec32 *__restrict__ sub = (const SegRec32 *)g.sub_rec;
    const bool sliced = a.k <= 3 && g.col_sliced != 0;
    const uint32_t lim2 = (uint32_t)__builtin_amdgcn_readfirstlane(2 * a.k);
    unsigned int n_cand = 0, n_direct = 0;
    // one-way pairs: to this block's private slot, wave-uniform fill level; a slot that is full sends
    // the rest to the list, one atomic per wave and batch
    uint32_t n_out = 0;
    uint2 *__restrict__ slot = g.priv_edges + (size_t)blockIdx.x * SEG_PRIV_CAP;
    auto emit = [&](bool has, uint32_t u, uint32_t v) {
        const unsigned long long bal = __ballot(has);
        if (!bal) return;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(bal);
        const uint32_t pos = n_out + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        unsigned long long base = 0;
        if (n_out + cnt > SEG_PRIV_CAP) {
            const uint32_t first_over = max(n_out, SEG_PRIV_CAP);
            const int leader = __builtin_ctzll(bal);
            if (lane == leader) base = atomicAdd(&a.counters[CNT_EDGES], (unsigned long long)(n_out + cnt - first_over));
            base = __shfl(base, leader);
            base -= first_over;
        }
        if (has) {
            if (pos < SEG_PRIV_CAP) slot[pos] = make_uint2(u, v);
            else if (base + pos < a.edge_cap) a.edges[base + pos] = make_uint2(u, v);
        }
        n_out += cnt;
    };
    uint32_t nq = 0;
    auto drain = [&]() {
        __syncthreads();
        for (uint32_t q0 = 0; q0 < nq; q0 += 64) {
            const uint32_t q = q0 + (uint32_t)lane;
            const bool live = q < nq;
            const uint32_t h = live ? hitq[q] : 0u;
            const uint32_t pa = h & 0xFFFFu, pb = h >> 16;
            const uint32_t ia = ix[pa], ib = ix[pb];
            const int32_t fa = (int32_t)fr[pa], fb = (int32_t)fr[pb];
            // entry indices in rank order (src/algo/directional.rs:67-72)
            const bool sw = ib < ia;
            const uint32_t gi = sw ? ib : ia, gj = sw ? ia : ib;
            const int32_t fi = sw ? fb : fa, fj = sw ? fa : fb;
            int dist = 0;
            if (live) {
                if (HAS_N) { // bitset.rs:85-87 (one word) and utils/mod.rs:25
                    const uint64_t ka = a.keys[gi], kb = a.keys[gj];
                    const uint64_t xn = a.nmask[gi] ^ a.nmask[gj];
                    dist = (__builtin_popcountll(xn | (ka ^ kb)) - __builtin_popcountll(xn) / 3) / 2;
                } else { // no N in the call: the bases outside the bin differ in two code bits each
                    dist = __builtin_popcount(ck[pa] ^ ck[pb]) / 2;
                }
                n_cand++;
            }
            const bool near = live && dist <= a.k;
            // naive.rs:31 under directional.rs:38-39
            const bool fwd = near && (CLUSTER || fj <= threshold_of(percentage, fi));
            const bool bwd = near && (CLUSTER || fi <= threshold_of(percentage, fj));
            if (fwd && bwd) { // reachability inside such a set is symmetric: one set
                n_direct++;
                lds_union(par, min(pa, pb), max(pa, pb));
            }
            emit(fwd != bwd, fwd ? gi : gj, fwd ? gj : gi);
        }
        nq = 0;
        __syncthreads();
    };
    // one hit per lane and round into the queue
    auto push = [&](bool has, uint32_t h) {
        const unsigned long long bal = __ballot(has);
        if (has) hitq[nq + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = h;
        nq += (uint32_t)__builtin_popcountll(bal);
        if (nq >= LOCAL_DRAIN_AT) drain();
    };

    const uint32_t n_ids = g.n_chunks * SEG_SCAN_CHUNK;
    for (uint32_t id = blockIdx.x; id < n_ids; id += gridDim.x) {
        const SegScanChunk ch = g.chunks[id / SEG_SCAN_CHUNK];
        const uint32_t bi = id % SEG_SCAN_CHUNK;
        if (ch.part != 0 || bi >= ch.nbins || super_bases(g, ch.seg)) continue; // (a segment with super-bins: not this kernel's)
        const uint32_t nb = g.segs[ch.seg].nb[0];
        const uint32_t b = ch.bin0 + bi;
        const uint32_t c = __builtin_amdgcn_readfirstlane(g.bin_cnt[b]); // (the scatter's cursor: the count again)
        if (c < 2 || c > cap) continue;
        const uint32_t start = __builtin_amdgcn_readfirstlane(g.bin_start[b]);
        const int ck_bases = __builtin_amdgcn_readfirstlane(g.umi_len - (int)nb);
        for (uint32_t p = lane; p < c; p += 64) {
            const SegRec32 r = sub[start + p];
            ck[p] = r.ckey;
            ix[p] = r.idx;
            fr[p] = (uint32_t)r.freq;
            par[p] = p;
        }
        __syncthreads();
        bool probed = false;
        if (!HAS_N && a.k == 1 && probe_part(g, nb) && c >= g.probe_min) { // (wave-uniform)
            for (uint32_t w = lane; w < SEG_PROBE_WORDS; w += 64) bm[w] = 0u;
            __syncthreads();
            bool twice = false;
            for (uint32_t p = lane; p < c; p += 64) {
                const uint32_t sc = rest_code(ck[p]), bit = 1u << (sc & 31u);
                twice = twice || (atomicOr(&bm[sc >> 5], bit) & bit) != 0u;
            }
            __syncthreads();
            probed = !__any(twice);
        }
        if (probed) {
            { // set bits before every word: a lane sums two words, the wave scans the sums
                static_assert(SEG_PROBE_WORDS == 128, "two words per lane");
                const uint32_t n0 = (uint32_t)__builtin_popcount(bm[2 * lane]), n1 = (uint32_t)__builtin_popcount(bm[2 * lane + 1]);
                uint32_t incl = n0 + n1;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d);
                    if (lane >= d) incl += up;
                }
                pre[2 * lane] = incl - n0 - n1;
                pre[2 * lane + 1] = incl - n1;
            }
            __syncthreads();
            auto rank_of = [&](uint32_t sc) { // entries of the bin with a smaller rest-code = the position of sc's
                return pre[sc >> 5] + (uint32_t)__builtin_popcount(bm[sc >> 5] & ((1u << (sc & 31u)) - 1u));
            };
            // the records again (L2), to the order of their rest-codes
            for (uint32_t p = lane; p < c; p += 64) {
                const SegRec32 r = sub[start + p];
                const uint32_t q = rank_of(rest_code(r.ckey));
                ck[q] = r.ckey;
                ix[q] = r.idx;
                fr[q] = (uint32_t)r.freq;
            }
            __syncthreads();
            for (uint32_t row0 = 0; row0 < c; row0 += 64) {
                const uint32_t r = row0 + (uint32_t)lane;
                const uint32_t sc = r < c ? rest_code(ck[r]) : 0u;
                uint32_t m = 0; // bit 3 b + d - 1: the entry with base b changed by d is there, behind this one
#pragma unroll
                for (int bb = 0; bb < SEG_PROBE_MAX_REST; bb++) {
#pragma unroll
                    for (int d = 1; d <= 3; d++) {
                        const uint32_t t = sc ^ ((uint32_t)d << (2 * bb));
                        const uint32_t there = (bm[t >> 5] >> (t & 31u)) & 1u;
                        if (bb < ck_bases && t > sc) m |= there << (3 * bb + d - 1);
                    }
                }
                if (r >= c) m = 0u;
                while (__any(m != 0u)) {
                    uint32_t h = 0;
                    const bool has = m != 0u;
                    if (has) {
                        const int j = __builtin_ctz(m), bb = j / 3;
                        m &= m - 1u;
                        h = r | (rank_of(sc ^ ((uint32_t)(j - 3 * bb + 1) << (2 * bb))) << 16);
                    }
                    push(has, h);
                }
            }
        } else {
            // the upper triangle: 64-row chunks against the columns behind their first row
            for (uint32_t row0 = 0; row0 < c; row0 += 64) {
                const uint32_t r = row0 + (uint32_t)lane;
                const uint32_t n_rows = min(64u, c - row0);
                const uint32_t x = r < c ? ck[r] : pad_row<uint32_t>();
                for (uint32_t c0 = row0 + 1; c0 < c; c0 += 64) {
                    const uint32_t ky = c0 + (uint32_t)lane < c ? ck[c0 + lane] : pad_col<uint32_t>();
                    const uint32_t nc = min(64u, c - c0);
                    unsigned long long h; // bit j: this lane's row is within k of column j of the tile
                    if (sliced) {
                        h = columns64_sliced_k(x, ky, a.k, ck_bases);
                    } else {
                        uint32_t hlo = 0, hhi = 0;
                        hlo = columns32<true, 0>(x, ky, a.k, lim2);
                        if (nc > 32) hhi = columns32<true, 32>(x, ky, a.k, lim2);
                        h = ((unsigned long long)hhi << 32) | hlo;
                    }
                    const int j_min = lane + 1 - (int)(c0 - row0);
                    if (nc < 64) h &= (1ull << nc) - 1ull;
                    if (j_min > 0) h = j_min >= 64 ? 0ull : h & ~((1ull << j_min) - 1ull);
                    if ((uint32_t)lane >= n_rows) h = 0ull;
                    while (__any(h != 0ull)) { // one hit per lane and round
                        uint32_t hit = 0;
                        const bool has = h != 0ull;
                        if (has) {
                            const int j = __builtin_ctzll(h);
                            h &= h - 1ull;
                            hit = r | ((c0 + (uint32_t)j) << 16);
                        }
                        push(has, hit);
                    }
                }
            }
        }
        if (nq) drain();
        // the bin's sets out: root position of every entry (into ck[], free now), the smallest entry
        // index of every set (fr[] of its root), label[] of every entry
        for (uint32_t p = lane; p < c; p += 64) {
            uint32_t q = lds_ld(&par[p]);
            for (;;) {
                const uint32_t up = lds_ld(&par[q]);
                if (up == q) break;
                q = up;
            }
            ck[p] = q;
            fr[p] = 0xFFFFFFFFu;
        }
        __syncthreads();
        for (uint32_t p = lane; p < c; p += 64) atomicMin(&fr[ck[p]], ix[p]);
        __syncthreads();
        for (uint32_t p = lane; p < c; p += 64) g.uf_parent[ix[p]] = fr[ck[p]];
        __syncthreads(); // (the next bin's records overwrite these arrays)
    }
    if (lane == 0) g.priv_cnt[blockIdx.x] = min(n_out, SEG_PRIV_CAP);
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off);
    for (int off = 32; off > 0; off >>= 1) n_direct += __shfl_down(n_direct, off);
    if (lane == 0) g.priv_stat[blockIdx.x] = make_uint2(n_cand, n_direct); // (the flatten launch adds them up)
}

// ---- super-bins: runs of adjacent part-0 bins in LDS (k = 1, no N in the call) ---------------------------
// The index orders part-0 bins by their code, so the 4^g bins that share the upper nb - g bases of it lie back to
// back in the sub-bucket arrays: one super-bin.  A block that holds a whole super-bin in LDS decides every pair
// that agrees on those shared bases -- a pair inside one of its bins and a pair that differs in one of the g low
// bases, which would otherwise be part 1's to find and a global union's to join.  An entry is its rest-code (the
// filter key's 2 bits per base without the shared bases, at most SEG_SUPER_MAX_REST bases: the bases outside the
// bins below, the g low bases of the bin code -- the fine bin -- on top, so that the ranks of 4^g codes give the
// entries per fine bin), the super-bin a bitmap of 4^rest bits; the rest is seg_local_kernel's lookup path with many waves: records read
// once and kept in registers until the rank of their code is known, 3 * rest single-bit tests per entry for the
// partners with the larger code, the hits queued per wave and decided 64 at a time (SUPER_HITQ below), symmetric
// pairs united in an LDS forest over positions (lds_union_halving: hooks
// are compare-and-swaps, waves may race), one-way pairs to a private slot per wave, and the local kernel's
// write-out: label[idx] = smallest entry index of idx's set, the forest flattened by pointer jumping first.  A key twice in the input shows when the map is
// built: that super-bin's positions are walked pair by pair instead, where equal codes are a hit of distance 0.
// (Components by rounds of min-label hooking in place of the unions were built and measured: slower)
// Which super-bins: those of 2..super_cap entries, read off bin_start as the scan and the pair kernel do.
constexpr int SUPER_RPT = 8; // records a thread keeps in registers: a block takes SUPER_RPT * its threads
// The hits are not decided where the bit tests find them -- a trip of that loop has a few lanes of 64 live and
// pays the whole chain of LDS latencies for them -- but queued per wave and worked off 64 at a time, as
// seg_local_kernel does it.  A word of the queue: the record's own position (13 bits) | its partner << 13, the
// partner's rest-code (16 bits; its rank is looked up in the drain) or, in the walk, the partner's position.
// A wave reads and writes its own queue alone: no block barrier.  A push finds fewer than SUPER_DRAIN_AT hits
// queued (else the push before it had drained) and adds one per lane at most.
constexpr uint32_t SUPER_DRAIN_AT = 64;
constexpr uint32_t SUPER_HITQ = SUPER_DRAIN_AT + 64; // words per wave
static_assert(SUPER_DRAIN_AT - 1 + 64 <= SUPER_HITQ, "the fullest queue a push can leave");
constexpr uint32_t SUPER_FINE = 1u << (2 * SEG_SUPER_MAX_BASES); // fine bins of the largest run (static LDS of the kernel)
static_assert(SEG_SUPER_MAX_CAP <= (1u << 13) && 2 * SEG_SUPER_MAX_REST + 13 <= 32, "a position and a rest-code in one word");

#ifdef UMIHIP_DEV
// development build: the 100 MHz clock once everything this wave has asked of memory and LDS is back
__device__ __forceinline__ unsigned long long super_clock()
{
    unsigned long long t;
    __builtin_amdgcn_sched_barrier(0);
    asm volatile("s_waitcnt vmcnt(0) lgkmcnt(0)\n\ts_memrealtime %0\n\ts_waitcnt lgkmcnt(0)" : "=s"(t) : : "memory");
    __builtin_amdgcn_sched_barrier(0);
    return t;
}
#endif

template <bool CLUSTER, int NT>
__global__ __launch_bounds__(NT) void seg_super_kernel(PairArgs a, SegArgs g, float percentage)
{
    extern __shared__ uint32_t lds[];
    constexpr int NW = NT / 64;
    constexpr int WPT = (int)SEG_SUPER_WORDS / NT; // words of the bitmap a thread sums for the prefix
    static_assert(WPT * NT == (int)SEG_SUPER_WORDS && WPT >= 1, "whole words per thread");
    const uint32_t cap = g.super_cap;
    uint32_t *sc = lds, *ix = lds + cap, *fr = lds + 2 * cap, *par = lds + 3 * cap; // rest-code, entry index, freq, forest
    uint32_t *bm = lds + 4 * cap, *pre = bm + SEG_SUPER_WORDS; // the bitmap, set bits before each word
    __shared__ uint32_t wsum[NW];
    const uint32_t tid = threadIdx.x, wave = tid >> 6;
    const int lane = (int)(tid & 63u);
    uint32_t *hitq = pre + SEG_SUPER_WORDS + wave * SUPER_HITQ; // this wave's hits (seg_super_lds_bytes)
    const SegRec32 *__restrict__ sub = (const SegRec32 *)g.sub_rec;
    unsigned int n_cand = 0, n_direct = 0;
    // one-way pairs: to this wave's private slot, wave-uniform fill level; a slot that is full sends the rest to
    // the list, one atomic per wave and batch
    const size_t my_slot = (size_t)blockIdx.x * NW + wave;
    uint32_t n_out = 0;
    uint2 *__restrict__ slot = g.priv_edges + my_slot * SEG_PRIV_CAP;
    auto emit = [&](bool has, uint32_t u, uint32_t v) {
        const unsigned long long bal = __ballot(has);
        if (!bal) return;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(bal);
        const uint32_t pos = n_out + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        unsigned long long base = 0;
        if (n_out + cnt > SEG_PRIV_CAP) {
            const uint32_t first_over = max(n_out, SEG_PRIV_CAP);
            const int leader = __builtin_ctzll(bal);
            if (lane == leader) base = atomicAdd(&a.counters[CNT_EDGES], (unsigned long long)(n_out + cnt - first_over));
            base = __shfl(base, leader);
            base -= first_over;
        }
        if (has) {
            if (pos < SEG_PRIV_CAP) slot[pos] = make_uint2(u, v);
            else if (base + pos < a.edge_cap) a.edges[base + pos] = make_uint2(u, v);
        }
        n_out += cnt;
    };
#ifdef UMIHIP_DEV
    // the time since the block's last stamp goes to phase i (thread 0: behind a barrier that is when the last wave
    // arrived; between the bit tests with their pushes and the drains, which no barrier parts, it is the first wave's own time)
    unsigned long long t_prev = g.super_stamps ? super_clock() : 0ull;
    auto stamp = [&](int i) {
        if (!g.super_stamps) return;
        const unsigned long long now = super_clock();
        if (tid == 0) g.super_stamps[(size_t)blockIdx.x * SEG_SUPER_PHASES + i] += now - t_prev;
        t_prev = now;
    };
#else
    auto stamp = [](int) {};
#endif
    // a pair within one substitution at positions pa, pb (the whole wave calls, `has` says which lanes hold one)
    auto decide = [&](bool has, uint32_t pa, uint32_t pb) {
        const uint32_t ia = ix[pa], ib = ix[pb];
        const int32_t fa = (int32_t)fr[pa], fb = (int32_t)fr[pb];
        // entry indices in rank order (src/algo/directional.rs:67-72)
        const bool sw = ib < ia;
        const uint32_t gi = sw ? ib : ia, gj = sw ? ia : ib;
        const int32_t fi = sw ? fb : fa, fj = sw ? fa : fb;
        if (has) n_cand++;
        // naive.rs:31 under directional.rs:38-39
        const bool fwd = has && (CLUSTER || fj <= threshold_of(percentage, fi));
        const bool bwd = has && (CLUSTER || fi <= threshold_of(percentage, fj));
        if (fwd && bwd) { // reachability inside such a set is symmetric: one set
            n_direct++;
            lds_union_halving(par, min(pa, pb), max(pa, pb));
        }
        emit(fwd != bwd, fwd ? gi : gj, fwd ? gj : gi);
    };
    auto rank_of = [&](uint32_t s) { // entries of the super-bin with a smaller rest-code = the position of s's
        return pre[s >> 5] + (uint32_t)__builtin_popcount(bm[s >> 5] & ((1u << (s & 31u)) - 1u));
    };
    // the wave's queue: the newest 64 hits decided, one per lane (fewer only in the drain that empties it);
    // walk (block-uniform): the partner is a position, not a rest-code
    uint32_t nq = 0; // (wave-uniform)
    auto drain = [&](bool walk) {
        const uint32_t n = min(nq, 64u);
        nq -= n;
        // (the wave's own stores, in program order on the LDS: the compiler must not move the loads above them)
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool has = (uint32_t)lane < n;
        const uint32_t h = has ? hitq[nq + (uint32_t)lane] : 0u;
        const uint32_t x = h >> 13;
        decide(has, h & 0x1FFFu, walk ? x : rank_of(x)); // (an idle lane: position 0 twice, nothing decided)
        __builtin_amdgcn_wave_barrier(); // (the queue is read before the next push writes it)
    };
    // one hit per lane and trip into the queue
    auto push = [&](bool has, uint32_t h, bool walk) {
        const unsigned long long bal = __ballot(has);
        if (has) hitq[nq + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = h;
        nq += (uint32_t)__builtin_popcountll(bal);
        if (nq >= SUPER_DRAIN_AT) {
            stamp(3);
            drain(walk);
            stamp(4);
        }
    };

    // Filed by super-bin (SegArgs::super_count_pairs): the pairs inside the run's fine bins, which the scan counted when
    // each was a bin of its own.  The fine bin of a record is the low 2g bits of its filter key.  A taken super-bin
    // reads the counts off the ranks (fine_pairs_ranked below); a run above the cap, which is only passed through
    // here, and a super-bin with a key twice are counted entry by entry.  fine[]: a counter per
    // fine bin, SUPER_FINE >> 2g copies of it next to each other (2g = 2, 4, 6, 8: 64, 16, 4, 1) -- a lane adds to the
    // copy of its number, so that a wave's adds spread over the banks -- then thread t of the first SUPER_FINE takes
    // word t, the copies of a bin are summed across 1..64 adjacent lanes, c (c - 1) / 2 each, one LDS add per wave.
    // The block's sum goes to the counter once, as the block's last access: a global atomic issued here would be
    // waited for at the next barrier (its fence), and all blocks' adds reach the one word together -- served at
    // ~90 per microsecond, that wait was 1.4 us per block with one add per super-bin and 4.3 us with one per wave.
    __shared__ uint32_t fine[SUPER_FINE];
    __shared__ unsigned long long fine_pairs; // (cleared here; first added to behind the barriers of the first super-bin)
    if (tid == 0) fine_pairs = 0ull;
    static_assert(SUPER_FINE == 256 && NT >= (int)SUPER_FINE, "at most 64 copies: inside a wave");
    auto fine_add = [&](uint32_t key, uint32_t lo_bits) {
        const uint32_t cb = 8u - lo_bits; // log2 of the copies
        atomicAdd(&fine[((key & ((1u << lo_bits) - 1u)) << cb) | ((uint32_t)lane & ((1u << cb) - 1u))], 1u);
    };
    auto fine_pairs_out = [&](uint32_t lo_bits) { // (behind a barrier that has the adds)
        if (tid >= SUPER_FINE) return; // (whole waves)
        const uint32_t cb = 8u - lo_bits;
        uint32_t n = fine[tid];
#pragma unroll
        for (uint32_t s = 0; s < 6; s++) {
            const uint32_t other = __shfl_xor(n, 1 << s);
            if (s < cb) n += other;
        }
        unsigned long long pairs = (tid & ((1u << cb) - 1u)) == 0u ? (unsigned long long)n * (n ? n - 1u : 0u) / 2ull : 0ull;
        for (int off = 32; off > 0; off >>= 1) pairs += __shfl_down(pairs, off);
        if (lane == 0 && pairs) atomicAdd(&fine_pairs, pairs);
    };
    // ... without a counter where no key stands twice: the fine bin is the top of the rest-code, so fine bin f holds
    // the entries ranked from rank_of(f << hi_bits) to the next bin's first rank (behind the barrier that has pre[])
    auto fine_pairs_ranked = [&](uint32_t lo_bits, uint32_t hi_bits, uint32_t c) {
        if (tid >= SUPER_FINE) return; // (whole waves)
        unsigned long long pairs = 0ull;
        if (tid < (1u << lo_bits)) {
            const uint32_t first = rank_of(tid << hi_bits);
            const uint32_t next = tid + 1u < (1u << lo_bits) ? rank_of((tid + 1u) << hi_bits) : c; // (4^rest: past the map)
            const uint32_t n = next - first;
            pairs = (unsigned long long)n * (n ? n - 1u : 0u) / 2ull;
        }
        for (int off = 32; off > 0; off >>= 1) pairs += __shfl_down(pairs, off);
        if (lane == 0 && pairs) atomicAdd(&fine_pairs, pairs);
    };

    for (uint32_t u = blockIdx.x; u < g.n_supers; u += gridDim.x) {
        const SegSuper su = g.supers[u];
        const uint32_t start = __builtin_amdgcn_readfirstlane(g.bin_start[su.bin0]);
        const uint32_t c = __builtin_amdgcn_readfirstlane(g.bin_start[su.bin0 + (1u << (2 * su.g))]) - start;
        const uint32_t lo_bits = 2u * su.g, hi_shift = 2u * su.nb, rest = su.rest;
        // cross segment: where this super-bin's map, prefix and ranks go (SegArgs::cross_map)
        uint32_t *__restrict__ x_map = nullptr;
        uint16_t *__restrict__ x_pre = nullptr;
        uint2 *__restrict__ x_rec = nullptr;
        if (su.cross) {
            const SegDesc *__restrict__ sd = g.segs + su.seg;
            x_map = g.cross_map + su.map0;
            x_pre = g.cross_pre + su.map0;
            x_rec = (uint2 *)((SegRec32 *)g.sub_rec + g.bin_start[sd->bin_off[1]]) + (start - g.bin_start[sd->bin_off[0]]);
        }
        if (su.cross && c < 2u) { // empty or a single entry: no pair inside, but its map has partners -- no phase chain for it
            uint32_t code = 0xFFFFFFFFu;
            if (c == 1u) {
                const SegRec32 rec = sub[start];
                const uint32_t hb = 2u * rest - lo_bits;
                code = ((rec.key >> hi_shift) & ((1u << hb) - 1u)) | ((rec.key & ((1u << lo_bits) - 1u)) << hb);
                if (tid == 0) {
                    x_pre[code >> 5] = 0;
                    x_rec[0] = make_uint2(rec.idx, (uint32_t)rec.freq);
                }
            }
            for (uint32_t w = tid; w < seg_cross_words(rest); w += NT) x_map[w] = w == (code >> 5) ? 1u << (code & 31u) : 0u;
            continue;
        }
        if (su.cross && c > cap && tid == 0) a.counters[CNT_SEG_CROSS_ABANDONED] = 1ull; // (a plain store: every block writes 1)
        if (!super_taken(g, c)) { // (block-uniform)
            if (g.super_count_pairs && c >= 2u) { // above the cap, the tiles' own: its keys once more, for that count alone
                for (uint32_t w = tid; w < SUPER_FINE; w += NT) fine[w] = 0u;
                __syncthreads();
                for (uint32_t p = tid; p < c; p += NT) fine_add(sub[start + p].key, lo_bits);
                __syncthreads();
                fine_pairs_out(lo_bits);
                __syncthreads(); // (the next super-bin clears the counters)
            }
            continue;
        }
        // the rest-code: the bases outside the bins in its low hi_bits, the fine bin above them (rest <= 8: 16 bits)
        const uint32_t hi_bits = 2u * rest - lo_bits;
        const uint32_t lo_mask = (1u << lo_bits) - 1u, hi_mask = (1u << hi_bits) - 1u;
        for (uint32_t w = tid; w < SEG_SUPER_WORDS; w += NT) bm[w] = 0u;
        if (g.super_count_pairs)
            for (uint32_t w = tid; w < SUPER_FINE; w += NT) fine[w] = 0u;
        uint32_t rc[SUPER_RPT], ri[SUPER_RPT], rf[SUPER_RPT], rq[SUPER_RPT];
#pragma unroll
        for (int r = 0; r < SUPER_RPT; r++) {
            const uint32_t p = tid + (uint32_t)r * NT;
            rc[r] = ri[r] = rf[r] = rq[r] = 0u;
            if (p < c) {
                const SegRec32 rec = sub[start + p];
                rc[r] = ((rec.key >> hi_shift) & hi_mask) | ((rec.key & lo_mask) << hi_bits);
                ri[r] = rec.idx;
                rf[r] = (uint32_t)rec.freq;
            }
        }
        __syncthreads();
        stamp(0);
        bool twice = false;
#pragma unroll
        for (int r = 0; r < SUPER_RPT; r++)
            if (tid + (uint32_t)r * NT < c) {
                const uint32_t bit = 1u << (rc[r] & 31u);
                twice = twice || (atomicOr(&bm[rc[r] >> 5], bit) & bit) != 0u;
            }
        const bool dup = __syncthreads_or(twice ? 1 : 0) != 0;
        stamp(1);
        if (dup && su.cross && tid == 0) a.counters[CNT_SEG_CROSS_ABANDONED] = 1ull; // (no rank per code here)
        if (dup && g.super_count_pairs) { // (the map holds fewer bits than there are entries: counted one by one)
#pragma unroll
            for (int r = 0; r < SUPER_RPT; r++)
                if (tid + (uint32_t)r * NT < c) fine_add(rc[r] >> hi_bits, lo_bits);
            __syncthreads();
            fine_pairs_out(lo_bits); // (fine[] is next written when the next super-bin clears it, barriers away)
            stamp(8);
        }
        if (!dup) {
            { // set bits before every word: a thread sums WPT words, the block scans the sums
                uint32_t n_w[WPT], mine = 0;
#pragma unroll
                for (int i = 0; i < WPT; i++) mine += n_w[i] = (uint32_t)__builtin_popcount(bm[tid * WPT + i]);
                uint32_t incl = mine;
                for (int d = 1; d < 64; d <<= 1) {
                    const uint32_t up = __shfl_up(incl, d);
                    if (lane >= d) incl += up;
                }
                if (lane == 63) wsum[wave] = incl;
                __syncthreads();
                uint32_t before = incl - mine;
                for (uint32_t w = 0; w < wave; w++) before += wsum[w];
#pragma unroll
                for (int i = 0; i < WPT; i++) {
                    pre[tid * WPT + i] = before;
                    before += n_w[i];
                }
            }
            __syncthreads();
            if (g.super_count_pairs) { // the fine bins' entries: the ranks of their first codes, one apart
                stamp(2);
                fine_pairs_ranked(lo_bits, hi_bits, c);
                stamp(8);
            }
#pragma unroll
            for (int r = 0; r < SUPER_RPT; r++)
                if (tid + (uint32_t)r * NT < c) {
                    const uint32_t q = rank_of(rc[r]);
                    rq[r] = q;
                    sc[q] = rc[r];
                    ix[q] = ri[r];
                    fr[q] = rf[r];
                    par[q] = q;
                }
            __syncthreads();
            stamp(2);
            if (su.cross) { // what seg_cross_kernel reads: plain coalesced stores, nothing waits for them
                for (uint32_t w = tid; w < seg_cross_words(rest); w += NT) {
                    x_map[w] = bm[w];
                    x_pre[w] = (uint16_t)pre[w];
                }
                for (uint32_t p = tid; p < c; p += NT) x_rec[p] = make_uint2(ix[p], fr[p]);
            }
#pragma unroll
            for (int r = 0; r < SUPER_RPT; r++) {
                if ((uint32_t)r * NT >= c) break; // (block-uniform)
                const uint32_t s = rc[r];
                // (the compiler puts each load under its test's condition, 24 LDS waits in a row; 17 words loaded by hand
                // ahead of the tests took 2 us off this phase and 15 more VGPRs, and the step did not show it: DESIGN.md 5a)
                uint32_t m = 0; // bit 3 b + d - 1: the entry with base b changed by d is there, behind this one
#pragma unroll
                for (int bb = 0; bb < SEG_SUPER_MAX_REST; bb++) {
#pragma unroll
                    for (int d = 1; d <= 3; d++) {
                        const uint32_t t = s ^ ((uint32_t)d << (2 * bb));
                        const uint32_t there = (bm[t >> 5] >> (t & 31u)) & 1u;
                        if ((uint32_t)bb < rest && t > s) m |= there << (3 * bb + d - 1);
                    }
                }
                if (tid + (uint32_t)r * NT >= c) m = 0u;
                while (__any(m != 0u)) { // one hit per lane and trip
                    const bool has = m != 0u;
                    uint32_t h = 0;
                    if (has) {
                        const int j = __builtin_ctz(m), bb = j / 3;
                        m &= m - 1u;
                        h = rq[r] | ((s ^ ((uint32_t)(j - 3 * bb + 1) << (2 * bb))) << 13);
                    }
                    push(has, h, false);
                }
            }
            stamp(3);
            if (nq) drain(false); // (what is left, fewer than 64: the queue is empty for the write-out and the next super-bin)
        } else {
#pragma unroll
            for (int r = 0; r < SUPER_RPT; r++) {
                const uint32_t p = tid + (uint32_t)r * NT;
                if (p < c) {
                    sc[p] = rc[r];
                    ix[p] = ri[r];
                    fr[p] = rf[r];
                    par[p] = p;
                }
            }
            __syncthreads();
            stamp(2);
            // every pair of positions p < q: a thread's own entries against the ones behind them, the wave in step
#pragma unroll
            for (int r = 0; r < SUPER_RPT; r++) {
                if ((uint32_t)r * NT >= c) break; // (block-uniform)
                const uint32_t p = tid + (uint32_t)r * NT, p_first = p - (uint32_t)lane;
                const uint32_t s = rc[r];
                const uint32_t n_it = c > p_first + 1u ? c - 1u - p_first : 0u; // (wave-uniform)
                for (uint32_t i = 1; i <= n_it; i++) {
                    const uint32_t q = p + i;
                    const uint32_t z = s ^ (q < c ? sc[q] : 0u);
                    const bool hit = p < c && q < c && __builtin_popcount((z | (z >> 1)) & 0x55555555u) <= 1;
                    if (__any(hit)) push(hit, p | (q << 13), true);
                }
            }
            stamp(3);
            if (nq) drain(true);
        }
        __syncthreads();
        stamp(4);
        // the sets out: root position of every entry (into sc[], free now), the smallest entry index of every
        // set (fr[] of its root), label[] of every entry
        // (the forest stands still now, and its chains can be hundreds of positions long: every position jumps to
        // its grandparent, all together, until none moves -- a handful of rounds instead of a climb per entry)
        for (;;) {
            bool moved = false;
            for (uint32_t p = tid; p < c; p += NT) {
                const uint32_t q = lds_ld(&par[p]), up = lds_ld(&par[q]);
                if (up != q) {
                    __hip_atomic_store(&par[p], up, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
                    moved = true;
                }
            }
            if (!__syncthreads_or(moved ? 1 : 0)) break;
        }
        stamp(5);
        for (uint32_t p = tid; p < c; p += NT) sc[p] = lds_ld(&par[p]);
        __syncthreads(); // (fr[] was read by the pairs until here)
        for (uint32_t p = tid; p < c; p += NT) fr[p] = 0xFFFFFFFFu;
        __syncthreads();
        for (uint32_t p = tid; p < c; p += NT) atomicMin(&fr[sc[p]], ix[p]);
        __syncthreads();
        stamp(6);
        for (uint32_t p = tid; p < c; p += NT) g.uf_parent[ix[p]] = fr[sc[p]];
        __syncthreads(); // (the next super-bin's records overwrite these arrays)
        stamp(7);
    }
    if (lane == 0) g.priv_cnt[my_slot] = min(n_out, SEG_PRIV_CAP);
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off);
    for (int off = 32; off > 0; off >>= 1) n_direct += __shfl_down(n_direct, off);
    if (lane == 0) g.priv_stat[my_slot] = make_uint2(n_cand, n_direct); // (the flatten launch adds them up)
    if (g.super_count_pairs) {
        __syncthreads(); // (a block without a super-bin of its own has met no barrier yet)
        if (tid == 0 && fine_pairs) atomicAdd(&a.counters[CNT_SEG_PAIRS], fine_pairs);
    }
}

// ---- cross segments: the pairs between super-bins (k = 1, no N in the call) -------------------------------
// A pair that seg_super_kernel does not see differs in one of the nb - g bases a super-bin shares, and in nothing
// else: the two entries have the same rest-code and lie in super-bins S and S' = S ^ (d << 2 b), d = 1..3, b one of
// those bases.  seg_super_kernel has left every super-bin's rest-code map, so these pairs are the set bits of
// map_S[w] & map_S'[w] -- a word AND where part 1 of the index would file every entry again and walk its bins' tiles.
// A pair is found once, from its smaller super-bin code.
// One wave per block, persistent.  Work items are computed: (super-bin, 64-word chunk of its map), SEG_CROSS_CHUNKS
// per super-bin whatever the map's length (the chunks past its end are skipped), a block takes a contiguous run of
// them -- mostly one super-bin's, whose hits share a queue.  Lane = word: the lane's own word, then the same word of
// every partner with the larger code, all loads issued before the first is looked at.  A hit is one queue word (word
// index, bit, partner number); 64 at a time they are decided as seg_super_kernel's are: both ranks from the prefix
// and the bits below, the two (entry index, freq) records, rank order, the freq predicate both ways; a symmetric pair
// is united through uf_parent, a one-way pair goes to the block's private slot.
constexpr uint32_t CROSS_DRAIN_AT = 64;
constexpr uint32_t CROSS_HITQ = CROSS_DRAIN_AT + 64;
constexpr int CROSS_MAX_PARTNERS = 3 * SEG_CROSS_MAX_SHARED;
static_assert(SEG_SUPER_WORDS <= (1u << 11) && CROSS_MAX_PARTNERS <= 32, "word index, bit and partner number in one queue word");

template <bool CLUSTER>
__global__ __launch_bounds__(64) void seg_cross_kernel(PairArgs a, SegArgs g, float percentage)
{
    __shared__ uint32_t hitq[CROSS_HITQ]; // word index | bit << 11 | partner number << 16
    const int lane = threadIdx.x;
    unsigned int n_cand = 0, n_direct = 0;
    uint32_t n_out = 0; // (wave-uniform)
    uint2 *__restrict__ slot = g.priv_edges + (size_t)blockIdx.x * SEG_PRIV_CAP;
    // one-way pairs: to this block's private slot; a slot that is full sends the rest to the list, one atomic per
    // wave and batch (seg_super_kernel's emit)
    auto emit = [&](bool has, uint32_t u, uint32_t v) {
        const unsigned long long bal = __ballot(has);
        if (!bal) return;
        const uint32_t cnt = (uint32_t)__builtin_popcountll(bal);
        const uint32_t pos = n_out + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull));
        unsigned long long base = 0;
        if (n_out + cnt > SEG_PRIV_CAP) {
            const uint32_t first_over = max(n_out, SEG_PRIV_CAP);
            const int leader = __builtin_ctzll(bal);
            if (lane == leader) base = atomicAdd(&a.counters[CNT_EDGES], (unsigned long long)(n_out + cnt - first_over));
            base = __shfl(base, leader);
            base -= first_over;
        }
        if (has) {
            if (pos < SEG_PRIV_CAP) slot[pos] = make_uint2(u, v);
            else if (base + pos < a.edge_cap) a.edges[base + pos] = make_uint2(u, v);
        }
        n_out += cnt;
    };
    // the super-bin in hand (wave-uniform): its code inside the segment, the segment's first map word, its map's words,
    // its own first map word, where the segment's ranks lie and how many, its first part-0 position and bin
    uint32_t have_u = 0xFFFFFFFFu, sb = 0, seg_map0 = 0, W = 0, my_map0 = 0, my_rec0 = 0, seg_entries = 1, seg_pos0 = 0, seg_bin0 = 0;
    uint32_t n_shared = 0, g2 = 0;
    const uint2 *__restrict__ seg_rec = nullptr;
    uint32_t nq = 0; // (wave-uniform)
    // the newest 64 hits of the queue, one per lane (fewer only in the drain that empties it)
    auto drain = [&]() {
        const uint32_t n = min(nq, 64u);
        nq -= n;
        __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
        __builtin_amdgcn_wave_barrier();
        const bool has = (uint32_t)lane < n;
        const uint32_t h = has ? hitq[nq + (uint32_t)lane] : 0u;
        const uint32_t w = h & 0x7FFu, bit = (h >> 11) & 31u, pn = h >> 16;
        const uint32_t b = pn / 3u, d = pn - 3u * b + 1u;
        const uint32_t sbp = has ? sb ^ (d << (2u * b)) : sb; // (an idle lane: this super-bin twice, nothing decided)
        const uint32_t wa_at = my_map0 + w, wb_at = seg_map0 + sbp * W + w;
        const uint32_t wa = g.cross_map[wa_at], wb = g.cross_map[wb_at];
        const uint32_t pa = g.cross_pre[wa_at], pb = g.cross_pre[wb_at];
        const uint32_t start_b = g.bin_start[seg_bin0 + (sbp << g2)];
        const uint32_t below = (1u << bit) - 1u;
        // (a rank is below its super-bin's count by construction; the clamp keeps a load inside the segment whatever it reads)
        const uint32_t ra = min(my_rec0 + pa + (uint32_t)__builtin_popcount(wa & below), seg_entries - 1u);
        const uint32_t rb = min(start_b - seg_pos0 + pb + (uint32_t)__builtin_popcount(wb & below), seg_entries - 1u);
        const uint2 ea = seg_rec[ra], eb = seg_rec[rb];
        const uint32_t ia = ea.x, ib = eb.x;
        const int32_t fa = (int32_t)ea.y, fb = (int32_t)eb.y;
        // entry indices in rank order (src/algo/directional.rs:67-72)
        const bool sw = ib < ia;
        const uint32_t gi = sw ? ib : ia, gj = sw ? ia : ib;
        const int32_t fi = sw ? fb : fa, fj = sw ? fa : fb;
        const bool ok = has && gi != gj && gj < a.n_entries;
        if (ok) n_cand++;
        // naive.rs:31 under directional.rs:38-39
        const bool fwd = ok && (CLUSTER || fj <= threshold_of(percentage, fi));
        const bool bwd = ok && (CLUSTER || fi <= threshold_of(percentage, fj));
        uint32_t uu[1] = {gi}, uv[1] = {gj};
        bool unite[1] = {fwd && bwd}; // reachability inside such a set is symmetric: one set
        if (unite[0]) n_direct++;
        uf_union_multi<1>(g.uf_parent, uu, uv, unite);
        emit(fwd != bwd, fwd ? gi : gj, fwd ? gj : gi);
        __builtin_amdgcn_wave_barrier(); // (the queue is read before the next push writes it)
    };

    // (a super-bin that could not be served has left no map: the host does this call's cross pairs again through part 1)
    const bool abandoned = a.counters[CNT_SEG_CROSS_ABANDONED] != 0ull;
    const uint32_t n_items = abandoned ? 0u : g.n_supers * SEG_CROSS_CHUNKS;
    const uint32_t per = (n_items + gridDim.x - 1u) / gridDim.x;
    const uint32_t it0 = min(n_items, blockIdx.x * per), it1 = min(n_items, it0 + per);
    for (uint32_t it = it0; it < it1; it++) {
        const uint32_t u = it / SEG_CROSS_CHUNKS, chunk = it % SEG_CROSS_CHUNKS;
        if (u != have_u) { // (wave-uniform)
            while (nq) drain(); // the queued hits belong to the super-bin in hand
            have_u = u;
            const SegSuper su = g.supers[u];
            W = 0u;
            if (su.cross) {
                const SegDesc *__restrict__ sd = g.segs + su.seg;
                g2 = 2u * su.g;
                n_shared = (uint32_t)su.nb - su.g;
                seg_bin0 = sd->bin_off[0];
                sb = (su.bin0 - seg_bin0) >> g2;
                W = seg_cross_words(su.rest);
                my_map0 = su.map0;
                seg_map0 = su.map0 - sb * W;
                seg_pos0 = g.bin_start[seg_bin0];
                my_rec0 = g.bin_start[su.bin0] - seg_pos0;
                seg_entries = max(1u, sd->end - sd->start);
                seg_rec = (const uint2 *)((const SegRec32 *)g.sub_rec + g.bin_start[sd->bin_off[1]]);
            }
        }
        const uint32_t w = chunk * 64u + (uint32_t)lane;
        if (chunk * 64u >= W) continue; // (past the map's end, or no cross segment's super-bin)
        const bool live = w < W;
        const uint32_t mine = live ? g.cross_map[my_map0 + w] : 0u;
        uint32_t m[CROSS_MAX_PARTNERS];
#pragma unroll
        for (int b = 0; b < SEG_CROSS_MAX_SHARED; b++) {
#pragma unroll
            for (int d = 1; d <= 3; d++) {
                const uint32_t sbp = sb ^ ((uint32_t)d << (2 * b));
                const bool there = (uint32_t)b < n_shared && sbp > sb; // (wave-uniform)
                m[3 * b + d - 1] = there && live ? g.cross_map[seg_map0 + sbp * W + w] : 0u;
            }
        }
        for (uint32_t pn = 0; pn < 3u * n_shared; pn++) { // (wave-uniform)
            uint32_t mp = 0;
#pragma unroll
            for (int q = 0; q < CROSS_MAX_PARTNERS; q++) mp = pn == (uint32_t)q ? m[q] : mp; // (no indexed registers)
            uint32_t x = mine & mp;
            while (__any(x != 0u)) { // one hit per lane and trip
                const bool has = x != 0u;
                const unsigned long long bal = __ballot(has);
                if (has) {
                    const uint32_t bit = (uint32_t)__builtin_ctz(x);
                    x &= x - 1u;
                    hitq[nq + (uint32_t)__builtin_popcountll(bal & ((1ull << lane) - 1ull))] = w | (bit << 11) | (pn << 16);
                }
                nq += (uint32_t)__builtin_popcountll(bal);
                if (nq >= CROSS_DRAIN_AT) drain();
            }
        }
    }
    while (nq) drain();
    if (lane == 0) g.priv_cnt[blockIdx.x] = min(n_out, SEG_PRIV_CAP);
    for (int off = 32; off > 0; off >>= 1) n_cand += __shfl_down(n_cand, off);
    for (int off = 32; off > 0; off >>= 1) n_direct += __shfl_down(n_direct, off);
    if (lane == 0) g.priv_stat[blockIdx.x] = make_uint2(n_cand, n_direct); // (the flatten launch adds them up)
}

// offsets of the blocks' slots behind what the list holds already (one block), the new total
__global__ __launch_bounds__(1024) void seg_edge_scan_kernel(uint32_t *priv_cnt, uint32_t n_blocks,
                                                             unsigned long long *counters)
{
    __shared__ uint32_t wsum[16];
    __shared__ uint32_t carry;
    if (threadIdx.x == 0) carry = 0;
    __syncthreads();
    const unsigned long long base = counters[CNT_EDGES];
    for (uint32_t b0 = 0; b0 < n_blocks; b0 += 1024) {
        const uint32_t i = b0 + threadIdx.x;
        const uint32_t v = i < n_blocks ? priv_cnt[i] : 0u;
        uint32_t incl = v;
        for (int d = 1; d < 64; d <<= 1) {
            const uint32_t up = __shfl_up(incl, d);
            if ((int)(threadIdx.x & 63) >= d) incl += up;
        }
        if ((threadIdx.x & 63) == 63) wsum[threadIdx.x >> 6] = incl;
        __syncthreads();
        uint32_t off = carry;
        for (uint32_t w = 0; w < (threadIdx.x >> 6); w++) off += wsum[w];
        if (i < n_blocks) priv_cnt[i] = (uint32_t)min(base + off + incl - v, 0xFFFFFFFFull);
        __syncthreads();
        if (threadIdx.x == 1023) carry = off + incl;
        __syncthreads();
    }
    if (threadIdx.x == 0) counters[CNT_EDGES] = base + carry;
}

__global__ __launch_bounds__(64) void seg_edge_move_kernel(SegArgs g, const uint32_t *__restrict__ priv_off,
                                                           uint32_t n_blocks, uint2 *__restrict__ edges,
                                                           uint8_t *__restrict__ edge_dist, uint32_t edge_cap,
                                                           const unsigned long long *counters)
{
    const uint32_t b = blockIdx.x;
    const unsigned long long first = priv_off[b];
    const unsigned long long next = b + 1 < n_blocks ? (unsigned long long)priv_off[b + 1] : counters[CNT_EDGES];
    const uint32_t cnt = (uint32_t)(next - first);
    for (uint32_t i = threadIdx.x; i < cnt; i += 64) {
        const unsigned long long pos = first + i;
        if (pos < edge_cap) {
            edges[pos] = g.priv_edges[(size_t)b * SEG_PRIV_CAP + i];
            if (edge_dist) edge_dist[pos] = g.priv_dist[(size_t)b * SEG_PRIV_CAP + i];
        }
    }
}

} // namespace

hipError_t launch_seg_build(const SegArgs &g, void *fkey, const int32_t *freq, bool key32,
                            unsigned long long *counters, hipStream_t s)
{
    if (g.n_chunks == 0 || g.n_ranges == 0) return hipSuccess;
    const size_t lds = (size_t)g.lds_bins * g.parts_per_pass * sizeof(uint32_t);
    if (g.blocks) { // the histogram (else prep_kernel has counted the entries, one atomic each)
        if (key32) seg_count_lds_kernel<uint32_t><<<g.n_blocks, SEG_BLOCK_THREADS, lds, s>>>(g, (uint32_t *)fkey);
        else seg_count_lds_kernel<uint64_t><<<g.n_blocks, SEG_BLOCK_THREADS, lds, s>>>(g, (uint64_t *)fkey);
    }
    seg_scan_kernel<<<g.n_chunks, SCAN_THREADS, 0, s>>>(g, counters);
    if (g.blocks) {
        if (key32) seg_scatter_lds_kernel<uint32_t><<<g.n_blocks, SEG_BLOCK_THREADS, lds, s>>>(g, (const uint32_t *)fkey, freq);
        else seg_scatter_lds_kernel<uint64_t><<<g.n_blocks, SEG_BLOCK_THREADS, lds, s>>>(g, (const uint64_t *)fkey, freq);
    } else {
        if (key32) seg_scatter_kernel<uint32_t><<<g.n_ranges, 256, 0, s>>>(g, (const uint32_t *)fkey, freq);
        else seg_scatter_kernel<uint64_t><<<g.n_ranges, 256, 0, s>>>(g, (const uint64_t *)fkey, freq);
    }
    return hipGetLastError();
}

// one-wave blocks of the pair kernel that fit a CU at once (the waves are persistent: a block that
// starts after the others have left finds its work done, or -- dealt statically -- does it alone)
int seg_pair_blocks_per_cu(bool key32, bool has_n, bool ckey)
{
    int nb = 0;
    hipError_t e;
    if (key32 && ckey)
        e = has_n ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint32_t, true, true>, 64, 0)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint32_t, false, true>, 64, 0);
    else if (key32)
        e = has_n ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint32_t, true, false>, 64, 0)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint32_t, false, false>, 64, 0);
    else
        e = has_n ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint64_t, true, false>, 64, 0)
                  : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_pair_kernel<uint64_t, false, false>, 64, 0);
    return e == hipSuccess && nb > 0 ? nb : 16;
}

hipError_t launch_seg_pairs(const PairArgs &a, const SegArgs &g, bool key32, float percentage,
                            uint32_t part, uint32_t n_parts, uint32_t n_blocks, hipStream_t s)
{
    if (g.n_chunks == 0 || n_blocks == 0) return hipSuccess;
    const bool has_n = a.nmask != nullptr;
    if (key32 && g.use_ckey) {
        if (has_n) seg_pair_kernel<uint32_t, true, true><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
        else seg_pair_kernel<uint32_t, false, true><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
    } else if (key32) {
        if (has_n) seg_pair_kernel<uint32_t, true, false><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
        else seg_pair_kernel<uint32_t, false, false><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
    } else if (g.key_words <= 1) {
        if (has_n) seg_pair_kernel<uint64_t, true, false><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
        else seg_pair_kernel<uint64_t, false, false><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);
    } else {
#define UMI_SEG_WIDE(WN)                                                                                           \
    do {                                                                                                           \
        if (has_n) seg_pair_kernel<uint64_t, true, false, WN><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);  \
        else seg_pair_kernel<uint64_t, false, false, WN><<<n_blocks, 64, 0, s>>>(a, g, percentage, part, n_parts);       \
    } while (0)
        switch (g.key_words) {
        case 2: UMI_SEG_WIDE(2); break;
        case 3: UMI_SEG_WIDE(3); break;
        case 4: UMI_SEG_WIDE(4); break;
        default: return hipErrorInvalidValue;
        }
#undef UMI_SEG_WIDE
    }
    return hipGetLastError();
}

// (the records, the forest, the hit queue, the bitmap and its prefix: 9,728 bytes at the default cap, 16
// blocks to a CU's 160 KB)
size_t seg_local_lds_bytes(uint32_t cap) { return ((size_t)4 * cap + LOCAL_HITQ + 2 * SEG_PROBE_WORDS) * sizeof(uint32_t); }

int seg_local_blocks_per_cu(bool has_n, uint32_t cap)
{
    int nb = 0;
    const size_t lds = seg_local_lds_bytes(cap);
    const hipError_t e = has_n ? hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_local_kernel<true>, 64, lds)
                               : hipOccupancyMaxActiveBlocksPerMultiprocessor(&nb, seg_local_kernel<false>, 64, lds);
    return e == hipSuccess && nb > 0 ? nb : 8;
}

hipError_t launch_seg_local(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s)
{
    if (g.n_chunks == 0 || n_blocks == 0 || g.local_cap == 0) return hipSuccess;
    if (g.local_cap > SEG_LOCAL_MAX_CAP || !g.uf_parent || !g.priv_stat || !g.use_ckey ||
        (a.mode != MODE_DIRECTIONAL && a.mode != MODE_CLUSTER))
        return hipErrorInvalidValue;
    const size_t lds = seg_local_lds_bytes(g.local_cap);
    if (a.mode == MODE_CLUSTER) {
        if (a.nmask) seg_local_kernel<true, true><<<n_blocks, 64, lds, s>>>(a, g, percentage);
        else seg_local_kernel<false, true><<<n_blocks, 64, lds, s>>>(a, g, percentage);
    } else if (a.nmask) seg_local_kernel<true><<<n_blocks, 64, lds, s>>>(a, g, percentage);
    else seg_local_kernel<false><<<n_blocks, 64, lds, s>>>(a, g, percentage);
    return hipGetLastError();
}

// (the records and the forest, 16 bytes per entry; the bitmap and its prefix, 16 KB; a hit queue of SUPER_HITQ words per
// wave, 8 KB for 1,024 threads and 2 KB for 256 -- the kernel lays them out in this order.  1,024 threads: 114,688 bytes
// at the default cap, 155,648 at SEG_SUPER_MAX_CAP; 256 threads: 51,200 at SEG_SUPER_SMALL.  One block to a CU's 160 KB.)
size_t seg_super_lds_bytes(uint32_t cap)
{
    const uint32_t n_waves = seg_super_threads(cap) / 64u;
    return ((size_t)4 * cap + 2 * SEG_SUPER_WORDS + (size_t)n_waves * SUPER_HITQ) * sizeof(uint32_t);
}
static_assert(((size_t)4 * SEG_SUPER_MAX_CAP + 2 * SEG_SUPER_WORDS + 16 * SUPER_HITQ + SUPER_FINE) * sizeof(uint32_t) + 64 <= 160 * 1024,
              "the largest block, its wave sums and its fine-bin counters fit a CU's LDS");

// its persistent grid: one block per CU at most, no more than there are super-bins
uint32_t seg_super_blocks(uint32_t n_supers, uint32_t n_cus) { return n_supers < n_cus ? n_supers : n_cus; }

template <bool CLUSTER, int NT>
static hipError_t launch_seg_super_as(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, size_t lds,
                                      hipStream_t s)
{
    // (beyond 64 KB of dynamic LDS a kernel has to be told so)
    const hipError_t e = hipFuncSetAttribute((const void *)seg_super_kernel<CLUSTER, NT>,
                                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    if (e != hipSuccess) return e;
    seg_super_kernel<CLUSTER, NT><<<n_blocks, NT, lds, s>>>(a, g, percentage);
    return hipGetLastError();
}

hipError_t launch_seg_super(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s)
{
    if (g.n_supers == 0 || n_blocks == 0 || g.super_cap == 0) return hipSuccess;
    if (g.super_cap > SEG_SUPER_MAX_CAP || !g.supers || !g.uf_parent || !g.priv_stat || a.nmask || a.k != 1 ||
        (a.mode != MODE_DIRECTIONAL && a.mode != MODE_CLUSTER))
        return hipErrorInvalidValue;
    const size_t lds = seg_super_lds_bytes(g.super_cap);
    static_assert(SEG_SUPER_SMALL <= 256 * SUPER_RPT && SEG_SUPER_MAX_CAP <= 1024 * SUPER_RPT, "a block holds the cap in registers");
    const bool small = seg_super_threads(g.super_cap) == 256u;
    if (a.mode == MODE_CLUSTER)
        return small ? launch_seg_super_as<true, 256>(a, g, percentage, n_blocks, lds, s)
                     : launch_seg_super_as<true, 1024>(a, g, percentage, n_blocks, lds, s);
    return small ? launch_seg_super_as<false, 256>(a, g, percentage, n_blocks, lds, s)
                 : launch_seg_super_as<false, 1024>(a, g, percentage, n_blocks, lds, s);
}

hipError_t launch_seg_cross(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s)
{
    if (g.n_supers == 0 || n_blocks == 0) return hipSuccess;
    if (!g.supers || !g.cross_map || !g.cross_pre || !g.uf_parent || !g.priv_stat || a.nmask || a.k != 1 || g.n_parts != 2 ||
        g.n_supers > 0xFFFFFFFFu / SEG_CROSS_CHUNKS || (a.mode != MODE_DIRECTIONAL && a.mode != MODE_CLUSTER))
        return hipErrorInvalidValue;
    if (a.mode == MODE_CLUSTER) seg_cross_kernel<true><<<n_blocks, 64, 0, s>>>(a, g, percentage);
    else seg_cross_kernel<false><<<n_blocks, 64, 0, s>>>(a, g, percentage);
    return hipGetLastError();
}

// what the pair kernel's blocks still held in their stages when they ended: from their private
// slots to the list
hipError_t launch_seg_edge_append(const PairArgs &a, const SegArgs &g, uint32_t n_blocks, hipStream_t s)
{
    if (g.n_chunks == 0 || n_blocks == 0) return hipSuccess;
    seg_edge_scan_kernel<<<1, 1024, 0, s>>>(g.priv_cnt, n_blocks, a.counters);
    seg_edge_move_kernel<<<n_blocks, 64, 0, s>>>(g, g.priv_cnt, n_blocks, a.edges,
                                                 a.mode == MODE_NEIGHBOURS ? a.edge_dist : nullptr, a.edge_cap,
                                                 a.counters);
    return hipGetLastError();
}

} // namespace umihip
