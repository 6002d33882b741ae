// Directional collapse, phase 1 by union-find (gfx950).
//
// What it replaces in the reference (tkob-vh/umi-collapse-rs): Directional::visit_and_remove and
// the root loop of Directional::apply (src/algo/directional.rs:30-54,78-88), as in
// umihip_kernels.hip: label[v] = smallest rank that reaches v.  Reachability inside a set of
// entries joined by symmetric pairs (both directions permitted) is symmetric, so those sets are
// plain connected components; this file finds them with a lock-free union-find over the edge list
// (one pass, any number of hops) where the hook/jump rounds of cc_hook_kernel need one launch per
// halving of the longest chain.  The one-way pairs (a DAG over the sets) are then propagated by
// dag_hook_kernel as before.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"
#include "umihip_device.h"

namespace umihip {

namespace {

__global__ __launch_bounds__(256) void uf_union_kernel(const uint2 *__restrict__ edges,
                                                       const unsigned long long *counters,
                                                       uint32_t edge_cap, uint32_t *parent)
{
    const unsigned long long ne = counters[CNT_EDGES];
    const uint32_t E = ne < edge_cap ? (uint32_t)ne : edge_cap;
    for (uint32_t e = blockIdx.x * blockDim.x + threadIdx.x; e < E; e += gridDim.x * blockDim.x) {
        const uint2 uv = edges[e];
        if (uv.x & SYM_FLAG) uf_union(parent, uv.x & ~SYM_FLAG, uv.y);
    }
}

// ---- the batched directional collapse behind the pair kernels ------------------------------------
// Inputs: parent[] (= label[]) holds the union-find forest of the symmetric pairs; the one-way pairs
// sit in the edge list.  (Reading the last staged edges of the segment index's pair kernel where its
// blocks leave them, 4,096 private slots, instead of moving them to the list first saved two small
// launches and cost the first round 47 us instead of 13: a slot per wave means 2,000 waves, and every
// one of them sends its own atomic for the giant component's word.)
//
// kept_only (the caller wants the mask and no root[]): the flatten is only there for root[].  lab[c] <= c
// (identity, then atomicMin) and comp[i] <= i (parents are smaller than children), so an entry that
// is not the root of its set has lab[comp[i]] <= comp[i] < i and is not kept whatever its root is,
// and a root is kept iff lab[i] == i: kept[i] = parent[i] == i && lab[i] == i, two streams over the
// forest as the unions left it.  Only the endpoints of the one-way pairs need their roots: round 0
// finds them by climbing (read only: no union runs behind the pair kernels in stream order) and
// writes each pair to its place in the list as (root of u, root of v); the rounds after it, the check and
// the host's continuation read lab[] at the stored endpoints.  Round 0 is the launch that gathers the
// private slots (gather_resolve_hook_kernel): a slot's pair is resolved and hooked by the thread that
// finds its place, not copied to the list by one launch and read back by the next.  lab[] is the identity
// when it starts: the entry kernels store it beside label[] (prep_kernel, seg_count_lds_kernel).
struct CollapseArgs {
    uint32_t *parent;       // in: the forest; out: comp[v] = root of v's set (flat; kept_only: left as it is)
    uint32_t *lab;          // lab[c] = smallest set that reaches set c along one-way pairs
    const uint2 *edges;     // the list (one-way pairs and, flagged, symmetric ones: skipped here);
                            // kept_only: round 0 stores the one-way pairs as (root, root)
    uint32_t edge_cap;
    const RangeTask *ranges; // the entries the collapse covers (the fused kernel finished the others); null: all n
    uint32_t n_ranges, n;
    uint8_t *kept;
    uint32_t *root;          // may be null
    bool kept_only;          // only kept[] is asked for (root is null): the forest is never flattened, see above
    unsigned long long *counters;
    uint32_t *changed;       // [MAX_ROUNDS_PER_SYNC] round r moved a label
    const uint2 *priv_edges; // the pair kernel's private slots (may be null), priv_blocks of SEG_PRIV_CAP edges
    const uint32_t *priv_cnt;
    const uint2 *priv_stat;  // (candidates, united pairs) of each slot's block, to the counters here (may be null)
    uint32_t priv_blocks;
};

// the length of the list: what the pair kernels appended themselves and what the flatten launch moved behind it
__device__ __forceinline__ uint32_t list_length(const CollapseArgs &a)
{
    const unsigned long long ne = a.counters[CNT_EDGES] + a.counters[CNT_EDGES_MOVED];
    return ne < a.edge_cap ? (uint32_t)ne : a.edge_cap;
}

// f(i) for the entries of ranges (null: all n), by the first n_blocks blocks of the grid
template <class F> __device__ __forceinline__ void collapse_entries(const CollapseArgs &a, uint32_t n_blocks, F f)
{
    if (a.ranges) {
        for (uint32_t r = blockIdx.x; r < a.n_ranges; r += n_blocks) {
            const RangeTask rt = a.ranges[r];
            for (uint32_t i = rt.start + threadIdx.x; i < rt.end; i += blockDim.x) f(i);
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += n_blocks * blockDim.x) f(i);
    }
}

// comp[v] = root of v (the smallest index of its set); lab[v] = v
__device__ __forceinline__ void flatten_entry(uint32_t *parent, uint32_t *lab, uint32_t v)
{
    uint32_t r = ld_parent(&parent[v]);
    if (r != v) {
        for (;;) {
            const uint32_t p = ld_parent(&parent[r]);
            if (p == r) break;
            r = p;
        }
        st_parent(&parent[v], r);
    }
    if (lab) lab[v] = v;
}

// One round along the one-way pairs over the flattened sets: lab[set of v] = min(.., lab[set of u])
// for every pair u -> v of the list (directional.rs:38-39: v falls to whatever
// removes u).  No pointer jump over lab[] behind it: a chain of one-way pairs is as deep as the freq
// ladder it descends -- two or three steps in sequencing data, where a pass over all of lab[] per
// round costs more than the round it might save; nothing bounds it (at p = 1.0 a ladder 2n, 2n - 2,
// ..., 2 is n - 1 one-way pairs in a row), and a deeper chain only takes more rounds: ladders of up
// to 768 pairs are in tests/test_gpu_deep_chains.py.  Only as many blocks walk the list as it needs
// (the count is on the device): the fewer waves, the more of a hot word's hooks meet in one wave's
// registers.
//
// The hook of one pair between the sets cu -> cv (live: this lane has a pair).  Returns whether the lane
// saw a label to move.  Every lane of a wave calls it together, and makes the same trips.
__device__ __forceinline__ bool hook_pair(const CollapseArgs &a, uint32_t cu, uint32_t cv, bool live, HotMin &hot)
{
    uint32_t lu = 0;
    bool todo = false;
    if (live) {
        lu = a.lab[cu];
        todo = lu < a.lab[cv];
    }
    wave_atomic_min(a.lab, cv, lu, todo, hot);
    return todo;
}

// PER_THREAD: the trips a thread makes when the list is at least as long as the grid covers; each is a
// chain of dependent loads.
template <uint32_t PER_THREAD> __device__ __forceinline__ bool one_way_round(const CollapseArgs &a)
{
    const uint32_t E = list_length(a);
    constexpr uint32_t PER_BLOCK = 256 * PER_THREAD;
    const uint32_t active = min(gridDim.x, (E + PER_BLOCK - 1) / PER_BLOCK);
    bool any = false;
    HotMin hot;
    if (blockIdx.x < active)
        for (uint32_t e0 = blockIdx.x * blockDim.x; e0 < E; e0 += active * blockDim.x) {
            const uint32_t e = e0 + threadIdx.x;
            const uint2 uv = e < E ? a.edges[e] : make_uint2(SYM_FLAG, 0u);
            const bool live = !(uv.x & SYM_FLAG);
            // kept_only: the list holds roots (resolve_hook_pair)
            const uint32_t cu = !live ? 0u : a.kept_only ? uv.x : a.parent[uv.x];
            const uint32_t cv = !live ? 0u : a.kept_only ? uv.y : a.parent[uv.y];
            any |= hook_pair(a, cu, cv, live, hot);
        }
    hot_flush(a.lab, hot);
    return any;
}

// kept_only's round 0, pair by pair: the endpoints of uv are climbed to their roots in the unflattened
// forest -- both climbs in one loop, two loads in flight per step; plain loads: the forest does not
// change any more -- the pair goes to slot pos of the list as (cu, cv) with one 8-byte store, and the
// roots are hooked.  A flagged uv (a symmetric pair of the list, or a lane without a pair) is left alone.
// A pair that is resolved a second time stays what it is (a root is its own root).
__device__ __forceinline__ bool resolve_hook_pair(const CollapseArgs &a, uint32_t pos, uint2 uv, HotMin &hot)
{
    const bool live = !(uv.x & SYM_FLAG);
    uint32_t cu = uv.x, cv = uv.y;
    if (live) {
        uint32_t pu = a.parent[cu], pv = a.parent[cv];
        while (pu != cu || pv != cv) {
            if (pu != cu) {
                cu = pu;
                pu = a.parent[cu];
            }
            if (pv != cv) {
                cv = pv;
                pv = a.parent[cv];
            }
        }
        const_cast<uint2 *>(a.edges)[pos] = make_uint2(cu, cv);
    }
    return hook_pair(a, cu, cv, live, hot);
}

// The same walk without a store: would a round still move a label?  (Rides in the finalize launch as
// blocks of its own, first_block .. gridDim.x - 1: lab[] is only read there, by both.)
__device__ __forceinline__ bool one_way_check(const CollapseArgs &a, uint32_t first_block)
{
    const uint32_t E = list_length(a);
    const uint32_t n_blocks = gridDim.x - first_block, me = blockIdx.x - first_block;
    bool any = false;
    for (uint32_t e = me * blockDim.x + threadIdx.x; e < E; e += n_blocks * blockDim.x) {
        const uint2 uv = a.edges[e];
        if (uv.x & SYM_FLAG) continue;
        any |= a.kept_only ? a.lab[uv.x] < a.lab[uv.y] // (resolved: round 0 always runs ahead of the check)
                           : a.lab[a.parent[uv.x]] < a.lab[a.parent[uv.y]];
    }
    return any;
}

__device__ __forceinline__ unsigned int finalize_entry(const CollapseArgs &a, uint32_t i)
{
    if (a.kept_only) { // no gather: an entry below its root is not kept, a root is if nothing reaches it
        const bool kp = a.parent[i] == i && a.lab[i] == i;
        a.kept[i] = kp ? 1 : 0;
        return kp ? 1u : 0u;
    }
    const uint32_t l = a.lab[a.parent[i]]; // label[v] = lab[comp[v]] (directional.rs:30-54,78-88)
    const bool kp = l == i;                // (deduplicate_sam.rs:217-231)
    a.kept[i] = kp ? 1 : 0;
    if (a.root) a.root[i] = l;
    return kp ? 1u : 0u;
}

// The phases are separate launches: flatten | a round per launch, each a no-op once the one before it
// was quiet | kept, root, survivor count.  One launch for all of them with grid-wide barriers in
// between was built and measured: 0.21 ms against 0.065 for the five launches -- a barrier that
// 1,536 blocks pass costs ~10 us however it is built (one counter: the word is served at ~90
// accesses per microsecond; grouped arrivals and a flag line per block: the slowest block's phase
// plus two trips to the memory side), a release / acquire fence per wave writes back and invalidates
// its XCD's L2 every time (0.37 ms with 512 blocks, 0.90 with 1,536), and without fences every load
// of parent[] and lab[] has to go past the L2 -- while launches the host has enqueued ahead follow
// each other without a gap on this chip.
__global__ __launch_bounds__(256) void dag_flat_hook_kernel(CollapseArgs a, int round)
{
    if (round > 0 && a.changed[round - 1] == 0) return;
    if (one_way_round<8>(a)) a.changed[round] = 1;
}

// The private slots to the list, GATHER_SLOTS slots per group (blocks behind the flatten pass's own, in
// the same launch: was a scan kernel and a move kernel, 11 us).  A block scans its group's counts, adds up
// the counts of the slots before the group itself (at most 4,096 words), and gives every edge of its
// slots a position behind what the list holds; the last group says how many there were in all.  Nobody
// writes CNT_EDGES meanwhile.  RESOLVE (kept_only): the edge does not go to its position as it is -- the
// thread that would copy it resolves and hooks it there (resolve_hook_pair: the launch is round 0), and
// sets changed[0] if a label moved.  An edge whose position lies at or beyond edge_cap is neither stored
// nor hooked (the host sees the count and runs the call again).  The slots hold one-way pairs only.
// n_sub blocks share a group, block `sub` taking every n_sub-th chunk of GATHER_CHUNK edges: a position of
// uniform UMIs leaves a few hundred pairs per group, one chunk, and a block without a chunk ends behind
// the scan of 64 counts; a clustered position leaves some thousand, and one block per group walked them
// in four and more trips of dependent loads per thread (config 2m took 0.156 ms that way, 0.145 before).
constexpr uint32_t GATHER_SLOTS = 64; // (a multiple of 64: GATHER_SLOTS / 64 slots per lane of the scan)
constexpr uint32_t GATHER_CHUNK = 256 * 2; // two pairs per thread, as the list blocks' RESOLVE_PER_THREAD
constexpr uint32_t GATHER_SPLIT = 8;       // blocks per group of the resolving launch
template <bool RESOLVE>
__device__ __forceinline__ void gather_private_edges(const CollapseArgs &a, uint32_t group, uint32_t sub, uint32_t n_sub)
{
    constexpr uint32_t PER_LANE = GATHER_SLOTS / 64;
    static_assert(GATHER_SLOTS % 64 == 0, "the scan deals whole slots to the first wave's lanes");
    __shared__ unsigned long long wsum[4];
    __shared__ uint32_t pre[GATHER_SLOTS + 1];
    const uint32_t s0 = group * GATHER_SLOTS, s1 = min(a.priv_blocks, s0 + GATHER_SLOTS);
    if (threadIdx.x < 64) { // the group's own counts, exclusive: PER_LANE consecutive slots per lane
        uint32_t c[PER_LANE], sum = 0;
        unsigned long long cand = 0, direct = 0;
#pragma unroll
        for (uint32_t q = 0; q < PER_LANE; q++) {
            const uint32_t sl = s0 + threadIdx.x * PER_LANE + q;
            c[q] = sl < s1 ? min(a.priv_cnt[sl], SEG_PRIV_CAP) : 0u;
            sum += c[q];
            if (a.priv_stat && sub == 0 && sl < s1) {
                const uint2 st = a.priv_stat[sl];
                cand += st.x;
                direct += st.y;
            }
        }
        uint32_t incl = sum;
        for (int o = 1; o < 64; o <<= 1) {
            const uint32_t up = __shfl_up(incl, o);
            if ((int)threadIdx.x >= o) incl += up;
        }
        uint32_t run = incl - sum;
#pragma unroll
        for (uint32_t q = 0; q < PER_LANE; q++) {
            pre[threadIdx.x * PER_LANE + q] = run;
            run += c[q];
        }
        if (threadIdx.x == 63) pre[GATHER_SLOTS] = incl;
        if (a.priv_stat && sub == 0) { // the blocks' counts: two atomics per group instead of two per block
            for (int o = 32; o > 0; o >>= 1) {
                cand += __shfl_down(cand, o);
                direct += __shfl_down(direct, o);
            }
            if (threadIdx.x == 0 && cand) atomicAdd(&a.counters[CNT_CANDIDATES], cand);
            if (threadIdx.x == 0 && direct) atomicAdd(&a.counters[CNT_UF_DIRECT], direct);
        }
    }
    __syncthreads();
    const uint32_t total = pre[GATHER_SLOTS];
    if (sub != 0 && sub * GATHER_CHUNK >= total) return; // (the whole block: no chunk of this group is its)
    unsigned long long before = 0;
    for (uint32_t i = threadIdx.x; i < s0; i += blockDim.x) before += a.priv_cnt[i];
    for (int o = 32; o > 0; o >>= 1) before += __shfl_down(before, o);
    if ((threadIdx.x & 63) == 0) wsum[threadIdx.x >> 6] = before;
    __syncthreads();
    const unsigned long long first = a.counters[CNT_EDGES] + wsum[0] + wsum[1] + wsum[2] + wsum[3];
    uint2 *list = const_cast<uint2 *>(a.edges);
    bool any = false;
    HotMin hot;
    // a thread per edge of the group, its slot by bisection of pre[]: a slot holds a handful of edges, and a
    // wave that walks its sixteen slots one after the other makes sixteen dependent trips to memory (with
    // the flatten's entry part gone from the launch, kept_only, it took 21 us that way and takes 16 so).
    // Whole blocks of threads make each trip (the hook is a wave's business), a lane past the end without a pair
    for (uint32_t c0 = sub * GATHER_CHUNK; c0 < total; c0 += n_sub * GATHER_CHUNK)
        for (uint32_t t0 = c0; t0 < min(total, c0 + GATHER_CHUNK); t0 += blockDim.x) {
            const uint32_t t = t0 + threadIdx.x;
            const unsigned long long pos = first + t;
            uint2 uv = make_uint2(SYM_FLAG, 0u);
            if (t < total && pos < a.edge_cap) {
                uint32_t lo = 0, hi = GATHER_SLOTS; // pre[lo] <= t < pre[hi]
                while (hi - lo > 1) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (pre[mid] <= t) lo = mid;
                    else hi = mid;
                }
                uv = a.priv_edges[(size_t)(s0 + lo) * SEG_PRIV_CAP + (t - pre[lo])];
                if (!RESOLVE) list[pos] = uv;
            }
            if (RESOLVE) any |= resolve_hook_pair(a, (uint32_t)pos, uv, hot);
        }
    if (RESOLVE) {
        hot_flush(a.lab, hot);
        if (any) a.changed[0] = 1;
    }
    if (s1 == a.priv_blocks && sub == 0 && threadIdx.x == 0) a.counters[CNT_EDGES_MOVED] = first + total - a.counters[CNT_EDGES];
}

// kept_only's round 0, one launch behind the unions: lab[] is the identity already (the entry kernels wrote
// it beside label[]), parent[] is only read.  The first gather_blocks blocks take the private slots'
// pairs (above: block b is block b / groups of group b % groups, so the blocks with the groups' first
// chunks start first); the blocks behind them take what the pair kernels appended to the list themselves --
// CNT_EDGES of them, not list_length(): CNT_EDGES_MOVED is written during this launch -- resolve them in
// place and hook them, flagged entries skipped, only as many blocks active as that length needs
// (RESOLVE_PER_THREAD pairs per thread: the climbs make a trip's chain of loads long, so the list is
// spread over more waves than in the rounds that follow).  The rounds, the check and the
// host's continuation behind this launch read lab[] at the stored roots.
constexpr uint32_t RESOLVE_PER_THREAD = 2;
__global__ __launch_bounds__(256) void gather_resolve_hook_kernel(CollapseArgs a, uint32_t gather_blocks)
{
    if (blockIdx.x < gather_blocks) {
        const uint32_t groups = gather_blocks / GATHER_SPLIT;
        gather_private_edges<true>(a, blockIdx.x % groups, blockIdx.x / groups, GATHER_SPLIT);
        return;
    }
    const unsigned long long ne = a.counters[CNT_EDGES];
    const uint32_t E = ne < a.edge_cap ? (uint32_t)ne : a.edge_cap;
    constexpr uint32_t PER_BLOCK = 256 * RESOLVE_PER_THREAD;
    const uint32_t me = blockIdx.x - gather_blocks, active = min(gridDim.x - gather_blocks, (E + PER_BLOCK - 1) / PER_BLOCK);
    if (me >= active) return;
    bool any = false;
    HotMin hot;
    for (uint32_t e0 = me * blockDim.x; e0 < E; e0 += active * blockDim.x) {
        const uint32_t e = e0 + threadIdx.x;
        any |= resolve_hook_pair(a, e, e < E ? a.edges[e] : make_uint2(SYM_FLAG, 0u), hot);
    }
    hot_flush(a.lab, hot);
    if (any) a.changed[0] = 1;
}

// the with-root path: comp[] flat and lab[] = identity by the entry blocks, the private slots moved to the
// list by the blocks behind them
__global__ __launch_bounds__(256) void uf_flatten_kernel(CollapseArgs a, uint32_t entry_blocks)
{
    if (blockIdx.x >= entry_blocks) {
        gather_private_edges<false>(a, blockIdx.x - entry_blocks, 0, 1);
        return;
    }
    if (a.ranges) {
        for (uint32_t r = blockIdx.x; r < a.n_ranges; r += entry_blocks) {
            const RangeTask rt = a.ranges[r];
            for (uint32_t i = rt.start + threadIdx.x; i < rt.end; i += blockDim.x) flatten_entry(a.parent, a.lab, i);
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += entry_blocks * blockDim.x)
            flatten_entry(a.parent, a.lab, i);
    }
}

// kept / root / survivor count of the entries of ranges (null: all n) from comp and lab, by the first
// entry_blocks blocks; the blocks behind them (check_round >= 0) look whether round check_round would
// still move a label -- the last of the rounds enqueued ahead of the host's look changes nothing in
// the common case and is there only to say so: as a check beside the finalize pass it costs no launch
// of its own (the result stands if changed[check_round] stays 0; else the host runs on and finalizes again)
__global__ __launch_bounds__(256) void map_finalize_kernel(CollapseArgs a, uint32_t entry_blocks, int check_round)
{
    if (blockIdx.x >= entry_blocks) {
        if (check_round > 0 && a.changed[check_round - 1] == 0) return; // (the round before was quiet already)
        if (one_way_check(a, entry_blocks)) a.changed[check_round] = 1;
        return;
    }
    unsigned int cnt = 0;
    if (a.kept_only && !a.ranges) {
        // two streams in, one out: a quarter of the other path's blocks (one add to CNT_KEPT each), a thread's
        // four entries loaded before the first byte is stored (kept[] may alias anything for the compiler).
        // Measured at config 2: 11.6 us, where the entry-by-entry loop over 2,048 blocks took 11.4 and the
        // path with the gather 12.2 -- neither the gather nor the adds are what this pass waits for
        const uint32_t stride = entry_blocks * blockDim.x;
        for (uint32_t i0 = blockIdx.x * blockDim.x + threadIdx.x; i0 < a.n; i0 += 4 * stride) {
            uint32_t p[4], l[4];
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t i = i0 + u * stride;
                p[u] = i < a.n ? a.parent[i] : 0xFFFFFFFFu;
                l[u] = i < a.n ? a.lab[i] : 0xFFFFFFFFu;
            }
#pragma unroll
            for (uint32_t u = 0; u < 4; u++) {
                const uint32_t i = i0 + u * stride;
                if (i < a.n) {
                    const bool kp = p[u] == i && l[u] == i;
                    a.kept[i] = kp ? 1 : 0;
                    cnt += kp ? 1u : 0u;
                }
            }
        }
    } else if (a.ranges) {
        for (uint32_t r = blockIdx.x; r < a.n_ranges; r += entry_blocks) {
            const RangeTask rt = a.ranges[r];
            for (uint32_t i = rt.start + threadIdx.x; i < rt.end; i += blockDim.x) cnt += finalize_entry(a, i);
        }
    } else {
        for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += entry_blocks * blockDim.x) cnt += finalize_entry(a, i);
    }
    block_count_add(cnt, &a.counters[CNT_KEPT]);
}

// kept[] (one byte per entry) as one bit per entry, little-endian inside a byte: a wave packs 64
// entries with one ballot (the multi-GPU gather moves n / 8 bytes instead of n)
__global__ __launch_bounds__(256) void pack_mask_kernel(const uint8_t *__restrict__ kept, uint64_t n,
                                                        uint8_t *__restrict__ bits)
{
    const uint64_t n_round = (n + 63) & ~63ull; // (whole waves: the ballot needs every lane)
    for (uint64_t i = (uint64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n_round; i += (uint64_t)gridDim.x * blockDim.x) {
        const unsigned long long bal = __ballot(i < n && kept[i] != 0);
        const uint32_t lane = threadIdx.x & 63;
        if (lane < 8 && (i - lane) + 8ull * lane < n) bits[((i - lane) >> 3) + lane] = (uint8_t)(bal >> (8 * lane));
    }
}

inline uint32_t grid_of(uint64_t work, int block, uint32_t cap)
{
    uint64_t g = (work + block - 1) / block;
    if (g < 1) g = 1;
    if (g > cap) g = cap;
    return (uint32_t)g;
}

CollapseArgs collapse_args(const CollapseDesc &d)
{
    CollapseArgs a;
    a.parent = d.parent;
    a.lab = d.lab;
    a.edges = d.edges;
    a.edge_cap = d.edge_cap;
    a.ranges = d.ranges;
    a.n_ranges = d.n_ranges;
    a.n = d.n;
    a.kept = d.kept;
    a.root = d.root;
    a.kept_only = d.kept_only;
    a.counters = d.counters;
    a.changed = d.changed;
    a.priv_edges = d.priv_edges;
    a.priv_cnt = d.priv_cnt;
    a.priv_stat = d.priv_stat;
    a.priv_blocks = d.priv_blocks;
    return a;
}

uint32_t entries_grid(const CollapseDesc &d, uint32_t cap)
{
    return d.ranges ? std::max(1u, std::min(d.n_ranges, cap)) : grid_of(d.n, 256, cap);
}

} // namespace

// the control block to the host's pinned mirror by a wave's own stores (a DMA copy of 256 bytes
// starts ~20 us after the kernel before it ends; a launch follows it within a few), then a sequence
// number in a line of its own: the host may watch for it instead of asking the runtime to wait for
// the stream (whose wake-up costs a call of 0.12 ms some 10 us)
namespace {
__global__ __launch_bounds__(64) void control_to_host_kernel(const unsigned long long *__restrict__ d_ctrl,
                                                             unsigned long long *h_ctrl, uint32_t n_words,
                                                             unsigned long long *h_seq, unsigned long long seq)
{
    for (uint32_t i = threadIdx.x; i < n_words; i += 64)
        __hip_atomic_store(&h_ctrl[i], __hip_atomic_load(&d_ctrl[i], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                           __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
    __threadfence_system();
    __builtin_amdgcn_s_waitcnt(0); // (every lane's stores have left before the one below)
    if (h_seq && threadIdx.x == 0) __hip_atomic_store(h_seq, seq, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
}
} // namespace
hipError_t launch_control_to_host(const void *d_ctrl, void *h_ctrl, size_t bytes, hipStream_t s, unsigned long long *h_seq,
                                  unsigned long long seq)
{
    control_to_host_kernel<<<1, 64, 0, s>>>((const unsigned long long *)d_ctrl, (unsigned long long *)h_ctrl,
                                            (uint32_t)(bytes / 8), h_seq, seq);
    return hipGetLastError();
}

hipError_t launch_collapse_flatten(const CollapseDesc &d, hipStream_t s)
{
    const uint32_t gather_blocks = d.priv_blocks ? (d.priv_blocks + GATHER_SLOTS - 1) / GATHER_SLOTS : 0u;
    if (d.kept_only) { // round 0 in the same launch: the slots' pairs where they are gathered, the list's in place
        const uint32_t list_blocks = grid_of(d.edge_cap, 256 * RESOLVE_PER_THREAD, 4096 / RESOLVE_PER_THREAD);
        gather_resolve_hook_kernel<<<gather_blocks * GATHER_SPLIT + list_blocks, 256, 0, s>>>(collapse_args(d), gather_blocks * GATHER_SPLIT);
        return hipGetLastError();
    }
    const bool entries = !(d.n == 0 || (d.ranges && d.n_ranges == 0));
    const uint32_t entry_blocks = entries ? entries_grid(d, 4096) : 0u;
    if (entry_blocks + gather_blocks == 0) return hipSuccess;
    uf_flatten_kernel<<<entry_blocks + gather_blocks, 256, 0, s>>>(collapse_args(d), entry_blocks);
    return hipGetLastError();
}

hipError_t launch_collapse_round(const CollapseDesc &d, int round, hipStream_t s)
{
    dag_flat_hook_kernel<<<grid_of(d.edge_cap, 256 * 8, 512), 256, 0, s>>>(collapse_args(d), round);
    return hipGetLastError();
}

hipError_t launch_collapse_finalize(const CollapseDesc &d, hipStream_t s, int check_round)
{
    if (d.n == 0 || (d.ranges && d.n_ranges == 0)) return hipSuccess;
    const uint32_t entry_blocks = entries_grid(d, d.kept_only && !d.ranges ? 512 : 2048);
    const uint32_t check_blocks = check_round >= 0 ? grid_of(d.edge_cap, 256 * 8, 256) : 0u;
    map_finalize_kernel<<<entry_blocks + check_blocks, 256, 0, s>>>(collapse_args(d), entry_blocks, check_round);
    return hipGetLastError();
}

// ---- connected components (MODE_CLUSTER): the write-out behind the unions ---------------------------
// Every pair within k was a union, so the forest is the whole answer: parent[v] <= v makes the root of a
// set its smallest index, which in rank order is the entry the algorithm keeps.  With root[] wanted an
// entry climbs to its root (the forest does not change any more: the unions ran in the launches before),
// leaves it in parent[] as the flatten pass does, and writes kept / root; with the mask alone
// (kept_only) kept[i] = parent[i] == i -- one stream in, one out, the forest left as it is.  No lab[], no
// list of one-way pairs, no round.  The blocks behind the entries' add up what the segment index's
// blocks counted (candidates, united pairs), as the directional flatten launch does; their private
// edge slots are empty, a cluster call has no pair that is not united where it is found or listed flagged.
namespace {
__global__ __launch_bounds__(256) void cluster_write_kernel(CollapseArgs a, uint32_t entry_blocks)
{
    if (blockIdx.x >= entry_blocks) {
        const uint32_t s0 = (blockIdx.x - entry_blocks) * 256u + threadIdx.x;
        const uint2 st = s0 < a.priv_blocks ? a.priv_stat[s0] : make_uint2(0u, 0u);
        block_count_add(st.x, &a.counters[CNT_CANDIDATES]);
        block_count_add(st.y, &a.counters[CNT_UF_DIRECT]);
        return;
    }
    unsigned int cnt = 0;
    collapse_entries(a, entry_blocks, [&](uint32_t i) {
        uint32_t r = a.parent[i];
        if (!a.kept_only && r != i) {
            for (;;) {
                const uint32_t p = a.parent[r];
                if (p == r) break;
                r = p;
            }
            a.parent[i] = r; // (a later climb through i ends here; any value on the way up is an ancestor)
        }
        const bool kp = r == i;
        a.kept[i] = kp ? 1 : 0;
        if (a.root) a.root[i] = r;
        cnt += kp ? 1u : 0u;
    });
    block_count_add(cnt, &a.counters[CNT_KEPT]);
}
} // namespace

hipError_t launch_cluster_write(const CollapseDesc &d, hipStream_t s)
{
    const bool entries = !(d.n == 0 || (d.ranges && d.n_ranges == 0));
    const uint32_t entry_blocks = entries ? entries_grid(d, 2048) : 0u;
    const uint32_t stat_blocks = d.priv_stat && d.priv_blocks ? (d.priv_blocks + 255u) / 256u : 0u;
    if (entry_blocks + stat_blocks == 0) return hipSuccess;
    CollapseArgs a = collapse_args(d);
    a.kept_only = d.kept_only && !d.root;
    cluster_write_kernel<<<entry_blocks + stat_blocks, 256, 0, s>>>(a, entry_blocks);
    return hipGetLastError();
}

namespace {
__global__ __launch_bounds__(256) void uf_flatten_all_kernel(uint32_t *parent, uint32_t *lab, uint32_t n)
{
    for (uint32_t v = blockIdx.x * blockDim.x + threadIdx.x; v < n; v += gridDim.x * blockDim.x) flatten_entry(parent, lab, v);
}
} // namespace

hipError_t launch_uf_components(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                                uint32_t *comp, uint32_t *lab, uint32_t n, uint32_t n_edges_hint,
                                hipStream_t s)
{
    if (n == 0) return hipSuccess;
    uf_union_kernel<<<grid_of(n_edges_hint, 256, 4096), 256, 0, s>>>(edges, counters, edge_cap, comp);
    uf_flatten_all_kernel<<<grid_of(n, 256, 4096), 256, 0, s>>>(comp, lab, n);
    return hipGetLastError();
}

hipError_t launch_pack_mask(const uint8_t *kept, uint64_t n, uint8_t *bits, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    pack_mask_kernel<<<grid_of(n, 256, 2048), 256, 0, s>>>(kept, n, bits);
    return hipGetLastError();
}

hipError_t launch_uf_union_list(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                                uint32_t *parent, uint32_t n_edges_hint, hipStream_t s)
{
    uf_union_kernel<<<grid_of(n_edges_hint, 256, 4096), 256, 0, s>>>(edges, counters, edge_cap, parent);
    return hipGetLastError();
}

} // namespace umihip
