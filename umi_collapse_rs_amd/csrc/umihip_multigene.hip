// UMIs that one cell shows under several genes (umi_filter_multigene, the program's --umi-filtering multi-gene),
// gfx950: the molecules (kept entries) of a batched call are joined across its buckets by (group, UMI); in a run
// of two or more only the molecule with strictly the most reads survives, none where the top is shared.  The
// rule is Cell Ranger's and STARsolo's MultiGeneUMI_CR; tests/multigene_model.py (filter_model) defines it.
// Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The host leaves the empty buckets out as umi_count_matrix does (umihip_count_api.cpp: cm_walk); everything below
// works on the n entries of the m non-empty buckets.
//
//   entry    a lane per entry: its bucket by a binary search of the offsets (every entry the same few steps, a
//            bucket of any size costs what its entries cost), root[] / kept[] checked against it, the bucket's group
//            checked once at its first entry; freq[i] is added onto total[root[i]] (64 bits; the lanes of a wave
//            that share the first pending lane's root send one atomic).  kept_out[i] = kept[i] != 0, streamed.
//            Where the whole sort key fits one word the pass writes it: UMI | group << 3 L | (not a molecule) <<
//            (3 L + gb), gb = bits of n_groups - 1.
//   sort     every entry is sorted, the ones that are no molecule behind all molecules by the key's top bit: the
//            number of molecules is known on the device only, and a sort of that many would cost the call a
//            second synchronisation.  One radix_sort_pairs_u64 over the 3 L + gb + 1 bits in use where they fit
//            64 (12 bases with up to 2^27 groups do); else a stable sort per key word, word 0 first, carrying the
//            entry, and a last one by group and the molecule bit (umihip_stats.hip's per-UMI table does the same).
//   heads    flag[i] = the sorted entry differs from its predecessor in the UMI's bits, the group or the molecule
//            bit; scan_inclusive_u64 numbers the runs.
//   max      a lane per sorted entry; whether it is a molecule is the top bit of the last sort's key.  A molecule
//            whose run is longer than one (it is no head, or its successor is none) takes part: it gathers its
//            total -- a run of one survives whatever it holds, so nearly every lane of a sample gathers nothing --
//            a segmented max scan over the wave follows, and the run's last lane in the wave sends one atomicMax
//            onto the run's zeroed word.  The gathered totals are kept in sorted order, over the keys.
//   ties     the same walk counts the molecules that hold the run's maximum: a segmented sum, one atomicAdd per
//            wave and run.  Maximum and count are integers put together by max and +: no order can change them,
//            and no thread walks a run (one UMI under every gene of a cell is a run as long as the input).
//   write    kept_out gets 0 at every molecule of a longer run that does not hold the maximum alone: the scattered
//            stores are the removed molecules' only.  The three counts are kept in registers over a grid-stride
//            loop and added to the control block once per block.  freq_out, where asked for, is a gather of
//            kept_out through root[].
//
// One synchronisation, at the end, brings the control block.  Workspace per entry: total 8, group 4, keys 2 x 8
// (after the scan: the flags' buffer holds nothing, the sorted keys' the totals in sorted order), values 2 x 4
// (the free one: the walk's flags), run numbers 8, run maximum 8, run ties 4: 56 bytes, the offsets (8 to 12 per
// non-empty bucket) and the sort's tables.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "umihip_internal.h"
#include "umihip_pair_table.h"

namespace umihip {

namespace {

constexpr int MG_THREADS = 256;
// the control block's words
constexpr int MG_BAD_GROUPS = 0, MG_BAD_ROOTS = 1, MG_RUNS = 2, MG_REMOVED = 3, MG_REMOVED_READS = 4;
// the walk's flags of a sorted entry
constexpr uint32_t MG_MOL = 1u, MG_MULTI = 2u, MG_HEAD = 4u;

struct MgWs {
    unsigned long long *ctl;
    uint64_t *off;  // [m + 1] the non-empty buckets' offsets
    uint32_t *idx;  // [m] their bucket numbers (null: nothing was left out)
    unsigned long long *total, *runmax;
    uint32_t *eg, *ties;
    uint64_t *ka, *kb, *incl;
    uint32_t *va, *vb;
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes, bytes;
};
MgWs mg_carve(void *ws, uint32_t n, uint32_t m, bool has_idx)
{
    MgWs w;
    Carver c(ws);
    w.ctl = c.take<unsigned long long>(256);
    w.off = c.take<uint64_t>(((size_t)m + 1) * 8);
    w.idx = has_idx ? c.take<uint32_t>((size_t)m * 4) : nullptr;
    w.total = c.take<unsigned long long>((size_t)n * 8);
    w.runmax = c.take<unsigned long long>((size_t)n * 8);
    w.eg = c.take<uint32_t>((size_t)n * 4);
    w.ties = c.take<uint32_t>((size_t)n * 4);
    w.ka = c.take<uint64_t>((size_t)n * 8);
    w.kb = c.take<uint64_t>((size_t)n * 8);
    w.incl = c.take<uint64_t>((size_t)n * 8);
    w.va = c.take<uint32_t>((size_t)n * 4);
    w.vb = c.take<uint32_t>((size_t)n * 4);
    w.radix_bytes = radix_sort_temp_bytes(n);
    w.radix_tmp = c.take(w.radix_bytes);
    w.scan_bytes = scan_temp_bytes(n);
    w.scan_tmp = c.take(w.scan_bytes);
    w.bytes = c.o;
    return w;
}

struct MgMasks {
    uint64_t wm[4]; // per key word: the bits below 3 L
};

// total[idx] += val for the lanes with `todo`, all lanes of the wave calling together: the lanes that share the
// first pending lane's word send one atomic for their sum, the others one each (a cluster's entries lie side by
// side and share their root)
__device__ __forceinline__ void wave_add_u64(unsigned long long *arr, uint32_t idx, unsigned long long val, bool todo)
{
    const int lane = (int)(threadIdx.x & 63u);
    const unsigned long long pending = __ballot(todo);
    if (pending) {
        const int leader = __ffsll(pending) - 1;
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

struct MgEntryArgs {
    const uint64_t *keys;
    const int32_t *freq;
    const uint8_t *kept;
    const uint32_t *root;
    const uint64_t *off;
    const uint32_t *idx; // may be null
    const uint32_t *group;
    uint32_t n, m, n_groups;
    int W, shift, gb; // key words; 3 L; bits of n_groups - 1
    uint64_t mask0;   // composed key: the UMI's bits of word 0 (0: the key does not fit a word, none is written)
    unsigned long long *total, *ctl;
    uint32_t *eg;
    uint64_t *key;
    uint32_t *val;
    uint8_t *kept_out;
};

__global__ __launch_bounds__(MG_THREADS) void mg_entry_kernel(MgEntryArgs a)
{
    uint32_t bad_groups = 0, bad_roots = 0;
    const uint64_t rounds = ((uint64_t)a.n + MG_THREADS - 1) / MG_THREADS;
    for (uint64_t r = blockIdx.x; r < rounds; r += gridDim.x) { // (whole waves go round: wave_add_u64 is a wave's call)
        const uint64_t i = r * MG_THREADS + threadIdx.x;
        const bool valid = i < a.n;
        bool ok = false;
        uint32_t rt = 0;
        unsigned long long f = 0;
        if (valid) {
            uint32_t lo = 0, hi = a.m; // the bucket: off[lo] <= i < off[hi] (off[0] = 0, off[m] = n)
            while (hi - lo > 1u) {
                const uint32_t mid = lo + (hi - lo) / 2u;
                if (a.off[mid] <= i) lo = mid;
                else hi = mid;
            }
            const uint64_t first = a.off[lo], end = a.off[lo + 1];
            uint32_t g = a.group[a.idx ? a.idx[lo] : lo];
            if (g >= a.n_groups) {
                bad_groups += i == first;
                g = 0;
            }
            rt = a.root[i];
            const bool k = a.kept[i] != 0;
            ok = rt >= first && rt < end;
            if (ok) ok = a.kept[rt] != 0 && (!k || rt == (uint32_t)i);
            bad_roots += !ok;
            f = (unsigned long long)(long long)a.freq[i];
            a.eg[i] = g;
            a.kept_out[i] = k ? 1 : 0; // (every molecule, in the entries' order: the write pass takes the removed ones out)
            if (a.mask0) {
                a.key[i] = (a.keys[i] & a.mask0) | ((uint64_t)g << a.shift) | ((uint64_t)!k << (a.shift + a.gb));
                a.val[i] = (uint32_t)i;
            }
        }
        wave_add_u64(a.total, rt, f, ok);
    }
    if (bad_groups) atomicAdd(a.ctl + MG_BAD_GROUPS, (unsigned long long)bad_groups);
    if (bad_roots) atomicAdd(a.ctl + MG_BAD_ROOTS, (unsigned long long)bad_roots);
}

// the sort key of one pass of the word-by-word sort: key word w of the entries in their order so far (w < W), or
// group | (not a molecule) << gb (w == W)
__global__ __launch_bounds__(MG_THREADS) void mg_word_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ eg,
                                                             const uint8_t *__restrict__ kept, int W, int w, uint64_t mask, int gb,
                                                             const uint32_t *__restrict__ order, uint32_t n,
                                                             uint64_t *__restrict__ out_key, uint32_t *__restrict__ out_val)
{
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t e = order ? order[i] : (uint32_t)i;
    out_key[i] = w < W ? keys[(uint64_t)e * (uint64_t)W + (uint64_t)w] & mask : (uint64_t)eg[e] | ((uint64_t)(kept[e] == 0) << gb);
    if (!order) out_val[i] = e;
}

__global__ __launch_bounds__(MG_THREADS) void mg_heads_wide_kernel(const uint64_t *__restrict__ keys, const uint32_t *__restrict__ eg,
                                                                   const uint8_t *__restrict__ kept, int W, MgMasks um,
                                                                   const uint32_t *__restrict__ order, uint32_t n,
                                                                   uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    bool head = i == 0;
    if (!head) {
        const uint64_t x = order[i], y = order[i - 1];
        head = eg[x] != eg[y] || (kept[x] != 0) != (kept[y] != 0);
        for (int w = 0; w < W; w++) head = head || ((keys[x * (uint64_t)W + w] ^ keys[y * (uint64_t)W + w]) & um.wm[w]) != 0;
    }
    flag[i] = head ? 1ull : 0ull;
}

// key_ts: the last sort's keys, whose bit mol_bit says "no molecule"; the totals of the runs longer than one are
// written over them, in sorted order (a lane reads its own word first)
__global__ __launch_bounds__(MG_THREADS) void mg_max_kernel(const uint32_t *__restrict__ order, const uint64_t *__restrict__ incl,
                                                            const unsigned long long *__restrict__ total, int mol_bit, uint32_t n,
                                                            unsigned long long *key_ts, uint32_t *__restrict__ vf,
                                                            unsigned long long *runmax)
{
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    const WaveRuns r(incl, i, n);
    const bool mol = r.valid && ((key_ts[i] >> mol_bit) & 1ull) == 0ull;
    const bool multi = mol && !(r.head && r.last); // (a run holds molecules only or none: the molecule bit is part of the key)
    unsigned long long t = 0;
    if (multi) t = total[order[i]]; // (a run of one survives whatever its total: nearly every lane gathers nothing)
    if (r.valid) {
        key_ts[i] = t;
        vf[i] = (mol ? MG_MOL : 0u) | (multi ? MG_MULTI : 0u) | (r.head ? MG_HEAD : 0u);
    }
    unsigned long long v = multi ? t : 0ull;
    r.scan([](unsigned long long x, unsigned long long y) { return max(x, y); }, v);
    if (multi && r.tail()) atomicMax(runmax + r.slot(), v);
}

__global__ __launch_bounds__(MG_THREADS) void mg_ties_kernel(const uint64_t *__restrict__ incl, const unsigned long long *__restrict__ ts,
                                                             const uint32_t *__restrict__ vf,
                                                             const unsigned long long *__restrict__ runmax, uint32_t n,
                                                             uint32_t *ties)
{
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    const WaveRuns r(incl, i, n);
    const bool multi = r.valid && (vf[i] & MG_MULTI) != 0u;
    uint32_t c = multi && ts[i] == runmax[r.slot()] ? 1u : 0u;
    r.scan([](uint32_t x, uint32_t y) { return x + y; }, c);
    if (multi && r.tail() && c) atomicAdd(ties + r.slot(), c);
}

// (grid-stride, the counts kept in registers: a block adds to the control block once -- a wave's worth of atomics
// per 64 sorted entries on its three words was a third of the call)
__global__ __launch_bounds__(MG_THREADS) void mg_write_kernel(const uint32_t *__restrict__ order, const uint64_t *__restrict__ incl,
                                                              const unsigned long long *__restrict__ ts, const uint32_t *__restrict__ vf,
                                                              const unsigned long long *__restrict__ runmax,
                                                              const uint32_t *__restrict__ ties, uint32_t n,
                                                              uint8_t *__restrict__ kept_out, unsigned long long *ctl)
{
    __shared__ unsigned long long part[MG_THREADS / 64][3];
    const int lane = (int)(threadIdx.x & 63u), wave = (int)(threadIdx.x >> 6);
    unsigned long long runs = 0, removed = 0, reads = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x; i < n; i += (uint64_t)gridDim.x * MG_THREADS) {
        const uint32_t f = vf[i];
        if (!(f & MG_MULTI)) continue; // (no molecule, or alone in its run: kept_out stands as the entry pass wrote it)
        const uint64_t slot = incl[i] - 1;
        runs += (f & MG_HEAD) != 0u;
        if (ts[i] == runmax[slot] && ties[slot] == 1u) continue;
        kept_out[order[i]] = 0;
        removed++;
        reads += ts[i];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
        runs += __shfl_xor(runs, o);
        removed += __shfl_xor(removed, o);
        reads += __shfl_xor(reads, o);
    }
    if (lane == 0) {
        part[wave][0] = runs;
        part[wave][1] = removed;
        part[wave][2] = reads;
    }
    __syncthreads();
    static_assert(MG_REMOVED == MG_RUNS + 1 && MG_REMOVED_READS == MG_RUNS + 2, "the three counts lie side by side");
    if (threadIdx.x < 3) {
        unsigned long long v = 0;
        for (int w = 0; w < MG_THREADS / 64; w++) v += part[w][threadIdx.x];
        if (v) atomicAdd(ctl + MG_RUNS + threadIdx.x, v);
    }
}

// (a root out of range has been counted: the outputs are then worthless, but nothing is read outside the arrays)
__global__ __launch_bounds__(MG_THREADS) void mg_freq_kernel(const int32_t *__restrict__ freq, const uint32_t *__restrict__ root,
                                                             const uint8_t *__restrict__ kept_out, uint32_t n,
                                                             int32_t *__restrict__ freq_out)
{
    const uint64_t i = (uint64_t)blockIdx.x * MG_THREADS + threadIdx.x;
    if (i >= n) return;
    const uint32_t r = root[i];
    freq_out[i] = r < n && kept_out[r] != 0 ? freq[i] : 0;
}

} // namespace

size_t multigene_workspace_bytes(uint32_t n, uint32_t m, bool has_idx) { return mg_carve(nullptr, n, m, has_idx).bytes; }

int multigene_on_device(void *workspace, const MultigeneCall &c, hipStream_t s)
{
    const uint32_t n = c.n, m = c.m;
    const int L = c.umi_len, W = c.n_words;
    const MgWs w = mg_carve(workspace, n, m, c.h_idx != nullptr);
    int gb = 0;
    while (((uint64_t)c.n_groups - 1) >> gb) gb++; // (n_groups >= 1, gb <= 32)
    const bool composed = 3 * L + gb + 1 <= 64;
    MgMasks um;
    for (int wd = 0; wd < 4; wd++) {
        const int bits = std::min(64, std::max(0, 3 * L - 64 * wd));
        um.wm[wd] = bits == 64 ? ~0ull : (1ull << bits) - 1ull;
    }
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, 256, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.total, 0, (size_t)n * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.runmax, 0, (size_t)n * 8, s)); // (the runs' words are added up in place)
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ties, 0, (size_t)n * 4, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(w.off, c.h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (c.h_idx) UMIHIP_TRY_NEG(hipMemcpyAsync(w.idx, c.h_idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    const uint32_t per_entry = blocks_for(n, MG_THREADS);
    MgEntryArgs a;
    a.keys = c.d_keys;
    a.freq = c.d_freq;
    a.kept = c.d_kept;
    a.root = c.d_root;
    a.off = w.off;
    a.idx = w.idx;
    a.group = c.d_group;
    a.n = n;
    a.m = m;
    a.n_groups = c.n_groups;
    a.W = W;
    a.shift = 3 * L;
    a.gb = gb;
    a.mask0 = composed ? um.wm[0] : 0ull; // (L >= 1: never 0 where the key is composed)
    a.total = w.total;
    a.ctl = w.ctl;
    a.eg = w.eg;
    a.key = w.ka;
    a.val = w.va;
    a.kept_out = c.d_kept_out;
    mg_entry_kernel<<<std::min(per_entry, c.n_cus * 8), MG_THREADS, 0, s>>>(a);
    UMIHIP_TRY_NEG(hipGetLastError());
    uint64_t *ka = w.ka, *kb = w.kb;
    uint32_t *va = w.va, *vb = w.vb;
    auto sort_by = [&](int bits) {
        bool in_b = false;
        const hipError_t e = radix_sort_pairs_u64(ka, kb, va, vb, n, 0, bits, w.radix_tmp, w.radix_bytes, &in_b, s);
        if (in_b) {
            std::swap(ka, kb);
            std::swap(va, vb);
        }
        return e;
    };
    if (composed) {
        UMIHIP_TRY_NEG(sort_by(3 * L + gb + 1));
        pair_heads_kernel<MG_THREADS><<<per_entry, MG_THREADS, 0, s>>>(ka, n, kb);
        UMIHIP_TRY_NEG(hipGetLastError());
    } else {
        for (int wd = 0; wd <= W; wd++) { // (stable sorts, the least significant word first)
            const int bits = wd < W ? std::min(64, 3 * L - 64 * wd) : gb + 1;
            mg_word_kernel<<<per_entry, MG_THREADS, 0, s>>>(c.d_keys, w.eg, c.d_kept, W, wd, wd < W ? um.wm[wd] : 0ull, gb,
                                                            wd ? va : nullptr, n, ka, va);
            UMIHIP_TRY_NEG(hipGetLastError());
            UMIHIP_TRY_NEG(sort_by(bits));
        }
        mg_heads_wide_kernel<<<per_entry, MG_THREADS, 0, s>>>(c.d_keys, w.eg, c.d_kept, W, um, va, n, kb);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    UMIHIP_TRY_NEG(scan_inclusive_u64(kb, w.incl, n, w.scan_tmp, w.scan_bytes, s));
    unsigned long long *ts = (unsigned long long *)ka; // (the sorted keys have been compared: the totals take their place)
    mg_max_kernel<<<per_entry, MG_THREADS, 0, s>>>(va, w.incl, w.total, composed ? 3 * L + gb : gb, n, ts, vb, w.runmax);
    UMIHIP_TRY_NEG(hipGetLastError());
    mg_ties_kernel<<<per_entry, MG_THREADS, 0, s>>>(w.incl, ts, vb, w.runmax, n, w.ties);
    UMIHIP_TRY_NEG(hipGetLastError());
    mg_write_kernel<<<std::min(per_entry, c.n_cus * 8), MG_THREADS, 0, s>>>(va, w.incl, ts, vb, w.runmax, w.ties, n, c.d_kept_out, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    if (c.d_freq_out) {
        mg_freq_kernel<<<per_entry, MG_THREADS, 0, s>>>(c.d_freq, c.d_root, c.d_kept_out, n, c.d_freq_out);
        UMIHIP_TRY_NEG(hipGetLastError());
    }
    UMIHIP_TRY_NEG(hipMemcpyAsync(c.h_pinned, w.ctl, 5 * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    return 0;
}

} // namespace umihip
