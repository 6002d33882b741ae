// Levenshtein (edit) distance between one-word UMI keys (gfx950): umi_dedup_batch_edit.
//
// No counterpart in the reference (tkob-vh/umi-collapse-rs compares by umi_dist, Hamming, only:
// src/utils/mod.rs:24-26); the distance is the one starcode and the long-read UMI pipelines cluster
// by, because a base lost or gained during oligo synthesis shifts the rest of a fixed-length UMI
// window.  d_E(a, b): substitution, insertion and deletion cost 1 each, over the umi_len letters of
// A T C G N, two letters matching iff they are the same letter.  Everything around the distance --
// rank order, thresholds, the edge list, the collapse -- is the Hamming path's.
//
// One wave per task (64 rows against the later entries of their bucket, as umihip_wide.hip), three
// steps per tile of 64 columns:
//   filter   the counts of A, C, G, T of a key, one byte each, are a point whose L1 distance to
//            another key's is at most 2 d_E (a substitution moves two counts by one, an insertion
//            with a deletion as well; N and the length stay out, which only lowers L1): one
//            v_sad_u8 per pair against 2 k, a row per lane, the column broadcast;
//   compact  the hits of a column go to an LDS queue as (row lane, column) behind a ballot and a
//            prefix count -- with a row per lane nearly every column has a lane that passes, so
//            the exact check must not run in that layout;
//   check    the queue is worked off 64 pairs at a time, one per lane: Myers' bit-vector
//            recurrence in its global form over the umi_len <= 21 bits of one register, the exact
//            distance for any k.  The match vector of a column letter comes from the bit planes of
//            the codes (bit b of every base's 3-bit code, packed once per entry by the prep pass).
// Integer / bitwise work, 64-lane waves, no MFMA.
#include <hip/hip_runtime.h>

#include <algorithm>

#include "umihip_internal.h"
#include "umihip_device.h"

namespace umihip {

namespace {

constexpr int EDIT_QUEUE = 1024;         // filter hits the queue holds: drained before a column could overrun it
constexpr uint32_t PLANE_MASK = 0x1FFFFFu; // 21 bases

// what the exact check needs of an entry, one ds_read_b128
struct __attribute__((aligned(16))) EditRec {
    uint64_t planes; // bit b of base i's code at bit 21 b + i
    int32_t freq, thr;
};

// Per entry: threshold, start label, contract check (as prep_kernel), and the two forms of the key the
// pair kernel reads -- the letter counts (A, C, G, T in bytes 0..3) and the code bit planes.
__global__ __launch_bounds__(256) void edit_prep_kernel(const uint64_t *__restrict__ keys,
                                                        const uint64_t *__restrict__ nmask,
                                                        const int32_t *__restrict__ freq, uint32_t n, int umi_len,
                                                        float percentage, uint64_t *__restrict__ planes,
                                                        uint32_t *__restrict__ counts, int32_t *__restrict__ thr,
                                                        uint32_t *__restrict__ label,
                                                        unsigned long long *__restrict__ counters)
{
    unsigned int bad = 0, rises = 0;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const uint64_t key = keys[i] & (umi_len >= 21 ? 0x7FFFFFFFFFFFFFFFull : ((1ull << (3 * umi_len)) - 1ull));
        const int32_t f = freq[i];
        thr[i] = threshold_of(percentage, f);
        label[i] = i;
        uint64_t p0 = 0, p1 = 0, p2 = 0;
        uint32_t cnt = 0;
        for (int b = 0; b < umi_len; b++) {
            const uint32_t c = (uint32_t)(key >> (3 * b)) & 7u;
            p0 |= (uint64_t)(c & 1u) << b;
            p1 |= (uint64_t)((c >> 1) & 1u) << b;
            p2 |= (uint64_t)(c >> 2) << b;
            // A 000, C 110, G 011, T 101 (src/utils/read.rs:23-31); N 100 counts for nothing
            cnt += c == 0u ? 1u : c == 6u ? 1u << 8 : c == 3u ? 1u << 16 : c == 5u ? 1u << 24 : 0u;
        }
        planes[i] = p0 | (p1 << 21) | (p2 << 42);
        counts[i] = cnt;
        bad += f < 1 ? 1u : 0u;
        if (nmask) { // a given nmask must cover every N code of its key (prep_kernel's check)
            const uint64_t k3 = key & ~nmask[i];
            const uint64_t b2 = k3 & 0x4924924924924924ull;
            bad += (b2 & ~((k3 << 1) | (k3 << 2))) != 0 ? 1u : 0u;
        }
        rises += (i > 0 && f > freq[i - 1]) ? 1u : 0u;
    }
    block_count_add(bad, &counters[CNT_ERROR]);
    block_count_add(rises, &counters[CNT_RISES]);
}

// rises at the first entry of a bucket: the only legal ones (the host compares the two counts)
__global__ __launch_bounds__(256) void edit_rise_kernel(const int32_t *__restrict__ freq,
                                                        const uint64_t *__restrict__ bucket_off, uint64_t n_buckets,
                                                        uint32_t n_entries, unsigned long long *__restrict__ counters)
{
    unsigned int rises = 0;
    for (uint64_t b = blockIdx.x * blockDim.x + threadIdx.x; b < n_buckets; b += (uint64_t)gridDim.x * blockDim.x) {
        const uint64_t s = bucket_off[b], e = bucket_off[b + 1];
        if (s > 0 && s < e && e <= (uint64_t)n_entries) rises += freq[s] > freq[s - 1] ? 1u : 0u;
    }
    block_count_add(rises, &counters[CNT_START_RISES]);
}

// Myers' bit-vector recurrence (1999) in Hyyro's formulation, global distance: pattern = the row's
// umi_len letters (bit i of a vector = letter i), text = the column's.  Pv / Mv: vertical deltas +1 / -1
// of the current DP column; the score is the DP cell (umi_len, j), starts at umi_len (column 0) and moves
// with the horizontal delta at bit umi_len - 1; the first DP row grows by one per letter, which is the 1
// shifted into Ph.  Bits above umi_len - 1 hold garbage that only ever moves upwards (carry, left shift).
__device__ __forceinline__ int edit_distance(uint64_t row_planes, uint64_t col_planes, int umi_len)
{
    const uint32_t p0 = (uint32_t)row_planes & PLANE_MASK, p1 = (uint32_t)(row_planes >> 21) & PLANE_MASK,
                   p2 = (uint32_t)(row_planes >> 42) & PLANE_MASK;
    const uint32_t t0 = (uint32_t)col_planes & PLANE_MASK, t1 = (uint32_t)(col_planes >> 21) & PLANE_MASK,
                   t2 = (uint32_t)(col_planes >> 42) & PLANE_MASK;
    uint32_t pv = 0xFFFFFFFFu, mv = 0u;
    int score = umi_len;
    const int top = umi_len - 1;
    for (int j = 0; j < umi_len; j++) { // (wave-uniform trip count)
        // letters of the row equal to the column's letter j: all three code bits agree
        // (bit j of a plane spread over the register: one v_bfe_i32)
        const uint32_t m0 = (uint32_t)__builtin_amdgcn_sbfe((int)t0, j, 1), m1 = (uint32_t)__builtin_amdgcn_sbfe((int)t1, j, 1),
                       m2 = (uint32_t)__builtin_amdgcn_sbfe((int)t2, j, 1);
        const uint32_t eq = ~((p0 ^ m0) | (p1 ^ m1) | (p2 ^ m2));
        const uint32_t xv = eq | mv;
        const uint32_t xh = (((eq & pv) + pv) ^ pv) | eq;
        uint32_t ph = mv | ~(xh | pv);
        uint32_t mh = pv & xh;
        score += (int)((ph >> top) & 1u) - (int)((mh >> top) & 1u);
        ph = (ph << 1) | 1u;
        mh <<= 1;
        pv = mh | ~(xv | ph);
        mv = ph & xv;
    }
    return score;
}

// One task: rows [row0, min(row0 + 64, row_end)) against columns [col0, col1) of the same bucket; only
// pairs with row < column count.  a.fkey: the entries' bit planes; counts: their letter counts.
__global__ __launch_bounds__(64) void edit_pair_kernel(PairArgs a, const uint32_t *__restrict__ counts, int umi_len)
{
    __shared__ EdgeStage stage;
    __shared__ EditRec rows[64], cols[64];
    __shared__ uint16_t queue[EDIT_QUEUE]; // row lane << 6 | column of the tile
    const int lane = threadIdx.x;
    if (lane == 0) {
        stage.count = 0;
        stage.candidates = 0;
    }
    const PairTask t = a.tasks[blockIdx.x];
    const uint64_t *__restrict__ planes = (const uint64_t *)a.fkey;
    const uint32_t r = t.row0 + (uint32_t)lane;
    const bool row_ok = r < t.row_end;
    const uint32_t cr = row_ok ? counts[r] : 0u;
    {
        EditRec rec;
        rec.planes = row_ok ? planes[r] : 0ull;
        rec.freq = row_ok ? a.freq[r] : 0;
        rec.thr = row_ok ? a.thr[r] : 0;
        rows[lane] = rec;
    }
    __syncthreads();
    const uint32_t lim = 2u * (uint32_t)a.k; // (k <= umi_len <= 21)
    const int k = a.k, mode = a.mode;
    uint32_t qn = 0;             // entries in the queue (wave-uniform)
    unsigned long long n_cand = 0; // pairs that reached the exact check (wave-uniform)
    uint32_t c0 = 0;

    // the exact check of the m <= 64 newest entries of the queue, one per lane
    auto check_group = [&](uint32_t m) {
        __syncthreads(); // (the queue's stores, by other lanes)
        const uint32_t base = qn - m;
        const bool active = (uint32_t)lane < m;
        const uint32_t e = active ? (uint32_t)queue[base + (uint32_t)lane] : 0u;
        const uint32_t rl = e >> 6, j = e & 63u;
        const EditRec R = rows[rl], C = cols[j];
        const int dist = edit_distance(R.planes, C.planes, umi_len);
        if (active && dist <= k) {
            const uint32_t gi = t.row0 + rl, gj = c0 + j;
            bool fwd, bwd;
            if (mode == MODE_DIRECTIONAL) { // naive.rs:31 with max_freq = threshold(start) (directional.rs:38-39)
                fwd = C.freq <= R.thr;
                bwd = R.freq <= C.thr;
            } else if (mode == MODE_CLUSTER) { // connected components: a union, nothing to ask of freq
                fwd = bwd = true;
            } else { // adjacency.rs:56: a root only ever sees entries of larger rank
                fwd = C.freq <= a.adj_max_freq;
                bwd = false;
            }
            if (fwd && bwd) emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gi | SYM_FLAG, gj, dist, false);
            else if (fwd) emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gi, gj, dist, false);
            else if (bwd) emit_edge(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, gj, gi, dist, false);
        }
        qn = base;
        n_cand += m;
        // (at most 64 more edges since the last look: the stage of 512 never runs over)
        flush_edges<64>(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, false, false);
    };

    for (c0 = t.col0; c0 < t.col1; c0 += 64) {
        const uint32_t c = c0 + (uint32_t)lane;
        const bool col_ok = c < t.col1;
        const uint32_t cc = col_ok ? counts[c] : 0u;
        {
            EditRec rec;
            rec.planes = col_ok ? planes[c] : 0ull;
            rec.freq = col_ok ? a.freq[c] : 0;
            rec.thr = col_ok ? a.thr[c] : 0;
            __syncthreads(); // (the tile before has been checked: the queue is empty)
            cols[lane] = rec;
        }
        __syncthreads();
        const uint32_t ncols = min(64u, t.col1 - c0);
        for (uint32_t j = 0; j < ncols; j++) { // (wave-uniform trip count)
            const uint32_t cb = (uint32_t)__builtin_amdgcn_readlane((int)cc, (int)j);
            const bool hit = row_ok && r < c0 + j && __builtin_amdgcn_sad_u8(cr, cb, 0u) <= lim;
            const unsigned long long mask = __ballot(hit);
            if (hit) {
                const uint32_t before = __builtin_amdgcn_mbcnt_hi((uint32_t)(mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)mask, 0u));
                queue[qn + before] = (uint16_t)(((uint32_t)lane << 6) | j); // qn <= EDIT_QUEUE - 64 here
            }
            qn += (uint32_t)__builtin_popcountll(mask);
            if (qn > (uint32_t)EDIT_QUEUE - 64u) // another column might not fit: whole groups off the top
                while (qn >= 64u) check_group(64u);
        }
        while (qn) check_group(min(qn, 64u)); // the columns leave LDS with the tile
    }
    flush_edges<64>(&stage, a.edges, a.edge_dist, a.counters, a.edge_cap, false, true);
    if (lane == 0 && n_cand) atomicAdd(&a.counters[CNT_CANDIDATES], n_cand);
}

uint32_t edit_grid(uint64_t n, uint32_t block, uint32_t cap)
{
    return (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((n + block - 1) / block, cap));
}

} // namespace

hipError_t launch_edit_prep(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq, const uint64_t *bucket_off,
                            uint64_t n_buckets, uint32_t n, int umi_len, float percentage, uint64_t *planes,
                            uint32_t *counts, int32_t *thr, uint32_t *label, unsigned long long *counters, hipStream_t s)
{
    if (n == 0) return hipSuccess;
    edit_prep_kernel<<<edit_grid(n, 256, 1u << 16), 256, 0, s>>>(keys, nmask, freq, n, umi_len, percentage, planes, counts,
                                                                thr, label, counters);
    edit_rise_kernel<<<edit_grid(n_buckets, 256, 512), 256, 0, s>>>(freq, bucket_off, n_buckets, n, counters);
    return hipGetLastError();
}

hipError_t launch_edit_pairs(const PairArgs &a, const uint32_t *counts, uint32_t n_tasks, int umi_len, hipStream_t s)
{
    if (n_tasks == 0) return hipSuccess;
    if (umi_len < 1 || umi_len > 21 || a.k < 0 || a.k > umi_len) return hipErrorInvalidValue;
    edit_pair_kernel<<<n_tasks, 64, 0, s>>>(a, counts, umi_len);
    return hipGetLastError();
}

} // namespace umihip
