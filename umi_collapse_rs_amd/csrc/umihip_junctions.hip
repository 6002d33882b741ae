// Molecules and reads per (column, splice junction) pair over the buckets of a batched call (umi_junction_matrix, the
// program's --junction-matrix), gfx950: the junctions of the reads' CIGARs are extracted, numbered in the order of
// (ref, start, end), carried to their reads' molecules and counted per column, as sorted triplets.  No counterpart in
// the reference; the matrix is STARsolo's --soloFeatures SJ without a strand and with the run's own collapse, and
// tests/junction_model.py defines it.  Integer work on HBM streams, 64-lane waves, no MFMA.
//
// The bucket table is walked on the host exactly as for umi_count_matrix (umihip_count.hip): the m non-empty buckets.
// The work has two halves with one look of the host between them, because the sorts' lengths are host arguments.
//
// First half (junction_count_on_device), sized by the reads and the buckets:
//   columns  a lane per non-empty bucket: its column, checked against n_cols, into bcol[].
//   count    a lane per read (umihip_junction_walk.hpp): 0 for a read that is unstaged or whose root is not kept, else
//            the junctions of its CIGAR.  A falling cigar_off, a read_entry or root out of range, a read_ref < 0 and an
//            op code above 8 go to the control block by atomicMin -- the smallest such read is told -- and count 0.
//            The wave's spliced reads, its largest ref and its largest position go there too, one atomic each per wave.
//   scan     the library's scan_inclusive_u64 over the counts: a read's first occurrence, and T = the last sum.
//   The host reads the control block and T: an error, T == 0 and T above the capacity or 2^30 - 1 end the call here.
// Second half (junction_fill_on_device), sized by T:
//   fill     the same walk writes the occurrences: the key word start << eb | end (eb the bits of the largest position
//            seen), the ref, the molecule r = root[read_entry[i]] and its column.  The column is bcol[] of the bucket
//            that holds r, found by a binary search of the m + 1 offsets -- once per spliced read, so no array of a
//            column per entry is kept and no thread walks a bucket.
//   number   radix_sort_pairs_u64 of (key word, occurrence) over the bits present, then of (ref, occurrence) where a
//            ref above 0 was seen: LSD, so the order is (ref, start, end).  Run heads, a scan: the junction's number;
//            the heads write the junction table, every occurrence takes its number.
//   count    a stable sort by molecule, then by column << jb | junction (jb the bits of T - 1): the order is (column,
//            junction, molecule).  One scan over two packed flags -- the head of a (column, junction) run in the upper
//            32 bits, of a (column, junction, molecule) run in the lower -- gives every triplet its slot and the
//            molecules in front of it.  The heads write junction, column and where they stand; a lane per triplet then
//            takes reads = the distance to the next head and molecules = the difference of the lower sums.
// No thread walks a run, a bucket or a molecule.  Workspace: 16 bytes a read and 12 a non-empty bucket for the first
// half, 48 bytes an occurrence for the second, and the sort's and the scan's temporaries.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_pair_table.h"
#include "umihip_junction_walk.hpp"

namespace umihip {

namespace {

constexpr int JN_THREADS = 256;
constexpr uint32_t JN_BLOCKS_PER_CU = 16;

enum JnCtl : int {
    JN_BAD_COLS = 0,   // non-empty buckets with a column out of range
    JN_BAD_ORDER = 1,  // the smallest read whose cigar_off falls (all ones: none)
    JN_BAD_ENTRY = 2,  // ... with a read_entry out of range
    JN_BAD_ROOT = 3,   // ... whose entry's root is out of range
    JN_BAD_REF = 4,    // ... with a read_ref < 0
    JN_BAD_OPCODE = 5, // ... with an op code above 8
    JN_SPLICED = 6,    // counted reads with a junction
    JN_MAX_REF = 7,    // the largest ref among them
    JN_MAX_POS = 8,    // the largest position among their junctions
    JN_CTL_COUNT = 9,
};
enum JnCtl2 : int { JN2_JUNCTIONS = 0, JN2_NNZ = 1, JN2_COUNT = 2 };

struct JnWs1 {
    unsigned long long *ctl;
    uint64_t *off;
    uint32_t *idx, *bcol;
    uint64_t *cnt, *incl;
    void *scan_tmp;
    size_t scan_bytes, total;
};
JnWs1 jn_carve1(void *ws, uint32_t n_reads, uint32_t m, bool has_idx)
{
    JnWs1 w;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = p + o;
        o += align256(bytes);
        return at;
    };
    w.ctl = (unsigned long long *)take(256);
    w.off = (uint64_t *)take(((size_t)m + 1) * 8);
    w.idx = has_idx ? (uint32_t *)take((size_t)m * 4) : nullptr;
    w.bcol = (uint32_t *)take((size_t)m * 4);
    w.cnt = (uint64_t *)take((size_t)n_reads * 8);
    w.incl = (uint64_t *)take((size_t)n_reads * 8);
    w.scan_bytes = scan_temp_bytes(n_reads);
    w.scan_tmp = take(w.scan_bytes);
    w.total = o;
    return w;
}

struct JnWs2 {
    unsigned long long *ctl;
    uint64_t *lo, *ka, *kb;
    uint32_t *va, *vb, *ref, *mol, *col, *jid;
    void *radix_tmp, *scan_tmp;
    size_t radix_bytes, scan_bytes, total;
};
JnWs2 jn_carve2(void *ws, uint32_t t)
{
    JnWs2 w;
    char *p = (char *)ws;
    size_t o = 0;
    auto take = [&](size_t bytes) {
        char *at = p + o;
        o += align256(bytes);
        return at;
    };
    w.ctl = (unsigned long long *)take(256);
    w.lo = (uint64_t *)take((size_t)t * 8);
    w.ka = (uint64_t *)take((size_t)t * 8);
    w.kb = (uint64_t *)take((size_t)t * 8);
    w.va = (uint32_t *)take((size_t)t * 4);
    w.vb = (uint32_t *)take((size_t)t * 4);
    w.ref = (uint32_t *)take((size_t)t * 4);
    w.mol = (uint32_t *)take((size_t)t * 4);
    w.col = (uint32_t *)take((size_t)t * 4);
    w.jid = (uint32_t *)take((size_t)t * 4);
    w.radix_bytes = radix_sort_temp_bytes(t);
    w.radix_tmp = take(w.radix_bytes);
    w.scan_bytes = scan_temp_bytes(t);
    w.scan_tmp = take(w.scan_bytes);
    w.total = o;
    return w;
}

__global__ __launch_bounds__(JN_THREADS) void junction_cols_kernel(const uint32_t *__restrict__ idx, const uint32_t *__restrict__ col,
                                                                   uint32_t m, uint32_t n_cols, uint32_t *__restrict__ bcol,
                                                                   unsigned long long *ctl)
{
    for (uint64_t j = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x; j < m; j += (uint64_t)gridDim.x * JN_THREADS) {
        const uint32_t c = col[idx ? idx[j] : (uint32_t)j];
        if (c >= n_cols) atomicAdd(ctl + JN_BAD_COLS, 1ull);
        bcol[j] = c;
    }
}

struct JnReads {
    const int32_t *ref, *pos;
    const uint32_t *cigar;
    const uint64_t *cigar_off;
    const uint32_t *entry;
    uint32_t n_reads;
    const uint8_t *kept;
    const uint32_t *root;
    uint64_t n; // entries
};

__global__ __launch_bounds__(JN_THREADS) void junction_count_kernel(JnReads a, uint64_t *__restrict__ cnt, unsigned long long *ctl)
{
    const uint64_t total = a.cigar_off[a.n_reads];
    unsigned long long spliced = 0, max_ref = 0, max_pos = 0;
    for (uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x; i < a.n_reads; i += (uint64_t)gridDim.x * JN_THREADS) {
        uint64_t k = 0;
        do {
            const uint64_t c0 = a.cigar_off[i], c1 = a.cigar_off[i + 1];
            if (c0 > c1 || c1 > total) {
                atomicMin(ctl + JN_BAD_ORDER, (unsigned long long)i);
                break;
            }
            const uint32_t e = a.entry[i];
            if (e == UMI_READ_UNSTAGED) break;
            if (e >= a.n) {
                atomicMin(ctl + JN_BAD_ENTRY, (unsigned long long)i);
                break;
            }
            const uint32_t r = a.root[e];
            if (r >= a.n) {
                atomicMin(ctl + JN_BAD_ROOT, (unsigned long long)i);
                break;
            }
            if (!a.kept[r]) break; // (what the multi-gene filter removed: its reads count nowhere)
            const int32_t ref = a.ref[i];
            if (ref < 0) {
                atomicMin(ctl + JN_BAD_REF, (unsigned long long)i);
                break;
            }
            int64_t last = 0;
            const int64_t got = junction_count(a.cigar + c0, c1 - c0, (int64_t)a.pos[i], &last);
            if (got < 0) {
                atomicMin(ctl + JN_BAD_OPCODE, (unsigned long long)i);
                break;
            }
            if (got) {
                k = (uint64_t)got;
                spliced++;
                max_ref = std::max(max_ref, (unsigned long long)ref);
                max_pos = std::max(max_pos, (unsigned long long)last);
            }
        } while (false);
        cnt[i] = k;
    }
    for (int d = 32; d; d >>= 1) {
        spliced += __shfl_xor(spliced, d, 64);
        max_ref = std::max(max_ref, (unsigned long long)__shfl_xor(max_ref, d, 64));
        max_pos = std::max(max_pos, (unsigned long long)__shfl_xor(max_pos, d, 64));
    }
    if ((threadIdx.x & 63) == 0 && spliced) {
        atomicAdd(ctl + JN_SPLICED, spliced);
        atomicMax(ctl + JN_MAX_REF, max_ref);
        atomicMax(ctl + JN_MAX_POS, max_pos);
    }
}

// the occurrences of every counted read (the first half has found all arrays in range)
__global__ __launch_bounds__(JN_THREADS) void junction_fill_kernel(JnReads a, const uint64_t *__restrict__ cnt,
                                                                   const uint64_t *__restrict__ incl, const uint64_t *__restrict__ off,
                                                                   const uint32_t *__restrict__ bcol, uint32_t m, int eb, uint32_t t,
                                                                   uint64_t *__restrict__ lo, uint64_t *__restrict__ key,
                                                                   uint32_t *__restrict__ val, uint32_t *__restrict__ oref,
                                                                   uint32_t *__restrict__ omol, uint32_t *__restrict__ ocol)
{
    for (uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x; i < a.n_reads; i += (uint64_t)gridDim.x * JN_THREADS) {
        const uint64_t k = cnt[i];
        if (!k) continue;
        uint64_t o = incl[i] - k;
        const uint32_t r = a.root[a.entry[i]], ref = (uint32_t)a.ref[i];
        // the bucket that holds r: the last j with off[j] <= r
        uint32_t b0 = 0, b1 = m;
        while (b1 - b0 > 1) {
            const uint32_t mid = b0 + (b1 - b0) / 2;
            if (off[mid] <= r)
                b0 = mid;
            else
                b1 = mid;
        }
        const uint32_t c = bcol[b0];
        const uint64_t c0 = a.cigar_off[i];
        JnWalk w = junction_walk_begin((int64_t)a.pos[i]);
        int64_t e, s;
        while (o < t && junction_next(a.cigar + c0, a.cigar_off[i + 1] - c0, w, &e, &s) == JN_FOUND) {
            const uint64_t word = ((uint64_t)e << eb) | (uint64_t)s;
            lo[o] = word;
            key[o] = word;
            val[o] = (uint32_t)o;
            oref[o] = ref;
            omol[o] = r;
            ocol[o] = c;
            o++;
        }
    }
}

// key[i] = src[val[i]], in place of the sorted key
__global__ __launch_bounds__(JN_THREADS) void junction_gather_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ src,
                                                                     uint32_t t, uint64_t *__restrict__ key)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i < t) key[i] = src[val[i]];
}

__global__ __launch_bounds__(JN_THREADS) void junction_heads_kernel(const uint32_t *__restrict__ val, const uint64_t *__restrict__ lo,
                                                                    const uint32_t *__restrict__ oref, uint32_t t,
                                                                    uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i >= t) return;
    bool head = i == 0;
    if (!head) {
        const uint32_t o = val[i], p = val[i - 1];
        head = lo[o] != lo[p] || oref[o] != oref[p];
    }
    flag[i] = head ? 1ull : 0ull;
}

// every occurrence takes its junction's number; the heads write the table
__global__ __launch_bounds__(JN_THREADS) void junction_table_kernel(const uint32_t *__restrict__ val, const uint64_t *__restrict__ incl,
                                                                    const uint64_t *__restrict__ lo, const uint32_t *__restrict__ oref,
                                                                    uint32_t t, int eb, uint32_t *__restrict__ jid,
                                                                    int32_t *__restrict__ jn_ref, int32_t *__restrict__ jn_start,
                                                                    int32_t *__restrict__ jn_end, unsigned long long *ctl2)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i >= t) return;
    const uint32_t o = val[i];
    const uint64_t slot1 = incl[i];
    jid[o] = (uint32_t)(slot1 - 1);
    if (i == 0 || incl[i - 1] != slot1) {
        const uint64_t word = lo[o];
        jn_ref[slot1 - 1] = (int32_t)oref[o];
        jn_start[slot1 - 1] = (int32_t)(word >> eb);
        jn_end[slot1 - 1] = (int32_t)(word & ((1ull << eb) - 1ull));
    }
    if (i + 1 == t) ctl2[JN2_JUNCTIONS] = slot1;
}

__global__ __launch_bounds__(JN_THREADS) void junction_molkey_kernel(const uint32_t *__restrict__ omol, uint32_t t,
                                                                     uint64_t *__restrict__ key, uint32_t *__restrict__ val)
{
    const uint64_t o = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (o >= t) return;
    key[o] = omol[o];
    val[o] = (uint32_t)o;
}

__global__ __launch_bounds__(JN_THREADS) void junction_pairkey_kernel(const uint32_t *__restrict__ val, const uint32_t *__restrict__ ocol,
                                                                      const uint32_t *__restrict__ jid, uint32_t t, int jb,
                                                                      uint64_t *__restrict__ key)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i >= t) return;
    const uint32_t o = val[i];
    key[i] = ((uint64_t)ocol[o] << jb) | jid[o];
}

// upper 32 bits: the head of a (column, junction) run; lower: of a (column, junction, molecule) run (t < 2^30: no carry)
__global__ __launch_bounds__(JN_THREADS) void junction_pair_heads_kernel(const uint64_t *__restrict__ key, const uint32_t *__restrict__ val,
                                                                         const uint32_t *__restrict__ omol, uint32_t t,
                                                                         uint64_t *__restrict__ flag)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i >= t) return;
    const bool pair = i == 0 || key[i] != key[i - 1];
    const bool mol = pair || omol[val[i]] != omol[val[i - 1]];
    flag[i] = (pair ? 1ull << 32 : 0ull) | (mol ? 1ull : 0ull);
}

__global__ __launch_bounds__(JN_THREADS) void junction_pair_slots_kernel(const uint64_t *__restrict__ key, const uint64_t *__restrict__ incl,
                                                                         uint32_t t, int jb, uint32_t *__restrict__ head_pos,
                                                                         uint32_t *__restrict__ out_jn, uint32_t *__restrict__ out_col,
                                                                         unsigned long long *ctl2)
{
    const uint64_t i = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x;
    if (i >= t) return;
    const uint64_t slot1 = incl[i] >> 32;
    if (i == 0 || (incl[i - 1] >> 32) != slot1) {
        const uint64_t k = key[i];
        head_pos[slot1 - 1] = (uint32_t)i;
        out_jn[slot1 - 1] = (uint32_t)(k & ((1ull << jb) - 1ull));
        out_col[slot1 - 1] = (uint32_t)(k >> jb);
    }
    if (i + 1 == t) ctl2[JN2_NNZ] = slot1;
}

__global__ __launch_bounds__(JN_THREADS) void junction_pair_counts_kernel(const uint32_t *__restrict__ head_pos,
                                                                          const uint64_t *__restrict__ incl, uint32_t t,
                                                                          const unsigned long long *__restrict__ ctl2,
                                                                          uint32_t *__restrict__ out_molecules,
                                                                          uint64_t *__restrict__ out_reads)
{
    const uint64_t k = (uint64_t)blockIdx.x * JN_THREADS + threadIdx.x, nnz = ctl2[JN2_NNZ];
    if (k >= nnz) return;
    const uint32_t i = head_pos[k], end = k + 1 < nnz ? head_pos[k + 1] : t;
    out_reads[k] = (uint64_t)(end - i);
    out_molecules[k] = (uint32_t)(incl[end - 1] & 0xFFFFFFFFull) - (uint32_t)(incl[i] & 0xFFFFFFFFull) + 1u;
}

} // namespace

size_t junction_count_workspace_bytes(uint32_t n_reads, uint32_t m, bool has_idx) { return jn_carve1(nullptr, n_reads, m, has_idx).total; }
size_t junction_fill_workspace_bytes(uint32_t t) { return jn_carve2(nullptr, t).total; }

int junction_count_on_device(void *workspace, const int32_t *d_ref, const int32_t *d_pos, const uint32_t *d_cigar,
                             const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                             const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx, uint32_t m,
                             const uint32_t *d_col, uint32_t n_cols, JunctionCounted *got, uint32_t n_cus, unsigned long long *h_pinned,
                             hipStream_t s)
{
    const JnWs1 w = jn_carve1(workspace, n_reads, m, h_idx != nullptr);
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl, 0, JN_CTL_COUNT * 8, s));
    UMIHIP_TRY_NEG(hipMemsetAsync(w.ctl + JN_BAD_ORDER, 0xFF, 5 * 8, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(w.off, h_off, ((size_t)m + 1) * 8, hipMemcpyHostToDevice, s));
    if (h_idx) UMIHIP_TRY_NEG(hipMemcpyAsync(w.idx, h_idx, (size_t)m * 4, hipMemcpyHostToDevice, s));
    junction_cols_kernel<<<std::min(blocks_for(m, JN_THREADS), n_cus * JN_BLOCKS_PER_CU), JN_THREADS, 0, s>>>(w.idx, d_col, m, n_cols,
                                                                                                            w.bcol, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    const JnReads a{d_ref, d_pos, d_cigar, d_cigar_off, d_read_entry, n_reads, d_kept, d_root, n};
    junction_count_kernel<<<std::min(blocks_for(n_reads, JN_THREADS), n_cus * JN_BLOCKS_PER_CU), JN_THREADS, 0, s>>>(a, w.cnt, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(scan_inclusive_u64(w.cnt, w.incl, n_reads, w.scan_tmp, w.scan_bytes, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, w.ctl, JN_CTL_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned + JN_CTL_COUNT, w.incl + (n_reads - 1), 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    got->bad_cols = h_pinned[JN_BAD_COLS];
    got->bad_kind = 0;
    got->bad_read = ~0ull;
    for (int k = JN_BAD_ORDER; k <= JN_BAD_OPCODE; k++)
        if (h_pinned[k] < got->bad_read) {
            got->bad_read = h_pinned[k];
            got->bad_kind = k;
        }
    got->spliced = h_pinned[JN_SPLICED];
    got->max_ref = h_pinned[JN_MAX_REF];
    got->max_pos = h_pinned[JN_MAX_POS];
    got->occurrences = h_pinned[JN_CTL_COUNT];
    return 0;
}

int junction_fill_on_device(void *workspace1, void *workspace2, const int32_t *d_ref, const int32_t *d_pos, const uint32_t *d_cigar,
                            const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                            const uint32_t *d_root, uint64_t n, uint32_t m, bool has_idx, uint32_t n_cols, const JunctionCounted &got,
                            int32_t *d_jn_ref, int32_t *d_jn_start, int32_t *d_jn_end, uint32_t *d_out_jn, uint32_t *d_out_col,
                            uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t *junctions, uint64_t *nnz, uint32_t n_cus,
                            unsigned long long *h_pinned, hipStream_t s)
{
    const uint32_t t = (uint32_t)got.occurrences; // 1 <= t < 2^30
    const JnWs1 w1 = jn_carve1(workspace1, n_reads, m, has_idx);
    const JnWs2 w = jn_carve2(workspace2, t);
    const int eb = bits_of(got.max_pos), rb = bits_of(got.max_ref), nb = bits_of(n - 1), cb = bits_of((uint64_t)n_cols - 1),
              jb = bits_of((uint64_t)t - 1);
    const uint32_t grid_t = blocks_for(t, JN_THREADS);
    const JnReads a{d_ref, d_pos, d_cigar, d_cigar_off, d_read_entry, n_reads, d_kept, d_root, n};
    junction_fill_kernel<<<std::min(blocks_for(n_reads, JN_THREADS), n_cus * JN_BLOCKS_PER_CU), JN_THREADS, 0, s>>>(
        a, w1.cnt, w1.incl, w1.off, w1.bcol, m, eb, t, w.lo, w.ka, w.va, w.ref, w.mol, w.col);
    UMIHIP_TRY_NEG(hipGetLastError());
    // the junctions in the order of (ref, start, end): the key word, then the ref
    bool in_b = false;
    UMIHIP_TRY_NEG(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, t, 0, 2 * eb, w.radix_tmp, w.radix_bytes, &in_b, s));
    uint64_t *kx = in_b ? w.kb : w.ka, *ky = in_b ? w.ka : w.kb;
    uint32_t *vx = in_b ? w.vb : w.va, *vy = in_b ? w.va : w.vb;
    if (rb) {
        junction_gather_kernel<<<grid_t, JN_THREADS, 0, s>>>(vx, w.ref, t, kx);
        UMIHIP_TRY_NEG(hipGetLastError());
        UMIHIP_TRY_NEG(radix_sort_pairs_u64(kx, ky, vx, vy, t, 0, rb, w.radix_tmp, w.radix_bytes, &in_b, s));
        if (in_b) {
            std::swap(kx, ky);
            std::swap(vx, vy);
        }
    }
    junction_heads_kernel<<<grid_t, JN_THREADS, 0, s>>>(vx, w.lo, w.ref, t, ky);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(scan_inclusive_u64(ky, kx, t, w.scan_tmp, w.scan_bytes, s)); // (the sorted keys have served: the numbers lie over them)
    junction_table_kernel<<<grid_t, JN_THREADS, 0, s>>>(vx, kx, w.lo, w.ref, t, eb, w.jid, d_jn_ref, d_jn_start, d_jn_end, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    // the occurrences in the order of (column, junction, molecule): by molecule, then, stable, by the pair
    junction_molkey_kernel<<<grid_t, JN_THREADS, 0, s>>>(w.mol, t, w.ka, w.va);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(radix_sort_pairs_u64(w.ka, w.kb, w.va, w.vb, t, 0, nb, w.radix_tmp, w.radix_bytes, &in_b, s));
    kx = in_b ? w.kb : w.ka, ky = in_b ? w.ka : w.kb;
    vx = in_b ? w.vb : w.va, vy = in_b ? w.va : w.vb;
    junction_pairkey_kernel<<<grid_t, JN_THREADS, 0, s>>>(vx, w.col, w.jid, t, jb, kx);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(radix_sort_pairs_u64(kx, ky, vx, vy, t, 0, jb + cb, w.radix_tmp, w.radix_bytes, &in_b, s));
    if (in_b) {
        std::swap(kx, ky);
        std::swap(vx, vy);
    }
    uint64_t *incl = w.lo;       // (the key words have served)
    uint32_t *head_pos = w.jid;  // (the numbers are in the pair keys)
    junction_pair_heads_kernel<<<grid_t, JN_THREADS, 0, s>>>(kx, vx, w.mol, t, ky);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(scan_inclusive_u64(ky, incl, t, w.scan_tmp, w.scan_bytes, s));
    junction_pair_slots_kernel<<<grid_t, JN_THREADS, 0, s>>>(kx, incl, t, jb, head_pos, d_out_jn, d_out_col, w.ctl);
    UMIHIP_TRY_NEG(hipGetLastError());
    junction_pair_counts_kernel<<<grid_t, JN_THREADS, 0, s>>>(head_pos, incl, t, w.ctl, d_out_molecules, d_out_reads);
    UMIHIP_TRY_NEG(hipGetLastError());
    UMIHIP_TRY_NEG(hipMemcpyAsync(h_pinned, w.ctl, JN2_COUNT * 8, hipMemcpyDeviceToHost, s));
    UMIHIP_TRY_NEG(hipStreamSynchronize(s));
    *junctions = h_pinned[JN2_JUNCTIONS];
    *nnz = h_pinned[JN2_NNZ];
    return 0;
}

} // namespace umihip
