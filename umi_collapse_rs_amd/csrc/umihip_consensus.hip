// Consensus of the clusters of whole reads (umi_consensus_seqs, fastq mode's --consensus), gfx950.
//
// A cluster is a kept entry r with every entry whose root is r; its members are the reads of those
// entries.  Per column c and base b of ACGT: S_b = sum of max(0, quality byte - 33) over the members
// that show b at c, n_b = their number (N votes for nothing).  The call is the b with the greatest
// (S_b, n_b), the first of ACGT on a tie; quality min(93, max(0, S_win - sum of the other S)); a
// column that nobody voted on is N with quality '!'.  Integer sums throughout, so the order in which
// the members are met does not matter -- which is what lets the reads be grouped by atomic cursors
// and a deep cluster be summed in pieces.
//
// Steps (one stream, two host looks: after the checks, and at the end):
//   entry   per entry: its bucket's length, root[e] kept and in range, the sum of freq
//   count   per read: entry_of_read in range, the read as long as its entry's bucket, cnt[root] += 1
//           (one atomic per distinct cluster among the 64 reads of a wave)
//   offsets per entry: the kept entries' lengths (a kept entry without a read is refused: its
//           consensus would lie beyond what the caller's buffers promise)
//   scans   of cnt (the clusters' ranges in the grouped read list) and of those lengths (cons_off)
//   scatter per read: its place in the cluster's range, from a cursor per cluster
//   vote    one wave per cluster: lane l owns columns 4l .. 4l+3, loads each member's four bases and
//           four quality bytes as one word each and keeps 4 x 4 (S, n) in registers.  A cluster of
//           "cons_split" reads or more only gets an accumulator slot here ...
//   deep    ... its reads are walked in pieces of CONS_CHUNK by all the waves of the grid, the
//           partial (S, n) added to the slot with atomics ...
//   call    ... and its columns are called from the slot by one wave.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_cons_group.h"

namespace umihip {

namespace {

#define CONS_TRY(expr)                              \
    do {                                            \
        const hipError_t e__ = (expr);              \
        if (e__ != hipSuccess) return -(int)e__;    \
    } while (0)

// the control block: what the host looks at
enum ConsCtl : int {
    CC_BAD_ROOT = 0, // entries whose root is out of range or not kept
    CC_BAD_READ = 1, // reads whose entry is out of range
    CC_BAD_LEN = 2,  // reads that are not as long as their entry's bucket
    CC_EMPTY = 3,    // kept entries without a read
    CC_FREQ = 4,     // sum of freq
    CC_DEEP = 5,     // deep clusters met by the vote kernel
    CC_DEEP_OVF = 6, // ... beyond the slots (cannot happen: a deep cluster has at least split reads)
    CC_COUNT = 8,
};

constexpr uint32_t CONS_COLS = UMI_MAX_SEQ_LEN; // columns of an accumulator slot: 4 bases x 256 of (S, n)
constexpr uint32_t CONS_CHUNK = 128;            // reads of a deep cluster one wave sums between two rounds of atomics

struct ConsBufs {
    unsigned long long *ctl;   // [CC_COUNT]
    unsigned long long *cnt;   // [n_entries] reads per cluster (at its kept entry)
    uint32_t *cursor;          // [n_entries]
    uint64_t *incl_reads;      // [n_entries] inclusive scan of cnt
    uint64_t *lenk;            // [n_entries] the bucket's length where kept, else 0
    uint64_t *incl_len;        // [n_entries] inclusive scan of lenk
    uint32_t *elen;            // [n_entries] the bucket's length
    uint32_t *slots;           // [n_reads] reads grouped by cluster
    uint64_t *boff;            // [n_buckets + 1]
    int32_t *blen;             // [n_buckets]
    void *scan_tmp;
    size_t scan_tmp_bytes;
    uint32_t *deep_list;       // [deep_cap] kept entry of a deep cluster
    unsigned long long *acc_s; // [deep_cap][4][CONS_COLS]
    uint32_t *acc_n;           // [deep_cap][4][CONS_COLS]
    size_t zero_bytes, total;
};

ConsBufs cons_carve(void *ws, uint32_t n_reads, uint32_t n_entries, uint32_t n_buckets, uint32_t deep_cap)
{
    ConsBufs b;
    char *p = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = p + off;
        off = (off + bytes + 255) & ~(size_t)255;
        return (void *)q;
    };
    const size_t ne = std::max<size_t>(n_entries, 1), nr = std::max<size_t>(n_reads, 1);
    b.ctl = (unsigned long long *)take(CC_COUNT * 8);
    b.cnt = (unsigned long long *)take(ne * 8);
    b.cursor = (uint32_t *)take(ne * 4);
    b.zero_bytes = off; // (cleared at the start of a call)
    b.incl_reads = (uint64_t *)take(ne * 8);
    b.lenk = (uint64_t *)take(ne * 8);
    b.incl_len = (uint64_t *)take(ne * 8);
    b.elen = (uint32_t *)take(ne * 4);
    b.slots = (uint32_t *)take(nr * 4);
    b.boff = (uint64_t *)take(((size_t)n_buckets + 1) * 8);
    b.blen = (int32_t *)take(std::max<size_t>(n_buckets, 1) * 4);
    b.scan_tmp_bytes = scan_temp_bytes((uint32_t)ne);
    b.scan_tmp = take(b.scan_tmp_bytes);
    b.deep_list = (uint32_t *)take((size_t)deep_cap * 4);
    b.acc_s = (unsigned long long *)take((size_t)deep_cap * 4 * CONS_COLS * 8);
    b.acc_n = (uint32_t *)take((size_t)deep_cap * 4 * CONS_COLS * 4);
    b.total = off;
    return b;
}

__global__ __launch_bounds__(256) void cons_entry_kernel(const uint8_t *__restrict__ kept, const uint32_t *__restrict__ root,
                                                         const int32_t *__restrict__ freq, uint32_t n_entries,
                                                         const uint64_t *__restrict__ boff, const int32_t *__restrict__ blen,
                                                         uint32_t n_buckets, uint32_t *__restrict__ elen,
                                                         unsigned long long *__restrict__ ctl)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    unsigned long long f = 0, bad = 0;
    if (e < n_entries) {
        const uint32_t r = root[e];
        bad = (r >= n_entries || kept[r] == 0) ? 1 : 0;
        f = (unsigned long long)(long long)freq[e];
        uint32_t lo = 0, hi = n_buckets; // the last bucket that starts at or before e
        while (hi - lo > 1) {
            const uint32_t mid = lo + (hi - lo) / 2;
            if (boff[mid] <= e) lo = mid;
            else hi = mid;
        }
        elen[e] = (uint32_t)blen[lo];
    }
    wave_add_to(f, &ctl[CC_FREQ], lane);
    wave_add_to(bad, &ctl[CC_BAD_ROOT], lane);
}

// what both passes over the reads start with: the read's cluster, or why it has none
__device__ __forceinline__ bool cluster_of_read(const uint32_t *__restrict__ eor, const uint32_t *__restrict__ root, uint32_t i,
                                                uint32_t n_reads, uint32_t n_entries, uint32_t &e, uint32_t &r)
{
    e = r = 0;
    if (i >= n_reads) return false;
    e = eor[i];
    if (e >= n_entries) return false;
    r = root[e];
    return r < n_entries; // (a root out of range is the entry pass's finding)
}

__global__ __launch_bounds__(256) void cons_count_kernel(const uint32_t *__restrict__ eor, const uint32_t *__restrict__ root,
                                                         const uint32_t *__restrict__ len, const uint32_t *__restrict__ elen,
                                                         uint32_t n_reads, uint32_t n_entries, unsigned long long *__restrict__ cnt,
                                                         unsigned long long *__restrict__ ctl)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t e, r;
    const bool valid = cluster_of_read(eor, root, i, n_reads, n_entries, e, r);
    const unsigned long long bad_read = (i < n_reads && e >= n_entries) ? 1 : 0;
    const unsigned long long bad_len = (i < n_reads && e < n_entries && len[i] != elen[e]) ? 1 : 0;
    int leader;
    uint32_t rank, c;
    wave_groups(r, valid, lane, leader, rank, c);
    if (valid && leader == lane) atomicAdd(&cnt[r], (unsigned long long)c);
    wave_add_to(bad_read, &ctl[CC_BAD_READ], lane);
    wave_add_to(bad_len, &ctl[CC_BAD_LEN], lane);
}

__global__ __launch_bounds__(256) void cons_offsets_kernel(const uint8_t *__restrict__ kept, const uint32_t *__restrict__ elen,
                                                           const unsigned long long *__restrict__ cnt, uint32_t n_entries,
                                                           uint64_t *__restrict__ lenk, unsigned long long *__restrict__ ctl)
{
    const uint32_t e = blockIdx.x * 256 + threadIdx.x;
    unsigned long long empty = 0;
    if (e < n_entries) {
        const bool k = kept[e] != 0;
        lenk[e] = k ? elen[e] : 0u;
        empty = (k && cnt[e] == 0) ? 1 : 0;
    }
    wave_add_to(empty, &ctl[CC_EMPTY], threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void cons_scatter_kernel(const uint32_t *__restrict__ eor, const uint32_t *__restrict__ root,
                                                           uint32_t n_reads, uint32_t n_entries,
                                                           const unsigned long long *__restrict__ cnt,
                                                           const uint64_t *__restrict__ incl_reads, uint32_t *__restrict__ cursor,
                                                           uint32_t *__restrict__ slots)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    uint32_t e, r;
    const bool valid = cluster_of_read(eor, root, i, n_reads, n_entries, e, r);
    int leader;
    uint32_t rank, c;
    wave_groups(r, valid, lane, leader, rank, c);
    uint32_t base = 0;
    if (valid && leader == lane) base = atomicAdd(&cursor[r], c);
    base = (uint32_t)__shfl((int)base, leader);
    if (valid) {
        const uint64_t at = incl_reads[r] - cnt[r] + base + rank;
        if (at < n_reads) slots[at] = i; // (always: the ranges were counted from the same reads)
    }
}

struct ConsArgs {
    const uint8_t *text;
    const uint64_t *seq_pos, *qual_pos;
    const uint32_t *len;
    const uint32_t *slots;
    const uint8_t *kept;
    const unsigned long long *cnt;
    const uint64_t *incl_reads, *lenk, *incl_len;
    uint32_t n_entries, n_reads;
    uint32_t split, deep_cap;
    uint8_t *cons_seq, *cons_qual;
    uint64_t *cons_off;
    uint32_t *cluster_reads; // may be null
    uint32_t *deep_list;
    unsigned long long *acc_s;
    uint32_t *acc_n;
    unsigned long long *ctl;
};

// (S, n) of a lane's four columns: [column][base of ACGT]
struct Votes {
    uint64_t s[4][4];
    uint32_t n[4][4];
};
__device__ __forceinline__ void votes_clear(Votes &v)
{
#pragma unroll
    for (int j = 0; j < 4; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v.s[j][c] = 0;
            v.n[j][c] = 0;
        }
}
__device__ __forceinline__ uint32_t base_char(int c) { return c == 0 ? 'A' : c == 1 ? 'C' : c == 2 ? 'G' : 'T'; }

__device__ __forceinline__ void vote4(uint32_t bw, uint32_t qw, Votes &v)
{
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const uint32_t b = (bw >> (8 * j)) & 0xFFu, qb = (qw >> (8 * j)) & 0xFFu;
        const uint32_t q = qb > 33u ? qb - 33u : 0u;
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const bool m = b == base_char(c);
            v.s[j][c] += m ? q : 0u;
            v.n[j][c] += m ? 1u : 0u;
        }
    }
}

// The members slots[first .. first + count) of a cluster of length L voted into v.  The lanes fetch
// 64 members' offsets at once; the members are then taken four at a time, their eight words loaded
// before the first is looked at.
__device__ __forceinline__ void accumulate(const ConsArgs &a, uint64_t first, uint32_t count, uint32_t L, int lane, Votes &v)
{
    const uint32_t b0 = 4u * (uint32_t)lane;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t m = base + (uint32_t)lane;
        uint64_t sp = 0, qp = 0;
        uint32_t li = 0;
        if (m < count) {
            const uint32_t i = a.slots[first + m];
            if (i < a.n_reads) {
                sp = a.seq_pos[i];
                qp = a.qual_pos[i];
                li = min(a.len[i], L);
            }
        }
        const uint32_t nb = min(64u, count - base);
        for (uint32_t t = 0; t < nb; t += 4) { // (lanes behind the last member hold length 0)
            uint32_t bw[4], qw[4];
#pragma unroll
            for (int u = 0; u < 4; u++) {
                const int src = (int)t + u;
                const uint64_t s = shfl64(sp, src), q = shfl64(qp, src);
                const uint32_t l = (uint32_t)__shfl((int)li, src);
                bw[u] = 0x4E4E4E4Eu; // N: no vote
                qw[u] = 0x21212121u;
                if (b0 < l) {
                    bw[u] = text4(a.text, s + b0, s + l, 0x4E4E4E4Eu);
                    qw[u] = text4(a.text, q + b0, q + l, 0x21212121u);
                }
            }
#pragma unroll
            for (int u = 0; u < 4; u++) vote4(bw[u], qw[u], v);
        }
    }
}

// a lane's four columns called and written at off + 4 lane (a word where it is whole and aligned)
__device__ __forceinline__ void call_store(const ConsArgs &a, uint64_t off, uint32_t L, int lane, const Votes &v)
{
    const uint32_t b0 = 4u * (uint32_t)lane;
    if (b0 >= L) return;
    uint32_t sw = 0, qw = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        uint64_t best_s = v.s[j][0], tot = v.s[j][0];
        uint32_t best_n = v.n[j][0], ch = base_char(0);
#pragma unroll
        for (int c = 1; c < 4; c++) {
            const bool better = v.s[j][c] > best_s || (v.s[j][c] == best_s && v.n[j][c] > best_n);
            best_s = better ? v.s[j][c] : best_s;
            best_n = better ? v.n[j][c] : best_n;
            ch = better ? base_char(c) : ch;
            tot += v.s[j][c];
        }
        uint32_t qc = '!';
        if (best_n == 0) {
            ch = 'N';
        } else {
            const uint64_t rest = tot - best_s;
            const uint64_t q = best_s > rest ? best_s - rest : 0ull;
            qc = 33u + (uint32_t)(q < 93ull ? q : 93ull);
        }
        sw |= ch << (8 * j);
        qw |= qc << (8 * j);
    }
    const uint32_t nbytes = min(4u, L - b0);
    uint8_t *ps = a.cons_seq + off + b0, *pq = a.cons_qual + off + b0;
    if (nbytes == 4 && ((uintptr_t)ps & 3) == 0) {
        *(uint32_t *)ps = sw;
    } else {
        for (uint32_t j = 0; j < nbytes; j++) ps[j] = (uint8_t)(sw >> (8 * j));
    }
    if (nbytes == 4 && ((uintptr_t)pq & 3) == 0) {
        *(uint32_t *)pq = qw;
    } else {
        for (uint32_t j = 0; j < nbytes; j++) pq[j] = (uint8_t)(qw >> (8 * j));
    }
}

// One wave per cluster.  Wave w of W looks at the entries w, w + W, w + 2 W, ... (the entries of a bucket
// are in freq-descending order, so neighbours are equally heavy: they go to different waves), 64 of
// them at a time -- one per lane -- and then works off the kept ones among them.
__global__ __launch_bounds__(256) void cons_vote_kernel(ConsArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    for (uint64_t tile = 0; tile * 64 * GW + gw < a.n_entries; tile++) {
        const uint64_t el = (tile * 64 + (uint64_t)lane) * GW + gw;
        uint64_t cnt_l = 0, len_l = 0, off_l = 0, first_l = 0;
        const bool k = el < a.n_entries && a.kept[el] != 0;
        if (k) {
            cnt_l = a.cnt[el];
            len_l = a.lenk[el];
            off_l = a.incl_len[el] - len_l;
            first_l = a.incl_reads[el] - cnt_l;
            a.cons_off[el] = off_l;
            if (a.cluster_reads) a.cluster_reads[el] = (uint32_t)cnt_l;
        }
        unsigned long long todo = __ballot(k);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t cnt = shfl64(cnt_l, t), off = shfl64(off_l, t), first = shfl64(first_l, t);
            const uint32_t L = (uint32_t)__shfl((int)(uint32_t)len_l, t);
            const uint32_t e = (uint32_t)shfl64(el, t);
            if (cnt >= a.split) { // a deep cluster: a cleared accumulator slot, the rest is the deep kernels'
                unsigned long long d = 0;
                if (lane == 0) d = atomicAdd(&a.ctl[CC_DEEP], 1ull);
                d = shfl64(d, 0);
                if (d >= a.deep_cap) {
                    if (lane == 0) atomicAdd(&a.ctl[CC_DEEP_OVF], 1ull);
                    continue;
                }
                if (lane == 0) a.deep_list[d] = e;
                unsigned long long *ps = a.acc_s + d * 4 * CONS_COLS;
                uint32_t *pn = a.acc_n + d * 4 * CONS_COLS;
                for (uint32_t x = (uint32_t)lane; x < 4 * CONS_COLS; x += 64) {
                    ps[x] = 0;
                    pn[x] = 0;
                }
                continue;
            }
            Votes v;
            votes_clear(v);
            accumulate(a, first, (uint32_t)cnt, L, lane, v);
            call_store(a, off, L, lane, v);
        }
    }
}

// The deep clusters' reads in pieces of CONS_CHUNK: piece c of deep cluster d is wave (d + c) mod W's, so
// that one huge cluster is spread over the grid and many small ones are too.  The lanes look at 64
// deep clusters at a time and the wave works off those it has a piece of.
__global__ __launch_bounds__(256) void cons_deep_kernel(ConsArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    const uint64_t n_deep = a.ctl[CC_DEEP] < a.deep_cap ? (uint64_t)a.ctl[CC_DEEP] : (uint64_t)a.deep_cap;
    const uint32_t b0 = 4u * (uint32_t)lane;
    for (uint64_t dbase = 0; dbase < n_deep; dbase += 64) {
        const uint64_t dl = dbase + (uint64_t)lane;
        uint64_t cnt_l = 0, first_l = 0, c0_l = 0;
        uint32_t len_l = 0;
        bool has = false;
        if (dl < n_deep) {
            const uint32_t e = a.deep_list[dl];
            cnt_l = a.cnt[e];
            len_l = (uint32_t)a.lenk[e];
            first_l = a.incl_reads[e] - cnt_l;
            c0_l = (gw + GW - dl % GW) % GW;
            has = c0_l < (cnt_l + CONS_CHUNK - 1) / CONS_CHUNK;
        }
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t d = dbase + (uint64_t)t, cnt = shfl64(cnt_l, t), first = shfl64(first_l, t);
            const uint32_t L = (uint32_t)__shfl((int)len_l, t);
            const uint64_t n_chunks = (cnt + CONS_CHUNK - 1) / CONS_CHUNK;
            for (uint64_t c = shfl64(c0_l, t); c < n_chunks; c += GW) {
                const uint64_t m0 = c * CONS_CHUNK;
                Votes v;
                votes_clear(v);
                accumulate(a, first + m0, (uint32_t)(cnt - m0 < CONS_CHUNK ? cnt - m0 : CONS_CHUNK), L, lane, v);
                unsigned long long *ps = a.acc_s + d * 4 * CONS_COLS;
                uint32_t *pn = a.acc_n + d * 4 * CONS_COLS;
#pragma unroll
                for (int j = 0; j < 4; j++)
#pragma unroll
                    for (int cc = 0; cc < 4; cc++)
                        if (v.n[j][cc]) {
                            atomicAdd(&ps[cc * CONS_COLS + b0 + j], (unsigned long long)v.s[j][cc]);
                            atomicAdd(&pn[cc * CONS_COLS + b0 + j], v.n[j][cc]);
                        }
            }
        }
    }
}

__global__ __launch_bounds__(256) void cons_deep_call_kernel(ConsArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    const uint64_t n_deep = a.ctl[CC_DEEP] < a.deep_cap ? (uint64_t)a.ctl[CC_DEEP] : (uint64_t)a.deep_cap;
    const uint32_t b0 = 4u * (uint32_t)lane;
    for (uint64_t d = gw; d < n_deep; d += GW) {
        const uint32_t e = a.deep_list[d];
        const uint32_t L = (uint32_t)a.lenk[e];
        const uint64_t off = a.incl_len[e] - L;
        const unsigned long long *ps = a.acc_s + d * 4 * CONS_COLS;
        const uint32_t *pn = a.acc_n + d * 4 * CONS_COLS;
        Votes v;
#pragma unroll
        for (int j = 0; j < 4; j++)
#pragma unroll
            for (int cc = 0; cc < 4; cc++) {
                v.s[j][cc] = ps[cc * CONS_COLS + b0 + j];
                v.n[j][cc] = pn[cc * CONS_COLS + b0 + j];
            }
        call_store(a, off, L, lane, v);
    }
}

inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

} // namespace

// Clusters of at least this many reads take the deep path: the option, raised where the accumulator
// slots (12 KB per deep cluster, at most n_reads / split of them) would pass CONS_ACC_BUDGET.
constexpr uint64_t CONS_ACC_BUDGET = 512ull << 20;
uint32_t consensus_effective_split(uint32_t n_reads, uint32_t split)
{
    const uint64_t slot = (uint64_t)4 * CONS_COLS * 12;
    const uint64_t floor_ = ((uint64_t)n_reads * slot + CONS_ACC_BUDGET - 1) / CONS_ACC_BUDGET;
    return (uint32_t)std::max<uint64_t>(std::max<uint64_t>(split, 2), floor_);
}
static uint32_t cons_deep_cap(uint32_t n_reads, uint32_t eff_split) { return n_reads / eff_split + 1; }

size_t consensus_workspace_bytes(uint32_t n_reads, uint32_t n_entries, uint32_t n_buckets, uint32_t split)
{
    return cons_carve(nullptr, n_reads, n_entries, n_buckets, cons_deep_cap(n_reads, consensus_effective_split(n_reads, split)))
        .total;
}

int consensus_on_device(void *workspace, const uint8_t *d_text, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                        const uint32_t *d_len, uint32_t n_reads, const uint32_t *d_eor, const int32_t *d_freq,
                        const uint8_t *d_kept, const uint32_t *d_root, uint32_t n_entries, const uint64_t *h_bucket_off,
                        const int32_t *h_bucket_len, uint32_t n_buckets, uint32_t split, uint32_t n_cus, uint8_t *d_cons_seq,
                        uint8_t *d_cons_qual, uint64_t *d_cons_off, uint32_t *d_cluster_reads, uint64_t *cons_bytes,
                        ConsFault *fault, unsigned long long *h_pinned, hipStream_t s)
{
    const uint32_t eff_split = consensus_effective_split(n_reads, split);
    const uint32_t deep_cap = cons_deep_cap(n_reads, eff_split);
    ConsBufs b = cons_carve(workspace, n_reads, n_entries, n_buckets, deep_cap);
    CONS_TRY(hipMemsetAsync(workspace, 0, b.zero_bytes, s));
    CONS_TRY(hipMemcpyAsync(b.boff, h_bucket_off, ((size_t)n_buckets + 1) * 8, hipMemcpyHostToDevice, s));
    CONS_TRY(hipMemcpyAsync(b.blen, h_bucket_len, (size_t)n_buckets * 4, hipMemcpyHostToDevice, s));
    cons_entry_kernel<<<blocks_for(n_entries, 256), 256, 0, s>>>(d_kept, d_root, d_freq, n_entries, b.boff, b.blen, n_buckets,
                                                                  b.elen, b.ctl);
    if (n_reads)
        cons_count_kernel<<<blocks_for(n_reads, 256), 256, 0, s>>>(d_eor, d_root, d_len, b.elen, n_reads, n_entries, b.cnt,
                                                                    b.ctl);
    cons_offsets_kernel<<<blocks_for(n_entries, 256), 256, 0, s>>>(d_kept, b.elen, b.cnt, n_entries, b.lenk, b.ctl);
    CONS_TRY(hipGetLastError());
    CONS_TRY(scan_inclusive_u64((const uint64_t *)b.cnt, b.incl_reads, n_entries, b.scan_tmp, b.scan_tmp_bytes, s));
    CONS_TRY(scan_inclusive_u64(b.lenk, b.incl_len, n_entries, b.scan_tmp, b.scan_tmp_bytes, s));
    CONS_TRY(hipMemcpyAsync(h_pinned, b.ctl, CC_COUNT * 8, hipMemcpyDeviceToHost, s));
    CONS_TRY(hipMemcpyAsync(h_pinned + CC_COUNT, b.incl_len + (n_entries - 1), 8, hipMemcpyDeviceToHost, s));
    CONS_TRY(hipStreamSynchronize(s));
    fault->bad_root = h_pinned[CC_BAD_ROOT];
    fault->bad_read = h_pinned[CC_BAD_READ];
    fault->bad_len = h_pinned[CC_BAD_LEN];
    fault->empty = h_pinned[CC_EMPTY];
    fault->freq_sum = h_pinned[CC_FREQ];
    if (fault->bad_root || fault->bad_read || fault->bad_len || fault->empty || fault->freq_sum != n_reads) return 1;
    *cons_bytes = h_pinned[CC_COUNT];

    ConsArgs a;
    a.text = d_text;
    a.seq_pos = d_seq_pos;
    a.qual_pos = d_qual_pos;
    a.len = d_len;
    a.slots = b.slots;
    a.kept = d_kept;
    a.cnt = b.cnt;
    a.incl_reads = b.incl_reads;
    a.lenk = b.lenk;
    a.incl_len = b.incl_len;
    a.n_entries = n_entries;
    a.n_reads = n_reads;
    a.split = eff_split;
    a.deep_cap = deep_cap;
    a.cons_seq = d_cons_seq;
    a.cons_qual = d_cons_qual;
    a.cons_off = d_cons_off;
    a.cluster_reads = d_cluster_reads;
    a.deep_list = b.deep_list;
    a.acc_s = b.acc_s;
    a.acc_n = b.acc_n;
    a.ctl = b.ctl;
    if (n_reads)
        cons_scatter_kernel<<<blocks_for(n_reads, 256), 256, 0, s>>>(d_eor, d_root, n_reads, n_entries, b.cnt, b.incl_reads,
                                                                      b.cursor, b.slots);
    // every wave resident at once (8 blocks of 4 per CU), fewer where there are fewer clusters
    const uint32_t grid = std::max(1u, std::min(blocks_for(n_entries, 4), n_cus * 8));
    cons_vote_kernel<<<grid, 256, 0, s>>>(a);
    // (both return at once where the vote kernel met no deep cluster; no host look in between)
    if (n_reads >= eff_split) {
        cons_deep_kernel<<<n_cus * 8, 256, 0, s>>>(a);
        cons_deep_call_kernel<<<std::max(1u, std::min(blocks_for(deep_cap, 4), n_cus * 8)), 256, 0, s>>>(a);
    }
    CONS_TRY(hipGetLastError());
    CONS_TRY(hipMemcpyAsync(h_pinned, b.ctl, CC_COUNT * 8, hipMemcpyDeviceToHost, s));
    CONS_TRY(hipStreamSynchronize(s));
    if (h_pinned[CC_DEEP_OVF]) return -(int)hipErrorAssert; // (a deep cluster without a slot: a bug, not an input)
    return 0;
}

#undef CONS_TRY

} // namespace umihip
