// Consensus of the clusters of aligned reads (umi_consensus_bam, BAM mode's --call-consensus), gfx950.
//
// The caller says which reads vote where: cluster[i] in [0, n_clusters), or UMI_NO_CLUSTER.  A voter of
// cluster c is cluster_len[c] bases long, packed two per byte (high nibble first) at data + seq_pos[i],
// with as many raw Phred bytes at data + qual_pos[i]; no offset is aligned.  Per column and base b of
// ACGT (nibble 1, 2, 4, 8; every other nibble votes for nothing): S_b = sum of min(quality, 93) over the
// voters that show b, n_b = their number.  The call is the b with the greatest (S_b, n_b), the first of
// ACGT on a tie; quality min(93, max(0, S_win - sum of the other S)); a column nobody voted on is nibble
// 15 with quality 0.  Integer sums, so the order in which the voters are met does not matter.
//
// Steps (one stream, two host looks: after the checks, and at the end) -- those of umihip_consensus.hip,
// the clusters being given instead of derived from entries and roots:
//   lens    per cluster: cluster_len within UMI_MAX_CONS_LEN, its bytes of sequence and of quality
//   count   per read: the cluster id in range, the read as long as its cluster, cnt[c] += 1
//   scans   of cnt (the clusters' ranges in the grouped voter list) and of the two byte counts
//   scatter per voter: its place in the cluster's range, from a cursor per cluster
//   vote    one wave per cluster, in passes of 512 columns: lane l owns columns 8l .. 8l+7 of the pass,
//           loads each voter's eight nibbles as one word and its eight quality bytes as two, and keeps
//           8 x 4 (S, n) in 32-bit registers (a one-wave cluster has fewer than 2^24 voters).  A cluster
//           of "cons_split" voters or more only gets an accumulator slot here ...
//   deep    ... its voters are walked in pieces of CONSB_CHUNK by all the waves of the grid, the partial
//           (S, n) added to the slot with atomics (S in 64 bits) ...
//   call    ... and its columns are called from the slot by one wave.
#include <hip/hip_runtime.h>
#include <algorithm>

#include "../../include/umihip.h"
#include "umihip_internal.h"
#include "umihip_cons_group.h"

namespace umihip {

namespace {

#define CONSB_TRY(expr)                             \
    do {                                            \
        const hipError_t e__ = (expr);              \
        if (e__ != hipSuccess) return -(int)e__;    \
    } while (0)

// the control block: what the host looks at
enum ConsBamCtl : int {
    CB_BAD_CLEN = 0, // clusters longer than UMI_MAX_CONS_LEN
    CB_BAD_ID = 1,   // reads whose cluster is neither in range nor UMI_NO_CLUSTER
    CB_BAD_LEN = 2,  // voters that are not as long as their cluster
    CB_DEEP = 3,     // deep clusters met by the vote kernel
    CB_DEEP_OVF = 4, // ... beyond the slots (cannot happen: a deep cluster has at least split voters)
    CB_COUNT = 8,
};

constexpr uint32_t CONSB_COLS = UMI_MAX_CONS_LEN; // columns of an accumulator slot: 4 bases x 1024 of (S, n)
constexpr uint32_t CONSB_PASS = 512;              // columns of a pass: 8 per lane
constexpr uint32_t CONSB_CHUNK = 128;             // voters of a deep cluster one wave sums between two rounds of atomics
constexpr int CONSB_FLIGHT = 4;                   // voters whose words are loaded before the first is looked at
constexpr uint32_t CONSB_ONE_WAVE_MAX = 1u << 24; // voters one wave sums in 32 bits: 2^24 x 93 < 2^32

struct ConsBamBufs {
    unsigned long long *ctl;   // [CB_COUNT]
    unsigned long long *cnt;   // [n_clusters] voters per cluster
    uint32_t *cursor;          // [n_clusters]
    uint64_t *incl_reads;      // [n_clusters] inclusive scan of cnt
    uint64_t *seqk, *qualk;    // [n_clusters] bytes of packed sequence / of quality
    uint64_t *incl_seq, *incl_qual;
    uint32_t *slots;           // [n_reads] voters grouped by cluster
    void *scan_tmp;
    size_t scan_tmp_bytes;
    uint32_t *deep_list;       // [deep_cap] cluster of a deep slot
    unsigned long long *acc_s; // [deep_cap][4][CONSB_COLS]
    uint32_t *acc_n;           // [deep_cap][4][CONSB_COLS]
    size_t zero_bytes, total;
};

ConsBamBufs consb_carve(void *ws, uint32_t n_reads, uint32_t n_clusters, uint32_t deep_cap)
{
    ConsBamBufs b;
    char *p = (char *)ws;
    size_t off = 0;
    auto take = [&](size_t bytes) {
        char *q = p + off;
        off = (off + bytes + 255) & ~(size_t)255;
        return (void *)q;
    };
    const size_t nc = std::max<size_t>(n_clusters, 1), nr = std::max<size_t>(n_reads, 1);
    b.ctl = (unsigned long long *)take(CB_COUNT * 8);
    b.cnt = (unsigned long long *)take(nc * 8);
    b.cursor = (uint32_t *)take(nc * 4);
    b.zero_bytes = off; // (cleared at the start of a call)
    b.incl_reads = (uint64_t *)take(nc * 8);
    b.seqk = (uint64_t *)take(nc * 8);
    b.qualk = (uint64_t *)take(nc * 8);
    b.incl_seq = (uint64_t *)take(nc * 8);
    b.incl_qual = (uint64_t *)take(nc * 8);
    b.slots = (uint32_t *)take(nr * 4);
    b.scan_tmp_bytes = scan_temp_bytes((uint32_t)nc);
    b.scan_tmp = take(b.scan_tmp_bytes);
    b.deep_list = (uint32_t *)take((size_t)deep_cap * 4);
    b.acc_s = (unsigned long long *)take((size_t)deep_cap * 4 * CONSB_COLS * 8);
    b.acc_n = (uint32_t *)take((size_t)deep_cap * 4 * CONSB_COLS * 4);
    b.total = off;
    return b;
}

__global__ __launch_bounds__(256) void consb_lens_kernel(const uint32_t *__restrict__ cluster_len, uint32_t n_clusters,
                                                         uint64_t *__restrict__ seqk, uint64_t *__restrict__ qualk,
                                                         unsigned long long *__restrict__ ctl)
{
    const uint32_t c = blockIdx.x * 256 + threadIdx.x;
    unsigned long long bad = 0;
    if (c < n_clusters) {
        const uint32_t L = cluster_len[c];
        bad = L > UMI_MAX_CONS_LEN ? 1 : 0;
        seqk[c] = bad ? 0u : (L + 1) / 2;
        qualk[c] = bad ? 0u : L;
    }
    wave_add_to(bad, &ctl[CB_BAD_CLEN], threadIdx.x & 63);
}

__global__ __launch_bounds__(256) void consb_count_kernel(const uint32_t *__restrict__ cluster, const uint32_t *__restrict__ len,
                                                          const uint32_t *__restrict__ cluster_len, uint32_t n_reads,
                                                          uint32_t n_clusters, unsigned long long *__restrict__ cnt,
                                                          unsigned long long *__restrict__ ctl)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t c = i < n_reads ? cluster[i] : UMI_NO_CLUSTER;
    const bool valid = c < n_clusters;
    const unsigned long long bad_id = (c != UMI_NO_CLUSTER && !valid) ? 1 : 0;
    const unsigned long long bad_len = (valid && len[i] != cluster_len[c]) ? 1 : 0;
    int leader;
    uint32_t rank, k;
    wave_groups(c, valid, lane, leader, rank, k);
    if (valid && leader == lane) atomicAdd(&cnt[c], (unsigned long long)k);
    wave_add_to(bad_id, &ctl[CB_BAD_ID], lane);
    wave_add_to(bad_len, &ctl[CB_BAD_LEN], lane);
}

__global__ __launch_bounds__(256) void consb_scatter_kernel(const uint32_t *__restrict__ cluster, uint32_t n_reads,
                                                            uint32_t n_clusters, const unsigned long long *__restrict__ cnt,
                                                            const uint64_t *__restrict__ incl_reads,
                                                            uint32_t *__restrict__ cursor, uint32_t *__restrict__ slots)
{
    const uint32_t i = blockIdx.x * 256 + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const uint32_t c = i < n_reads ? cluster[i] : UMI_NO_CLUSTER;
    const bool valid = c < n_clusters;
    int leader;
    uint32_t rank, k;
    wave_groups(c, valid, lane, leader, rank, k);
    uint32_t base = 0;
    if (valid && leader == lane) base = atomicAdd(&cursor[c], k);
    base = (uint32_t)__shfl((int)base, leader);
    if (valid) {
        const uint64_t at = incl_reads[c] - cnt[c] + base + rank;
        if (at < n_reads) slots[at] = i; // (always: the ranges were counted from the same reads)
    }
}

struct ConsBamArgs {
    const uint8_t *data;
    const uint64_t *seq_pos, *qual_pos;
    const uint32_t *len;
    const uint32_t *slots;
    const uint32_t *cluster_len;
    const unsigned long long *cnt;
    const uint64_t *incl_reads, *incl_seq, *incl_qual;
    uint32_t n_clusters, n_reads;
    uint32_t split, deep_cap;
    uint8_t *cons_seq, *cons_qual;
    uint64_t *seq_off, *qual_off;
    uint32_t *depth, *disagree; // disagree may be null
    uint32_t *deep_list;
    unsigned long long *acc_s;
    uint32_t *acc_n;
    unsigned long long *ctl;
};

// (S, n) of a lane's eight columns: [column][base of ACGT]; S in 32 bits while summing, 64 from a slot
template <class S> struct VotesB {
    S s[8][4];
    uint32_t n[8][4];
};
template <class S> __device__ __forceinline__ void votes_clear(VotesB<S> &v)
{
#pragma unroll
    for (int j = 0; j < 8; j++)
#pragma unroll
        for (int c = 0; c < 4; c++) {
            v.s[j][c] = 0;
            v.n[j][c] = 0;
        }
}

// eight columns of one voter: sw its nibbles (column j the high nibble of byte j / 2 where j is even),
// q0 / q1 its quality bytes
__device__ __forceinline__ void vote8(uint32_t sw, uint32_t q0, uint32_t q1, VotesB<uint32_t> &v)
{
#pragma unroll
    for (int j = 0; j < 8; j++) {
        const uint32_t nib = (sw >> (8 * (j >> 1) + ((j & 1) ? 0 : 4))) & 0xFu;
        const uint32_t w = min(((j < 4 ? q0 : q1) >> (8 * (j & 3))) & 0xFFu, 93u);
#pragma unroll
        for (int c = 0; c < 4; c++) {
            const bool m = nib == (1u << c);
            v.s[j][c] += m ? w : 0u;
            v.n[j][c] += m ? 1u : 0u;
        }
    }
}

// the nibbles of a word that are columns below nvalid (of the eight a lane owns)
__device__ __forceinline__ uint32_t nibble_mask(uint32_t nvalid)
{
    if (nvalid >= 8) return 0xFFFFFFFFu;
    const uint32_t whole = nvalid >> 1;
    return ((1u << (8 * whole)) - 1u) | ((nvalid & 1) ? (0xF0u << (8 * whole)) : 0u);
}

// The voters slots[first .. first + count) of a cluster of length L voted into v for the pass that starts
// at column c_base.  The lanes fetch 64 voters' offsets at once; the voters are then taken CONSB_FLIGHT at a
// time, their words loaded before the first is looked at.
__device__ __forceinline__ void accumulate(const ConsBamArgs &a, uint64_t first, uint32_t count, uint32_t L, uint32_t c_base,
                                           int lane, VotesB<uint32_t> &v)
{
    const uint32_t c0 = c_base + 8u * (uint32_t)lane;
    const bool mine = c0 < L;
    const uint32_t keep = mine ? nibble_mask(L - c0) : 0u;
    const uint32_t sbytes = (L + 1) / 2;
    for (uint32_t base = 0; base < count; base += 64) {
        const uint32_t m = base + (uint32_t)lane;
        uint64_t sp = 0, qp = 0;
        uint32_t ok = 0;
        if (m < count) {
            const uint32_t i = a.slots[first + m];
            if (i < a.n_reads && a.len[i] == L) { // (always: the count kernel refused any other)
                sp = a.seq_pos[i];
                qp = a.qual_pos[i];
                ok = 1;
            }
        }
        const uint32_t nb = min(64u, count - base);
        for (uint32_t t = 0; t < nb; t += CONSB_FLIGHT) { // (lanes behind the last voter hold ok = 0)
            uint32_t sw[CONSB_FLIGHT], q0[CONSB_FLIGHT], q1[CONSB_FLIGHT];
#pragma unroll
            for (int u = 0; u < CONSB_FLIGHT; u++) {
                const int src = (int)t + u;
                const uint64_t s = shfl64(sp, src), q = shfl64(qp, src);
                const uint32_t o = (uint32_t)__shfl((int)ok, src);
                sw[u] = q0[u] = q1[u] = 0u; // nibble 0: no vote
                if (mine && o) {
                    sw[u] = text4(a.data, s + c0 / 2, s + sbytes, 0u) & keep;
                    q0[u] = text4(a.data, q + c0, q + L, 0u);
                    if (c0 + 4 < L) q1[u] = text4(a.data, q + c0 + 4, q + L, 0u);
                }
            }
#pragma unroll
            for (int u = 0; u < CONSB_FLIGHT; u++) vote8(sw[u], q0[u], q1[u], v);
        }
    }
}

// A lane's eight columns of the pass at c_base called and written: four bytes of sequence at
// soff + (c_base + 8 lane) / 2, eight of quality at qoff + c_base + 8 lane (words where they are whole and
// aligned).  Returns the base votes of these columns that lost.
template <class S>
__device__ __forceinline__ uint32_t call_store(const ConsBamArgs &a, uint64_t soff, uint64_t qoff, uint32_t L, uint32_t c_base,
                                               int lane, const VotesB<S> &v)
{
    const uint32_t c0 = c_base + 8u * (uint32_t)lane;
    if (c0 >= L) return 0;
    uint32_t sw = 0, qw[2] = {0, 0}, lost = 0;
#pragma unroll
    for (int j = 0; j < 8; j++) {
        S best_s = v.s[j][0];
        uint64_t tot = v.s[j][0];
        uint32_t best_n = v.n[j][0], nib = 1u, voted = v.n[j][0];
#pragma unroll
        for (int c = 1; c < 4; c++) {
            const bool better = v.s[j][c] > best_s || (v.s[j][c] == best_s && v.n[j][c] > best_n);
            best_s = better ? v.s[j][c] : best_s;
            best_n = better ? v.n[j][c] : best_n;
            nib = better ? (1u << c) : nib;
            tot += v.s[j][c];
            voted += v.n[j][c];
        }
        uint32_t qc = 0;
        if (best_n == 0) {
            nib = 15u;
        } else {
            const uint64_t rest = tot - (uint64_t)best_s;
            const uint64_t q = (uint64_t)best_s > rest ? (uint64_t)best_s - rest : 0ull;
            qc = (uint32_t)(q < 93ull ? q : 93ull);
        }
        if (c0 + (uint32_t)j >= L) { // (behind the read: the padding nibble of an odd length is 0)
            nib = 0u;
            qc = 0u;
        } else {
            lost += voted - best_n;
        }
        sw |= nib << (8 * (j >> 1) + ((j & 1) ? 0 : 4));
        qw[j >> 2] |= qc << (8 * (j & 3));
    }
    const uint32_t ns = min(4u, (L + 1) / 2 - c0 / 2), nq = min(8u, L - c0);
    uint8_t *ps = a.cons_seq + soff + c0 / 2, *pq = a.cons_qual + qoff + c0;
    if (ns == 4 && ((uintptr_t)ps & 3) == 0) {
        *(uint32_t *)ps = sw;
    } else {
        for (uint32_t j = 0; j < ns; j++) ps[j] = (uint8_t)(sw >> (8 * j));
    }
    if (nq == 8 && ((uintptr_t)pq & 3) == 0) {
        *(uint32_t *)pq = qw[0];
        *(uint32_t *)(pq + 4) = qw[1];
    } else {
        for (uint32_t j = 0; j < nq; j++) pq[j] = (uint8_t)(qw[j >> 2] >> (8 * (j & 3)));
    }
    return lost;
}

__device__ __forceinline__ uint32_t wave_sum(uint32_t v, int lane)
{
    for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl((int)v, lane ^ o);
    return v;
}

// One wave per cluster.  Wave w of W looks at the clusters w, w + W, w + 2 W, ..., 64 of them at a time --
// one per lane -- and then works them off.
__global__ __launch_bounds__(256) void consb_vote_kernel(ConsBamArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    for (uint64_t tile = 0; tile * 64 * GW + gw < a.n_clusters; tile++) {
        const uint64_t cl = (tile * 64 + (uint64_t)lane) * GW + gw;
        uint64_t cnt_l = 0, soff_l = 0, qoff_l = 0, first_l = 0;
        uint32_t len_l = 0;
        const bool k = cl < a.n_clusters;
        if (k) {
            cnt_l = a.cnt[cl];
            len_l = a.cluster_len[cl];
            soff_l = a.incl_seq[cl] - (len_l + 1) / 2;
            qoff_l = a.incl_qual[cl] - len_l;
            first_l = a.incl_reads[cl] - cnt_l;
            a.seq_off[cl] = soff_l;
            a.qual_off[cl] = qoff_l;
            a.depth[cl] = (uint32_t)cnt_l;
        }
        unsigned long long todo = __ballot(k);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t cnt = shfl64(cnt_l, t), soff = shfl64(soff_l, t), qoff = shfl64(qoff_l, t), first = shfl64(first_l, t);
            const uint32_t L = (uint32_t)__shfl((int)len_l, t);
            const uint32_t c = (uint32_t)shfl64(cl, t);
            if (cnt >= a.split) { // a deep cluster: a cleared accumulator slot, the rest is the deep kernels'
                unsigned long long d = 0;
                if (lane == 0) d = atomicAdd(&a.ctl[CB_DEEP], 1ull);
                d = shfl64(d, 0);
                if (d >= a.deep_cap) {
                    if (lane == 0) atomicAdd(&a.ctl[CB_DEEP_OVF], 1ull);
                    continue;
                }
                if (lane == 0) a.deep_list[d] = c;
                unsigned long long *ps = a.acc_s + d * 4 * CONSB_COLS;
                uint32_t *pn = a.acc_n + d * 4 * CONSB_COLS;
                for (uint32_t x = (uint32_t)lane; x < 4 * CONSB_COLS; x += 64) {
                    ps[x] = 0;
                    pn[x] = 0;
                }
                continue;
            }
            uint32_t lost = 0;
            for (uint32_t c_base = 0; c_base < L; c_base += CONSB_PASS) {
                VotesB<uint32_t> v;
                votes_clear(v);
                accumulate(a, first, (uint32_t)cnt, L, c_base, lane, v);
                lost += call_store(a, soff, qoff, L, c_base, lane, v);
            }
            if (a.disagree) {
                lost = wave_sum(lost, lane);
                if (lane == 0) a.disagree[c] = lost;
            }
        }
    }
}

// The deep clusters' voters in pieces of CONSB_CHUNK: piece p of deep cluster d is wave (d + p) mod W's, so
// that one huge cluster is spread over the grid and many small ones are too.  The lanes look at 64 deep
// clusters at a time and the wave works off those it has a piece of.
__global__ __launch_bounds__(256) void consb_deep_kernel(ConsBamArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    const uint64_t n_deep = a.ctl[CB_DEEP] < a.deep_cap ? (uint64_t)a.ctl[CB_DEEP] : (uint64_t)a.deep_cap;
    for (uint64_t dbase = 0; dbase < n_deep; dbase += 64) {
        const uint64_t dl = dbase + (uint64_t)lane;
        uint64_t cnt_l = 0, first_l = 0, p0_l = 0;
        uint32_t len_l = 0;
        bool has = false;
        if (dl < n_deep) {
            const uint32_t c = a.deep_list[dl];
            cnt_l = a.cnt[c];
            len_l = a.cluster_len[c];
            first_l = a.incl_reads[c] - cnt_l;
            p0_l = (gw + GW - dl % GW) % GW;
            has = p0_l < (cnt_l + CONSB_CHUNK - 1) / CONSB_CHUNK;
        }
        unsigned long long todo = __ballot(has);
        while (todo) {
            const int t = __builtin_ctzll(todo);
            todo &= todo - 1;
            const uint64_t d = dbase + (uint64_t)t, cnt = shfl64(cnt_l, t), first = shfl64(first_l, t);
            const uint32_t L = (uint32_t)__shfl((int)len_l, t);
            const uint64_t n_pieces = (cnt + CONSB_CHUNK - 1) / CONSB_CHUNK;
            unsigned long long *ps = a.acc_s + d * 4 * CONSB_COLS;
            uint32_t *pn = a.acc_n + d * 4 * CONSB_COLS;
            for (uint64_t p = shfl64(p0_l, t); p < n_pieces; p += GW) {
                const uint64_t m0 = p * CONSB_CHUNK;
                const uint32_t count = (uint32_t)(cnt - m0 < CONSB_CHUNK ? cnt - m0 : CONSB_CHUNK);
                for (uint32_t c_base = 0; c_base < L; c_base += CONSB_PASS) {
                    const uint32_t c0 = c_base + 8u * (uint32_t)lane;
                    VotesB<uint32_t> v;
                    votes_clear(v);
                    accumulate(a, first + m0, count, L, c_base, lane, v);
#pragma unroll
                    for (int j = 0; j < 8; j++)
#pragma unroll
                        for (int cc = 0; cc < 4; cc++)
                            if (v.n[j][cc]) { // (only columns below L were voted on: c0 + j < CONSB_COLS)
                                atomicAdd(&ps[cc * CONSB_COLS + c0 + j], (unsigned long long)v.s[j][cc]);
                                atomicAdd(&pn[cc * CONSB_COLS + c0 + j], v.n[j][cc]);
                            }
                }
            }
        }
    }
}

__global__ __launch_bounds__(256) void consb_deep_call_kernel(ConsBamArgs a)
{
    const int lane = threadIdx.x & 63;
    const uint64_t gw = (uint64_t)blockIdx.x * 4 + (threadIdx.x >> 6), GW = (uint64_t)gridDim.x * 4;
    const uint64_t n_deep = a.ctl[CB_DEEP] < a.deep_cap ? (uint64_t)a.ctl[CB_DEEP] : (uint64_t)a.deep_cap;
    for (uint64_t d = gw; d < n_deep; d += GW) {
        const uint32_t c = a.deep_list[d];
        const uint32_t L = a.cluster_len[c];
        const uint64_t soff = a.incl_seq[c] - (L + 1) / 2, qoff = a.incl_qual[c] - L;
        const unsigned long long *ps = a.acc_s + d * 4 * CONSB_COLS;
        const uint32_t *pn = a.acc_n + d * 4 * CONSB_COLS;
        uint32_t lost = 0;
        for (uint32_t c_base = 0; c_base < L; c_base += CONSB_PASS) {
            const uint32_t c0 = c_base + 8u * (uint32_t)lane;
            VotesB<uint64_t> v;
#pragma unroll
            for (int j = 0; j < 8; j++)
#pragma unroll
                for (int cc = 0; cc < 4; cc++) {
                    v.s[j][cc] = ps[cc * CONSB_COLS + c0 + j];
                    v.n[j][cc] = pn[cc * CONSB_COLS + c0 + j];
                }
            lost += call_store(a, soff, qoff, L, c_base, lane, v);
        }
        if (a.disagree) {
            lost = wave_sum(lost, lane);
            if (lane == 0) a.disagree[c] = lost;
        }
    }
}

inline uint32_t blocks_for(uint64_t n, uint32_t per_block) { return (uint32_t)((n + per_block - 1) / per_block); }

// Clusters of at least this many voters take the deep path: the option, raised where the accumulator
// slots (48 KB per deep cluster, at most n_reads / split of them) would pass CONSB_ACC_BUDGET, and never
// above what one wave sums in 32 bits.
constexpr uint64_t CONSB_ACC_BUDGET = 512ull << 20;
uint32_t consb_effective_split(uint32_t n_reads, uint32_t split)
{
    const uint64_t slot = (uint64_t)4 * CONSB_COLS * 12;
    const uint64_t floor_ = ((uint64_t)n_reads * slot + CONSB_ACC_BUDGET - 1) / CONSB_ACC_BUDGET;
    return (uint32_t)std::max<uint64_t>(std::min<uint64_t>(std::max<uint64_t>(split, 2), CONSB_ONE_WAVE_MAX), floor_);
}
uint32_t consb_deep_cap(uint32_t n_reads, uint32_t eff_split) { return n_reads / eff_split + 1; }

} // namespace

size_t consensus_bam_workspace_bytes(uint32_t n_reads, uint32_t n_clusters, uint32_t split)
{
    return consb_carve(nullptr, n_reads, n_clusters, consb_deep_cap(n_reads, consb_effective_split(n_reads, split))).total;
}

int consensus_bam_on_device(void *workspace, const uint8_t *d_data, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                            const uint32_t *d_len, const uint32_t *d_cluster, uint32_t n_reads, const uint32_t *d_cluster_len,
                            uint32_t n_clusters, uint32_t split, uint32_t n_cus, uint8_t *d_cons_seq, uint8_t *d_cons_qual,
                            uint64_t *d_seq_off, uint64_t *d_qual_off, uint32_t *d_depth, uint32_t *d_disagree,
                            uint64_t *seq_bytes, uint64_t *qual_bytes, ConsBamFault *fault, unsigned long long *h_pinned,
                            hipStream_t s)
{
    const uint32_t eff_split = consb_effective_split(n_reads, split);
    const uint32_t deep_cap = consb_deep_cap(n_reads, eff_split);
    ConsBamBufs b = consb_carve(workspace, n_reads, n_clusters, deep_cap);
    CONSB_TRY(hipMemsetAsync(workspace, 0, b.zero_bytes, s));
    if (n_clusters) consb_lens_kernel<<<blocks_for(n_clusters, 256), 256, 0, s>>>(d_cluster_len, n_clusters, b.seqk, b.qualk, b.ctl);
    CONSB_TRY(hipGetLastError());
    // (the voters' lengths are compared with cluster_len as it is: a cluster that is too long is refused
    // by the host look below, whatever its voters are)
    if (n_reads)
        consb_count_kernel<<<blocks_for(n_reads, 256), 256, 0, s>>>(d_cluster, d_len, d_cluster_len, n_reads, n_clusters, b.cnt,
                                                                     b.ctl);
    CONSB_TRY(hipGetLastError());
    h_pinned[CB_COUNT] = h_pinned[CB_COUNT + 1] = 0;
    if (n_clusters) {
        CONSB_TRY(scan_inclusive_u64((const uint64_t *)b.cnt, b.incl_reads, n_clusters, b.scan_tmp, b.scan_tmp_bytes, s));
        CONSB_TRY(scan_inclusive_u64(b.seqk, b.incl_seq, n_clusters, b.scan_tmp, b.scan_tmp_bytes, s));
        CONSB_TRY(scan_inclusive_u64(b.qualk, b.incl_qual, n_clusters, b.scan_tmp, b.scan_tmp_bytes, s));
        CONSB_TRY(hipMemcpyAsync(h_pinned + CB_COUNT, b.incl_seq + (n_clusters - 1), 8, hipMemcpyDeviceToHost, s));
        CONSB_TRY(hipMemcpyAsync(h_pinned + CB_COUNT + 1, b.incl_qual + (n_clusters - 1), 8, hipMemcpyDeviceToHost, s));
    }
    CONSB_TRY(hipMemcpyAsync(h_pinned, b.ctl, CB_COUNT * 8, hipMemcpyDeviceToHost, s));
    CONSB_TRY(hipStreamSynchronize(s));
    fault->bad_cluster_len = h_pinned[CB_BAD_CLEN];
    fault->bad_id = h_pinned[CB_BAD_ID];
    fault->bad_len = h_pinned[CB_BAD_LEN];
    if (fault->bad_cluster_len || fault->bad_id || fault->bad_len) return 1;
    *seq_bytes = h_pinned[CB_COUNT];
    *qual_bytes = h_pinned[CB_COUNT + 1];
    if (n_clusters == 0) return 0;

    ConsBamArgs a;
    a.data = d_data;
    a.seq_pos = d_seq_pos;
    a.qual_pos = d_qual_pos;
    a.len = d_len;
    a.slots = b.slots;
    a.cluster_len = d_cluster_len;
    a.cnt = b.cnt;
    a.incl_reads = b.incl_reads;
    a.incl_seq = b.incl_seq;
    a.incl_qual = b.incl_qual;
    a.n_clusters = n_clusters;
    a.n_reads = n_reads;
    a.split = eff_split;
    a.deep_cap = deep_cap;
    a.cons_seq = d_cons_seq;
    a.cons_qual = d_cons_qual;
    a.seq_off = d_seq_off;
    a.qual_off = d_qual_off;
    a.depth = d_depth;
    a.disagree = d_disagree;
    a.deep_list = b.deep_list;
    a.acc_s = b.acc_s;
    a.acc_n = b.acc_n;
    a.ctl = b.ctl;
    if (n_reads)
        consb_scatter_kernel<<<blocks_for(n_reads, 256), 256, 0, s>>>(d_cluster, n_reads, n_clusters, b.cnt, b.incl_reads,
                                                                       b.cursor, b.slots);
    // every wave resident at once (2 blocks of 4 per CU: the accumulators and the words in flight leave
    // room for two waves per SIMD), fewer where there are fewer clusters
    const uint32_t grid = std::max(1u, std::min(blocks_for(n_clusters, 4), n_cus * 2));
    consb_vote_kernel<<<grid, 256, 0, s>>>(a);
    // (both return at once where the vote kernel met no deep cluster; no host look in between)
    if (n_reads >= eff_split) {
        consb_deep_kernel<<<n_cus * 2, 256, 0, s>>>(a);
        consb_deep_call_kernel<<<std::max(1u, std::min(blocks_for(deep_cap, 4), n_cus * 2)), 256, 0, s>>>(a);
    }
    CONSB_TRY(hipGetLastError());
    CONSB_TRY(hipMemcpyAsync(h_pinned, b.ctl, CB_COUNT * 8, hipMemcpyDeviceToHost, s));
    CONSB_TRY(hipStreamSynchronize(s));
    if (h_pinned[CB_DEEP_OVF]) return -(int)hipErrorAssert; // (a deep cluster without a slot: a bug, not an input)
    return 0;
}

#undef CONSB_TRY

} // namespace umihip
