// Whole-read keys and the consensus of their clusters: umi_encode_seqs, umi_dedup_seqs*,
// umi_consensus_seqs*, umi_consensus_bam*.
#include "umihip_host.hpp"

#include <algorithm>

using namespace umihip;

// ---- whole-read keys (FASTQ mode): umi_dedup_seqs* ----------------------------------------------
namespace {

constexpr uint32_t SEQ_PART_MIN = 512;      // buckets from this many entries up go through the partition ...
constexpr uint32_t SEQ_MIN_PART_BASES = 8; // ... where their k + 1 parts are at least this many bases
constexpr int SEQ_MAX_K = 400;             // a key of 12 words has at most 384 units of distance

int seq_words(uint32_t len) { return (int)((3 * len + 63) / 64); } // bitset.rs:17-18

int seq_check(umi_ctx *ctx, int n_words, const uint64_t *bucket_off, const int32_t *bucket_len, uint64_t n_buckets,
              int k, int algo, uint64_t *n_out)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty() && ctx->subs.size() > 1)
        return fail(UMI_ERR_ARG, "umi_dedup_seqs takes a single-device context");
    if (!bucket_off || (n_buckets && !bucket_len)) return fail(UMI_ERR_ARG, "bucket_off/bucket_len is NULL");
    if (n_words < 1 || n_words > SEQ_MAX_WORDS) return fail(UMI_ERR_ARG, "n_words %d outside 1..%d", n_words, SEQ_MAX_WORDS);
    if (k < 0) return fail(UMI_ERR_ARG, "k must be >= 0 (got %d)", k);
    if (!known_algo(algo)) return fail(UMI_ERR_ARG, "unknown algo %d", algo);
    if (n_buckets && bucket_off[0] != 0) return fail(UMI_ERR_ARG, "bucket_off[0] must be 0");
    for (uint64_t b = 0; b < n_buckets; b++) {
        if (bucket_off[b + 1] < bucket_off[b])
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
        if (bucket_len[b] < 0 || bucket_len[b] > UMI_MAX_SEQ_LEN)
            return fail(UMI_ERR_ARG, "bucket_len[%llu] = %d outside 0..%d", (unsigned long long)b, bucket_len[b],
                        UMI_MAX_SEQ_LEN);
        if (seq_words((uint32_t)bucket_len[b]) > n_words)
            return fail(UMI_ERR_ARG, "bucket_len[%llu] = %d needs %d words, n_words is %d", (unsigned long long)b,
                        bucket_len[b], seq_words((uint32_t)bucket_len[b]), n_words);
    }
    const uint64_t n = n_buckets ? bucket_off[n_buckets] : 0;
    if (n >= 0x7FFFFFF0ull) // bit 31 of an edge endpoint is a flag
        return fail(UMI_ERR_ARG, "%llu entries exceed the 31-bit index space of one call", (unsigned long long)n);
    *n_out = n;
    return UMI_OK;
}

int seq_pipeline(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, int n_words, const int32_t *d_freq,
                 const uint64_t *bucket_off, const int32_t *bucket_len, uint64_t n_buckets, uint32_t n, int k,
                 float percentage, int algo, int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root, hipStream_t s,
                 umi_stats *stats)
{
    settle(ctx);
    HIP_TRY(hipSetDevice(ctx->device));
    int rc;
    umi_stats st;
    memset(&st, 0, sizeof(st));
    st.n_umis = n;
    st.n_buckets = n_buckets;
    const int mode = mode_of(algo);
    const int kk = std::min(k, SEQ_MAX_K);
    // groups: k + 1 parts of a deep bucket with parts of SEQ_MIN_PART_BASES bases or more, else one
    std::vector<SeqGroup> groups;
    uint64_t n_rec = 0;
    for (uint64_t b = 0; b < n_buckets; b++) {
        const uint64_t nb = bucket_off[b + 1] - bucket_off[b];
        st.max_bucket = std::max(st.max_bucket, nb);
        st.n_pairs += nb * (nb - (nb > 0)) / 2;
        if (nb < 2) continue;
        const uint32_t len = (uint32_t)bucket_len[b], parts = (uint32_t)kk + 1;
        const bool split = nb >= SEQ_PART_MIN && len / parts >= SEQ_MIN_PART_BASES;
        for (uint32_t j = 0; j < (split ? parts : 1u); j++) {
            SeqGroup g;
            g.rec_off = (uint32_t)std::min<uint64_t>(n_rec, 0xFFFFFFFFull);
            g.bstart = (uint32_t)bucket_off[b];
            g.n = (uint32_t)nb;
            g.len = len;
            g.nw = (uint32_t)seq_words(len);
            g.part = split ? j : SEQ_ALL_PAIRS;
            g.n_parts = split ? parts : 1u;
            g.pad = 0;
            groups.push_back(g);
            n_rec += nb;
        }
    }
    if (n_rec >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu partition records exceed the 2^30 of one call", (unsigned long long)n_rec);
    const uint32_t R = (uint32_t)n_rec, G = (uint32_t)groups.size();
    unsigned long long *d_cnt;
    if ((rc = ctx->counters.reserve(CTRL_BYTES)) || (rc = ctx->thr.reserve((size_t)n * 4))) return rc;
    d_cnt = ctx->counters.as<unsigned long long>();
    HIP_TRY(hipMemsetAsync(d_cnt, 0, CNT_COUNT * sizeof(unsigned long long), s));
    if (ctx->profile) HIP_TRY(hipEventRecord(ctx->ev[0], s));
    const bool need_pairs = !(mode == MODE_ADJACENCY && adj_max_freq < 1); // reference adj: only the query goes
    uint64_t n_edges = 0;
    if (R && need_pairs) {
        const size_t tmp = std::max(radix_sort_temp_bytes(R), scan_temp_bytes(R));
        if ((rc = ctx->seq_groups.reserve(G * sizeof(SeqGroup))) || (rc = ctx->seq_ka.reserve((size_t)R * 8)) ||
            (rc = ctx->seq_kb.reserve((size_t)R * 8)) || (rc = ctx->seq_va.reserve((size_t)R * 4)) ||
            (rc = ctx->seq_vb.reserve((size_t)R * 4)) || (rc = ctx->seq_flag.reserve((size_t)R * 8)) ||
            (rc = ctx->seq_runid.reserve((size_t)R * 8)) || (rc = ctx->seq_rs.reserve((size_t)(R + 1) * 4)) ||
            (rc = ctx->seq_tend.reserve((size_t)R * 8)) || (rc = ctx->seq_tmp.reserve(tmp)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ctx->seq_groups.p, groups.data(), G * sizeof(SeqGroup), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_seq_records(ctx->seq_groups.as<SeqGroup>(), G, R, d_keys, d_nmask, n_words, d_freq, percentage,
                                   ctx->thr.as<int32_t>(), ctx->seq_ka.as<uint64_t>(), ctx->seq_va.as<uint32_t>(), d_cnt, s));
        int gbits = 1;
        while ((1u << gbits) < G) gbits++;
        bool in_b = false;
        HIP_TRY(radix_sort_pairs_u64(ctx->seq_ka.as<uint64_t>(), ctx->seq_kb.as<uint64_t>(), ctx->seq_va.as<uint32_t>(),
                                     ctx->seq_vb.as<uint32_t>(), R, 0, 32 + gbits, ctx->seq_tmp.p, ctx->seq_tmp.cap, &in_b, s));
        const uint64_t *rkey = in_b ? ctx->seq_kb.as<uint64_t>() : ctx->seq_ka.as<uint64_t>();
        const uint32_t *rval = in_b ? ctx->seq_vb.as<uint32_t>() : ctx->seq_va.as<uint32_t>();
        HIP_TRY(launch_seq_runs(rkey, R, ctx->seq_flag.as<uint64_t>(), ctx->seq_runid.as<uint64_t>(),
                                ctx->seq_rs.as<uint32_t>(), ctx->seq_tend.as<uint64_t>(), ctx->seq_tmp.p, ctx->seq_tmp.cap,
                                d_cnt, s));
        if (ctx->profile) HIP_TRY(hipEventRecord(ctx->ev[1], s));
        SeqPairArgs a;
        a.groups = ctx->seq_groups.as<SeqGroup>();
        a.rkey = rkey;
        a.rval = rval;
        a.n_rec = R;
        a.run_id = ctx->seq_runid.as<uint64_t>();
        a.run_start = ctx->seq_rs.as<uint32_t>();
        a.task_end = ctx->seq_tend.as<uint64_t>();
        a.keys = d_keys;
        a.nmask = d_nmask;
        a.stride = n_words;
        a.freq = d_freq;
        a.thr = ctx->thr.as<int32_t>();
        a.counters = d_cnt;
        a.k = kk;
        a.mode = mode;
        a.adj_max_freq = adj_max_freq;
        const uint32_t blocks = (uint32_t)ctx->n_cus * 16; // persistent: every resident wave deals itself tiles
        for (int attempt = 0;; attempt++) { // an edge list that overflowed is grown and the pair work redone
            if ((rc = ctx->edges.reserve(std::max<uint64_t>(ctx->edge_capacity, 1) * sizeof(uint2)))) return rc;
            a.edges = ctx->edges.as<uint2>();
            a.edge_cap = (uint32_t)std::min<size_t>(ctx->edges.cap / sizeof(uint2), 0xFFFFFFF0u);
            if (ctx->profile) HIP_TRY(hipEventRecord(ctx->ev[7], s));
            HIP_TRY(launch_seq_pairs(a, blocks, s));
            if (ctx->profile) HIP_TRY(hipEventRecord(ctx->ev[8], s));
            st.n_pair_launches++;
            HIP_TRY(hipMemcpyAsync(ctx->h_counters, d_cnt, CNT_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
            if (ctx->h_counters[CNT_ERROR]) break;
            n_edges = ctx->h_counters[CNT_EDGES];
            if (n_edges <= a.edge_cap) break;
            if (n_edges >= 0x7FFFFFF0ull || attempt > 4)
                return fail(UMI_ERR_NOMEM, "%llu edges exceed the list of one call", (unsigned long long)n_edges);
            ctx->edge_capacity = n_edges + n_edges / 4;
            HIP_TRY(hipMemsetAsync(&d_cnt[CNT_EDGES], 0, 2 * sizeof(unsigned long long), s)); // edges, candidates
        }
        st.n_pairs_evaluated = ctx->h_counters[CNT_SEG_PAIRS];
        st.n_candidates = ctx->h_counters[CNT_CANDIDATES];
    } else if (R) { // adjacency with adj_max_freq < 1: the contract check and nothing else
        if ((rc = ctx->seq_groups.reserve(G * sizeof(SeqGroup))) || (rc = ctx->seq_ka.reserve((size_t)R * 8)) ||
            (rc = ctx->seq_va.reserve((size_t)R * 4)))
            return rc;
        HIP_TRY(hipMemcpyAsync(ctx->seq_groups.p, groups.data(), G * sizeof(SeqGroup), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_seq_records(ctx->seq_groups.as<SeqGroup>(), G, R, d_keys, d_nmask, n_words, d_freq, percentage,
                                   ctx->thr.as<int32_t>(), ctx->seq_ka.as<uint64_t>(), ctx->seq_va.as<uint32_t>(), d_cnt, s));
        HIP_TRY(hipMemcpyAsync(ctx->h_counters, d_cnt, CNT_COUNT * sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    if (R && ctx->h_counters[CNT_ERROR])
        return fail(UMI_ERR_ORDER,
                    "%llu entries break the input contract (freq < 1, not in freq-descending rank order inside a "
                    "bucket, or an N base without nmask)",
                    (unsigned long long)ctx->h_counters[CNT_ERROR]);
    // a bucket of one entry, or whole buckets of entries ruled out above, need no record: every entry
    // starts as its own root
    umi_stats cst;
    if ((rc = collapse_edges(ctx, n, ctx->edges.as<uint2>(), (uint32_t)n_edges, mode, d_kept, d_root, s, &cst)))
        return rc;
    if (ctx->profile) {
        HIP_TRY(hipEventRecord(ctx->ev[4], s));
        HIP_TRY(hipEventSynchronize(ctx->ev[4]));
        if (R && need_pairs) {
            HIP_TRY(hipEventElapsedTime(&st.ms_prep, ctx->ev[0], ctx->ev[1]));
            HIP_TRY(hipEventElapsedTime(&st.ms_pairs, ctx->ev[7], ctx->ev[8]));
            HIP_TRY(hipEventElapsedTime(&st.ms_collapse, ctx->ev[8], ctx->ev[4]));
            st.ms_kernel = st.ms_pairs;
            st.kernel_id = UMI_KERNEL_SEQ_PAIRS;
        }
        HIP_TRY(hipEventElapsedTime(&st.ms_total, ctx->ev[0], ctx->ev[4]));
    } else if (R && need_pairs) {
        st.kernel_id = UMI_KERNEL_SEQ_PAIRS;
    }
    st.n_edges = n_edges;
    st.n_rounds = cst.n_rounds;
    st.n_kept = cst.n_kept;
    if (stats) *stats = st;
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_encode_seqs(const uint8_t *ascii, const uint64_t *seq_off, uint64_t n, int n_words, uint64_t *keys,
                    uint64_t *nmask)
{ // src/utils/mod.rs:63-83 per read: base i at bits 3i .. 3i+2 of the word string, the words behind it zero
    if (n && (!ascii || !seq_off || !keys)) return fail(UMI_ERR_ARG, "ascii/seq_off/keys is NULL");
    if (n_words < 1 || n_words > SEQ_MAX_WORDS) return fail(UMI_ERR_ARG, "n_words %d outside 1..%d", n_words, SEQ_MAX_WORDS);
    for (uint64_t i = 0; i < n; i++) {
        if (seq_off[i + 1] < seq_off[i]) return fail(UMI_ERR_ARG, "seq_off not monotone at read %llu", (unsigned long long)i);
        const uint64_t len = seq_off[i + 1] - seq_off[i];
        if (len > UMI_MAX_SEQ_LEN)
            return fail(UMI_ERR_ARG, "read %llu has %llu bases, more than %d", (unsigned long long)i,
                        (unsigned long long)len, UMI_MAX_SEQ_LEN);
        if (seq_words((uint32_t)len) > n_words)
            return fail(UMI_ERR_ARG, "read %llu of %llu bases needs %d words, n_words is %d", (unsigned long long)i,
                        (unsigned long long)len, seq_words((uint32_t)len), n_words);
        uint64_t *kw = keys + i * (uint64_t)n_words, *m = nmask ? nmask + i * (uint64_t)n_words : nullptr;
        for (int w = 0; w < n_words; w++) {
            kw[w] = 0;
            if (m) m[w] = 0;
        }
        const uint8_t *p = ascii + seq_off[i];
        for (uint64_t b = 0; b < len; b++) {
            uint64_t c;
            switch (p[b]) { // read.rs:23-31
            case 'A': c = 0; break;
            case 'T': c = 5; break;
            case 'C': c = 6; break;
            case 'G': c = 3; break;
            case 'N': c = 4; break;
            default: return fail(UMI_ERR_CHAR, "Unknown character in sequence: %u (read %llu)", (unsigned)p[b],
                                 (unsigned long long)i);
            }
            for (int j = 0; j < 3; j++) { // bit by bit: a base may straddle two words (bitset.rs:52-61)
                const uint64_t bit = 3 * b + j;
                if ((c >> j) & 1) kw[bit >> 6] |= 1ull << (bit & 63);
                if (c == 4 && m) m[bit >> 6] |= 1ull << (bit & 63); // set_n_bit, bitset.rs:63-75
            }
        }
    }
    return UMI_OK;
}

int umi_dedup_seqs_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, int n_words,
                          const int32_t *d_freq, const uint64_t *bucket_off, const int32_t *bucket_len,
                          uint64_t n_buckets, int k, float percentage, int algo, int32_t adj_max_freq, uint8_t *d_kept,
                          uint32_t *d_root, void *hip_stream, umi_stats *stats)
{
    uint64_t n = 0;
    int rc = seq_check(ctx, n_words, bucket_off, bucket_len, n_buckets, k, algo, &n);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return seq_pipeline(ctx, d_keys, d_nmask, n_words, d_freq, bucket_off, bucket_len, n_buckets, (uint32_t)n, k,
                        percentage, algo, adj_max_freq, d_kept, d_root, (hipStream_t)hip_stream, stats);
}

int umi_dedup_seqs(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                   const uint64_t *bucket_off, const int32_t *bucket_len, uint64_t n_buckets, int k, float percentage,
                   int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats)
{
    uint64_t n = 0;
    int rc = seq_check(ctx, n_words, bucket_off, bucket_len, n_buckets, k, algo, &n);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    const size_t kb = (size_t)n * 8 * (size_t)n_words;
    HostIo io(ctx);
    const auto d_keys = io.in(keys, kb), d_nmask = io.in(nmask, kb);
    const auto d_freq = io.in(freq, n * 4);
    const auto d_kept = io.out(kept, n);
    const auto d_root = io.out(root, n * 4);
    if ((rc = io.open()) ||
        (rc = seq_pipeline(ctx, d_keys, d_nmask, n_words, d_freq, bucket_off, bucket_len, n_buckets, (uint32_t)n, k, percentage,
                           algo, adj_max_freq, d_kept, d_root, io.stream(), stats)) ||
        (rc = io.fetch(kept, d_kept, n)) || (rc = io.fetch(root, d_root, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- consensus of the clusters of whole reads ---------------------------------------------------
namespace {
int cons_check(umi_ctx *ctx, uint64_t n_reads, uint64_t n_entries, const uint64_t *bucket_off, const int32_t *bucket_len,
               uint64_t n_buckets)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (ctx->subs.size() > 1) return fail(UMI_ERR_ARG, "umi_consensus_seqs takes a single-device context");
    if (n_reads >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one call", (unsigned long long)n_reads);
    if (!bucket_off || (n_buckets && !bucket_len)) return fail(UMI_ERR_ARG, "bucket_off/bucket_len is NULL");
    if (n_buckets >= (1ull << 31)) return fail(UMI_ERR_ARG, "too many buckets");
    if (n_buckets && bucket_off[0] != 0) return fail(UMI_ERR_ARG, "bucket_off[0] must be 0");
    for (uint64_t b = 0; b < n_buckets; b++) {
        if (bucket_off[b + 1] < bucket_off[b])
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
        if (bucket_len[b] < 0 || bucket_len[b] > UMI_MAX_SEQ_LEN)
            return fail(UMI_ERR_ARG, "bucket_len[%llu] = %d outside 0..%d", (unsigned long long)b, bucket_len[b],
                        UMI_MAX_SEQ_LEN);
    }
    if ((n_buckets ? bucket_off[n_buckets] : 0) != n_entries)
        return fail(UMI_ERR_ARG, "bucket_off ends at %llu, n_entries is %llu",
                    (unsigned long long)(n_buckets ? bucket_off[n_buckets] : 0), (unsigned long long)n_entries);
    if (n_entries > n_reads)
        return fail(UMI_ERR_ARG, "%llu entries for %llu reads", (unsigned long long)n_entries, (unsigned long long)n_reads);
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_consensus_seqs_device(umi_ctx *ctx, const uint8_t *d_text, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                              const uint32_t *d_len, uint64_t n_reads, const uint32_t *d_entry_of_read,
                              const int32_t *d_freq, const uint8_t *d_kept, const uint32_t *d_root, uint64_t n_entries,
                              const uint64_t *bucket_off, const int32_t *bucket_len, uint64_t n_buckets,
                              uint8_t *d_cons_seq, uint8_t *d_cons_qual, uint64_t *d_cons_off, uint32_t *d_cluster_reads,
                              uint64_t *cons_bytes, void *hip_stream)
{
    int rc = cons_check(ctx, n_reads, n_entries, bucket_off, bucket_len, n_buckets);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (!cons_bytes) return fail(UMI_ERR_ARG, "cons_bytes is NULL");
    if (n_reads && !d_qual_pos) return fail(UMI_ERR_ARG, "d_qual_pos is NULL: a consensus needs the qualities");
    if (n_reads && (!d_text || !d_seq_pos || !d_len || !d_entry_of_read || !d_freq || !d_kept || !d_root || !d_cons_seq ||
                    !d_cons_qual || !d_cons_off))
        return fail(UMI_ERR_ARG, "a required device pointer is NULL");
    *cons_bytes = 0;
    if (n_reads == 0) return UMI_OK; // (and no entry: there are at most as many as reads)
    if (n_entries == 0)
        return fail(UMI_ERR_ORDER, "%llu reads break the input contract (entry_of_read outside the 0 entries)",
                    (unsigned long long)n_reads);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    if ((rc = ctx->call_ws.reserve(consensus_workspace_bytes((uint32_t)n_reads, (uint32_t)n_entries, (uint32_t)n_buckets,
                                                             ctx->cons_split))))
        return rc;
    ConsFault f;
    const int r = consensus_on_device(ctx->call_ws.p, d_text, d_seq_pos, d_qual_pos, d_len, (uint32_t)n_reads, d_entry_of_read,
                                      d_freq, d_kept, d_root, (uint32_t)n_entries, bucket_off, bucket_len, (uint32_t)n_buckets,
                                      ctx->cons_split, (uint32_t)ctx->n_cus, d_cons_seq, d_cons_qual, d_cons_off,
                                      d_cluster_reads, cons_bytes, &f, ctx->h_counters, (hipStream_t)hip_stream);
    if (r == 1) {
        if (f.bad_read)
            return fail(UMI_ERR_ORDER, "%llu reads break the input contract (entry_of_read outside the %llu entries)",
                        f.bad_read, (unsigned long long)n_entries);
        if (f.bad_root)
            return fail(UMI_ERR_ORDER, "%llu entries break the input contract (root outside the entries, or not a kept entry)",
                        f.bad_root);
        if (f.bad_len)
            return fail(UMI_ERR_ORDER, "%llu reads break the input contract (not as long as the bucket of their entry)",
                        f.bad_len);
        if (f.empty)
            return fail(UMI_ERR_ORDER, "%llu kept entries break the input contract (no read belongs to their cluster)", f.empty);
        return fail(UMI_ERR_ORDER, "freq sums to %lld over the entries, there are %llu reads", (long long)f.freq_sum,
                    (unsigned long long)n_reads);
    }
    if (r < 0) return fail(UMI_ERR_HIP, "consensus: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

int umi_consensus_seqs(umi_ctx *ctx, const uint8_t *text, const uint64_t *seq_pos, const uint64_t *qual_pos,
                       const uint32_t *len, uint64_t n_reads, const uint32_t *entry_of_read, const int32_t *freq,
                       const uint8_t *kept, const uint32_t *root, uint64_t n_entries, const uint64_t *bucket_off,
                       const int32_t *bucket_len, uint64_t n_buckets, uint8_t *cons_seq, uint8_t *cons_qual,
                       uint64_t *cons_off, uint32_t *cluster_reads, uint64_t *cons_bytes)
{
    int rc = cons_check(ctx, n_reads, n_entries, bucket_off, bucket_len, n_buckets);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (!cons_bytes) return fail(UMI_ERR_ARG, "cons_bytes is NULL");
    if (n_reads && !qual_pos) return fail(UMI_ERR_ARG, "qual_pos is NULL: a consensus needs the qualities");
    if (n_reads && (!text || !seq_pos || !len || !entry_of_read || !freq || !kept || !root || !cons_seq || !cons_qual || !cons_off))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    *cons_bytes = 0;
    if (n_reads == 0) return UMI_OK;
    // the text that is looked at, and what the consensus may fill: the caller's capacity
    size_t text_bytes = 1, cap = 0;
    for (uint64_t i = 0; i < n_reads; i++) {
        if (len[i] > UMI_MAX_SEQ_LEN)
            return fail(UMI_ERR_ARG, "read %llu has %u bases, more than %d", (unsigned long long)i, len[i], UMI_MAX_SEQ_LEN);
        text_bytes = std::max<size_t>(text_bytes, std::max(seq_pos[i], qual_pos[i]) + len[i]);
        cap += len[i];
    }
    const size_t n = (size_t)n_reads, ne = std::max<size_t>((size_t)n_entries, 1);
    // what comes out, where it is defined: the kept entries' offsets and counts, the bytes in front of cons_bytes
    std::vector<uint64_t> off_all((size_t)n_entries);
    std::vector<uint32_t> cr_all((size_t)n_entries);
    HostIo io(ctx);
    const auto d_text = io.in(text, text_bytes);
    const auto d_pos = io.in(seq_pos, n * 8, n * 8); // (pad: qual_pos behind seq_pos, from d_pos + n)
    io.also(d_pos, n * 8, qual_pos, n * 8);
    const auto d_len = io.in(len, n * 4), d_eor = io.in(entry_of_read, n * 4);
    // (pads: room for max(n_entries, 1) entries)
    const auto d_freq = io.in(freq, n_entries * 4, (ne - n_entries) * 4);
    const auto d_kept = io.in(kept, n_entries, ne - n_entries);
    const auto d_root = io.in(root, n_entries * 4, (ne - n_entries) * 4);
    // (+ 8: a whole word behind the consensus bytes, for kernels that touch them a word at a time)
    const auto d_cons_seq = io.out<uint8_t>(cap + 8), d_cons_qual = io.out<uint8_t>(cap + 8);
    const auto d_cons_off = io.out<uint64_t>(ne * 8);
    const auto d_cr = io.out<uint32_t>(ne * 4);
    if ((rc = io.open()) ||
        (rc = umi_consensus_seqs_device(ctx, d_text, d_pos, d_pos + n, d_len, n_reads, d_eor, d_freq, d_kept, d_root, n_entries,
                                        bucket_off, bucket_len, n_buckets, d_cons_seq, d_cons_qual, d_cons_off, d_cr, cons_bytes,
                                        io.stream())) ||
        (rc = io.fetch(cons_seq, d_cons_seq, (size_t)*cons_bytes)) || (rc = io.fetch(cons_qual, d_cons_qual, (size_t)*cons_bytes)) ||
        (rc = io.fetch(off_all.data(), d_cons_off, (size_t)n_entries)) ||
        (rc = io.fetch(cr_all.data(), d_cr, (size_t)n_entries)) || (rc = io.close()))
        return rc;
    for (uint64_t e = 0; e < n_entries; e++)
        if (kept[e]) {
            cons_off[e] = off_all[e];
            if (cluster_reads) cluster_reads[e] = cr_all[e];
        }
    return UMI_OK;
}

} // extern "C"

// ---- consensus of the clusters of aligned reads ---------------------------------------------------
namespace {
int cons_bam_check(umi_ctx *ctx, uint64_t n_reads, uint64_t n_clusters, const uint64_t *seq_bytes, const uint64_t *qual_bytes)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (ctx->subs.size() > 1) return fail(UMI_ERR_ARG, "umi_consensus_bam takes a single-device context");
    if (n_reads >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one call", (unsigned long long)n_reads);
    if (n_clusters >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu clusters exceed the 30-bit index space of one call", (unsigned long long)n_clusters);
    if (!seq_bytes || !qual_bytes) return fail(UMI_ERR_ARG, "seq_bytes / qual_bytes is NULL");
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_consensus_bam_device(umi_ctx *ctx, const uint8_t *d_data, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                             const uint32_t *d_len, const uint32_t *d_cluster, uint64_t n_reads,
                             const uint32_t *d_cluster_len, uint64_t n_clusters, uint8_t *d_cons_seq, uint8_t *d_cons_qual,
                             uint64_t *d_seq_off, uint64_t *d_qual_off, uint32_t *d_depth, uint32_t *d_disagree,
                             uint64_t *seq_bytes, uint64_t *qual_bytes, void *hip_stream)
{
    int rc = cons_bam_check(ctx, n_reads, n_clusters, seq_bytes, qual_bytes);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (n_reads && (!d_data || !d_seq_pos || !d_qual_pos || !d_len || !d_cluster))
        return fail(UMI_ERR_ARG, "a required device pointer is NULL");
    if (n_clusters && (!d_cluster_len || !d_cons_seq || !d_cons_qual || !d_seq_off || !d_qual_off || !d_depth))
        return fail(UMI_ERR_ARG, "a required device pointer is NULL");
    *seq_bytes = *qual_bytes = 0;
    if (n_reads == 0 && n_clusters == 0) return UMI_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    if ((rc = ctx->call_ws.reserve(consensus_bam_workspace_bytes((uint32_t)n_reads, (uint32_t)n_clusters, ctx->cons_split))))
        return rc;
    ConsBamFault f;
    uint64_t sb = 0, qb = 0;
    const int r = consensus_bam_on_device(ctx->call_ws.p, d_data, d_seq_pos, d_qual_pos, d_len, d_cluster, (uint32_t)n_reads,
                                          d_cluster_len, (uint32_t)n_clusters, ctx->cons_split, (uint32_t)ctx->n_cus, d_cons_seq,
                                          d_cons_qual, d_seq_off, d_qual_off, d_depth, d_disagree, &sb, &qb, &f,
                                          ctx->h_counters, (hipStream_t)hip_stream);
    if (r == 1) {
        if (f.bad_cluster_len)
            return fail(UMI_ERR_ORDER, "%llu clusters break the input contract (cluster_len above %d)", f.bad_cluster_len,
                        UMI_MAX_CONS_LEN);
        if (f.bad_id)
            return fail(UMI_ERR_ORDER, "%llu reads break the input contract (cluster outside the %llu clusters)", f.bad_id,
                        (unsigned long long)n_clusters);
        return fail(UMI_ERR_ORDER, "%llu voters break the input contract (not as long as their cluster)", f.bad_len);
    }
    if (r < 0) return fail(UMI_ERR_HIP, "consensus: %s", hipGetErrorString((hipError_t)(-r)));
    *seq_bytes = sb;
    *qual_bytes = qb;
    return UMI_OK;
}

int umi_consensus_bam(umi_ctx *ctx, const uint8_t *data, const uint64_t *seq_pos, const uint64_t *qual_pos, const uint32_t *len,
                      const uint32_t *cluster, uint64_t n_reads, const uint32_t *cluster_len, uint64_t n_clusters,
                      uint8_t *cons_seq, uint8_t *cons_qual, uint64_t *seq_off, uint64_t *qual_off, uint32_t *depth,
                      uint32_t *disagree, uint64_t *seq_bytes, uint64_t *qual_bytes)
{
    int rc = cons_bam_check(ctx, n_reads, n_clusters, seq_bytes, qual_bytes);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (n_reads && (!data || !seq_pos || !qual_pos || !len || !cluster)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_clusters && (!cluster_len || !cons_seq || !cons_qual || !seq_off || !qual_off || !depth))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    *seq_bytes = *qual_bytes = 0;
    if (n_reads == 0 && n_clusters == 0) return UMI_OK;
    // what of the data is looked at: the voters' bytes (a voter of a length the device refuses adds nothing);
    // what the consensus may fill (likewise for a cluster that is too long)
    size_t data_bytes = 1, cap_s = 0, cap_q = 0;
    for (uint64_t i = 0; i < n_reads; i++)
        if (cluster[i] != UMI_NO_CLUSTER && len[i] <= UMI_MAX_CONS_LEN)
            data_bytes = std::max<size_t>(data_bytes, std::max(seq_pos[i] + (len[i] + 1) / 2, qual_pos[i] + len[i]));
    for (uint64_t c = 0; c < n_clusters; c++) {
        const size_t L = std::min<uint32_t>(cluster_len[c], UMI_MAX_CONS_LEN);
        cap_s += (L + 1) / 2;
        cap_q += L;
    }
    const size_t n = std::max<size_t>((size_t)n_reads, 1), nc = std::max<size_t>((size_t)n_clusters, 1);
    // (pads of the inputs: room for max(n_reads, 1) reads and max(n_clusters, 1) clusters, a byte of data at least)
    const size_t nr = (size_t)n_reads, ncl = (size_t)n_clusters;
    HostIo io(ctx);
    const auto d_data = io.in(data, nr ? data_bytes : 0, nr ? 0 : 1);
    const auto d_pos = io.in(seq_pos, nr * 8, n * 16 - nr * 8); // (... and qual_pos behind seq_pos, from d_pos + n)
    io.also(d_pos, n * 8, qual_pos, nr * 8);
    const auto d_len = io.in(len, nr * 4, (n - nr) * 4), d_cluster = io.in(cluster, nr * 4, (n - nr) * 4);
    const auto d_clen = io.in(cluster_len, ncl * 4, (nc - ncl) * 4);
    // (+ 8: a whole word behind the consensus bytes, for kernels that touch them a word at a time)
    const auto d_cons_seq = io.out(cons_seq, cap_s + 8), d_cons_qual = io.out(cons_qual, cap_q + 8);
    const auto d_seq_off = io.out(seq_off, nc * 8), d_qual_off = io.out(qual_off, nc * 8);
    const auto d_depth = io.out(depth, nc * 4), d_disagree = io.out(disagree, nc * 4);
    if ((rc = io.open()) ||
        (rc = umi_consensus_bam_device(ctx, d_data, d_pos, nr ? d_pos + n : nullptr, d_len, d_cluster, n_reads, d_clen, n_clusters, d_cons_seq,
                                       d_cons_qual, d_seq_off, d_qual_off, d_depth, d_disagree, seq_bytes, qual_bytes,
                                       io.stream())) ||
        (rc = io.fetch(cons_seq, d_cons_seq, (size_t)*seq_bytes)) || (rc = io.fetch(cons_qual, d_cons_qual, (size_t)*qual_bytes)) ||
        (rc = io.fetch(seq_off, d_seq_off, ncl)) || (rc = io.fetch(qual_off, d_qual_off, ncl)) ||
        (rc = io.fetch(depth, d_depth, ncl)) || (rc = io.fetch(disagree, d_disagree, ncl)))
        return rc;
    return io.close();
}

} // extern "C"
