// The batched calls: umi_encode_umis*, every umi_dedup_batch*, the multi-device calls.
#include "umihip_host.hpp"

#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <deque>
#include <thread>

using namespace umihip;

// ---- multi-device host-buffer call ------------------------------------------------------------
// Buckets are independent (src/deduplicate_sam.rs:207-233 shares nothing between iterations but
// additive counters), so a call shards with no exchange between the devices: every bucket goes to
// one device (longest processing time first on n_b^2, partition_buckets_lpt), a host thread per
// device gathers its buckets' entries into pinned staging, runs the ordinary pipeline on its
// device's own stream and workspace, and scatters kept / root back to the caller's arrays at the
// buckets' own offsets.  One giant bucket does not shard that way: then every device evaluates its
// share of the bucket's sub-bucket tasks (umi_pairs_partial_device's path), the edge lists are
// copied to the first device and collapsed there.
namespace {

struct ShardResult {
    int rc = UMI_OK;
    std::string err;
    umi_stats st;
};

void merge_stats(umi_stats &a, const umi_stats &b)
{
    a.n_kept += b.n_kept;
    a.n_pairs_evaluated += b.n_pairs_evaluated;
    a.n_candidates += b.n_candidates;
    a.n_edges += b.n_edges;
    a.n_rounds = std::max(a.n_rounds, b.n_rounds);
    a.n_pair_launches += b.n_pair_launches;
    a.ms_total = std::max(a.ms_total, b.ms_total);
    a.ms_prep = std::max(a.ms_prep, b.ms_prep);
    a.ms_pairs = std::max(a.ms_pairs, b.ms_pairs);
    a.ms_collapse = std::max(a.ms_collapse, b.ms_collapse);
    a.ms_finalize = std::max(a.ms_finalize, b.ms_finalize);
}

int dedup_batch_single(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                       const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k, float percentage,
                       int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats, int n_words = 1);

// one device's share of a bucket-sharded call (runs on its own host thread)
void run_shard(umi_ctx *sub, const std::vector<uint64_t> &mine, const uint64_t *keys, const uint64_t *nmask,
               const int32_t *freq, const uint64_t *bucket_off, int umi_len, int k, float percentage, int algo,
               int32_t adj_max_freq, uint8_t *kept, uint32_t *root, ShardResult &res, int n_words)
{
    const size_t kw = 8 * (size_t)n_words; // bytes of a key (entry-major: the words of an entry are adjacent)
    memset(&res.st, 0, sizeof(res.st));
    uint64_t n_local = 0;
    sub->sh_boff.assign(1, 0);
    for (uint64_t b : mine) {
        n_local += bucket_off[b + 1] - bucket_off[b];
        sub->sh_boff.push_back(n_local);
    }
    if (n_local == 0) return;
    // pinned staging: keys | nmask | freq in, kept | root out
    const size_t o_keys = 0, o_nmask = o_keys + n_local * kw, o_freq = o_nmask + (nmask ? n_local * kw : 0);
    const size_t in_bytes = o_freq + n_local * 4;
    const size_t o_kept = 0, o_root = (n_local + 15) & ~(size_t)15, out_bytes = o_root + (root ? n_local * 4 : 0);
    auto fail_here = [&](int rc) {
        res.rc = rc;
        res.err = umi_last_error(); // (this thread's message)
    };
    if (hipSetDevice(sub->device) != hipSuccess) {
        res.rc = UMI_ERR_HIP;
        res.err = "hipSetDevice failed on a worker thread";
        return;
    }
    int rc;
    // UMIHIP_TIMING=1: where the wall time of a sharded host-buffer call goes, per device, on stderr
    const bool timing = getenv("UMIHIP_TIMING") != nullptr;
    auto now = [] { return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count(); };
    const double t0 = now();
    if ((rc = sub->sh_in.reserve(in_bytes)) || (rc = sub->sh_out.reserve(out_bytes))) return fail_here(rc);
    uint64_t at = 0;
    for (uint64_t b : mine) {
        const uint64_t s0 = bucket_off[b], len = bucket_off[b + 1] - s0;
        memcpy(sub->sh_in.p + o_keys + at * kw, keys + s0 * (size_t)n_words, len * kw);
        if (nmask) memcpy(sub->sh_in.p + o_nmask + at * kw, nmask + s0 * (size_t)n_words, len * kw);
        memcpy(sub->sh_in.p + o_freq + at * 4, freq + s0, len * 4);
        at += len;
    }
    umi_stats st;
    const double t1 = now();
    rc = dedup_batch_single(sub, (const uint64_t *)(sub->sh_in.p + o_keys),
                            nmask ? (const uint64_t *)(sub->sh_in.p + o_nmask) : nullptr,
                            (const int32_t *)(sub->sh_in.p + o_freq), sub->sh_boff.data(), mine.size(), umi_len, k,
                            percentage, algo, adj_max_freq, (uint8_t *)(sub->sh_out.p + o_kept),
                            root ? (uint32_t *)(sub->sh_out.p + o_root) : nullptr, &st, n_words);
    if (rc) return fail_here(rc);
    res.st = st;
    const double t2 = now();
    // back to the caller's index space: a bucket's entries keep their order, a root index moves
    // with its bucket
    at = 0;
    for (uint64_t b : mine) {
        const uint64_t s0 = bucket_off[b], len = bucket_off[b + 1] - s0;
        memcpy(kept + s0, sub->sh_out.p + o_kept + at, len);
        if (root) {
            const uint32_t *src = (const uint32_t *)(sub->sh_out.p + o_root) + at;
            const uint32_t shift = (uint32_t)(s0 - at); // (mod 2^32: local index + shift = global index)
            for (uint64_t i = 0; i < len; i++) root[s0 + i] = src[i] + shift;
        }
        at += len;
    }
    if (timing)
        fprintf(stderr, "umihip multi: device %d: %llu entries in %zu buckets: host gather %.4f s, call (H2D + GPU + D2H) "
                        "%.4f s, host scatter %.4f s\n",
                sub->device, (unsigned long long)n_local, mine.size(), t1 - t0, t2 - t1, now() - t2);
}

// the multi-device split of a call whose work is one giant bucket
int dedup_batch_split(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                      const uint64_t *bucket_off, uint64_t n_buckets, uint64_t n, int umi_len, int k,
                      float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
                      umi_stats *stats)
{
    const uint32_t n_dev = (uint32_t)ctx->subs.size();
    const int mode = mode_of(algo);
    std::vector<ShardResult> res(n_dev);
    std::vector<uint64_t> n_edges(n_dev, 0);
    // every device gets the whole input; the first one's block holds kept and root as well (the collapse below)
    std::deque<HostIo> io;
    IoPtr<uint8_t> d_kept;
    IoPtr<uint32_t> d_root;
    std::vector<std::thread> pool;
    for (umi_ctx *sub : ctx->subs) io.emplace_back(sub);
    for (uint32_t r = 0; r < n_dev; r++) {
        HostIo *my = &io[r];
        const auto d_keys = my->in(keys, n * 8), d_nmask = my->in(nmask, n * 8);
        const auto d_freq = my->in(freq, n * 4);
        if (r == 0) {
            d_kept = my->out(kept, n);
            d_root = my->out(root, n * 4);
        }
        pool.emplace_back([&, r, my, d_keys, d_nmask, d_freq] {
            ShardResult &out = res[r];
            memset(&out.st, 0, sizeof(out.st));
            int rc;
            if ((rc = my->open()) ||
                (rc = run_pipeline_part(ctx->subs[r], d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k,
                                        percentage, mode, adj_max_freq, my->stream(), r, n_dev, &out.st, &n_edges[r]))) {
                out.rc = rc;
                out.err = umi_last_error(); // (this thread's message)
            }
            if (rc || r) (void)my->close(); // (here, where its device is current; the first one's stays open for the collapse)
        });
    }
    for (auto &t : pool) t.join();
    for (uint32_t r = 0; r < n_dev; r++)
        if (res[r].rc) return fail(res[r].rc, "device %d: %s", ctx->subs[r]->device, res[r].err.c_str());
    // the edge lists to the first device (peer copy, or through the host where peers cannot see
    // each other), the collapse there
    umi_ctx *c0 = ctx->subs[0];
    uint64_t total = 0;
    for (uint64_t e : n_edges) total += e;
    if (total >= 0x7FFFFFF0ull) return fail(UMI_ERR_NOMEM, "gathered edge list too large");
    HIP_TRY(hipSetDevice(c0->device));
    int rc;
    DevBuf gathered; // (freed on leaving: after the collapse and the downloads behind it have been waited for)
    if ((rc = gathered.reserve(std::max<uint64_t>(total, 1) * sizeof(uint2)))) return rc;
    uint64_t at = 0;
    hipError_t e = hipSuccess;
    for (uint32_t r = 0; r < n_dev && e == hipSuccess; r++) {
        if (!n_edges[r]) continue;
        // (on the stream the collapse runs on: a device-to-device hipMemcpy may return before the copy has landed,
        // and that stream -- non-blocking -- would not wait for it.  The lists themselves are finished: every
        // device's pipeline has seen its end.)
        e = hipMemcpyAsync((char *)gathered.p + at * sizeof(uint2), ctx->subs[r]->edges.p, n_edges[r] * sizeof(uint2),
                           hipMemcpyDefault, c0->own_stream);
        at += n_edges[r];
    }
    if (e != hipSuccess) return fail(UMI_ERR_HIP, "edge gather failed: %s", hipGetErrorString(e));
    umi_stats st;
    memset(&st, 0, sizeof(st));
    if ((rc = collapse_edges(c0, (uint32_t)n, gathered.as<uint2>(), (uint32_t)total, mode, d_kept, d_root, c0->own_stream, &st)) ||
        (rc = io[0].fetch(kept, d_kept, n)) || (rc = io[0].fetch(root, d_root, n)) || (rc = io[0].close()))
        return rc;
    if (stats) {
        umi_stats total_st = res[0].st;
        for (uint32_t r = 1; r < n_dev; r++) merge_stats(total_st, res[r].st);
        total_st.n_umis = n;
        total_st.n_buckets = n_buckets;
        total_st.max_bucket = res[0].st.max_bucket;
        total_st.n_pairs = res[0].st.n_pairs;
        total_st.n_kept = st.n_kept;
        total_st.n_edges = total;
        total_st.n_rounds = st.n_rounds;
        *stats = total_st;
    }
    return UMI_OK;
}

int dedup_batch_multi(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                      const uint64_t *bucket_off, uint64_t n_buckets, uint64_t n, int umi_len, int k,
                      float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
                      umi_stats *stats, int n_words = 1)
{
    const uint32_t n_dev = (uint32_t)ctx->subs.size();
    // one bucket with more than half of the call's n_b^2: its pairs are split, not the buckets
    // (only where pairs are evaluated at all: the reference's adjacency needs none)
    long double cost = 0, top = 0;
    uint64_t max_bucket = 0;
    for (uint64_t b = 0; b < n_buckets; b++) {
        const long double sz = (long double)(bucket_off[b + 1] - bucket_off[b]);
        cost += sz * sz;
        top = std::max(top, sz * sz);
        max_bucket = std::max<uint64_t>(max_bucket, (uint64_t)sz);
    }
    const bool need_pairs = !(algo == UMI_ALGO_ADJACENCY && adj_max_freq < 1);
    if (n_dev > 1 && need_pairs && max_bucket >= ctx->split_min && top * 2 > cost && n_words == 1)
        return dedup_batch_split(ctx, keys, nmask, freq, bucket_off, n_buckets, n, umi_len, k, percentage, algo,
                                 adj_max_freq, kept, root, stats);
    std::vector<uint32_t> owner;
    partition_buckets_lpt(bucket_off, n_buckets, n_dev, owner);
    std::vector<std::vector<uint64_t>> mine(n_dev);
    for (uint64_t b = 0; b < n_buckets; b++) mine[owner[b]].push_back(b);
    std::vector<ShardResult> res(n_dev);
    std::vector<std::thread> pool;
    for (uint32_t r = 0; r < n_dev; r++)
        pool.emplace_back([&, r] {
            run_shard(ctx->subs[r], mine[r], keys, nmask, freq, bucket_off, umi_len, k, percentage, algo, adj_max_freq,
                      kept, root, res[r], n_words);
        });
    for (auto &t : pool) t.join();
    for (uint32_t r = 0; r < n_dev; r++)
        if (res[r].rc) return fail(res[r].rc, "device %d: %s", ctx->subs[r]->device, res[r].err.c_str());
    if (stats) {
        umi_stats total = res[0].st;
        for (uint32_t r = 1; r < n_dev; r++) {
            merge_stats(total, res[r].st);
            total.max_bucket = std::max(total.max_bucket, res[r].st.max_bucket);
            total.n_pairs += res[r].st.n_pairs;
        }
        total.n_umis = n;
        total.n_buckets = n_buckets;
        *stats = total;
    }
    return UMI_OK;
}

// a checked, non-empty call on one device: its arrays staged, the pipeline, kept and root back
int dedup_batch_staged(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                       const uint64_t *bucket_off, uint64_t n_buckets, uint64_t n, int umi_len, int k, float percentage,
                       int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats, int n_words, bool edit)
{
    const size_t kb = (size_t)n * 8 * (size_t)n_words;
    HostIo io(ctx);
    const auto d_keys = io.in(keys, kb), d_nmask = io.in(nmask, kb);
    const auto d_freq = io.in(freq, n * 4);
    const auto d_kept = io.out(kept, n);
    const auto d_root = io.out(root, n * 4);
    int rc;
    if ((rc = io.open()) ||
        (rc = run_pipeline(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k, percentage,
                           mode_of(algo), adj_max_freq, d_kept, d_root, io.stream(), stats, nullptr, n_words, false, edit)) ||
        (rc = io.fetch(kept, d_kept, n)) || (rc = io.fetch(root, d_root, n)))
        return rc;
    return io.close();
}

int dedup_batch_single(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                    const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k,
                    float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
                    umi_stats *stats, int n_words)
{
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n, n_words > 1 ? UMI_MAX_WIDE_UMI_LEN : UMI_MAX_UMI_LEN);
    if (rc) return rc;
    if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return dedup_batch_staged(ctx, keys, nmask, freq, bucket_off, n_buckets, n, umi_len, k, percentage, algo, adj_max_freq,
                              kept, root, stats, n_words, false);
}

} // namespace

extern "C" {

int umi_partition_buckets(const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n_ranks, uint32_t *owner)
{
    if (!bucket_off || (!owner && n_buckets)) return fail(UMI_ERR_ARG, "bucket_off/owner is NULL");
    if (n_ranks < 1) return fail(UMI_ERR_ARG, "n_ranks must be >= 1");
    for (uint64_t b = 0; b < n_buckets; b++) {
        if (bucket_off[b + 1] < bucket_off[b]) return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
        // (the cost n_b^2 + n_b is kept in 64 bits; the batched calls take no larger bucket either)
        if (bucket_off[b + 1] - bucket_off[b] >= 0x7FFFFFF0ull)
            return fail(UMI_ERR_ARG, "bucket %llu holds %llu entries: beyond the 31-bit index space of one call",
                        (unsigned long long)b, (unsigned long long)(bucket_off[b + 1] - bucket_off[b]));
    }
    std::vector<uint32_t> o;
    partition_buckets_lpt(bucket_off, n_buckets, n_ranks, o);
    for (uint64_t b = 0; b < n_buckets; b++) owner[b] = o[b];
    return UMI_OK;
}

int umi_dedup_batch(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                    const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k,
                    float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
                    umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        uint64_t n = 0;
        int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
        if (rc) return rc;
        if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
        for (uint64_t b = 0; b < n_buckets; b++)
            if (bucket_off[b + 1] < bucket_off[b])
                return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
        if (n == 0) {
            if (stats) {
                memset(stats, 0, sizeof(*stats));
                stats->n_buckets = n_buckets;
            }
            return UMI_OK;
        }
        if (ctx->subs.size() == 1)
            return dedup_batch_single(ctx->subs[0], keys, nmask, freq, bucket_off, n_buckets, umi_len, k, percentage,
                                      algo, adj_max_freq, kept, root, stats);
        return dedup_batch_multi(ctx, keys, nmask, freq, bucket_off, n_buckets, n, umi_len, k, percentage, algo,
                                 adj_max_freq, kept, root, stats);
    }
    return dedup_batch_single(ctx, keys, nmask, freq, bucket_off, n_buckets, umi_len, k, percentage, algo,
                              adj_max_freq, kept, root, stats);
}

int umi_pack_mask_device(umi_ctx *ctx, const uint8_t *d_kept, uint64_t n, uint8_t *d_bits, void *hip_stream)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    if (n && (!d_kept || !d_bits)) return fail(UMI_ERR_ARG, "kept/bits is NULL");
    HIP_TRY(hipSetDevice(ctx->device));
    HIP_TRY(launch_pack_mask(d_kept, n, d_bits, (hipStream_t)hip_stream));
    return UMI_OK;
}

// ---- multi-word keys: umi_len 22..UMI_MAX_WIDE_UMI_LEN -------------------------------------------
int umi_encode_umis_wide(const uint8_t *ascii, uint64_t n, int umi_len, int n_words, uint64_t *keys, uint64_t *nmask)
{ // src/utils/mod.rs:63-83 for keys of any length: base i at bits 3i .. 3i+2 of the word string
    if (!ascii || !keys) return fail(UMI_ERR_ARG, "ascii/keys is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN) return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    for (uint64_t i = 0; i < n; i++) {
        uint64_t *k = keys + i * (uint64_t)n_words, *m = nmask ? nmask + i * (uint64_t)n_words : nullptr;
        for (int w = 0; w < n_words; w++) {
            k[w] = 0;
            if (m) m[w] = 0;
        }
        for (int b = 0; b < umi_len; b++) {
            uint64_t c;
            switch (ascii[i * (uint64_t)umi_len + b]) { // read.rs:23-31
            case 'A': c = 0; break;
            case 'T': c = 5; break;
            case 'C': c = 6; break;
            case 'G': c = 3; break;
            case 'N': c = 4; break;
            default: return fail(UMI_ERR_CHAR, "Unknown character in UMI sequence: %u (UMI %llu)",
                                 (unsigned)ascii[i * (uint64_t)umi_len + b], (unsigned long long)i);
            }
            for (int j = 0; j < 3; j++) { // bit by bit: a base may straddle two words (bitset.rs:52-61)
                const int bit = 3 * b + j;
                if ((c >> j) & 1) k[bit >> 6] |= 1ull << (bit & 63);
                if (c == 4 && m) m[bit >> 6] |= 1ull << (bit & 63); // set_n_bit, bitset.rs:63-75
            }
        }
    }
    return UMI_OK;
}

int umi_dedup_batch_wide_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, int n_words,
                                const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len,
                                int k, float percentage, int algo, int32_t adj_max_freq, uint8_t *d_kept,
                                uint32_t *d_root, void *hip_stream, umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n, UMI_MAX_WIDE_UMI_LEN);
    if (rc) return rc;
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return run_pipeline(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k, percentage,
                        mode_of(algo), adj_max_freq, d_kept, d_root,
                        (hipStream_t)hip_stream, stats, nullptr, n_words);
}

int umi_dedup_batch_wide(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                         const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k, float percentage,
                         int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats)
{
    if (n_words == 1) // one word: the ordinary call
        return umi_dedup_batch(ctx, keys, nmask, freq, bucket_off, n_buckets, umi_len, k, percentage, algo,
                               adj_max_freq, kept, root, stats);
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n, UMI_MAX_WIDE_UMI_LEN);
    if (rc) return rc;
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    for (uint64_t b = 0; b < n_buckets; b++)
        if (bucket_off[b + 1] < bucket_off[b])
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    // a multi-device context shards the buckets over its devices exactly as for one-word keys
    if (!ctx->subs.empty() && ctx->subs.size() > 1)
        return dedup_batch_multi(ctx, keys, nmask, freq, bucket_off, n_buckets, n, umi_len, k, percentage, algo,
                                 adj_max_freq, kept, root, stats, n_words);
    return dedup_batch_single(ctx->subs.empty() ? ctx : ctx->subs[0], keys, nmask, freq, bucket_off, n_buckets, umi_len, k,
                              percentage, algo, adj_max_freq, kept, root, stats, n_words);
}

int umi_encode_umis(const uint8_t *ascii, uint64_t n, int umi_len, uint64_t *keys, uint64_t *nmask)
{
    if ((!ascii && n) || !keys) return fail(UMI_ERR_ARG, "ascii/keys is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_UMI_LEN)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_UMI_LEN);
    // code table of src/utils/read.rs:23-31; 0xFF = the reference panics
    uint8_t code[256];
    memset(code, 0xFF, sizeof(code));
    code['A'] = 0x0; code['T'] = 0x5; code['C'] = 0x6; code['G'] = 0x3; code['N'] = 0x4;
    for (uint64_t i = 0; i < n; i++) {
        const uint8_t *s = ascii + i * (uint64_t)umi_len;
        uint64_t key = 0, nm = 0;
        for (int b = 0; b < umi_len; b++) {
            const uint8_t c = code[s[b]];
            if (c == 0xFF)
                return fail(UMI_ERR_CHAR, "Unknown character in UMI sequence: %u (UMI %llu)",
                            (unsigned)s[b], (unsigned long long)i);
            key |= (uint64_t)c << (3 * b);
            if (c == 0x4) nm |= (uint64_t)0x7 << (3 * b);
        }
        keys[i] = key;
        if (nmask) nmask[i] = nm;
    }
    return UMI_OK;
}

int umi_dedup_batch_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                           const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets,
                           int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                           uint8_t *d_kept, uint32_t *d_root, void *hip_stream, umi_stats *stats)
{
    return umi_dedup_batch_device_table(ctx, d_keys, d_nmask, d_freq, bucket_off, nullptr, n_buckets, umi_len, k,
                                        percentage, algo, adj_max_freq, d_kept, d_root, hip_stream, stats);
}

int umi_dedup_batch_device_table(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                                 const int32_t *d_freq, const uint64_t *bucket_off, const uint64_t *d_bucket_off,
                                 uint64_t n_buckets, int umi_len, int k, float percentage, int algo,
                                 int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root, void *hip_stream,
                                 umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
    if (rc) return rc;
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return run_pipeline(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len,
                        k, percentage,
                        mode_of(algo),
                        adj_max_freq, d_kept, d_root, (hipStream_t)hip_stream, stats, d_bucket_off);
}

// ---- Levenshtein distance between one-word keys (umihip_edit.hip) ----------------------------------
int umi_dedup_batch_edit_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                                const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k, float percentage,
                                int algo, int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root, void *hip_stream,
                                umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1) return fail(UMI_ERR_ARG, "edit distance takes a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
    if (rc) return rc;
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return run_pipeline(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k, percentage,
                        mode_of(algo), adj_max_freq, d_kept, d_root,
                        (hipStream_t)hip_stream, stats, nullptr, 1, false, true);
}

int umi_dedup_batch_edit(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                         const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k, float percentage, int algo,
                         int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1) return fail(UMI_ERR_ARG, "edit distance takes a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
    if (rc) return rc;
    if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    for (uint64_t b = 0; b < n_buckets; b++)
        if (bucket_off[b + 1] < bucket_off[b])
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
    if (n == 0) {
        if (stats) {
            memset(stats, 0, sizeof(*stats));
            stats->n_buckets = n_buckets;
        }
        return UMI_OK;
    }
    return dedup_batch_staged(ctx, keys, nmask, freq, bucket_off, n_buckets, n, umi_len, k, percentage, algo, adj_max_freq,
                              kept, root, stats, 1, true);
}

int umi_dedup_batch_device_begin(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                                 const uint64_t *bucket_off, const uint64_t *d_bucket_off, uint64_t n_buckets,
                                 int umi_len, int k, float percentage, int algo, int32_t adj_max_freq, uint8_t *d_kept,
                                 uint32_t *d_root, void *hip_stream)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
    if (rc) return rc;
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    settle(ctx);
    umi_ctx::PendingCall &pc = ctx->pending;
    pc.have_result = false;
    memset(&pc.st, 0, sizeof(pc.st));
    if (n == 0) {
        pc.st.n_buckets = n_buckets;
        pc.rc = UMI_OK;
        pc.have_result = true;
        return UMI_OK;
    }
    umi_stats st;
    memset(&st, 0, sizeof(st));
    rc = run_pipeline(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k, percentage,
                      mode_of(algo), adj_max_freq, d_kept, d_root,
                      (hipStream_t)hip_stream, &st, d_bucket_off, 1, true);
    if (rc) return rc; // (nothing is pending: the call failed where a plain call would have)
    if (!pc.deferred) { // the call had decisions to take on the host and has run to its end
        pc.st = st;
        pc.rc = UMI_OK;
        pc.have_result = true;
    }
    return UMI_OK;
}

int umi_dedup_batch_end(umi_ctx *ctx, umi_stats *stats)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    return finish_pending(ctx, stats);
}

int umi_dedup_batch_device_multi(umi_ctx *ctx, const uint64_t *const *d_keys, const uint64_t *const *d_nmask,
                                 const int32_t *const *d_freq, const uint64_t *const *bucket_off,
                                 const uint64_t *n_buckets, int umi_len, int k, float percentage, int algo,
                                 int32_t adj_max_freq, uint8_t *const *d_kept, uint32_t *const *d_root,
                                 uint8_t *const *d_mask_bits_all, uint64_t slice_bytes, umi_stats *stats)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (ctx->subs.empty()) return fail(UMI_ERR_ARG, "a multi-device context is needed (umi_ctx_create_multi; one device will do)");
    const uint32_t n_dev = (uint32_t)ctx->subs.size();
    if (!d_keys || !d_freq || !bucket_off || !n_buckets || !d_kept) return fail(UMI_ERR_ARG, "a required array of pointers is NULL");
    for (uint32_t r = 0; r < n_dev; r++)
        for (uint32_t q = 0; q < r; q++)
            if (d_mask_bits_all && ctx->subs[r]->device == ctx->subs[q]->device)
                return fail(UMI_ERR_ARG, "device %d is named twice: RCCL wants one rank per device", ctx->subs[r]->device);
    std::vector<uint64_t> n(n_dev, 0);
    for (uint32_t r = 0; r < n_dev; r++) {
        int rc = check_common(ctx->subs[r], bucket_off[r], n_buckets[r], umi_len, k, algo, &n[r]);
        if (rc) return rc;
        if (n[r] && (!d_keys[r] || !d_freq[r] || !d_kept[r])) return fail(UMI_ERR_ARG, "device %u: keys/freq/kept is NULL", r);
        if (d_mask_bits_all && (!d_mask_bits_all[r] || slice_bytes < (n[r] + 7) / 8))
            return fail(UMI_ERR_ARG, "device %u: the gathered mask needs %u slices of at least %llu bytes", r, n_dev,
                        (unsigned long long)((n[r] + 7) / 8));
    }
    // the communicators, once per context
    if (d_mask_bits_all && ctx->comms.empty()) {
        if (!ctx->rccl.load()) return fail(UMI_ERR_HIP, "%s", ctx->rccl.error.c_str());
        std::vector<int> ids;
        for (umi_ctx *sub : ctx->subs) ids.push_back(sub->device);
        ctx->comms.assign(n_dev, nullptr);
        const ncclResult_t e = ctx->rccl.CommInitAll(ctx->comms.data(), (int)n_dev, ids.data());
        if (e != ncclSuccess) {
            ctx->comms.clear();
            return fail(UMI_ERR_HIP, "ncclCommInitAll: %s", ctx->rccl.GetErrorString(e));
        }
    }
    // every device's shard through the ordinary pipeline on its own stream (a host thread each: the
    // pipeline plans and synchronises), its mask packed to bits into its slot of its gather buffer
    const int mode = mode_of(algo);
    std::vector<ShardResult> res(n_dev);
    std::vector<std::thread> pool;
    for (uint32_t r = 0; r < n_dev; r++)
        pool.emplace_back([&, r] {
            umi_ctx *sub = ctx->subs[r];
            ShardResult &out = res[r];
            memset(&out.st, 0, sizeof(out.st));
            out.st.n_buckets = n_buckets[r];
            hipError_t e = hipSetDevice(sub->device);
            int rc = UMI_OK;
            if (e == hipSuccess && n[r])
                rc = run_pipeline(sub, d_keys[r], d_nmask ? d_nmask[r] : nullptr, d_freq[r], bucket_off[r], n_buckets[r],
                                  (uint32_t)n[r], umi_len, k, percentage, mode, adj_max_freq, d_kept[r],
                                  d_root ? d_root[r] : nullptr, sub->own_stream, &out.st);
            if (rc == UMI_OK && e == hipSuccess && d_mask_bits_all) {
                uint8_t *slot = d_mask_bits_all[r] + (size_t)r * slice_bytes;
                e = hipMemsetAsync(slot, 0, slice_bytes, sub->own_stream);
                if (e == hipSuccess && n[r]) e = launch_pack_mask(d_kept[r], n[r], slot, sub->own_stream);
            }
            if (rc) {
                out.rc = rc;
                out.err = umi_last_error();
            } else if (e != hipSuccess) {
                out.rc = UMI_ERR_HIP;
                out.err = hipGetErrorString(e);
            }
        });
    for (auto &t : pool) t.join();
    // an error return lets every device's stream run dry first: the healthy shards' packing may still be
    // writing the caller's buffers
    auto drain = [&] {
        for (umi_ctx *sub : ctx->subs)
            if (hipSetDevice(sub->device) == hipSuccess) (void)hipStreamSynchronize(sub->own_stream);
    };
    for (uint32_t r = 0; r < n_dev; r++)
        if (res[r].rc) {
            drain();
            return fail(res[r].rc, "device %d: %s", ctx->subs[r]->device, res[r].err.c_str());
        }
    // the all-gatherv of the kept mask: every device's slice to every device over RCCL / xGMI, as
    // padded slices in place (a device's send buffer is its own slot of its receive buffer) --
    // <= 1 bit per unique UMI, latency-bound; one group, so the ranks of this one process progress together
    if (d_mask_bits_all) {
        ncclResult_t e = ctx->rccl.GroupStart();
        for (uint32_t r = 0; r < n_dev && e == ncclSuccess; r++)
            e = ctx->rccl.AllGather(d_mask_bits_all[r] + (size_t)r * slice_bytes, d_mask_bits_all[r], slice_bytes, ncclUint8,
                                    ctx->comms[r], ctx->subs[r]->own_stream);
        const ncclResult_t e2 = ctx->rccl.GroupEnd();
        if (e != ncclSuccess || e2 != ncclSuccess) {
            drain();
            return fail(UMI_ERR_HIP, "ncclAllGather: %s", ctx->rccl.GetErrorString(e != ncclSuccess ? e : e2));
        }
        hipError_t he = hipSuccess;
        for (uint32_t r = 0; r < n_dev; r++) { // (every device's, whatever one of them reports)
            hipError_t hr = hipSetDevice(ctx->subs[r]->device);
            if (hr == hipSuccess) hr = hipStreamSynchronize(ctx->subs[r]->own_stream);
            if (he == hipSuccess) he = hr;
        }
        if (he != hipSuccess) return fail(UMI_ERR_HIP, "the gather's end: %s", hipGetErrorString(he));
    }
    if (stats) {
        umi_stats total = res[0].st;
        total.n_umis = n[0];
        for (uint32_t r = 1; r < n_dev; r++) {
            merge_stats(total, res[r].st);
            total.max_bucket = std::max(total.max_bucket, res[r].st.max_bucket);
            total.n_pairs += res[r].st.n_pairs;
            total.n_umis += n[r];
            total.n_buckets += n_buckets[r];
        }
        *stats = total;
    }
    return UMI_OK;
}

int umi_pairs_partial_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                             const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets,
                             int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                             uint32_t part, uint32_t n_parts, uint64_t *d_edges,
                             uint64_t edge_capacity, uint64_t *n_edges_out, void *hip_stream,
                             umi_stats *stats)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    uint64_t n = 0;
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, k, algo, &n);
    if (rc) return rc;
    if (!n_edges_out) return fail(UMI_ERR_ARG, "n_edges_out is NULL");
    if (n_parts < 2) return fail(UMI_ERR_ARG, "n_parts must be >= 2 (use umi_dedup_batch_device)");
    if (part >= n_parts) return fail(UMI_ERR_ARG, "part %u outside 0..%u", part, n_parts - 1);
    *n_edges_out = 0;
    if (n == 0) return UMI_OK;
    if (!d_keys || !d_freq) return fail(UMI_ERR_ARG, "keys/freq is NULL");
    const int mode = mode_of(algo);
    hipStream_t s = (hipStream_t)hip_stream;
    settle(ctx); // (a deferred call owns the workspace until its end has been seen)
    uint64_t found = 0;
    if ((rc = run_pipeline_part(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, k,
                                percentage, mode, adj_max_freq, s, part, n_parts, stats, &found)))
        return rc;
    *n_edges_out = found;
    if (found > edge_capacity)
        return fail(UMI_ERR_NOMEM, "edge buffer holds %llu entries, %llu needed",
                    (unsigned long long)edge_capacity, (unsigned long long)found);
    if (found) {
        if (!d_edges) return fail(UMI_ERR_ARG, "d_edges is NULL");
        HIP_TRY(hipMemcpyAsync(d_edges, ctx->edges.p, found * sizeof(uint2),
                               hipMemcpyDeviceToDevice, s));
        HIP_TRY(hipStreamSynchronize(s));
    }
    return UMI_OK;
}

int umi_collapse_edges_device(umi_ctx *ctx, uint64_t n, const uint64_t *d_edges, uint64_t n_edges,
                              int algo, uint8_t *d_kept, uint32_t *d_root, void *hip_stream,
                              umi_stats *stats)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) {
        if (ctx->subs.size() > 1)
            return fail(UMI_ERR_ARG, "device pointers belong to one device: use a single-device context");
        ctx = ctx->subs[0];
    }
    if (!known_algo(algo))
        return fail(UMI_ERR_ARG, "unknown algo %d", algo);
    if (n >= 0x7FFFFFF0ull || n_edges >= 0x7FFFFFF0ull) return fail(UMI_ERR_ARG, "too many entries/edges");
    settle(ctx);
    if (n == 0) return UMI_OK;
    if (!d_kept || (n_edges && !d_edges)) return fail(UMI_ERR_ARG, "kept/edges is NULL");
    return collapse_edges(ctx, (uint32_t)n, (const uint2 *)d_edges, (uint32_t)n_edges, mode_of(algo), d_kept, d_root,
                          (hipStream_t)hip_stream, stats);
}

} // extern "C"
