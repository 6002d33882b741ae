// The one-mismatch correction after Cell Ranger: umi_dedup_batch_cr[_device] (kernels: umihip_cr.hip).
// The host side sorts the call's buckets into the two paths, carves the call's workspace, runs the small buckets'
// kernel, hands the larger buckets to the pipeline in MODE_NEIGHBOURS at k = 1 and resolves the list it leaves.
#include "umihip_host.hpp"

#include <algorithm>

using namespace umihip;

namespace {

// the checks both forms start with; ctx becomes the one device's context
int cr_check_args(umi_ctx *&ctx, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t *n)
{
    if (ctx && !ctx->subs.empty()) {
        if (ctx->subs.size() > 1) return fail(UMI_ERR_ARG, "the one-mismatch correction takes a single-device context");
        ctx = ctx->subs[0];
    }
    int rc = check_common(ctx, bucket_off, n_buckets, umi_len, 1, UMI_ALGO_DIRECTIONAL, n);
    if (rc) return rc;
    for (uint64_t b = 0; b < n_buckets; b++)
        if (bucket_off[b + 1] < bucket_off[b])
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
    return UMI_OK;
}

void cr_empty_stats(umi_stats *stats, uint64_t n_buckets)
{
    if (!stats) return;
    memset(stats, 0, sizeof(*stats));
    stats->n_buckets = n_buckets;
}

// the events of a profiled call (the pipeline in the middle uses the context's own)
struct CrEvents {
    static constexpr int N = 5;
    hipEvent_t ev[N] = {};
    bool on = false;
    ~CrEvents()
    {
        for (hipEvent_t e : ev)
            if (e) (void)hipEventDestroy(e);
    }
    hipError_t create()
    {
        on = true;
        for (hipEvent_t &e : ev)
            if (hipError_t rc = hipEventCreate(&e)) return rc;
        return hipSuccess;
    }
    hipError_t mark(int i, hipStream_t s) { return on ? hipEventRecord(ev[i], s) : hipSuccess; }
};

// a checked call of n >= 1 entries, everything on the device but the table
int cr_run(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq, const uint64_t *bucket_off,
           uint64_t n_buckets, uint32_t n, int umi_len, uint8_t *d_kept, uint32_t *d_root, uint32_t *d_target, hipStream_t s,
           umi_stats *stats)
{
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call owns the workspace until its end has been seen)
    const uint32_t small_max = ctx->cr_small_max, n_cus = (uint32_t)ctx->n_cus;

    // the buckets by path: the larger ones' entries lie back to back in arrays of their own, with a table of their own,
    // for the pipeline (the call's arrays themselves where no small bucket holds an entry)
    umi_stats st;
    memset(&st, 0, sizeof(st));
    st.n_umis = n;
    st.n_buckets = n_buckets;
    std::vector<uint64_t> lboff(1, 0);
    std::vector<CrGatherTask> tasks;
    uint64_t n_small = 0, pairs_small = 0;
    for (uint64_t b = 0; b < n_buckets; b++) {
        const uint64_t s0 = bucket_off[b], sz = bucket_off[b + 1] - s0;
        st.max_bucket = std::max(st.max_bucket, sz);
        st.n_pairs += sz * (sz - (sz ? 1 : 0)) / 2;
        if (sz == 0) continue;
        if (sz <= small_max) {
            n_small += sz;
            pairs_small += sz * (sz - 1) / 2;
            continue;
        }
        const uint64_t dst0 = lboff.back();
        for (uint64_t at = 0; at < sz; at += CR_GATHER_CHUNK)
            tasks.push_back({(uint32_t)(s0 + at), (uint32_t)(dst0 + at), (uint32_t)std::min<uint64_t>(CR_GATHER_CHUNK, sz - at)});
        lboff.push_back(dst0 + sz);
    }
    const uint32_t nl = (uint32_t)lboff.back();
    const bool gather = nl && n_small;
    if (!gather) tasks.clear();

    // the workspace
    IoLayout lay;
    const size_t o_cnt = lay.add(true, CR_COUNT * sizeof(unsigned long long));
    const size_t o_span = lay.add(n_small != 0, (size_t)n * 4);
    const size_t o_target = lay.add(!d_target, (size_t)n * 4);
    const size_t o_bf = lay.add(nl != 0, (size_t)nl * 4), o_bk = lay.add(nl != 0, (size_t)nl * 8);
    const size_t o_nm = lay.add(nl != 0, (size_t)nl * 8);
    const size_t o_ck = lay.add(gather, (size_t)nl * 8), o_cf = lay.add(gather, (size_t)nl * 4);
    const size_t o_gi = lay.add(gather, (size_t)nl * 4), o_tk = lay.add(gather, tasks.size() * sizeof(CrGatherTask));
    int rc;
    if ((rc = ctx->cr_ws.reserve(lay.total + 1)) || (rc = ctx->cr_boff.reserve((n_buckets + 1) * 8))) return rc;
    void *ws = ctx->cr_ws.p;
    unsigned long long *d_cnt = (unsigned long long *)io_at(ws, o_cnt);
    uint32_t *d_span = (uint32_t *)io_at(ws, o_span);
    uint32_t *target = d_target ? d_target : (uint32_t *)io_at(ws, o_target);
    const uint64_t *ckeys = gather ? (const uint64_t *)io_at(ws, o_ck) : d_keys;
    const int32_t *cfreq = gather ? (const int32_t *)io_at(ws, o_cf) : d_freq;
    const uint32_t *gidx = gather ? (const uint32_t *)io_at(ws, o_gi) : nullptr;

    CrEvents ev;
    if (ctx->profile) HIP_TRY(ev.create());
    HIP_TRY(ev.mark(0, s));
    HIP_TRY(hipMemsetAsync(d_cnt, 0, CR_COUNT * sizeof(unsigned long long), s));
    HIP_TRY(hipMemsetAsync(d_kept, 0, n, s));
    HIP_TRY(hipMemcpyAsync(ctx->cr_boff.p, bucket_off, (n_buckets + 1) * 8, hipMemcpyHostToDevice, s));
    if (n_small && nl) HIP_TRY(hipMemsetAsync(d_span, 0, (size_t)n * 4, s)); // (the larger buckets' entries: no word of their own)
    HIP_TRY(launch_cr_check(d_keys, d_nmask, d_freq, n, umi_len, d_cnt, n_cus, s));
    HIP_TRY(launch_cr_spans(ctx->cr_boff.as<uint64_t>(), n_buckets, n, n_small ? small_max : 0, d_freq, d_span, d_cnt, n_cus, s));
    if (gather) {
        HIP_TRY(hipMemcpyAsync(io_at(ws, o_tk), tasks.data(), tasks.size() * sizeof(CrGatherTask), hipMemcpyHostToDevice, s));
        HIP_TRY(launch_cr_gather((const CrGatherTask *)io_at(ws, o_tk), (uint32_t)tasks.size(), d_keys, d_freq,
                                 (uint64_t *)io_at(ws, o_ck), (int32_t *)io_at(ws, o_cf), (uint32_t *)io_at(ws, o_gi), s));
    }
    HIP_TRY(ev.mark(1, s));
    if (n_small) HIP_TRY(launch_cr_small(d_keys, d_freq, d_span, n, umi_len, target, d_kept, d_cnt, n_cus, s));
    HIP_TRY(ev.mark(2, s));
    // the contract's verdict, and whether any key holds an N (the pipeline wants an nmask then, and takes its
    // paths for keys without N otherwise)
    unsigned long long got[CR_COUNT];
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, d_cnt, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s)); // (the tasks and the table have been read as well)
    memcpy(got, ctx->h_counters, sizeof(got));
    const unsigned long long bad = got[CR_BAD] + (got[CR_RISES] - got[CR_START_RISES]);
    if (bad)
        return fail(UMI_ERR_ORDER,
                    "%llu entries break the input contract (freq < 1, not in freq-descending rank order inside a bucket, "
                    "or an N base a given nmask does not cover)",
                    bad);
    umi_stats pst;
    memset(&pst, 0, sizeof(pst));
    if (nl) {
        uint64_t *nm = nullptr;
        if (got[CR_HAS_N]) {
            nm = (uint64_t *)io_at(ws, o_nm);
            HIP_TRY(launch_cr_nmask(ckeys, nl, umi_len, nm, n_cus, s));
        }
        if ((rc = run_pipeline(ctx, ckeys, nm, cfreq, lboff.data(), lboff.size() - 1, nl, umi_len, 1, 0.0f, MODE_NEIGHBOURS, 0,
                               nullptr, nullptr, s, &pst)))
            return rc;
        HIP_TRY(launch_cr_resolve(ctx->edges.as<uint2>(), (uint32_t)pst.n_edges, ckeys, cfreq, nl, umi_len, gidx,
                                  (int32_t *)io_at(ws, o_bf), (unsigned long long *)io_at(ws, o_bk), target, d_kept, d_cnt,
                                  n_cus, s));
    }
    HIP_TRY(ev.mark(3, s));
    HIP_TRY(launch_cr_finish(d_kept, target, n, d_root, d_cnt, n_cus, s));
    HIP_TRY(ev.mark(4, s));
    HIP_TRY(hipMemcpyAsync(ctx->h_counters, d_cnt, sizeof(got), hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    memcpy(got, ctx->h_counters, sizeof(got));
    st.n_kept = got[CR_KEPT];
    st.n_edges = got[CR_PAIRS];
    st.n_pairs_evaluated = pairs_small + pst.n_pairs_evaluated;
    st.n_candidates = pst.n_candidates;
    st.n_pair_launches = pst.n_pair_launches + (n_small ? 1u : 0u);
    if (ev.on) {
        float small_ms = 0, rest_ms = 0;
        HIP_TRY(hipEventElapsedTime(&st.ms_prep, ev.ev[0], ev.ev[1]));
        HIP_TRY(hipEventElapsedTime(&small_ms, ev.ev[1], ev.ev[2]));
        HIP_TRY(hipEventElapsedTime(&rest_ms, ev.ev[2], ev.ev[3]));
        HIP_TRY(hipEventElapsedTime(&st.ms_finalize, ev.ev[3], ev.ev[4]));
        HIP_TRY(hipEventElapsedTime(&st.ms_total, ev.ev[0], ev.ev[4]));
        st.ms_pairs = small_ms + pst.ms_total;                     // the small buckets' kernel and the pipeline
        st.ms_collapse = std::max(0.0f, rest_ms - pst.ms_total);   // the list's resolution (and the host's share of the wait)
    }
    if (stats) *stats = st;
    return UMI_OK;
}

} // namespace

extern "C" {

int umi_dedup_batch_cr_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                              const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint8_t *d_kept, uint32_t *d_root,
                              uint32_t *d_target, void *hip_stream, umi_stats *stats)
{
    uint64_t n = 0;
    int rc = cr_check_args(ctx, bucket_off, n_buckets, umi_len, &n);
    if (rc) return rc;
    if (n && (!d_keys || !d_freq || !d_kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        cr_empty_stats(stats, n_buckets);
        return UMI_OK;
    }
    return cr_run(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, d_kept, d_root, d_target,
                  (hipStream_t)hip_stream, stats);
}

int umi_dedup_batch_cr(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq, const uint64_t *bucket_off,
                       uint64_t n_buckets, int umi_len, uint8_t *kept, uint32_t *root, uint32_t *target, umi_stats *stats)
{
    uint64_t n = 0;
    int rc = cr_check_args(ctx, bucket_off, n_buckets, umi_len, &n);
    if (rc) return rc;
    if (n && (!keys || !freq || !kept)) return fail(UMI_ERR_ARG, "keys/freq/kept is NULL");
    if (n == 0) {
        cr_empty_stats(stats, n_buckets);
        return UMI_OK;
    }
    HostIo io(ctx);
    const auto d_keys = io.in(keys, (size_t)n * 8), d_nmask = io.in(nmask, (size_t)n * 8);
    const auto d_freq = io.in(freq, (size_t)n * 4);
    const auto d_kept = io.out(kept, n);
    const auto d_root = io.out(root, (size_t)n * 4), d_target = io.out(target, (size_t)n * 4);
    if ((rc = io.open()) ||
        (rc = cr_run(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, (uint32_t)n, umi_len, d_kept, d_root, d_target, io.stream(),
                     stats)) ||
        (rc = io.fetch(kept, d_kept, n)) || (rc = io.fetch(root, d_root, n)) || (rc = io.fetch(target, d_target, n)))
        return rc;
    return io.close();
}

} // extern "C"
