// The per-bucket DataStruct path: struct umi_data, umi_data_*.
#include "umihip_host.hpp"

#include <algorithm>
#include <memory>
#include <new>

using namespace umihip;

struct umi_data {
    umi_ctx *ctx = nullptr;
    uint32_t n = 0;
    int max_edits = 0;
    std::vector<int32_t> freq;
    std::vector<uint8_t> present;
    // CSR of neighbours with dist <= max_edits (both directions), sorted by index
    std::vector<uint64_t> off;
    std::vector<uint32_t> nbr;
    std::vector<uint8_t> nbr_dist;
};

extern "C" {

int umi_data_new(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                 uint32_t n, int umi_len, int max_edits, umi_data **out)
{
    return umi_data_new_wide(ctx, keys, nmask, 1, freq, n, umi_len, max_edits, out);
}

int umi_data_new_wide(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                      uint32_t n, int umi_len, int max_edits, umi_data **out)
{
    if (!out) return fail(UMI_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // one bucket's store lives on one device
    if (n && (!keys || !freq)) return fail(UMI_ERR_ARG, "keys/freq is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != (3 * umi_len + 63) / 64) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", (3 * umi_len + 63) / 64, umi_len);
    if (max_edits < 0) return fail(UMI_ERR_ARG, "max_edits must be >= 0");
    if (n >= 0x7FFFFFF0u) // same index space as the batched calls (bit 31 of an edge endpoint is a flag)
        return fail(UMI_ERR_ARG, "%u entries exceed the 31-bit index space of one store", n);
    std::unique_ptr<umi_data> d(new (std::nothrow) umi_data());
    if (!d) return fail(UMI_ERR_NOMEM, "out of host memory");
    d->ctx = ctx;
    d->n = n;
    d->max_edits = max_edits;
    d->freq.assign(freq, freq + n);
    d->present.assign(n, 1);
    d->off.assign((size_t)n + 1, 0);
    if (n >= 2) {
        int rc;
        const size_t kb = (size_t)n * 8 * (size_t)n_words;
        // the neighbour build ignores freq and order; feed ones so that prep's
        // contract check (rank order) does not apply to an unordered map
        const std::vector<int32_t> ones(n, 1);
        HostIo io(ctx);
        const auto d_keys = io.in(keys, kb), d_nmask = io.in(nmask, kb);
        const auto d_freq = io.in(ones.data(), (size_t)n * 4);
        if ((rc = io.open()) || (rc = io.close())) return rc; // (closed at once: the copies are done while `ones` lives)
        const uint64_t boff[2] = {0, n};
        umi_stats st;
        rc = run_pipeline(ctx, d_keys, d_nmask, d_freq, boff, 1, n, umi_len, max_edits, 0.0f, MODE_NEIGHBOURS, 0, nullptr,
                          nullptr, io.stream(), &st, nullptr, n_words);
        if (rc) return rc;
        const size_t E = (size_t)st.n_edges;
        std::vector<uint2> pairs(E);
        std::vector<uint8_t> pd(E);
        if (E) {
            hipError_t e = hipMemcpy(pairs.data(), ctx->edges.p, E * sizeof(uint2), hipMemcpyDeviceToHost);
            if (e == hipSuccess) e = hipMemcpy(pd.data(), ctx->edge_dist.p, E, hipMemcpyDeviceToHost);
            if (e != hipSuccess)
                return fail(UMI_ERR_HIP, "download failed: %s", hipGetErrorString(e));
        }
        for (size_t i = 0; i < E; i++) {
            d->off[pairs[i].x + 1]++;
            d->off[pairs[i].y + 1]++;
        }
        for (uint32_t i = 0; i < n; i++) d->off[i + 1] += d->off[i];
        d->nbr.resize(2 * E);
        d->nbr_dist.resize(2 * E);
        std::vector<uint64_t> fill(d->off.begin(), d->off.end() - 1);
        for (size_t i = 0; i < E; i++) {
            uint64_t pa = fill[pairs[i].x]++, pb = fill[pairs[i].y]++;
            d->nbr[pa] = pairs[i].y; d->nbr_dist[pa] = pd[i];
            d->nbr[pb] = pairs[i].x; d->nbr_dist[pb] = pd[i];
        }
        // ascending neighbour index inside each row (the device appends in arrival order)
        std::vector<std::pair<uint32_t, uint8_t>> tmp;
        for (uint32_t i = 0; i < n; i++) {
            const uint64_t a = d->off[i], b = d->off[i + 1];
            tmp.clear();
            for (uint64_t t = a; t < b; t++) tmp.emplace_back(d->nbr[t], d->nbr_dist[t]);
            std::sort(tmp.begin(), tmp.end());
            for (uint64_t t = a; t < b; t++) {
                d->nbr[t] = tmp[t - a].first;
                d->nbr_dist[t] = tmp[t - a].second;
            }
        }
    }
    *out = d.release();
    return UMI_OK;
}

int umi_data_remove_near(umi_data *d, uint32_t query, int k, int32_t max_freq, uint32_t *out_idx,
                         uint32_t *out_n)
{
    if (!d || !out_n || (!out_idx && d->n)) return fail(UMI_ERR_ARG, "NULL argument");
    if (query >= d->n) return fail(UMI_ERR_ARG, "query %u outside 0..%u", query, d->n);
    if (k > d->max_edits)
        return fail(UMI_ERR_ARG, "k %d exceeds max_edits %d given to umi_data_new", k, d->max_edits);
    // naive.rs:29-37 over the precomputed neighbour row; merge the query itself
    // (dist 0, removed whatever its freq) in index order
    uint32_t cnt = 0;
    bool self_done = false;
    auto emit_self = [&]() {
        if (!self_done && k >= 0 && d->present[query]) {
            d->present[query] = 0;
            out_idx[cnt++] = query;
        }
        self_done = true;
    };
    for (uint64_t t = d->off[query]; t < d->off[query + 1]; t++) {
        const uint32_t o = d->nbr[t];
        if (o > query) emit_self();
        if (d->present[o] && (int)d->nbr_dist[t] <= k &&
            (d->nbr_dist[t] == 0 || d->freq[o] <= max_freq)) {
            d->present[o] = 0;
            out_idx[cnt++] = o;
        }
    }
    emit_self();
    *out_n = cnt;
    return UMI_OK;
}

int umi_data_contains(const umi_data *d, uint32_t idx)
{
    if (!d) return fail(UMI_ERR_ARG, "d is NULL");
    if (idx >= d->n) return fail(UMI_ERR_ARG, "idx %u outside 0..%u", idx, d->n);
    return d->present[idx] ? 1 : 0;
}

void umi_data_free(umi_data *d) { delete d; }

} // extern "C"
