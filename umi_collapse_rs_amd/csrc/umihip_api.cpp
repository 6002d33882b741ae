// Host side of libumihip.so, the C ABI of include/umihip.h: the error text, the context and its options
// here; the pipeline of a batched call in umihip_pipeline.cpp, the entry points in files of their own
// (umihip_batch.cpp, umihip_*_api.cpp, umihip_data.cpp); umihip_host.hpp is what they share.
// The product path has no CPU fallback: every entry point that computes needs the
// gfx950 kernels in this same library and a live HIP device.
#include "umihip_host.hpp"

#include <algorithm>
#include <cstdarg>
#include <cstdio>
#include <new>

using namespace umihip;

namespace umihip {

namespace {
thread_local std::string g_err;
}

int fail(int code, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

const std::string &last_error() { return g_err; }

int check_common(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k,
                 int algo, uint64_t *n_out, int max_len)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!bucket_off) return fail(UMI_ERR_ARG, "bucket_off is NULL");
    if (umi_len < 1 || umi_len > max_len)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, max_len);
    if (k < 0) return fail(UMI_ERR_ARG, "k must be >= 0 (got %d)", k);
    if (!known_algo(algo))
        return fail(UMI_ERR_ARG, "unknown algo %d", algo);
    // (that the table is monotone is checked while it is copied to its pinned staging buffer,
    // before anything is launched: Pipeline::upload_table, umihip_pipeline.cpp)
    const uint64_t n = n_buckets ? bucket_off[n_buckets] : 0;
    if (n_buckets && bucket_off[0] != 0) return fail(UMI_ERR_ARG, "bucket_off[0] must be 0");
    if (n >= 0x7FFFFFF0ull) // bit 31 of an edge endpoint is a flag
        return fail(UMI_ERR_ARG, "%llu entries exceed the 31-bit index space of one call",
                    (unsigned long long)n);
    *n_out = n;
    return UMI_OK;
}

} // namespace umihip

extern "C" {

const char *umi_last_error(void) { return last_error().c_str(); }

int umi_abi_version(void) { return UMI_ABI_VERSION; }

int umi_ctx_create(int device_id, umi_ctx **out)
{
    if (!out) return fail(UMI_ERR_ARG, "out is NULL");
    *out = nullptr;
    int n_dev = 0;
    hipError_t e = hipGetDeviceCount(&n_dev);
    if (e != hipSuccess || n_dev == 0)
        return fail(UMI_ERR_NODEV, "no HIP device visible (%s)",
                    e == hipSuccess ? "device count 0" : hipGetErrorString(e));
    if (device_id < 0 || device_id >= n_dev)
        return fail(UMI_ERR_ARG, "device_id %d outside 0..%d", device_id, n_dev - 1);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(UMI_ERR_NODEV, "device %d is %s; this library carries gfx950 code only",
                    device_id, prop.gcnArchName);
    HIP_TRY(hipSetDevice(device_id));
    umi_ctx *ctx = new (std::nothrow) umi_ctx();
    if (!ctx) return fail(UMI_ERR_NOMEM, "out of host memory");
    ctx->device = device_id;
    ctx->device_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    ctx->n_cus = ctx->device_cus;
    hipError_t err = hipStreamCreateWithFlags(&ctx->own_stream, hipStreamNonBlocking);
    if (err == hipSuccess)
        err = hipHostMalloc((void **)&ctx->h_counters, CTRL_BYTES + 64);
    if (err == hipSuccess) *ctx->h_seq() = 0;
    for (int i = 0; i < umi_ctx::N_EVENTS && err == hipSuccess; i++) err = hipEventCreate(&ctx->ev[i]);

    if (err != hipSuccess) {
        umi_ctx_destroy(ctx);
        return fail(UMI_ERR_HIP, "context setup failed: %s", hipGetErrorString(err));
    }
    *out = ctx;
    return UMI_OK;
}

void umi_ctx_destroy(umi_ctx *ctx)
{
    if (!ctx) return;
    if (!ctx->subs.empty()) { // a multi-device context: nothing of its own on a device
        for (ncclComm_t c : ctx->comms)
            if (c && ctx->rccl.CommDestroy) (void)ctx->rccl.CommDestroy(c);
        for (umi_ctx *sub : ctx->subs) umi_ctx_destroy(sub);
        delete ctx;
        return;
    }
    settle(ctx);
    (void)hipSetDevice(ctx->device); // the workspace frees itself in `delete`: with its device current
    // The control block's mirror, the events and the stream go ahead of the buffers; the order does not matter:
    // every host-buffer call drains own_stream before it returns, settle() has ended a deferred call, and
    // hipFree synchronises.
    if (ctx->h_counters) (void)hipHostFree(ctx->h_counters);
    for (int i = 0; i < umi_ctx::N_EVENTS; i++)
        if (ctx->ev[i]) (void)hipEventDestroy(ctx->ev[i]);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int umi_ctx_get_counter(const umi_ctx *ctx, const char *name, uint64_t *out)
{
    if (!ctx || !name || !out) return fail(UMI_ERR_ARG, "ctx/name/out is NULL");
    if (!strcmp(name, "seg_cross_launches")) *out = ctx->seg_cross_launches;
    else if (!strcmp(name, "seg_cross_abandoned")) *out = ctx->seg_cross_abandoned_calls;
    else return fail(UMI_ERR_ARG, "unknown counter '%s'", name);
    return UMI_OK;
}

int umi_ctx_set_option(umi_ctx *ctx, const char *name, int64_t value)
{
    if (!ctx || !name) return fail(UMI_ERR_ARG, "ctx/name is NULL");
    if (!strcmp(name, "split_min")) {
        if (value < 2) return fail(UMI_ERR_ARG, "split_min must be >= 2");
        ctx->split_min = (uint64_t)value;
        return UMI_OK;
    }
    if (!ctx->subs.empty()) { // every device of a multi-device context
        for (umi_ctx *sub : ctx->subs) {
            const int rc = umi_ctx_set_option(sub, name, value);
            if (rc) return rc;
        }
        return UMI_OK;
    }
    if (!strcmp(name, "profile")) {
        ctx->profile = value != 0;
    } else if (!strcmp(name, "edge_capacity")) {
        if (value < 1) return fail(UMI_ERR_ARG, "edge_capacity must be >= 1");
        ctx->edge_capacity = (uint64_t)value;
#ifdef UMIHIP_DEV
    } else if (!strcmp(name, "prune")) {
        ctx->prune = value != 0;
    } else if (!strcmp(name, "bs_unit")) {
        if (value < 1 || value > 3) return fail(UMI_ERR_ARG, "bs_unit must be 1, 2 or 3");
        ctx->bs_unit = (int)value;
    } else if (!strcmp(name, "bs_sorted")) {
        ctx->bs_sorted = value != 0;
    } else if (!strcmp(name, "bs_tables")) {
        ctx->bs_tables = value != 0;
    } else if (!strcmp(name, "two_phase")) {
        if (value < 0 || value > 2) return fail(UMI_ERR_ARG, "two_phase must be 0, 1 or 2");
        ctx->two_phase = (int)value;
    } else if (!strcmp(name, "bs_col_chunk")) {
        if (value < BS_COL_TILE || value > (1 << 24) || value % BS_COL_TILE)
            return fail(UMI_ERR_ARG, "bs_col_chunk must be a multiple of %d in %d..%d", BS_COL_TILE,
                        BS_COL_TILE, 1 << 24);
        ctx->bs_col_chunk = (uint32_t)value;
    } else if (!strcmp(name, "bs_tab_min_run")) {
        if (value < 0 || value > (1 << 30)) return fail(UMI_ERR_ARG, "bs_tab_min_run must be in 0..2^30");
        ctx->bs_tab_min_run = (uint32_t)value;
    } else if (!strcmp(name, "bs_transposed")) {
        ctx->bs_transposed = value != 0;
    } else if (!strcmp(name, "bs_tab_waves")) {
        if (value < 0 || value > (1 << 20)) return fail(UMI_ERR_ARG, "bs_tab_waves must be in 0..%d", 1 << 20);
        ctx->bs_tab_waves = (uint32_t)value;
    } else if (!strcmp(name, "bitslice")) {
        ctx->use_bitslice = value != 0;
    } else if (!strcmp(name, "ovf_capacity")) {
        if (value < 1) return fail(UMI_ERR_ARG, "ovf_capacity must be >= 1");
        ctx->ovf_capacity = (uint64_t)value;
#endif
    } else if (!strcmp(name, "seg_index")) {
        ctx->seg_index = value != 0;
    } else if (!strcmp(name, "table_pieces")) {
        if (value < 1 || value > 64) return fail(UMI_ERR_ARG, "table_pieces must be in 1..64");
        ctx->table_pieces = (uint32_t)value;
    } else if (!strcmp(name, "seg_ckey")) {
        ctx->seg_ckey = value != 0;
    } else if (!strcmp(name, "spin_wait")) {
        ctx->spin_wait = value != 0;
    } else if (!strcmp(name, "seg_sliced")) {
        ctx->seg_sliced = value != 0;
    } else if (!strcmp(name, "seg_unite")) {
        ctx->seg_unite = value != 0;
    } else if (!strcmp(name, "seg_lds")) {
        ctx->seg_lds = value != 0;
    } else if (!strcmp(name, "seg_local")) {
        ctx->seg_local = value != 0;
    } else if (!strcmp(name, "seg_probe")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "seg_probe must be 0 or 1");
        ctx->seg_probe = value != 0;
    } else if (!strcmp(name, "seg_probe_min")) {
        if (value < 2 || value > SEG_LOCAL_MAX_CAP) return fail(UMI_ERR_ARG, "seg_probe_min must be in 2..%u", SEG_LOCAL_MAX_CAP);
        ctx->seg_probe_min = (uint32_t)value;
    } else if (!strcmp(name, "seg_super")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "seg_super must be 0 or 1");
        ctx->seg_super = value != 0;
    } else if (!strcmp(name, "seg_super_coarse")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "seg_super_coarse must be 0 or 1");
        ctx->seg_super_coarse = value != 0;
    } else if (!strcmp(name, "seg_cross")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "seg_cross must be 0 or 1");
        ctx->seg_cross = value != 0;
        ctx->seg_cross_failed = false; // (armed again)
    } else if (!strcmp(name, "seg_cross_map_mb")) {
        if (value < 0 || value > 64) return fail(UMI_ERR_ARG, "seg_cross_map_mb must be in 0..64");
        ctx->seg_cross_map_mb = (uint32_t)value;
    } else if (!strcmp(name, "seg_super_bases")) {
        if (value < 0 || value > SEG_SUPER_MAX_BASES) return fail(UMI_ERR_ARG, "seg_super_bases must be in 0..%d", SEG_SUPER_MAX_BASES);
        ctx->seg_super_bases = (int)value;
    } else if (!strcmp(name, "seg_super_cap")) {
        if (value < 2 || value > SEG_SUPER_MAX_CAP) return fail(UMI_ERR_ARG, "seg_super_cap must be in 2..%u", SEG_SUPER_MAX_CAP);
        ctx->seg_super_cap = (uint32_t)value;
    } else if (!strcmp(name, "seg_super_min")) {
        if (value < 2 || value > SEG_SUPER_MAX_CAP) return fail(UMI_ERR_ARG, "seg_super_min must be in 2..%u", SEG_SUPER_MAX_CAP);
        ctx->seg_super_min = (uint32_t)value;
    } else if (!strcmp(name, "collapse_kept_only")) {
        ctx->collapse_kept_only = value != 0;
    } else if (!strcmp(name, "seg_local_cap")) {
        if (value < 2 || value > SEG_LOCAL_MAX_CAP) return fail(UMI_ERR_ARG, "seg_local_cap must be in 2..%u", SEG_LOCAL_MAX_CAP);
        ctx->seg_local_cap = (uint32_t)value;
    } else if (!strcmp(name, "seg_blocks")) {
        if (value < 0 || value > (1 << 22)) return fail(UMI_ERR_ARG, "seg_blocks must be in 0..2^22");
        ctx->seg_blocks = (uint32_t)value;
    } else if (!strcmp(name, "grid_cus")) {
        if (value < 0 || value > ctx->device_cus)
            return fail(UMI_ERR_ARG, "grid_cus must be in 0..%d (the device's CUs)", ctx->device_cus);
        ctx->n_cus = value ? (int)value : ctx->device_cus;
    } else if (!strcmp(name, "seg_min")) {
        if (value < 2 || value > (1ll << 31)) return fail(UMI_ERR_ARG, "seg_min must be in 2..2^31");
        ctx->seg_min = (uint32_t)value;
    } else if (!strcmp(name, "cons_split")) {
        if (value < 2 || value > (1ll << 30)) return fail(UMI_ERR_ARG, "cons_split must be in 2..2^30");
        ctx->cons_split = (uint32_t)value;
    } else if (!strcmp(name, "cr_small_max")) {
        if (value < 0 || value > CR_SMALL_MAX_CAP) return fail(UMI_ERR_ARG, "cr_small_max must be in 0..%u", CR_SMALL_MAX_CAP);
        ctx->cr_small_max = (uint32_t)value;
    } else if (!strcmp(name, "stats_split")) {
        if (value < 64 || value > (1ll << 30)) return fail(UMI_ERR_ARG, "stats_split must be in 64..2^30");
        ctx->stats_split = (uint32_t)value;
    } else if (!strcmp(name, "gene_top")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "gene_top must be 0 or 1");
        ctx->gene_top = value != 0;
    } else if (!strcmp(name, "gene_body_top")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "gene_body_top must be 0 or 1");
        ctx->gene_body_top = value != 0;
    } else if (!strcmp(name, "velocity_skip")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "velocity_skip must be 0 or 1");
        ctx->velocity_skip = value != 0;
    } else if (!strcmp(name, "saturation_skip")) {
        if (value != 0 && value != 1) return fail(UMI_ERR_ARG, "saturation_skip must be 0 or 1");
        ctx->saturation_skip = value != 0;
    } else if (!strcmp(name, "fused_sliced")) {
        ctx->fused_sliced = value != 0;
    } else if (!strcmp(name, "fused_blocks")) {
        if (value < 1 || value > 64) return fail(UMI_ERR_ARG, "fused_blocks must be in 1..64");
        ctx->fused_blocks = (uint32_t)value;
    } else if (!strcmp(name, "fused_max")) {
        if (value < 0) return fail(UMI_ERR_ARG, "fused_max must be >= 0");
        ctx->fused_max = (uint32_t)std::min<int64_t>(value, FUSED_MAX);
    } else if (!strcmp(name, "small_max")) {
        if (value < 0) return fail(UMI_ERR_ARG, "small_max must be >= 0");
        ctx->small_max = (uint32_t)std::min<int64_t>(value, 1 << 30);
    } else {
        return fail(UMI_ERR_ARG, "unknown option '%s'", name);
    }
    return UMI_OK;
}

int umi_ctx_create_multi(const int *device_ids, int n_devices, umi_ctx **out)
{
    if (!out) return fail(UMI_ERR_ARG, "out is NULL");
    *out = nullptr;
    if (!device_ids || n_devices < 1 || n_devices > 64)
        return fail(UMI_ERR_ARG, "device_ids is NULL or n_devices outside 1..64");
    umi_ctx *ctx = new (std::nothrow) umi_ctx();
    if (!ctx) return fail(UMI_ERR_NOMEM, "out of host memory");
    for (int i = 0; i < n_devices; i++) {
        umi_ctx *sub = nullptr;
        const int rc = umi_ctx_create(device_ids[i], &sub);
        if (rc) {
            const std::string msg = umi_last_error();
            umi_ctx_destroy(ctx);
            return fail(rc, "%s", msg.c_str());
        }
        ctx->subs.push_back(sub);
    }
    ctx->device = device_ids[0];
    *out = ctx;
    return UMI_OK;
}

int umi_ctx_device_count(const umi_ctx *ctx) { return !ctx ? 0 : (ctx->subs.empty() ? 1 : (int)ctx->subs.size()); }

} // extern "C"
