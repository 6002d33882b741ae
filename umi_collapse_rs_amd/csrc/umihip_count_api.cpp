// Tables over a call's result, and its filters: umi_count_matrix*, umi_velocity_matrix*, umi_saturation_curve*, umi_filter_multigene*, umi_dedup_stats*, umi_call_cells*.
#include "umihip_host.hpp"

#include <algorithm>

using namespace umihip;

// ---- what the calls over a bucket table share ---------------------------------------------------------
namespace {
// the first device of a multi-device context (as umi_correct_barcodes)
umi_ctx *first_device(umi_ctx *ctx) { return ctx->subs.empty() ? ctx : ctx->subs[0]; }

// what every *_check asks of the table itself (limit: the call files buckets by a 30-bit index)
int check_bucket_table(const uint64_t *bucket_off, uint64_t n_buckets, bool limit = true)
{
    if (limit && n_buckets >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu buckets exceed the 30-bit index space of one call", (unsigned long long)n_buckets);
    if (n_buckets && !bucket_off) return fail(UMI_ERR_ARG, "bucket_off is NULL");
    if (n_buckets && bucket_off[0] != 0) return fail(UMI_ERR_ARG, "bucket_off[0] must be 0");
    return UMI_OK;
}

// A table as the device code takes it, in the pinned staging: the m non-empty buckets' m + 1 offsets (a run of
// equal offsets is one) and, from the first empty bucket on, their numbers (null where nothing was left out).
struct BucketTable {
    uint32_t m = 0;
    const uint64_t *off = nullptr;
    const uint32_t *idx = nullptr;
};

// The table walked once into the pinned staging.  extra: pinned bytes of the call's own behind it, at *extra_at.
int cm_walk(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, BucketTable *t, size_t extra, unsigned long long **extra_at)
{
    int rc;
    const size_t off_bytes = ((size_t)n_buckets + 1) * 8, tables = (off_bytes + (size_t)n_buckets * 4 + 7) & ~(size_t)7;
    if ((rc = ctx->cm_h.reserve(tables + extra))) return rc;
    if (extra_at) *extra_at = (unsigned long long *)(ctx->cm_h.p + tables);
    uint64_t *o = (uint64_t *)ctx->cm_h.p;
    uint32_t *x = (uint32_t *)(ctx->cm_h.p + off_bytes);
    uint32_t k = 0;
    o[0] = 0;
    for (uint64_t b = 0; b < n_buckets; b++) {
        const uint64_t lo = bucket_off[b], hi = bucket_off[b + 1];
        if (hi < lo) return fail(UMI_ERR_ARG, "bucket_off is not monotone at bucket %llu", (unsigned long long)b);
        if (hi == lo) continue;
        x[k] = (uint32_t)b;
        o[++k] = hi;
    }
    t->m = k;
    t->off = o;
    t->idx = k == n_buckets ? nullptr : x;
    return UMI_OK;
}

// What a call does first once it has to touch its device (n_buckets >= 1): the device made current, a deferred call
// let end (its counters lie in the pinned block this call reads through), the table walked.
int table_begin(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, BucketTable *t, size_t extra = 0,
                unsigned long long **extra_at = nullptr)
{
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx);
    return cm_walk(ctx, bucket_off, n_buckets, t, extra, extra_at);
}
// ... and a matrix of no rows or no columns refused where a bucket is not empty
int matrix_begin(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n_rows, uint32_t n_cols, BucketTable *t,
                 size_t extra = 0, unsigned long long **extra_at = nullptr)
{
    if (int rc = table_begin(ctx, bucket_off, n_buckets, t, extra, extra_at)) return rc;
    if (t->m && (n_rows == 0 || n_cols == 0))
        return fail(UMI_ERR_ARG, "a matrix of %u rows and %u columns with a non-empty bucket", n_rows, n_cols);
    return UMI_OK;
}
} // namespace

// ---- molecules and reads per (column, row) pair ---------------------------------------------------
namespace {
// what both forms check before a device is looked at (the context last)
int cm_check(umi_ctx *ctx, const void *kept, const void *freq, const uint64_t *bucket_off, uint64_t n_buckets, const void *row,
             const void *col, const void *out_row, const void *out_col, const void *out_molecules, const void *out_reads,
             const uint64_t *nnz)
{
    if (!nnz) return fail(UMI_ERR_ARG, "nnz is NULL");
    if (int rc = check_bucket_table(bucket_off, n_buckets)) return rc;
    if (n_buckets && (!row || !col || !out_row || !out_col || !out_molecules || !out_reads))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] && (!kept || !freq)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

int cm_run(umi_ctx *ctx, const uint8_t *d_kept, const int32_t *d_freq, const BucketTable &t, const uint32_t *d_row,
           const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col,
           uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t *nnz, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(count_workspace_bytes(t.m, t.idx != nullptr)))) return rc;
    uint64_t bad = 0;
    const int r = count_matrix_on_device(ctx->call_ws.p, d_kept, d_freq, t.off, t.idx, t.m, d_row, d_col, n_rows, n_cols, d_out_row,
                                         d_out_col, d_out_molecules, d_out_reads, nnz, &bad, (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r < 0) return fail(UMI_ERR_HIP, "count matrix: %s", hipGetErrorString((hipError_t)(-r)));
    if (bad) {
        *nnz = 0;
        return fail(UMI_ERR_ARG, "%llu non-empty buckets have a row id of %u or more, or a column id of %u or more",
                    (unsigned long long)bad, n_rows, n_cols);
    }
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_count_matrix_device(umi_ctx *ctx, const uint8_t *d_kept, const int32_t *d_freq, const uint64_t *bucket_off,
                            uint64_t n_buckets, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols,
                            uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules, uint64_t *d_out_reads,
                            uint64_t *nnz, void *hip_stream)
{
    int rc = cm_check(ctx, d_kept, d_freq, bucket_off, n_buckets, d_row, d_col, d_out_row, d_out_col, d_out_molecules, d_out_reads, nnz);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz = 0;
    if (n_buckets == 0) return UMI_OK;
    BucketTable t;
    if ((rc = matrix_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, &t)) || t.m == 0) return rc;
    return cm_run(ctx, d_kept, d_freq, t, d_row, d_col, n_rows, n_cols, d_out_row, d_out_col, d_out_molecules,
                  d_out_reads, nnz, (hipStream_t)hip_stream);
}

int umi_count_matrix(umi_ctx *ctx, const uint8_t *kept, const int32_t *freq, const uint64_t *bucket_off, uint64_t n_buckets,
                     const uint32_t *row, const uint32_t *col, uint32_t n_rows, uint32_t n_cols, uint32_t *out_row,
                     uint32_t *out_col, uint32_t *out_molecules, uint64_t *out_reads, uint64_t *nnz)
{
    int rc = cm_check(ctx, kept, freq, bucket_off, n_buckets, row, col, out_row, out_col, out_molecules, out_reads, nnz);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz = 0;
    if (n_buckets == 0) return UMI_OK;
    BucketTable t;
    if ((rc = matrix_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, &t)) || t.m == 0) return rc;
    const size_t n = (size_t)bucket_off[n_buckets], nb = (size_t)n_buckets, cap = (size_t)t.m;
    HostIo io(ctx);
    const auto d_freq = io.in(freq, n * 4);
    const auto d_row = io.in(row, nb * 4), d_col = io.in(col, nb * 4);
    const auto d_orow = io.out(out_row, cap * 4), d_ocol = io.out(out_col, cap * 4), d_omol = io.out(out_molecules, cap * 4);
    const auto d_oreads = io.out(out_reads, cap * 8);
    const auto d_kept = io.in(kept, n);
    uint64_t got = 0;
    if ((rc = io.open()) ||
        (rc = cm_run(ctx, d_kept, d_freq, t, d_row, d_col, n_rows, n_cols, d_orow, d_ocol, d_omol, d_oreads, &got,
                     io.stream())) ||
        (rc = io.fetch(out_row, d_orow, (size_t)got)) || (rc = io.fetch(out_col, d_ocol, (size_t)got)) ||
        (rc = io.fetch(out_molecules, d_omol, (size_t)got)) || (rc = io.fetch(out_reads, d_oreads, (size_t)got)) ||
        (rc = io.close()))
        return rc;
    *nnz = got;
    return UMI_OK;
}

} // extern "C"

// ---- spliced, unspliced and ambiguous molecules per (column, row) pair --------------------------------
namespace {
// what both forms check before a device is looked at (the context last)
int vm_check(umi_ctx *ctx, const void *read_entry, const void *read_class, uint64_t n_reads, const void *kept, const void *root,
             const uint64_t *bucket_off, uint64_t n_buckets, const void *row, const void *col, const void *out_row, const void *out_col,
             const void *out_spliced, const void *out_unspliced, const void *out_ambiguous, const uint64_t *nnz)
{
    if (!nnz) return fail(UMI_ERR_ARG, "nnz is NULL");
    // (the reads' limit is told between the table's: after too many buckets, before a table that is missing)
    if (n_buckets < (1ull << 30) && n_reads >= (1ull << 32))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 32-bit index space of one call", (unsigned long long)n_reads);
    if (int rc = check_bucket_table(bucket_off, n_buckets)) return rc;
    if (n_buckets && (!row || !col || !out_row || !out_col || !out_spliced || !out_unspliced || !out_ambiguous))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] && (!kept || !root)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] && n_reads && (!read_entry || !read_class)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] >= (1ull << 32))
        return fail(UMI_ERR_ARG, "%llu entries exceed the 32-bit index space of root", (unsigned long long)bucket_off[n_buckets]);
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

int vm_run(umi_ctx *ctx, const uint32_t *d_read_entry, const uint8_t *d_read_class, uint64_t n_reads, const uint8_t *d_kept,
           const uint32_t *d_root, uint64_t n, const BucketTable &t, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows,
           uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_spliced,
           uint32_t *d_out_unspliced, uint32_t *d_out_ambiguous, uint64_t *nnz, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(velocity_workspace_bytes(n, t.m, t.idx != nullptr)))) return rc;
    uint64_t bad = 0, bad_read = 0;
    int kind = 0;
    const int r = velocity_matrix_on_device(ctx->call_ws.p, d_read_entry, d_read_class, (uint32_t)n_reads, d_kept, d_root, n, t.off,
                                            t.idx, t.m, d_row, d_col, n_rows, n_cols, d_out_row, d_out_col, d_out_spliced,
                                            d_out_unspliced, d_out_ambiguous, ctx->velocity_skip, nnz, &bad, &kind, &bad_read,
                                            (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r < 0) return fail(UMI_ERR_HIP, "velocity matrix: %s", hipGetErrorString((hipError_t)(-r)));
    if (bad || kind) *nnz = 0;
    if (bad)
        return fail(UMI_ERR_ARG, "%llu non-empty buckets have a row id of %u or more, or a column id of %u or more",
                    (unsigned long long)bad, n_rows, n_cols);
    if (kind == 1)
        return fail(UMI_ERR_ARG, "read %llu: its read_entry is neither below the %llu entries nor UMI_READ_UNSTAGED",
                    (unsigned long long)bad_read, (unsigned long long)n);
    if (kind == 2) return fail(UMI_ERR_ARG, "read %llu: a read_class above 4", (unsigned long long)bad_read);
    if (kind == 3)
        return fail(UMI_ERR_ARG, "read %llu: the root of its entry is not below the %llu entries", (unsigned long long)bad_read,
                    (unsigned long long)n);
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_velocity_matrix_device(umi_ctx *ctx, const uint32_t *d_read_entry, const uint8_t *d_read_class, uint64_t n_reads,
                               const uint8_t *d_kept, const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets,
                               const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols,
                               uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_spliced, uint32_t *d_out_unspliced,
                               uint32_t *d_out_ambiguous, uint64_t *nnz, void *hip_stream)
{
    int rc = vm_check(ctx, d_read_entry, d_read_class, n_reads, d_kept, d_root, bucket_off, n_buckets, d_row, d_col, d_out_row,
                      d_out_col, d_out_spliced, d_out_unspliced, d_out_ambiguous, nnz);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz = 0;
    if (n_buckets == 0) return UMI_OK;
    BucketTable t;
    if ((rc = matrix_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, &t)) || t.m == 0) return rc;
    return vm_run(ctx, d_read_entry, d_read_class, n_reads, d_kept, d_root, bucket_off[n_buckets], t, d_row, d_col,
                  n_rows, n_cols, d_out_row, d_out_col, d_out_spliced, d_out_unspliced, d_out_ambiguous, nnz, (hipStream_t)hip_stream);
}

int umi_velocity_matrix(umi_ctx *ctx, const uint32_t *read_entry, const uint8_t *read_class, uint64_t n_reads,
                        const uint8_t *kept, const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets,
                        const uint32_t *row, const uint32_t *col, uint32_t n_rows, uint32_t n_cols, uint32_t *out_row,
                        uint32_t *out_col, uint32_t *out_spliced, uint32_t *out_unspliced, uint32_t *out_ambiguous,
                        uint64_t *nnz)
{
    int rc = vm_check(ctx, read_entry, read_class, n_reads, kept, root, bucket_off, n_buckets, row, col, out_row, out_col, out_spliced,
                      out_unspliced, out_ambiguous, nnz);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz = 0;
    if (n_buckets == 0) return UMI_OK;
    BucketTable t;
    if ((rc = matrix_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, &t)) || t.m == 0) return rc;
    const size_t n = (size_t)bucket_off[n_buckets], nb = (size_t)n_buckets, cap = (size_t)t.m, nr = (size_t)n_reads;
    HostIo io(ctx);
    const auto d_entry = io.in(read_entry, nr * 4);
    const auto d_root = io.in(root, n * 4);
    const auto d_row = io.in(row, nb * 4), d_col = io.in(col, nb * 4);
    const auto d_orow = io.out(out_row, cap * 4), d_ocol = io.out(out_col, cap * 4);
    const auto d_os = io.out(out_spliced, cap * 4), d_ou = io.out(out_unspliced, cap * 4), d_oa = io.out(out_ambiguous, cap * 4);
    const auto d_class = io.in(read_class, nr);
    const auto d_kept = io.in(kept, n);
    uint64_t got = 0;
    if ((rc = io.open()) ||
        (rc = vm_run(ctx, d_entry, d_class, n_reads, d_kept, d_root, n, t, d_row, d_col, n_rows, n_cols, d_orow, d_ocol,
                     d_os, d_ou, d_oa, &got, io.stream())) ||
        (rc = io.fetch(out_row, d_orow, (size_t)got)) || (rc = io.fetch(out_col, d_ocol, (size_t)got)) ||
        (rc = io.fetch(out_spliced, d_os, (size_t)got)) || (rc = io.fetch(out_unspliced, d_ou, (size_t)got)) ||
        (rc = io.fetch(out_ambiguous, d_oa, (size_t)got)) || (rc = io.close()))
        return rc;
    *nnz = got;
    return UMI_OK;
}

} // extern "C"

// ---- saturation and medians per depth ---------------------------------------------------------------
namespace {
// what both forms check before a device is looked at (the context last)
int sc_check(umi_ctx *ctx, const void *read_entry, uint64_t n_reads, const void *kept, const void *root, const uint64_t *bucket_off,
             uint64_t n_buckets, const void *row, const void *col, uint32_t n_cols, int n_levels, const uint64_t *curve)
{
    if (!curve) return fail(UMI_ERR_ARG, "curve is NULL");
    if (n_levels < 1 || n_levels > 32) return fail(UMI_ERR_ARG, "n_levels %d outside 1..32", n_levels);
    if (n_reads >= (1ull << 32)) return fail(UMI_ERR_ARG, "%llu reads exceed the 32-bit index space of one call", (unsigned long long)n_reads);
    if (int rc = check_bucket_table(bucket_off, n_buckets)) return rc;
    if (n_buckets && (!row || !col)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] && (!kept || !root)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] && n_reads && !read_entry) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_buckets && bucket_off[n_buckets] >= (1ull << 32))
        return fail(UMI_ERR_ARG, "%llu entries exceed the 32-bit index space of root", (unsigned long long)bucket_off[n_buckets]);
    if (n_buckets && 2ull * (uint64_t)n_levels * n_cols >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%u columns at %d levels exceed the 30-bit index space of the call's sort", n_cols, n_levels);
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

// the table walked, with the pinned block of the call's own behind it; t->m == 0: the curve is all zeros and written
int sc_begin(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n_rows, uint32_t n_cols, int n_levels,
             uint64_t *curve, BucketTable *t, unsigned long long **h_pinned)
{
    int rc;
    if (n_buckets && (rc = matrix_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, t, (4 + 8 * (size_t)n_levels) * 8, h_pinned)))
        return rc;
    if (t->m == 0) memset(curve, 0, (size_t)n_levels * 8 * sizeof(uint64_t));
    return UMI_OK;
}

int sc_run(umi_ctx *ctx, const uint32_t *d_read_entry, uint64_t n_reads, const uint8_t *d_kept, const uint32_t *d_root, uint64_t n,
           const BucketTable &t, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint64_t seed,
           int n_levels, const uint8_t *d_cell_mask, unsigned long long *h_pinned, uint64_t *curve, hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(saturation_workspace_bytes(n, t.m, t.idx != nullptr, n_cols, n_levels)))) return rc;
    uint64_t bad = 0, bad_read = 0;
    int kind = 0;
    const int r = saturation_curve_on_device(ctx->call_ws.p, d_read_entry, (uint32_t)n_reads, d_kept, d_root, n, t.off, t.idx, t.m, d_row,
                                             d_col, n_rows, n_cols, seed, n_levels, d_cell_mask, ctx->saturation_skip, &bad, &kind,
                                             &bad_read, (uint32_t)ctx->n_cus, h_pinned, s);
    if (r < 0) return fail(UMI_ERR_HIP, "saturation curve: %s", hipGetErrorString((hipError_t)(-r)));
    if (bad)
        return fail(UMI_ERR_ARG, "%llu non-empty buckets have a row id of %u or more, or a column id of %u or more",
                    (unsigned long long)bad, n_rows, n_cols);
    if (kind == 1)
        return fail(UMI_ERR_ARG, "read %llu: its read_entry is neither below the %llu entries nor UMI_READ_UNSTAGED",
                    (unsigned long long)bad_read, (unsigned long long)n);
    if (kind == 2)
        return fail(UMI_ERR_ARG, "read %llu: the root of its entry is not below the %llu entries", (unsigned long long)bad_read,
                    (unsigned long long)n);
    memcpy(curve, h_pinned + 4, (size_t)n_levels * 8 * sizeof(uint64_t));
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_saturation_curve_device(umi_ctx *ctx, const uint32_t *d_read_entry, uint64_t n_reads, const uint8_t *d_kept,
                                const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *d_row,
                                const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint64_t seed, int n_levels,
                                const uint8_t *d_cell_mask, uint64_t *curve, void *hip_stream)
{
    int rc = sc_check(ctx, d_read_entry, n_reads, d_kept, d_root, bucket_off, n_buckets, d_row, d_col, n_cols, n_levels, curve);
    if (rc) return rc;
    ctx = first_device(ctx);
    BucketTable t;
    unsigned long long *h_pinned = nullptr;
    if ((rc = sc_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, n_levels, curve, &t, &h_pinned)) || t.m == 0) return rc;
    return sc_run(ctx, d_read_entry, n_reads, d_kept, d_root, bucket_off[n_buckets], t, d_row, d_col, n_rows, n_cols, seed,
                  n_levels, d_cell_mask, h_pinned, curve, (hipStream_t)hip_stream);
}

int umi_saturation_curve(umi_ctx *ctx, const uint32_t *read_entry, uint64_t n_reads, const uint8_t *kept, const uint32_t *root,
                         const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *row, const uint32_t *col, uint32_t n_rows,
                         uint32_t n_cols, uint64_t seed, int n_levels, const uint8_t *cell_mask, uint64_t *curve)
{
    int rc = sc_check(ctx, read_entry, n_reads, kept, root, bucket_off, n_buckets, row, col, n_cols, n_levels, curve);
    if (rc) return rc;
    ctx = first_device(ctx);
    BucketTable t;
    unsigned long long *h_pinned = nullptr;
    if ((rc = sc_begin(ctx, bucket_off, n_buckets, n_rows, n_cols, n_levels, curve, &t, &h_pinned)) || t.m == 0) return rc;
    const size_t n = (size_t)bucket_off[n_buckets], nb = (size_t)n_buckets;
    HostIo io(ctx);
    const auto d_entry = io.in(read_entry, (size_t)n_reads * 4);
    const auto d_root = io.in(root, n * 4);
    const auto d_row = io.in(row, nb * 4), d_col = io.in(col, nb * 4);
    const auto d_kept = io.in(kept, n);
    const auto d_mask = io.in(cell_mask, (size_t)n_cols);
    if ((rc = io.open()) ||
        (rc = sc_run(ctx, d_entry, n_reads, d_kept, d_root, n, t, d_row, d_col, n_rows, n_cols, seed, n_levels, d_mask,
                     h_pinned, curve, io.stream())) ||
        (rc = io.close()))
        return rc;
    return UMI_OK;
}

} // extern "C"

// ---- molecules and reads per (column, splice junction) pair --------------------------------------------
namespace {
// what both forms check before a device is looked at (the context last)
int jm_check(umi_ctx *ctx, const void *read_ref, const void *read_pos, const void *cigar, const void *cigar_off, const void *read_entry,
             uint64_t n_reads, const void *kept, const void *root, const uint64_t *bucket_off, uint64_t n_buckets, const void *col,
             const void *jn_ref, const void *jn_start, const void *jn_end, const void *out_jn, const void *out_col,
             const void *out_molecules, const void *out_reads, const uint64_t *counts)
{
    if (!counts) return fail(UMI_ERR_ARG, "counts is NULL");
    // (the reads' limit is told between the table's: after too many buckets, before a table that is missing)
    if (n_buckets < (1ull << 30) && n_reads >= (1ull << 32))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 32-bit index space of one call", (unsigned long long)n_reads);
    if (int rc = check_bucket_table(bucket_off, n_buckets)) return rc;
    if (n_buckets && bucket_off[n_buckets] && n_reads) {
        if (!col || !kept || !root) return fail(UMI_ERR_ARG, "a required pointer is NULL");
        if (!read_ref || !read_pos || !cigar || !cigar_off || !read_entry) return fail(UMI_ERR_ARG, "a required pointer is NULL");
        if (!jn_ref || !jn_start || !jn_end || !out_jn || !out_col || !out_molecules || !out_reads)
            return fail(UMI_ERR_ARG, "a required pointer is NULL");
    }
    if (n_buckets && bucket_off[n_buckets] >= (1ull << 32))
        return fail(UMI_ERR_ARG, "%llu entries exceed the 32-bit index space of root", (unsigned long long)bucket_off[n_buckets]);
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

// the table walked; t->m == 0: nothing to do
int jm_begin(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, uint64_t n_reads, uint32_t n_cols, BucketTable *t)
{
    int rc;
    if (n_buckets == 0 || n_reads == 0) return UMI_OK;
    if ((rc = table_begin(ctx, bucket_off, n_buckets, t))) return rc;
    if (t->m && n_cols == 0) return fail(UMI_ERR_ARG, "a matrix of no columns with a non-empty bucket");
    return UMI_OK;
}

int jm_run(umi_ctx *ctx, const int32_t *d_ref, const int32_t *d_pos, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
           const uint32_t *d_read_entry, uint64_t n_reads, const uint8_t *d_kept, const uint32_t *d_root, uint64_t n,
           const BucketTable &t, const uint32_t *d_col, uint32_t n_cols, uint64_t capacity, int32_t *d_jn_ref,
           int32_t *d_jn_start, int32_t *d_jn_end, uint32_t *d_out_jn, uint32_t *d_out_col, uint32_t *d_out_molecules,
           uint64_t *d_out_reads, uint64_t counts[4], hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(junction_count_workspace_bytes((uint32_t)n_reads, t.m, t.idx != nullptr)))) return rc;
    JunctionCounted got;
    int r = junction_count_on_device(ctx->call_ws.p, d_ref, d_pos, d_cigar, d_cigar_off, d_read_entry, (uint32_t)n_reads, d_kept, d_root, n,
                                     t.off, t.idx, t.m, d_col, n_cols, &got, (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r < 0) return fail(UMI_ERR_HIP, "junction matrix: %s", hipGetErrorString((hipError_t)(-r)));
    const unsigned long long at = (unsigned long long)got.bad_read;
    switch (got.bad_kind) {
    case 1: return fail(UMI_ERR_ORDER, "read %llu: cigar_off falls", at);
    case 2:
        return fail(UMI_ERR_ARG, "read %llu: its read_entry is neither below the %llu entries nor UMI_READ_UNSTAGED", at,
                    (unsigned long long)n);
    case 3: return fail(UMI_ERR_ARG, "read %llu: the root of its entry is not below the %llu entries", at, (unsigned long long)n);
    case 4: return fail(UMI_ERR_ARG, "read %llu: read_ref < 0", at);
    case 5: return fail(UMI_ERR_ARG, "read %llu: a CIGAR op code above 8", at);
    default: break;
    }
    if (got.bad_cols)
        return fail(UMI_ERR_ARG, "%llu non-empty buckets have a column id of %u or more", (unsigned long long)got.bad_cols, n_cols);
    if (got.occurrences > capacity || got.occurrences >= (1ull << 30)) {
        counts[1] = got.occurrences;
        return fail(UMI_ERR_ARG, "%llu junction occurrences exceed the capacity of %llu, or the 30-bit index space of one call",
                    (unsigned long long)got.occurrences, (unsigned long long)capacity);
    }
    if (got.occurrences == 0) return UMI_OK;
    if ((rc = ctx->jn_ws.reserve(junction_fill_workspace_bytes((uint32_t)got.occurrences)))) return rc;
    uint64_t junctions = 0, nnz = 0;
    r = junction_fill_on_device(ctx->call_ws.p, ctx->jn_ws.p, d_ref, d_pos, d_cigar, d_cigar_off, d_read_entry, (uint32_t)n_reads, d_kept,
                                d_root, n, t.m, t.idx != nullptr, n_cols, got, d_jn_ref, d_jn_start, d_jn_end, d_out_jn, d_out_col,
                                d_out_molecules, d_out_reads, &junctions, &nnz, (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r < 0) return fail(UMI_ERR_HIP, "junction matrix: %s", hipGetErrorString((hipError_t)(-r)));
    counts[0] = got.spliced;
    counts[1] = got.occurrences;
    counts[2] = junctions;
    counts[3] = nnz;
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_junction_matrix_device(umi_ctx *ctx, const int32_t *d_read_ref, const int32_t *d_read_pos, const uint32_t *d_cigar,
                               const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint64_t n_reads, const uint8_t *d_kept,
                               const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *d_col,
                               uint32_t n_cols, uint64_t capacity, int32_t *d_jn_ref, int32_t *d_jn_start, int32_t *d_jn_end,
                               uint32_t *d_out_jn, uint32_t *d_out_col, uint32_t *d_out_molecules, uint64_t *d_out_reads,
                               uint64_t counts[4], void *hip_stream)
{
    int rc = jm_check(ctx, d_read_ref, d_read_pos, d_cigar, d_cigar_off, d_read_entry, n_reads, d_kept, d_root, bucket_off, n_buckets,
                      d_col, d_jn_ref, d_jn_start, d_jn_end, d_out_jn, d_out_col, d_out_molecules, d_out_reads, counts);
    if (rc) return rc;
    ctx = first_device(ctx);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    BucketTable t;
    if ((rc = jm_begin(ctx, bucket_off, n_buckets, n_reads, n_cols, &t)) || t.m == 0) return rc;
    return jm_run(ctx, d_read_ref, d_read_pos, d_cigar, d_cigar_off, d_read_entry, n_reads, d_kept, d_root, bucket_off[n_buckets], t,
                  d_col, n_cols, capacity, d_jn_ref, d_jn_start, d_jn_end, d_out_jn, d_out_col, d_out_molecules,
                  d_out_reads, counts, (hipStream_t)hip_stream);
}

int umi_junction_matrix(umi_ctx *ctx, const int32_t *read_ref, const int32_t *read_pos, const uint32_t *cigar,
                        const uint64_t *cigar_off, const uint32_t *read_entry, uint64_t n_reads, const uint8_t *kept,
                        const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *col, uint32_t n_cols,
                        uint64_t capacity, int32_t *jn_ref, int32_t *jn_start, int32_t *jn_end, uint32_t *out_jn, uint32_t *out_col,
                        uint32_t *out_molecules, uint64_t *out_reads, uint64_t counts[4])
{
    int rc = jm_check(ctx, read_ref, read_pos, cigar, cigar_off, read_entry, n_reads, kept, root, bucket_off, n_buckets, col, jn_ref,
                      jn_start, jn_end, out_jn, out_col, out_molecules, out_reads, counts);
    if (rc) return rc;
    ctx = first_device(ctx);
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    BucketTable t;
    if ((rc = jm_begin(ctx, bucket_off, n_buckets, n_reads, n_cols, &t)) || t.m == 0) return rc;
    const size_t n = (size_t)bucket_off[n_buckets], nb = (size_t)n_buckets, nr = (size_t)n_reads;
    const size_t cap = (size_t)std::min<uint64_t>(capacity, (1ull << 30) - 1), words = (size_t)cigar_off[n_reads];
    HostIo io(ctx);
    const auto d_off = io.in(cigar_off, (nr + 1) * 8);
    const auto d_oreads = io.out(out_reads, cap * 8);
    const auto d_ref = io.in(read_ref, nr * 4), d_pos = io.in(read_pos, nr * 4);
    const auto d_cigar = io.in(cigar, words * 4, 4); // (a slot, and an address, even for no word)
    const auto d_entry = io.in(read_entry, nr * 4);
    const auto d_root = io.in(root, n * 4);
    const auto d_col = io.in(col, nb * 4);
    const auto d_jref = io.out(jn_ref, cap * 4), d_jstart = io.out(jn_start, cap * 4), d_jend = io.out(jn_end, cap * 4);
    const auto d_ojn = io.out(out_jn, cap * 4), d_ocol = io.out(out_col, cap * 4), d_omol = io.out(out_molecules, cap * 4);
    const auto d_kept = io.in(kept, n);
    uint64_t got[4] = {0, 0, 0, 0};
    if ((rc = io.open()) ||
        (rc = jm_run(ctx, d_ref, d_pos, d_cigar, d_off, d_entry, n_reads, d_kept, d_root, n, t, d_col, n_cols, capacity,
                     d_jref, d_jstart, d_jend, d_ojn, d_ocol, d_omol, d_oreads, got, io.stream()))) {
        counts[1] = got[1]; // (the occurrences a larger capacity has to hold)
        return rc;
    }
    if ((rc = io.fetch(jn_ref, d_jref, (size_t)got[2])) || (rc = io.fetch(jn_start, d_jstart, (size_t)got[2])) ||
        (rc = io.fetch(jn_end, d_jend, (size_t)got[2])) || (rc = io.fetch(out_jn, d_ojn, (size_t)got[3])) ||
        (rc = io.fetch(out_col, d_ocol, (size_t)got[3])) || (rc = io.fetch(out_molecules, d_omol, (size_t)got[3])) ||
        (rc = io.fetch(out_reads, d_oreads, (size_t)got[3])) || (rc = io.close()))
        return rc;
    for (int k = 0; k < 4; k++) counts[k] = got[k];
    return UMI_OK;
}

} // extern "C"

// ---- UMIs a group shows in several buckets ----------------------------------------------------------
namespace {
// what both forms check before a device is looked at (the context last)
int mg_check(umi_ctx *ctx, const void *keys, int n_words, int umi_len, const void *freq, const void *kept, const void *root,
             const uint64_t *bucket_off, uint64_t n_buckets, const void *group, const void *kept_out, const void *freq_out,
             const uint64_t *counts)
{
    if (!counts) return fail(UMI_ERR_ARG, "counts is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    if (int rc = check_bucket_table(bucket_off, n_buckets)) return rc;
    const uint64_t n = n_buckets ? bucket_off[n_buckets] : 0; // (a table that falls: cm_walk's finding, on its one walk)
    if (n >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu entries exceed the 30-bit index space of the call's sort", (unsigned long long)n);
    if (n && (!keys || !freq || !kept || !root || !group || !kept_out)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n && (kept_out == kept || (freq_out && freq_out == freq))) return fail(UMI_ERR_ARG, "an output is its own input");
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

// everything on the device (the context is the call's device, settled)
int mg_run(umi_ctx *ctx, const uint64_t *d_keys, int n_words, int umi_len, const int32_t *d_freq, const uint8_t *d_kept,
           const uint32_t *d_root, const BucketTable &t, const uint32_t *d_group,
           uint32_t n_groups, uint8_t *d_kept_out, int32_t *d_freq_out, uint64_t counts[3], hipStream_t s)
{
    int rc;
    MultigeneCall c;
    c.d_keys = d_keys;
    c.d_freq = d_freq;
    c.d_kept = d_kept;
    c.d_root = d_root;
    c.d_group = d_group;
    c.h_off = t.off;
    c.h_idx = t.idx;
    c.n = (uint32_t)t.off[t.m];
    c.m = t.m;
    c.n_groups = n_groups;
    c.n_cus = (uint32_t)ctx->n_cus;
    c.umi_len = umi_len;
    c.n_words = n_words;
    c.d_kept_out = d_kept_out;
    c.d_freq_out = d_freq_out;
    c.h_pinned = ctx->h_counters;
    if ((rc = ctx->call_ws.reserve(multigene_workspace_bytes(c.n, t.m, t.idx != nullptr)))) return rc;
    const int r = multigene_on_device(ctx->call_ws.p, c, s);
    if (r < 0) return fail(UMI_ERR_HIP, "multi-gene filter: %s", hipGetErrorString((hipError_t)(-r)));
    if (ctx->h_counters[0])
        return fail(UMI_ERR_ARG, "%llu non-empty buckets have a group id of %u or more", (unsigned long long)ctx->h_counters[0], n_groups);
    if (ctx->h_counters[1])
        return fail(UMI_ERR_ARG, "%llu entries have a root outside their bucket, at an entry that was not kept, or are kept "
                                 "with another root than themselves", (unsigned long long)ctx->h_counters[1]);
    for (int i = 0; i < 3; i++) counts[i] = ctx->h_counters[2 + i];
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_filter_multigene_device(umi_ctx *ctx, const uint64_t *d_keys, int n_words, int umi_len, const int32_t *d_freq,
                                const uint8_t *d_kept, const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets,
                                const uint32_t *d_group, uint32_t n_groups, uint8_t *d_kept_out, int32_t *d_freq_out,
                                uint64_t counts[3], void *hip_stream)
{
    int rc = mg_check(ctx, d_keys, n_words, umi_len, d_freq, d_kept, d_root, bucket_off, n_buckets, d_group, d_kept_out, d_freq_out, counts);
    if (rc) return rc;
    ctx = first_device(ctx);
    counts[0] = counts[1] = counts[2] = 0;
    if (n_buckets == 0 || bucket_off[n_buckets] == 0) return UMI_OK;
    if (n_groups == 0) return fail(UMI_ERR_ARG, "no groups with a non-empty bucket");
    BucketTable t;
    if ((rc = table_begin(ctx, bucket_off, n_buckets, &t))) return rc;
    return mg_run(ctx, d_keys, n_words, umi_len, d_freq, d_kept, d_root, t, d_group, n_groups, d_kept_out, d_freq_out, counts,
                  (hipStream_t)hip_stream);
}

int umi_filter_multigene(umi_ctx *ctx, const uint64_t *keys, int n_words, int umi_len, const int32_t *freq, const uint8_t *kept,
                         const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *group,
                         uint32_t n_groups, uint8_t *kept_out, int32_t *freq_out, uint64_t counts[3])
{
    int rc = mg_check(ctx, keys, n_words, umi_len, freq, kept, root, bucket_off, n_buckets, group, kept_out, freq_out, counts);
    if (rc) return rc;
    ctx = first_device(ctx);
    counts[0] = counts[1] = counts[2] = 0;
    if (n_buckets == 0 || bucket_off[n_buckets] == 0) return UMI_OK;
    if (n_groups == 0) return fail(UMI_ERR_ARG, "no groups with a non-empty bucket");
    BucketTable t;
    if ((rc = table_begin(ctx, bucket_off, n_buckets, &t))) return rc; // (before anything is copied)
    const size_t n = (size_t)bucket_off[n_buckets], nb = (size_t)n_buckets;
    HostIo io(ctx);
    const auto d_keys = io.in(keys, n * 8 * (size_t)n_words);
    const auto d_freq = io.in(freq, n * 4);
    const auto d_root = io.in(root, n * 4);
    const auto d_group = io.in(group, nb * 4);
    const auto d_fout = io.out(freq_out, n * 4);
    const auto d_kept = io.in(kept, n);
    const auto d_kout = io.out(kept_out, n);
    if ((rc = io.open()) ||
        (rc = mg_run(ctx, d_keys, n_words, umi_len, d_freq, d_kept, d_root, t, d_group, n_groups, d_kout, d_fout, counts, io.stream())) ||
        (rc = io.fetch(kept_out, d_kout, n)) || (rc = io.fetch(freq_out, d_fout, n)) || (rc = io.close()))
        return rc;
    return UMI_OK;
}

} // extern "C"

// ---- family sizes, UMI distances and UMI usage of a batched call ------------------------------------
namespace {
struct DsShape { // what the checks find out
    uint64_t n = 0;  // entries
    uint32_t m = 0;  // non-empty buckets
    bool per_umi = false;
};
// what both forms check before a device is looked at (the context last)
int ds_check(umi_ctx *ctx, const void *keys, int n_words, const void *freq, const void *kept, const void *root,
             const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint32_t hist_bins, const void *count_pre,
             const void *count_post, const void *dist, const void *umi_entry, const void *times_pre, const void *reads_pre,
             const void *times_post, const void *reads_post, const uint64_t *n_umis, DsShape *shape)
{
    if (!count_pre || !count_post || !dist) return fail(UMI_ERR_ARG, "count_pre, count_post or dist is NULL");
    const int given = (umi_entry != nullptr) + (times_pre != nullptr) + (reads_pre != nullptr) + (times_post != nullptr) +
                      (reads_post != nullptr);
    if (given != 0 && given != 5) return fail(UMI_ERR_ARG, "the five arrays of the per-UMI table are given together or not at all");
    if (given && !n_umis) return fail(UMI_ERR_ARG, "n_umis is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != (3 * umi_len + 63) / 64) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", (3 * umi_len + 63) / 64, umi_len);
    if (hist_bins < 2 || hist_bins > (1u << 24)) return fail(UMI_ERR_ARG, "hist_bins %u outside 2..2^24", hist_bins);
    // (any number of buckets: it is the entries that are limited, below)
    if (int rc = check_bucket_table(bucket_off, n_buckets, false)) return rc;
    uint64_t m = 0;
    for (uint64_t b = 0; b < n_buckets; b++) {
        const uint64_t lo = bucket_off[b], hi = bucket_off[b + 1];
        if (hi < lo) return fail(UMI_ERR_ARG, "bucket_off is not monotone at bucket %llu", (unsigned long long)b);
        if (hi - lo >= (1ull << 28))
            return fail(UMI_ERR_ARG, "bucket %llu has %llu entries, 2^28 or more", (unsigned long long)b, (unsigned long long)(hi - lo));
        if (hi >= (1ull << 31)) return fail(UMI_ERR_ARG, "%llu entries exceed the 31-bit index space of one call", (unsigned long long)hi);
        m += hi != lo;
    }
    const uint64_t n = n_buckets ? bucket_off[n_buckets] : 0;
    if (n && (!keys || !freq || !kept || !root)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (given && n >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu entries exceed the 30-bit index space of the per-UMI table's sort", (unsigned long long)n);
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    shape->n = n;
    shape->m = (uint32_t)m;
    shape->per_umi = given != 0;
    return UMI_OK;
}

// everything on the device; *rows: the per-UMI table's rows
int ds_run(umi_ctx *ctx, const DsShape &shape, const uint64_t *d_keys, int n_words, const int32_t *d_freq, const uint8_t *d_kept,
           const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t seed, uint32_t hist_bins,
           uint64_t *d_count_pre, uint64_t *d_count_post, uint64_t *d_dist, uint32_t *d_umi_entry, uint32_t *d_times_pre,
           uint64_t *d_reads_pre, uint32_t *d_times_post, uint64_t *d_reads_post, uint64_t *rows, hipStream_t s)
{
    int rc;
    const uint32_t n = (uint32_t)shape.n, m = shape.m;
    // the pinned block: the non-empty buckets' offsets | the deep buckets' pieces | their numbers (room for the most
    // there can be: a deep bucket has at least 64 entries)
    const size_t deep_max = std::min<size_t>(m, n / 64), tasks_max = n / STATS_PIECE + deep_max;
    const size_t o_tasks = ((size_t)m + 1) * 8, o_deep = o_tasks + tasks_max * sizeof(StatsTask);
    if ((rc = ctx->ds_h.reserve(o_deep + deep_max * 4))) return rc;
    uint64_t *h_off = (uint64_t *)ctx->ds_h.p;
    {
        uint32_t k = 0;
        h_off[0] = 0;
        for (uint64_t b = 0; b < n_buckets; b++)
            if (bucket_off[b + 1] != bucket_off[b]) h_off[++k] = bucket_off[b + 1];
    }
    StatsCall c;
    stats_plan(h_off, m, ctx->stats_split, umi_len, &c.split, &c.n_deep, &c.n_tasks);
    if (c.n_deep > deep_max || c.n_tasks > tasks_max) return fail(UMI_ERR_HIP, "internal: %u deep buckets in %u pieces", c.n_deep, c.n_tasks);
    if ((rc = ctx->call_ws.reserve(stats_workspace_bytes(n, m, c.n_deep, c.n_tasks, umi_len, shape.per_umi)))) return rc;
    c.d_keys = d_keys;
    c.d_freq = d_freq;
    c.d_kept = d_kept;
    c.d_root = d_root;
    c.h_off = h_off;
    c.n = n;
    c.m = m;
    c.hist_bins = hist_bins;
    c.n_cus = (uint32_t)ctx->n_cus;
    c.umi_len = umi_len;
    c.n_words = n_words;
    c.seed = seed;
    c.d_count_pre = d_count_pre;
    c.d_count_post = d_count_post;
    c.d_dist = d_dist;
    c.d_umi_entry = d_umi_entry;
    c.d_times_pre = d_times_pre;
    c.d_times_post = d_times_post;
    c.d_reads_pre = d_reads_pre;
    c.d_reads_post = d_reads_post;
    c.h_tasks = (StatsTask *)(ctx->ds_h.p + o_tasks);
    c.h_deep_j = (uint32_t *)(ctx->ds_h.p + o_deep);
    c.h_pinned = ctx->h_counters;
    ctx->h_counters[2] = 0;
    const int r = stats_on_device(ctx->call_ws.p, c, s);
    if (r < 0) return fail(UMI_ERR_HIP, "dedup stats: %s", hipGetErrorString((hipError_t)(-r)));
    if (ctx->h_counters[0])
        return fail(UMI_ERR_ARG, "%llu keys hold a code that is none of A, C, G, T, N below base %d",
                    (unsigned long long)ctx->h_counters[0], umi_len);
    if (ctx->h_counters[1])
        return fail(UMI_ERR_ARG, "%llu entries have a root outside their bucket, at an entry that was not kept, or are kept "
                                 "with another root than themselves", (unsigned long long)ctx->h_counters[1]);
    *rows = shape.per_umi ? ctx->h_counters[2] : 0;
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_dedup_stats_device(umi_ctx *ctx, const uint64_t *d_keys, int n_words, const int32_t *d_freq, const uint8_t *d_kept,
                           const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t seed,
                           uint32_t hist_bins, uint64_t *d_count_pre, uint64_t *d_count_post, uint64_t *d_dist,
                           uint32_t *d_umi_entry, uint32_t *d_times_pre, uint64_t *d_reads_pre, uint32_t *d_times_post,
                           uint64_t *d_reads_post, uint64_t *n_umis, void *hip_stream)
{
    DsShape shape;
    int rc = ds_check(ctx, d_keys, n_words, d_freq, d_kept, d_root, bucket_off, n_buckets, umi_len, hist_bins, d_count_pre,
                      d_count_post, d_dist, d_umi_entry, d_times_pre, d_reads_pre, d_times_post, d_reads_post, n_umis, &shape);
    if (rc) return rc;
    ctx = first_device(ctx);
    if (n_umis) *n_umis = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    if (shape.m == 0) {
        HIP_TRY(hipMemsetAsync(d_count_pre, 0, (size_t)hist_bins * 8, s));
        HIP_TRY(hipMemsetAsync(d_count_post, 0, (size_t)hist_bins * 8, s));
        HIP_TRY(hipMemsetAsync(d_dist, 0, 4 * ((size_t)umi_len + 2) * 8, s));
        HIP_TRY(hipStreamSynchronize(s));
        return UMI_OK;
    }
    uint64_t rows = 0;
    rc = ds_run(ctx, shape, d_keys, n_words, d_freq, d_kept, d_root, bucket_off, n_buckets, umi_len, seed, hist_bins, d_count_pre,
                d_count_post, d_dist, d_umi_entry, d_times_pre, d_reads_pre, d_times_post, d_reads_post, &rows, s);
    if (rc) return rc;
    if (n_umis) *n_umis = rows;
    return UMI_OK;
}

int umi_dedup_stats(umi_ctx *ctx, const uint64_t *keys, int n_words, const int32_t *freq, const uint8_t *kept, const uint32_t *root,
                    const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t seed, uint32_t hist_bins,
                    uint64_t *count_pre, uint64_t *count_post, uint64_t *dist, uint32_t *umi_entry, uint32_t *times_pre,
                    uint64_t *reads_pre, uint32_t *times_post, uint64_t *reads_post, uint64_t *n_umis)
{
    DsShape shape;
    int rc = ds_check(ctx, keys, n_words, freq, kept, root, bucket_off, n_buckets, umi_len, hist_bins, count_pre, count_post, dist,
                      umi_entry, times_pre, reads_pre, times_post, reads_post, n_umis, &shape);
    if (rc) return rc;
    ctx = first_device(ctx);
    if (n_umis) *n_umis = 0;
    const size_t dist_words = 4 * ((size_t)umi_len + 2);
    if (shape.m == 0) { // (nothing is launched)
        memset(count_pre, 0, (size_t)hist_bins * 8);
        memset(count_post, 0, (size_t)hist_bins * 8);
        memset(dist, 0, dist_words * 8);
        return UMI_OK;
    }
    const size_t n = (size_t)shape.n, hist = (size_t)hist_bins;
    HostIo io(ctx);
    const auto d_keys = io.in(keys, n * 8 * (size_t)n_words);
    const auto d_freq = io.in(freq, n * 4);
    const auto d_root = io.in(root, n * 4);
    const auto d_pre = io.out(count_pre, hist * 8), d_post = io.out(count_post, hist * 8), d_dist = io.out(dist, dist_words * 8);
    // (the per-UMI table: absent as one)
    const auto d_entry = io.out(umi_entry, n * 4), d_tpre = io.out(times_pre, n * 4);
    const auto d_rpre = io.out(reads_pre, n * 8);
    const auto d_tpost = io.out(times_post, n * 4);
    const auto d_rpost = io.out(reads_post, n * 8);
    const auto d_kept = io.in(kept, n);
    uint64_t rows = 0;
    if ((rc = io.open()) ||
        (rc = ds_run(ctx, shape, d_keys, n_words, d_freq, d_kept, d_root, bucket_off, n_buckets, umi_len, seed, hist_bins, d_pre,
                     d_post, d_dist, d_entry, d_tpre, d_rpre, d_tpost, d_rpost, &rows, io.stream())) ||
        (rc = io.fetch(count_pre, d_pre, hist)) || (rc = io.fetch(count_post, d_post, hist)) ||
        (rc = io.fetch(dist, d_dist, dist_words)) || (rc = io.fetch(umi_entry, d_entry, (size_t)rows)) ||
        (rc = io.fetch(times_pre, d_tpre, (size_t)rows)) || (rc = io.fetch(reads_pre, d_rpre, (size_t)rows)) ||
        (rc = io.fetch(times_post, d_tpost, (size_t)rows)) || (rc = io.fetch(reads_post, d_rpost, (size_t)rows)) ||
        (rc = io.close()))
        return rc;
    if (n_umis) *n_umis = rows;
    return UMI_OK;
}

} // extern "C"

// ---- which columns of a count matrix are cells ------------------------------------------------------
namespace {
static_assert(UMI_CELLS_CR22 == CELLS_CR22 && UMI_CELLS_TOP == CELLS_TOP && UMI_CELLS_MIN == CELLS_MIN, "one numbering of the rules");

struct CellsRuleArgs { // what the kernels take of a rule's parameters
    unsigned long long pick = 0, ratio = 1, min_molecules = 0;
};
// what both forms check before a device is looked at (the context last)
int cc_check(umi_ctx *ctx, const void *row, const void *col, const void *molecules, const void *reads, uint64_t nnz, uint32_t n_rows,
             uint32_t n_cols, int rule, int64_t expect_cells, int percentile_permille, int64_t max_min_ratio, int64_t min_molecules,
             const void *cell_molecules, const void *cell_reads, const void *cell_genes, const void *called, const void *new_col,
             const void *out_row, const void *out_col, const void *out_molecules, const void *out_reads, const uint64_t *nnz_out,
             const uint64_t *counts, CellsRuleArgs *ra)
{
    if (!nnz_out || !counts) return fail(UMI_ERR_ARG, "nnz_out or counts is NULL");
    if (nnz >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu triplets exceed the 30-bit index space of one call", (unsigned long long)nnz);
    if (n_cols >= (1u << 30)) return fail(UMI_ERR_ARG, "%u columns exceed the 30-bit index space of the call's sort", n_cols);
    if (nnz && (n_rows == 0 || n_cols == 0)) return fail(UMI_ERR_ARG, "a matrix of %u rows and %u columns with a triplet", n_rows, n_cols);
    if (rule != UMI_CELLS_CR22 && rule != UMI_CELLS_TOP && rule != UMI_CELLS_MIN) return fail(UMI_ERR_ARG, "unknown rule %d", rule);
    if (rule != UMI_CELLS_MIN && expect_cells < 1) return fail(UMI_ERR_ARG, "expect_cells %lld below 1", (long long)expect_cells);
    if (rule == UMI_CELLS_CR22 && (percentile_permille < 0 || percentile_permille > 1000))
        return fail(UMI_ERR_ARG, "percentile_permille %d outside 0..1000", percentile_permille);
    if (rule == UMI_CELLS_CR22 && max_min_ratio < 1) return fail(UMI_ERR_ARG, "max_min_ratio %lld below 1", (long long)max_min_ratio);
    if (n_cols && (!cell_molecules || !cell_reads || !cell_genes || !called || !new_col)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (nnz && (!row || !col || !molecules || !reads || !out_row || !out_col || !out_molecules || !out_reads))
        return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    // (the index is the smaller of this and n - 1 < 2^30: 2^40 cells stand for any number above)
    const unsigned long long cells = (unsigned long long)std::min<int64_t>(std::max<int64_t>(expect_cells, 1), (int64_t)1 << 40);
    ra->pick = rule == UMI_CELLS_CR22 ? cells * (unsigned long long)(1000 - percentile_permille) / 1000ull : cells - 1ull;
    ra->ratio = (unsigned long long)std::max<int64_t>(max_min_ratio, 1);
    ra->min_molecules = (unsigned long long)std::max<int64_t>(min_molecules, 0);
    return UMI_OK;
}

// everything on the device (the context is the call's device, settled; nnz >= 1)
int cc_run(umi_ctx *ctx, const uint32_t *d_row, const uint32_t *d_col, const uint32_t *d_molecules, const uint64_t *d_reads, uint64_t nnz,
           uint32_t n_rows, uint32_t n_cols, int rule, const CellsRuleArgs &ra, uint64_t *d_cell_molecules, uint64_t *d_cell_reads,
           uint32_t *d_cell_genes, uint8_t *d_called, uint32_t *d_new_col, uint32_t *d_out_row, uint32_t *d_out_col,
           uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t *nnz_out, uint64_t counts[10], hipStream_t s)
{
    int rc;
    CellsCall c;
    c.d_row = d_row;
    c.d_col = d_col;
    c.d_molecules = d_molecules;
    c.d_reads = d_reads;
    c.nnz = (uint32_t)nnz;
    c.n_rows = n_rows;
    c.n_cols = n_cols;
    c.n_cus = (uint32_t)ctx->n_cus;
    c.rule = rule;
    c.pick = ra.pick;
    c.ratio = ra.ratio;
    c.min_molecules = ra.min_molecules;
    c.d_cell_molecules = d_cell_molecules;
    c.d_cell_reads = d_cell_reads;
    c.d_cell_genes = d_cell_genes;
    c.d_new_col = d_new_col;
    c.d_called = d_called;
    c.d_out_row = d_out_row;
    c.d_out_col = d_out_col;
    c.d_out_molecules = d_out_molecules;
    c.d_out_reads = d_out_reads;
    c.h_pinned = ctx->h_counters;
    static_assert(CELLS_CTL_WORDS + 1 <= CNT_COUNT, "the pinned words of the call lie in the control block's mirror");
    if ((rc = ctx->call_ws.reserve(cells_workspace_bytes(c.nnz, n_cols)))) return rc;
    const int r = call_cells_on_device(ctx->call_ws.p, c, s);
    if (r < 0) return fail(UMI_ERR_HIP, "call cells: %s", hipGetErrorString((hipError_t)(-r)));
    const unsigned long long *h = ctx->h_counters;
    if (h[0])
        return fail(UMI_ERR_ARG, "%llu triplets have a row id of %u or more, or a column id of %u or more", h[0], n_rows, n_cols);
    if (h[1]) return fail(UMI_ERR_ORDER, "%llu triplets are not above their predecessor in (col, row)", h[1]);
    // candidates, called, t, m, molecules and reads in called columns, all molecules, all reads, the two medians
    const int from[10] = {2, 9, 5, 6, 7, 8, 3, 4, 10, 11};
    for (int i = 0; i < 10; i++) counts[i] = h[from[i]];
    *nnz_out = h[CELLS_CTL_WORDS];
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_call_cells_device(umi_ctx *ctx, const uint32_t *d_row, const uint32_t *d_col, const uint32_t *d_molecules,
                          const uint64_t *d_reads, uint64_t nnz, uint32_t n_rows, uint32_t n_cols, int rule, int64_t expect_cells,
                          int percentile_permille, int64_t max_min_ratio, int64_t min_molecules, uint64_t *d_cell_molecules,
                          uint64_t *d_cell_reads, uint32_t *d_cell_genes, uint8_t *d_called, uint32_t *d_new_col, uint32_t *d_out_row,
                          uint32_t *d_out_col, uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t *nnz_out, uint64_t counts[10],
                          void *hip_stream)
{
    CellsRuleArgs ra;
    int rc = cc_check(ctx, d_row, d_col, d_molecules, d_reads, nnz, n_rows, n_cols, rule, expect_cells, percentile_permille, max_min_ratio,
                      min_molecules, d_cell_molecules, d_cell_reads, d_cell_genes, d_called, d_new_col, d_out_row, d_out_col,
                      d_out_molecules, d_out_reads, nnz_out, counts, &ra);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz_out = 0;
    for (int i = 0; i < 10; i++) counts[i] = 0;
    hipStream_t s = (hipStream_t)hip_stream;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    if (nnz == 0) { // (no kernel is launched)
        if (n_cols == 0) return UMI_OK;
        HIP_TRY(hipMemsetAsync(d_cell_molecules, 0, (size_t)n_cols * 8, s));
        HIP_TRY(hipMemsetAsync(d_cell_reads, 0, (size_t)n_cols * 8, s));
        HIP_TRY(hipMemsetAsync(d_cell_genes, 0, (size_t)n_cols * 4, s));
        HIP_TRY(hipMemsetAsync(d_called, 0, (size_t)n_cols, s));
        HIP_TRY(hipMemsetAsync(d_new_col, 0xFF, (size_t)n_cols * 4, s));
        HIP_TRY(hipStreamSynchronize(s));
        return UMI_OK;
    }
    return cc_run(ctx, d_row, d_col, d_molecules, d_reads, nnz, n_rows, n_cols, rule, ra, d_cell_molecules, d_cell_reads, d_cell_genes,
                  d_called, d_new_col, d_out_row, d_out_col, d_out_molecules, d_out_reads, nnz_out, counts, s);
}

int umi_call_cells(umi_ctx *ctx, const uint32_t *row, const uint32_t *col, const uint32_t *molecules, const uint64_t *reads,
                   uint64_t nnz, uint32_t n_rows, uint32_t n_cols, int rule, int64_t expect_cells, int percentile_permille,
                   int64_t max_min_ratio, int64_t min_molecules, uint64_t *cell_molecules, uint64_t *cell_reads, uint32_t *cell_genes,
                   uint8_t *called, uint32_t *new_col, uint32_t *out_row, uint32_t *out_col, uint32_t *out_molecules,
                   uint64_t *out_reads, uint64_t *nnz_out, uint64_t counts[10])
{
    CellsRuleArgs ra;
    int rc = cc_check(ctx, row, col, molecules, reads, nnz, n_rows, n_cols, rule, expect_cells, percentile_permille, max_min_ratio,
                      min_molecules, cell_molecules, cell_reads, cell_genes, called, new_col, out_row, out_col, out_molecules, out_reads,
                      nnz_out, counts, &ra);
    if (rc) return rc;
    ctx = first_device(ctx);
    *nnz_out = 0;
    for (int i = 0; i < 10; i++) counts[i] = 0;
    const size_t nc = (size_t)n_cols, nz = (size_t)nnz;
    if (nnz == 0) { // (nothing is launched)
        if (nc) {
            memset(cell_molecules, 0, nc * 8);
            memset(cell_reads, 0, nc * 8);
            memset(cell_genes, 0, nc * 4);
            memset(called, 0, nc);
            memset(new_col, 0xFF, nc * 4);
        }
        return UMI_OK;
    }
    HostIo io(ctx);
    const auto d_reads = io.in(reads, nz * 8);
    const auto d_row = io.in(row, nz * 4), d_col = io.in(col, nz * 4), d_mol = io.in(molecules, nz * 4);
    const auto d_cmol = io.out(cell_molecules, nc * 8), d_creads = io.out(cell_reads, nc * 8);
    const auto d_oreads = io.out(out_reads, nz * 8);
    const auto d_cgenes = io.out(cell_genes, nc * 4), d_newcol = io.out(new_col, nc * 4);
    const auto d_orow = io.out(out_row, nz * 4), d_ocol = io.out(out_col, nz * 4), d_omol = io.out(out_molecules, nz * 4);
    const auto d_called = io.out(called, nc);
    uint64_t got = 0;
    if ((rc = io.open()) ||
        (rc = cc_run(ctx, d_row, d_col, d_mol, d_reads, nnz, n_rows, n_cols, rule, ra, d_cmol, d_creads, d_cgenes, d_called, d_newcol,
                     d_orow, d_ocol, d_omol, d_oreads, &got, counts, io.stream())) ||
        (rc = io.fetch(cell_molecules, d_cmol, nc)) || (rc = io.fetch(cell_reads, d_creads, nc)) ||
        (rc = io.fetch(cell_genes, d_cgenes, nc)) || (rc = io.fetch(called, d_called, nc)) || (rc = io.fetch(new_col, d_newcol, nc)) ||
        (rc = io.fetch(out_row, d_orow, (size_t)got)) || (rc = io.fetch(out_col, d_ocol, (size_t)got)) ||
        (rc = io.fetch(out_molecules, d_omol, (size_t)got)) || (rc = io.fetch(out_reads, d_oreads, (size_t)got)) || (rc = io.close())) {
        for (int i = 0; i < 10; i++) counts[i] = 0;
        return rc;
    }
    *nnz_out = got;
    return UMI_OK;
}

} // extern "C"
