// Correction to a fixed list: umi_correct_umis*, umi_correct_barcodes*, umi_correct_barcodes_multi*.
#include "umihip_host.hpp"

#include <algorithm>

using namespace umihip;

// ---- correction of UMIs to a fixed list -----------------------------------------------------------
namespace {
// the checks both forms share, and the list packed for the device (2 bits per base)
int corr_check(umi_ctx *ctx, const void *umi, uint64_t n_reads, int umi_len, const uint8_t *whitelist_ascii, uint32_t n_wl,
               int max_mismatches, int min_distance, const void *match, const uint64_t *counts, std::vector<uint32_t> &packed)
{
    // (the context is looked at last: everything before it is decided without a device)
    if (!counts) return fail(UMI_ERR_ARG, "counts is NULL");
    if (!whitelist_ascii) return fail(UMI_ERR_ARG, "whitelist_ascii is NULL");
    if (n_wl == 0) return fail(UMI_ERR_ARG, "the whitelist is empty");
    if (n_wl > CORR_MAX_LIST) return fail(UMI_ERR_ARG, "a whitelist of %u UMIs, more than %u", n_wl, CORR_MAX_LIST);
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN)
        return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (max_mismatches < 0) return fail(UMI_ERR_ARG, "max_mismatches must be >= 0 (got %d)", max_mismatches);
    if (min_distance < 0) return fail(UMI_ERR_ARG, "min_distance must be >= 0 (got %d)", min_distance);
    if (n_reads >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one call", (unsigned long long)n_reads);
    if (n_reads && (!umi || !match)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    packed.resize((size_t)n_wl * correct_words(umi_len));
    uint64_t bad = 0;
    if (correct_pack_list(whitelist_ascii, n_wl, umi_len, packed.data(), &bad)) {
        const uint8_t *e = whitelist_ascii + (size_t)bad * umi_len;
        int b = 0;
        while (e[b] == 'A' || e[b] == 'C' || e[b] == 'G' || e[b] == 'T') b++;
        return fail(UMI_ERR_CHAR, "Unknown character in whitelist: %u (entry %llu)", (unsigned)e[b], (unsigned long long)bad);
    }
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

int corr_run(umi_ctx *ctx, const uint8_t *d_umi_ascii, uint64_t n_reads, int umi_len, const std::vector<uint32_t> &packed,
             uint32_t n_wl, int max_mismatches, int min_distance, uint8_t *d_out_ascii, int32_t *d_match, uint8_t *d_best,
             uint8_t *d_second, uint64_t counts[3], hipStream_t s)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(correct_workspace_bytes(n_wl, umi_len)))) return rc;
    uint64_t bad_read = 0;
    // (a max_mismatches of umi_len or more lets every distance pass; min_distance is compared as it is)
    const int r = correct_on_device(ctx->call_ws.p, d_umi_ascii, (uint32_t)n_reads, umi_len, packed.data(), n_wl,
                                    std::min(max_mismatches, umi_len), min_distance, d_out_ascii, d_match, d_best, d_second,
                                    counts, &bad_read, (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r == 1) {
        uint8_t u[UMI_MAX_WIDE_UMI_LEN];
        HIP_TRY(hipMemcpyAsync(u, d_umi_ascii + (size_t)bad_read * umi_len, (size_t)umi_len, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int b = 0;
        while (b < umi_len - 1 && (u[b] == 'A' || u[b] == 'T' || u[b] == 'C' || u[b] == 'G' || u[b] == 'N')) b++;
        return fail(UMI_ERR_CHAR, "Unknown character in UMI sequence: %u (read %llu)", (unsigned)u[b],
                    (unsigned long long)bad_read);
    }
    if (r < 0) return fail(UMI_ERR_HIP, "UMI correction: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}
} // namespace

extern "C" {

int umi_correct_umis_device(umi_ctx *ctx, const uint8_t *d_umi_ascii, uint64_t n_reads, int umi_len,
                            const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int min_distance,
                            uint8_t *d_out_ascii, int32_t *d_match, uint8_t *d_best, uint8_t *d_second, uint64_t counts[3],
                            void *hip_stream)
{
    std::vector<uint32_t> packed;
    int rc = corr_check(ctx, d_umi_ascii, n_reads, umi_len, whitelist_ascii, n_wl, max_mismatches, min_distance, d_match, counts,
                        packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (the first device of a multi-device context, as umi_data_new)
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return corr_run(ctx, d_umi_ascii, n_reads, umi_len, packed, n_wl, max_mismatches, min_distance, d_out_ascii, d_match, d_best,
                    d_second, counts, (hipStream_t)hip_stream);
}

int umi_correct_umis(umi_ctx *ctx, const uint8_t *umi_ascii, uint64_t n_reads, int umi_len, const uint8_t *whitelist_ascii,
                     uint32_t n_wl, int max_mismatches, int min_distance, uint8_t *out_ascii, int32_t *match, uint8_t *best,
                     uint8_t *second, uint64_t counts[3])
{
    std::vector<uint32_t> packed;
    int rc = corr_check(ctx, umi_ascii, n_reads, umi_len, whitelist_ascii, n_wl, max_mismatches, min_distance, match, counts,
                        packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = 0;
    if (n_reads == 0) return UMI_OK;
    const size_t n = (size_t)n_reads, bytes = n * (size_t)umi_len;
    HostIo io(ctx);
    const auto d_umi = io.in(umi_ascii, bytes);
    const auto d_out = io.out(out_ascii, bytes);
    const auto d_match = io.out(match, n * 4);
    const auto d_best = io.out(best, n), d_second = io.out(second, n);
    if ((rc = io.open()) ||
        (rc = corr_run(ctx, d_umi, n_reads, umi_len, packed, n_wl, max_mismatches, min_distance, d_out, d_match, d_best, d_second,
                       counts, io.stream())) ||
        (rc = io.fetch(out_ascii, d_out, bytes)) || (rc = io.fetch(match, d_match, n)) || (rc = io.fetch(best, d_best, n)) ||
        (rc = io.fetch(second, d_second, n)))
        return rc;
    return io.close();
}

} // extern "C"

// ---- correction of cell barcodes to a kit's list ----------------------------------------------------
namespace {
// the checks both forms share, and the list packed for the device (2 bits per base, one word per entry)
int bc_check(umi_ctx *ctx, const void *bc, uint64_t n_reads, int bc_len, const uint8_t *whitelist_ascii, uint32_t n_wl,
             int max_mismatches, const void *match, const uint64_t *counts, std::vector<uint64_t> &packed)
{
    // (the context is looked at last: everything before it is decided without a device)
    if (!counts) return fail(UMI_ERR_ARG, "counts is NULL");
    if (!whitelist_ascii) return fail(UMI_ERR_ARG, "whitelist_ascii is NULL");
    if (n_wl == 0) return fail(UMI_ERR_ARG, "the barcode whitelist is empty");
    if (n_wl > CORR_MAX_LIST) return fail(UMI_ERR_ARG, "a whitelist of %u barcodes, more than %u", n_wl, CORR_MAX_LIST);
    if (bc_len < 1 || bc_len > BARCODE_MAX_LEN) return fail(UMI_ERR_ARG, "bc_len %d outside 1..%d", bc_len, BARCODE_MAX_LEN);
    if (max_mismatches < 0 || max_mismatches > 1)
        return fail(UMI_ERR_ARG, "max_mismatches must be 0 or 1 (got %d)", max_mismatches);
    if (n_reads >= (1ull << 30))
        return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one call", (unsigned long long)n_reads);
    if (n_reads && (!bc || !match)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    packed.resize(n_wl);
    uint64_t bad = 0;
    if (barcode_pack_list(whitelist_ascii, n_wl, bc_len, packed.data(), &bad)) {
        const uint8_t *e = whitelist_ascii + (size_t)bad * bc_len;
        int b = 0;
        while (e[b] == 'A' || e[b] == 'C' || e[b] == 'G' || e[b] == 'T') b++;
        return fail(UMI_ERR_CHAR, "Unknown character in whitelist: %u (entry %llu)", (unsigned)e[b], (unsigned long long)bad);
    }
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    return UMI_OK;
}

// (umi_correct_barcodes_multi*: d_qual given, with the two parameters of its rule, d_exact_reads and five counts)
int bc_run(umi_ctx *ctx, const uint8_t *d_bc_ascii, uint64_t n_reads, int bc_len, const std::vector<uint64_t> &packed,
           uint32_t n_wl, int max_mismatches, int32_t *d_match, uint8_t *d_status, uint64_t *counts, hipStream_t s,
           const uint8_t *d_qual = nullptr, int permille = 0, int pseudocount = 0, uint32_t *d_exact_reads = nullptr)
{
    int rc;
    if ((rc = ctx->call_ws.reserve(d_qual ? barcode_multi_workspace_bytes(n_wl, (uint32_t)n_reads) : barcode_workspace_bytes(n_wl))))
        return rc;
    uint64_t bad = 0;
    const int r = barcode_multi_on_device(ctx->call_ws.p, d_bc_ascii, d_qual, (uint32_t)n_reads, bc_len, packed.data(), n_wl,
                                          max_mismatches, (uint32_t)permille, (uint32_t)pseudocount, d_match, d_status,
                                          d_exact_reads, counts, &bad, (uint32_t)ctx->n_cus, ctx->h_counters, s);
    if (r == 1) {
        uint8_t u[BARCODE_MAX_LEN];
        HIP_TRY(hipMemcpyAsync(u, d_bc_ascii + (size_t)bad * bc_len, (size_t)bc_len, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int b = 0;
        while (b < bc_len - 1 && (u[b] == 'A' || u[b] == 'T' || u[b] == 'C' || u[b] == 'G' || u[b] == 'N')) b++;
        return fail(UMI_ERR_CHAR, "Unknown character in cell barcode: %u (read %llu)", (unsigned)u[b], (unsigned long long)bad);
    }
    if (r == 3) {
        uint8_t u[BARCODE_MAX_LEN];
        HIP_TRY(hipMemcpyAsync(u, d_qual + (size_t)bad * bc_len, (size_t)bc_len, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        int b = 0;
        while (b < bc_len - 1 && u[b] >= 33 && u[b] <= 126) b++;
        return fail(UMI_ERR_CHAR, "Unknown character in cell barcode quality: %u (read %llu)", (unsigned)u[b],
                    (unsigned long long)bad);
    }
    if (r == 2)
        return fail(UMI_ERR_ARG, "duplicate entry in the barcode whitelist: entry %llu equals an earlier one",
                    (unsigned long long)bad);
    if (r < 0) return fail(UMI_ERR_HIP, "barcode correction: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

// the host-buffer form of both: the reads (and their qualities) staged, bc_run, the results back
int bc_staged(umi_ctx *ctx, const uint8_t *bc_ascii, const uint8_t *bc_qual, uint64_t n_reads, int bc_len,
              const std::vector<uint64_t> &packed, uint32_t n_wl, int max_mismatches, int permille, int pseudocount, int32_t *match,
              uint8_t *status, uint32_t *exact_reads, uint64_t *counts)
{
    const size_t n = (size_t)n_reads, bytes = n * (size_t)bc_len;
    HostIo io(ctx);
    const auto d_bc = io.in(bc_ascii, bytes), d_qual = io.in(bc_qual, bytes);
    const auto d_match = io.out(match, n * 4);
    const auto d_status = io.out(status, n);
    const auto d_exact = io.out(exact_reads, (size_t)n_wl * 4);
    int rc;
    if ((rc = io.open()) ||
        (rc = bc_run(ctx, d_bc, n_reads, bc_len, packed, n_wl, max_mismatches, d_match, d_status, counts, io.stream(), d_qual,
                     permille, pseudocount, d_exact)) ||
        (rc = io.fetch(match, d_match, n)) || (rc = io.fetch(status, d_status, n)) ||
        (rc = io.fetch(exact_reads, d_exact, (size_t)n_wl)))
        return rc;
    return io.close();
}

// what umi_correct_barcodes_multi* refuses beyond bc_check (which looks at the rest, the context last)
int bc_multi_check(umi_ctx *ctx, const void *bc, const void *qual, uint64_t n_reads, int bc_len, const uint8_t *whitelist_ascii,
                   uint32_t n_wl, int min_posterior_permille, int pseudocount, const void *match, const uint64_t *counts,
                   std::vector<uint64_t> &packed)
{
    if (min_posterior_permille < 0 || min_posterior_permille > 1000)
        return fail(UMI_ERR_ARG, "min_posterior_permille %d outside 0..1000", min_posterior_permille);
    if (pseudocount < 0 || pseudocount > 1000) return fail(UMI_ERR_ARG, "pseudocount %d outside 0..1000", pseudocount);
    if (n_reads && !qual) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    return bc_check(ctx, bc, n_reads, bc_len, whitelist_ascii, n_wl, 1, match, counts, packed);
}
} // namespace

extern "C" {

int umi_correct_barcodes_device(umi_ctx *ctx, const uint8_t *d_bc_ascii, uint64_t n_reads, int bc_len,
                                const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int32_t *d_match,
                                uint8_t *d_status, uint64_t counts[4], void *hip_stream)
{
    std::vector<uint64_t> packed;
    int rc = bc_check(ctx, d_bc_ascii, n_reads, bc_len, whitelist_ascii, n_wl, max_mismatches, d_match, counts, packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (the first device of a multi-device context, as umi_data_new)
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_reads == 0) return UMI_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx); // (a deferred call's counters lie in the pinned block this call reads through)
    return bc_run(ctx, d_bc_ascii, n_reads, bc_len, packed, n_wl, max_mismatches, d_match, d_status, counts,
                  (hipStream_t)hip_stream);
}

int umi_correct_barcodes(umi_ctx *ctx, const uint8_t *bc_ascii, uint64_t n_reads, int bc_len, const uint8_t *whitelist_ascii,
                         uint32_t n_wl, int max_mismatches, int32_t *match, uint8_t *status, uint64_t counts[4])
{
    std::vector<uint64_t> packed;
    int rc = bc_check(ctx, bc_ascii, n_reads, bc_len, whitelist_ascii, n_wl, max_mismatches, match, counts, packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    counts[0] = counts[1] = counts[2] = counts[3] = 0;
    if (n_reads == 0) return UMI_OK;
    return bc_staged(ctx, bc_ascii, nullptr, n_reads, bc_len, packed, n_wl, max_mismatches, 0, 0, match, status, nullptr, counts);
}

int umi_correct_barcodes_multi_device(umi_ctx *ctx, const uint8_t *d_bc_ascii, const uint8_t *d_bc_qual, uint64_t n_reads,
                                      int bc_len, const uint8_t *whitelist_ascii, uint32_t n_wl, int min_posterior_permille,
                                      int pseudocount, int32_t *d_match, uint8_t *d_status, uint32_t *d_exact_reads,
                                      uint64_t counts[5], void *hip_stream)
{
    std::vector<uint64_t> packed;
    int rc = bc_multi_check(ctx, d_bc_ascii, d_bc_qual, n_reads, bc_len, whitelist_ascii, n_wl, min_posterior_permille, pseudocount,
                            d_match, counts, packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    for (int c = 0; c < 5; c++) counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx);
    return bc_run(ctx, d_bc_ascii, n_reads, bc_len, packed, n_wl, 1, d_match, d_status, counts, (hipStream_t)hip_stream, d_bc_qual,
                  min_posterior_permille, pseudocount, d_exact_reads);
}

int umi_correct_barcodes_multi(umi_ctx *ctx, const uint8_t *bc_ascii, const uint8_t *bc_qual, uint64_t n_reads, int bc_len,
                               const uint8_t *whitelist_ascii, uint32_t n_wl, int min_posterior_permille, int pseudocount,
                               int32_t *match, uint8_t *status, uint32_t *exact_reads, uint64_t counts[5])
{
    std::vector<uint64_t> packed;
    int rc = bc_multi_check(ctx, bc_ascii, bc_qual, n_reads, bc_len, whitelist_ascii, n_wl, min_posterior_permille, pseudocount, match,
                            counts, packed);
    if (rc) return rc;
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    for (int c = 0; c < 5; c++) counts[c] = 0;
    if (n_reads == 0) return UMI_OK;
    return bc_staged(ctx, bc_ascii, bc_qual, n_reads, bc_len, packed, n_wl, 1, min_posterior_permille, pseudocount, match, status,
                     exact_reads, counts);
}

} // extern "C"
