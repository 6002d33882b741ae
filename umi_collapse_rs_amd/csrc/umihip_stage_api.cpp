// Read staging: umi_stage_reads*, umi_stage_seqs*.
#include "umihip_host.hpp"

#include <algorithm>

using namespace umihip;

extern "C" {

int umi_stage_reads_grouped_wide_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                                        const uint64_t *d_group_key, int group_key_bits, const uint8_t *d_umi_ascii,
                                        const int32_t *d_score, uint64_t n_reads, int umi_len, int n_words, int merge,
                                        uint64_t *d_keys, uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep,
                                        uint64_t *d_bucket_off, uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (staging runs on the first device of a multi-device context)
    if (!n_entries || !n_buckets || !d_bucket_off) return fail(UMI_ERR_ARG, "n_entries / n_buckets / d_bucket_off is NULL");
    if (n_reads && (!d_align_key || !d_umi_ascii || !d_keys || !d_freq || !d_rep))
        return fail(UMI_ERR_ARG, "a required device pointer is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN) return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    if (align_key_bits < 1 || align_key_bits > 64) return fail(UMI_ERR_ARG, "align_key_bits must be in 1..64");
    if (group_key_bits < 0 || group_key_bits > 64) return fail(UMI_ERR_ARG, "group_key_bits must be in 0..64");
    if (group_key_bits && n_reads && !d_group_key) return fail(UMI_ERR_ARG, "d_group_key is NULL with group_key_bits %d", group_key_bits);
    if (merge != 0 && merge != 1) return fail(UMI_ERR_ARG, "merge must be 0 (any) or 1 (highest score, first on ties)");
    if (n_reads >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one staging call", (unsigned long long)n_reads);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx);
    int rc;
    if ((rc = ctx->call_ws.reserve(stage_workspace_bytes((uint32_t)n_reads, n_words, group_key_bits > 0)))) return rc;
    hipStream_t s = (hipStream_t)hip_stream; // (NULL = the default stream, as in every device-pointer call)
    const int r = stage_reads_on_device(ctx->call_ws.p, d_align_key, align_key_bits, group_key_bits ? d_group_key : nullptr,
                                        group_key_bits, d_umi_ascii, d_score, (uint32_t)n_reads, umi_len, n_words, merge,
                                        d_keys, d_nmask, d_freq, d_rep, d_bucket_off, n_entries, n_buckets, ctx->h_counters, s);
    if (r == 1) return fail(UMI_ERR_CHAR, "Unknown character in UMI sequence");
    if (r < 0) return fail(UMI_ERR_HIP, "staging: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

int umi_stage_reads_wide_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits, const uint8_t *d_umi_ascii,
                                const int32_t *d_score, uint64_t n_reads, int umi_len, int n_words, int merge,
                                uint64_t *d_keys, uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep,
                                uint64_t *d_bucket_off, uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream)
{
    return umi_stage_reads_grouped_wide_device(ctx, d_align_key, align_key_bits, nullptr, 0, d_umi_ascii, d_score, n_reads,
                                               umi_len, n_words, merge, d_keys, d_nmask, d_freq, d_rep, d_bucket_off,
                                               n_entries, n_buckets, hip_stream);
}

int umi_stage_reads_grouped_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                                   const uint64_t *d_group_key, int group_key_bits, const uint8_t *d_umi_ascii,
                                   const int32_t *d_score, uint64_t n_reads, int umi_len, int merge, uint64_t *d_keys,
                                   uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep, uint64_t *d_bucket_off,
                                   uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream)
{
    if (umi_len < 1 || umi_len > UMI_MAX_UMI_LEN) return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_UMI_LEN);
    return umi_stage_reads_grouped_wide_device(ctx, d_align_key, align_key_bits, d_group_key, group_key_bits, d_umi_ascii,
                                               d_score, n_reads, umi_len, 1, merge, d_keys, d_nmask, d_freq, d_rep,
                                               d_bucket_off, n_entries, n_buckets, hip_stream);
}

int umi_stage_reads_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits, const uint8_t *d_umi_ascii,
                           const int32_t *d_score, uint64_t n_reads, int umi_len, int merge, uint64_t *d_keys,
                           uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep, uint64_t *d_bucket_off,
                           uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream)
{
    return umi_stage_reads_grouped_device(ctx, d_align_key, align_key_bits, nullptr, 0, d_umi_ascii, d_score, n_reads, umi_len,
                                          merge, d_keys, d_nmask, d_freq, d_rep, d_bucket_off, n_entries, n_buckets,
                                          hip_stream);
}

int umi_stage_reads_grouped_wide(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint64_t *group_key,
                                 int group_key_bits, const uint8_t *umi_ascii, const int32_t *score, uint64_t n_reads,
                                 int umi_len, int n_words, int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq,
                                 uint64_t *rep, uint64_t *bucket_off, uint64_t *n_entries, uint64_t *n_buckets)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (!n_entries || !n_buckets || !bucket_off) return fail(UMI_ERR_ARG, "n_entries / n_buckets / bucket_off is NULL");
    if (n_reads && (!align_key || !umi_ascii || !keys || !freq || !rep)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (umi_len < 1 || umi_len > UMI_MAX_WIDE_UMI_LEN) return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_WIDE_UMI_LEN);
    if (n_words != wide_words(umi_len)) return fail(UMI_ERR_ARG, "n_words must be %d for umi_len %d", wide_words(umi_len), umi_len);
    if (group_key_bits < 0 || group_key_bits > 64) return fail(UMI_ERR_ARG, "group_key_bits must be in 0..64");
    if (group_key_bits && n_reads && !group_key) return fail(UMI_ERR_ARG, "group_key is NULL with group_key_bits %d", group_key_bits);
    if (n_reads >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one staging call", (unsigned long long)n_reads);
    int rc;
    // (sizes for max(n, 1) reads: no array without room; the pad of an input is that room beyond its n reads)
    const size_t n = (size_t)n_reads, m = std::max<size_t>(n, 1), kw = 8 * (size_t)n_words;
    HostIo io(ctx);
    const auto d_align = io.in(align_key, n * 8, (m - n) * 8);
    const auto d_group = io.in(group_key_bits ? group_key : nullptr, n * 8, (m - n) * 8);
    const auto d_umi = io.in(umi_ascii, n * (size_t)umi_len, (m - n) * (size_t)umi_len);
    const auto d_score = io.in(score, n * 4, (m - n) * 4);
    const auto d_keys = io.out<uint64_t>(m * kw), d_nmask = io.out<uint64_t>(m * kw); // (the mask is written, asked for or not)
    const auto d_freq = io.out<int32_t>(m * 4);
    const auto d_rep = io.out<uint64_t>(m * 8), d_boff = io.out<uint64_t>((m + 1) * 8);
    if ((rc = io.open()) ||
        (rc = umi_stage_reads_grouped_wide_device(ctx, d_align, align_key_bits, d_group, group_key_bits, d_umi, d_score, n_reads,
                                                  umi_len, n_words, merge, d_keys, d_nmask, d_freq, d_rep, d_boff, n_entries,
                                                  n_buckets, io.stream())))
        return rc;
    const size_t e = (size_t)*n_entries, b = (size_t)*n_buckets;
    if ((rc = io.fetch(keys, d_keys, e * (size_t)n_words)) || (rc = io.fetch(nmask, d_nmask, e * (size_t)n_words)) ||
        (rc = io.fetch(freq, d_freq, e)) || (rc = io.fetch(rep, d_rep, e)) || (rc = io.fetch(bucket_off, d_boff, b + 1)))
        return rc;
    return io.close();
}

int umi_stage_reads_wide(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint8_t *umi_ascii,
                         const int32_t *score, uint64_t n_reads, int umi_len, int n_words, int merge, uint64_t *keys,
                         uint64_t *nmask, int32_t *freq, uint64_t *rep, uint64_t *bucket_off, uint64_t *n_entries,
                         uint64_t *n_buckets)
{
    return umi_stage_reads_grouped_wide(ctx, align_key, align_key_bits, nullptr, 0, umi_ascii, score, n_reads, umi_len, n_words,
                                        merge, keys, nmask, freq, rep, bucket_off, n_entries, n_buckets);
}

int umi_stage_reads_grouped(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint64_t *group_key,
                            int group_key_bits, const uint8_t *umi_ascii, const int32_t *score, uint64_t n_reads, int umi_len,
                            int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq, uint64_t *rep, uint64_t *bucket_off,
                            uint64_t *n_entries, uint64_t *n_buckets)
{
    if (umi_len < 1 || umi_len > UMI_MAX_UMI_LEN) return fail(UMI_ERR_ARG, "umi_len %d outside 1..%d", umi_len, UMI_MAX_UMI_LEN);
    return umi_stage_reads_grouped_wide(ctx, align_key, align_key_bits, group_key, group_key_bits, umi_ascii, score, n_reads,
                                        umi_len, 1, merge, keys, nmask, freq, rep, bucket_off, n_entries, n_buckets);
}

int umi_stage_reads(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint8_t *umi_ascii,
                    const int32_t *score, uint64_t n_reads, int umi_len, int merge, uint64_t *keys, uint64_t *nmask,
                    int32_t *freq, uint64_t *rep, uint64_t *bucket_off, uint64_t *n_entries, uint64_t *n_buckets)
{
    return umi_stage_reads_grouped(ctx, align_key, align_key_bits, nullptr, 0, umi_ascii, score, n_reads, umi_len, merge, keys,
                                   nmask, freq, rep, bucket_off, n_entries, n_buckets);
}

int umi_stage_seqs_device(umi_ctx *ctx, const uint8_t *d_text, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                          const uint32_t *d_len, uint64_t n_reads, int n_words, int merge, uint64_t *d_keys, uint64_t *d_nmask,
                          int32_t *d_freq, uint64_t *d_rep, uint32_t *d_entry_of_read, uint64_t *bucket_off,
                          int32_t *bucket_len, uint64_t *n_entries, uint64_t *n_buckets, int *any_n, void *hip_stream)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0]; // (staging runs on the first device of a multi-device context)
    if (!n_entries || !n_buckets || !any_n || !bucket_off || !bucket_len)
        return fail(UMI_ERR_ARG, "n_entries / n_buckets / any_n / bucket_off / bucket_len is NULL");
    if (n_reads && (!d_text || !d_seq_pos || !d_len || !d_keys || !d_freq || !d_rep))
        return fail(UMI_ERR_ARG, "a required device pointer is NULL");
    if (n_words < 1 || n_words > SEQ_MAX_WORDS) return fail(UMI_ERR_ARG, "n_words %d outside 1..%d", n_words, SEQ_MAX_WORDS);
    if (merge != 0 && merge != 1) return fail(UMI_ERR_ARG, "merge must be 0 (any) or 1 (highest average quality, first on ties)");
    if (merge == 1 && n_reads && !d_qual_pos) return fail(UMI_ERR_ARG, "merge 1 needs d_qual_pos");
    if (n_reads >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one staging call", (unsigned long long)n_reads);
    HIP_TRY(hipSetDevice(ctx->device));
    settle(ctx);
    int rc;
    if ((rc = ctx->call_ws.reserve(stage_seqs_workspace_bytes((uint32_t)n_reads, n_words)))) return rc;
    SeqFault fault;
    const int r = stage_seqs_on_device(ctx->call_ws.p, d_text, d_seq_pos, d_qual_pos, d_len, (uint32_t)n_reads, n_words, merge,
                                       d_keys, d_nmask, d_freq, d_rep, d_entry_of_read, bucket_off, bucket_len, n_entries,
                                       n_buckets, any_n, &fault, ctx->h_counters, (hipStream_t)hip_stream);
    if (r == 1)
        return fail(UMI_ERR_CHAR, "Unknown character in sequence: %u (read %llu)", (unsigned)fault.value,
                    (unsigned long long)fault.read);
    if (r == 2)
        return fail(UMI_ERR_ARG, "a read of %llu bases, more than %d", (unsigned long long)fault.value, UMI_MAX_SEQ_LEN);
    if (r == 3)
        return fail(UMI_ERR_ARG, "a read of %llu bases needs %d words, n_words is %d", (unsigned long long)fault.value,
                    (int)((3 * fault.value + 63) / 64), n_words);
    if (r < 0) return fail(UMI_ERR_HIP, "staging: %s", hipGetErrorString((hipError_t)(-r)));
    return UMI_OK;
}

int umi_stage_seqs(umi_ctx *ctx, const uint8_t *text, const uint64_t *seq_pos, const uint64_t *qual_pos, const uint32_t *len,
                   uint64_t n_reads, int n_words, int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq, uint64_t *rep,
                   uint32_t *entry_of_read, uint64_t *bucket_off, int32_t *bucket_len, uint64_t *n_entries,
                   uint64_t *n_buckets, int *any_n)
{
    if (!ctx) return fail(UMI_ERR_ARG, "ctx is NULL");
    if (!ctx->subs.empty()) ctx = ctx->subs[0];
    if (n_reads && (!text || !seq_pos || !len || !keys || !freq || !rep)) return fail(UMI_ERR_ARG, "a required pointer is NULL");
    if (n_words < 1 || n_words > SEQ_MAX_WORDS) return fail(UMI_ERR_ARG, "n_words %d outside 1..%d", n_words, SEQ_MAX_WORDS);
    if (merge == 1 && n_reads && !qual_pos) return fail(UMI_ERR_ARG, "merge 1 needs qual_pos");
    if (n_reads >= (1ull << 30)) return fail(UMI_ERR_ARG, "%llu reads exceed the 30-bit index space of one staging call", (unsigned long long)n_reads);
    // the text that is looked at: up to the end of the last byte of any read (lengths beyond
    // UMI_MAX_SEQ_LEN are refused inside; their first UMI_MAX_SEQ_LEN bytes are what the device reads)
    size_t text_bytes = 1;
    for (uint64_t i = 0; i < n_reads; i++) {
        const uint64_t l = std::min<uint64_t>(len[i], UMI_MAX_SEQ_LEN);
        text_bytes = std::max<size_t>(text_bytes, seq_pos[i] + l);
        if (merge == 1) text_bytes = std::max<size_t>(text_bytes, qual_pos[i] + l);
    }
    int rc;
    const size_t n = (size_t)n_reads, m = std::max<size_t>(n, 1), kw = 8 * (size_t)n_words;
    HostIo io(ctx);
    const auto d_text = io.in(text, n ? text_bytes : 0, n ? 0 : 1); // (pad: a byte of text where there is no read)
    // (pad: qual_pos behind seq_pos, from d_pos + m -- and, as for every array here, room for max(n, 1) reads)
    const auto d_pos = io.in(seq_pos, n * 8, m * 16 - n * 8);
    io.also(d_pos, m * 8, qual_pos, n * 8);
    const auto d_len = io.in(len, n * 4, (m - n) * 4);
    const auto d_keys = io.out(keys, m * kw), d_nmask = io.out(nmask, m * kw);
    const auto d_freq = io.out(freq, m * 4);
    const auto d_rep = io.out(rep, m * 8);
    const auto d_eor = io.out(entry_of_read, m * 4);
    if ((rc = io.open()) ||
        (rc = umi_stage_seqs_device(ctx, d_text, d_pos, qual_pos && n ? d_pos + m : nullptr, d_len, n_reads, n_words, merge, d_keys,
                                    d_nmask, d_freq, d_rep, d_eor, bucket_off, bucket_len, n_entries, n_buckets, any_n,
                                    io.stream())))
        return rc;
    const size_t e = (size_t)*n_entries;
    if ((rc = io.fetch(keys, d_keys, e * (size_t)n_words)) || (rc = io.fetch(nmask, d_nmask, e * (size_t)n_words)) ||
        (rc = io.fetch(freq, d_freq, e)) || (rc = io.fetch(rep, d_rep, e)) || (rc = io.fetch(entry_of_read, d_eor, n)))
        return rc;
    return io.close();
}

} // extern "C"
