// --mode fastq: a TODO in the reference (main.rs:49-50), defined by this build after UMICollapse's
// fastq mode (run_fastq).  Input: one FASTQ file, plain or gzip (detected by its magic bytes; several
// members, BGZF included), records of four lines (@header, sequence, +line, quality).  The whole
// sequence (<= 256 bases, ATCGN) is the key, to_bitset'd into ceil(3L/64) words; distance is the
// reference's per-word bit_count_xor.  One bucket per read length (first appearance), one entry per
// distinct sequence (freq = reads; rep = the first read with --merge any, the highest average quality
// -- (int)(sum(q - 33) as f32 / len as f32) -- first on ties, with avgqual, the default; mapqual is
// refused), entries in rank order (freq descending, first appearance), dir / adj per bucket as for
// BAM.  Output: the rep reads of the survivors in file order, header and + lines byte for byte,
// -u N trimming N bases and quality characters (a read shorter than N is an error); gzip (BGZF at
// --compress-level) when -o ends in .gz.  --tag writes every read with " cluster_id=<i>" (index of
// its cluster's root among the survivors in output order), " cluster_size=<reads>" on the root's
// rep read and " same_umi=<freq>" on every sequence's rep read.  A truncated record, a missing @ or
// +, sequence and quality of different lengths, a base outside ATCGN ("Unknown character"), a read
// over 256 bases end the run with status 101.  Refused with it: --paired, --remove-unpaired,
// --remove-chimeric, --keep-unmapped, --two-pass, several --devices, --stage gpu with --dump-staging;
// --umi_sep and --data are accepted and ignored.  --stage gpu / auto stage the reads on the device
// (umi_stage_seqs_device; auto means host only with --dump-staging or 2^30 reads or more), --stage host
// on the host; same output and messages either way.
// --consensus (fastq mode; not the reference's, tests/consensus_model.py defines it): the same records in
// the same order, but of each the sequence and quality lines are its cluster's consensus -- per column the
// base with the greatest sum of (quality - 33) over all the cluster's reads, ties by the number of reads and
// then the order ACGT, quality min(93, winner's sum - the others'), N and '!' where every read has N
// (umi_consensus_seqs, include/umihip.h) -- trimmed by -u N like any read, and the header gets
// " cluster_size=<reads>" appended.  --consensus-min-reads M (default 1) leaves out the clusters of fewer
// than M reads; the summary gains "Number of clusters below --consensus-min-reads: <n>".  With the device
// staging nothing more goes up (text, offsets, entry of every read and the collapse's result are resident);
// with --stage host the text and the offsets go up for the one call.  Refused with status 101: --consensus
// outside fastq mode, with --tag or --dump-staging; --consensus-min-reads without it or not a number >= 1.
#pragma once
#include <unordered_map>

#include "bgzf.hpp"
#include "fastq.hpp"
#include "hiplib.hpp"

namespace {

// What the writer of fastq mode takes from either staging side: entries in canonical order (n of them
// in nb buckets), the collapse's kept / root, and with --tag every read's entry.
struct FastqResult {
    size_t n, nb;
    std::vector<uint64_t> off;
    std::vector<int32_t> freq;
    std::vector<uint32_t> rep;
    std::vector<uint8_t> kept;
    std::vector<uint32_t> root;
    std::vector<uint32_t> entry_of_read;
    // --consensus: the kept entries' consensus back to back (entry e's at cons_off[e], its bucket's length) and
    // the reads of their clusters
    std::vector<uint8_t> cons_seq, cons_qual;
    std::vector<uint64_t> cons_off;
    std::vector<uint32_t> cluster_reads;
    umi_stats st;
    double t_staging, t_init, t_hot;
    bool gpu_staged;
};
[[noreturn]] void write_fastq(const Cli &args, const umi::bgzf::Bytes &text, const std::vector<umi::fastq::Record> &recs,
                              const FastqResult &res, double t_start, double t_read, double t_gpu1);

// the checks of a record that both stagings make, with the same messages: what is wrong with its length (over
// 256 bases, under -u; empty if nothing), and the end of the run at a base outside ATCGN
std::string fastq_length_problem(const Cli &args, size_t i, const umi::fastq::Record &r)
{
    if (r.len <= UMI_MAX_SEQ_LEN && r.len >= args.umi_length) return "";
    const std::string what = "FASTQ record " + std::to_string(i + 1) + ": " + std::to_string(r.len) + " bases, ";
    if (r.len > UMI_MAX_SEQ_LEN) return what + "more than " + std::to_string(UMI_MAX_SEQ_LEN);
    if (r.len < args.umi_length) return what + "shorter than -u " + std::to_string(args.umi_length);
    return "";
}
void check_fastq_bases(const uint8_t *text, size_t i, const umi::fastq::Record &r)
{
    for (size_t b = 0; b < r.len; b++) {
        const uint8_t c = text[r.seq + b];
        if (c != 'A' && c != 'T' && c != 'C' && c != 'G' && c != 'N')
            die("Unknown character in sequence: " + std::to_string((unsigned)c) + " (FASTQ record " + std::to_string(i + 1) +
                ")"); // utils/mod.rs:77-79
    }
}

// fastq mode with the staging on the device.  The checks of the host staging come in the same order and
// with the same messages: per record in file order its length (over 256, under -u), then its characters.
// A file with a length problem is an error either way: the reads before it are checked for characters
// on the host and the earlier problem is named, no GPU needed.  Otherwise the device checks the
// characters and reports the first bad read.
[[noreturn]] void run_fastq_gpu_stage(const Cli &args, HipLib &lib, GpuWarmup &gpu, const umi::bgzf::Bytes &text,
                                      const std::vector<umi::fastq::Record> &recs, double t_start, double t_read)
{
    const int algo = args.algo_id, merge = args.merge_id;
    const size_t n_reads = recs.size();
    size_t n_ok = n_reads; // reads before the first length problem
    std::string len_problem;
    for (size_t i = 0; i < n_reads && n_ok == n_reads; i++) {
        len_problem = fastq_length_problem(args, i, recs[i]);
        if (!len_problem.empty()) n_ok = i;
    }
    if (!len_problem.empty()) {
        for (size_t i = 0; i < n_ok; i++) check_fastq_bases(text.data(), i, recs[i]);
        die(len_problem);
    }
    std::vector<uint64_t> pos(2 * n_ok + 1);
    std::vector<uint32_t> len(n_ok + 1);
    int n_words = 1;
    for (size_t i = 0; i < n_ok; i++) {
        pos[i] = recs[i].seq;
        pos[n_ok + i] = recs[i].qual;
        len[i] = (uint32_t)recs[i].len;
        n_words = std::max(n_words, (int)((3 * recs[i].len + 63) / 64));
    }
    umi_ctx *ctx = gpu.get();
    // the buffers below go to the context's device: this thread's current device is 0 until it is set
    if (lib.hip_set_device(args.devices[0]) != 0) die("hipSetDevice(" + std::to_string(args.devices[0]) + ") failed");
    const double t_init = now_s();
    auto dev = [&](size_t bytes) -> void * {
        void *p = nullptr;
        if (lib.hip_malloc(&p, std::max<size_t>(bytes, 8)) != 0) die("hipMalloc of " + std::to_string(bytes) + " bytes failed");
        return p;
    };
    auto up = [&](void *dst, const void *src, size_t bytes) {
        if (bytes && lib.hip_memcpy(dst, src, bytes, 1) != 0) die("hipMemcpy to the device failed");
    };
    auto down = [&](void *dst, const void *src, size_t bytes) {
        if (bytes && lib.hip_memcpy(dst, src, bytes, 2) != 0) die("hipMemcpy from the device failed");
    };
    const size_t m = std::max<size_t>(n_ok, 1);
    uint8_t *d_text = (uint8_t *)dev(text.size());
    uint64_t *d_pos = (uint64_t *)dev(16 * m);
    uint32_t *d_len = (uint32_t *)dev(4 * m);
    uint64_t *d_keys = (uint64_t *)dev(8 * m * n_words), *d_nmask = (uint64_t *)dev(8 * m * n_words);
    int32_t *d_freq = (int32_t *)dev(4 * m);
    uint64_t *d_rep = (uint64_t *)dev(8 * m);
    uint32_t *d_eor = args.track_clusters || args.consensus ? (uint32_t *)dev(4 * m) : nullptr;
    up(d_text, text.data(), text.size());
    up(d_pos, pos.data(), 8 * n_ok);
    up(d_pos + n_ok, pos.data() + n_ok, 8 * n_ok);
    up(d_len, len.data(), 4 * n_ok);
    FastqResult res;
    res.off.assign(UMI_MAX_SEQ_LEN + 2, 0);
    std::vector<int32_t> blen(UMI_MAX_SEQ_LEN + 1, 0);
    uint64_t n = 0, nb = 0;
    int any_n = 0;
    if (lib.stage_seqs_device(ctx, d_text, d_pos, merge == 1 ? d_pos + n_ok : nullptr, d_len, n_ok, n_words, merge, d_keys,
                              d_nmask, d_freq, d_rep, d_eor, res.off.data(), blen.data(), &n, &nb, &any_n, nullptr) != UMI_OK) {
        const std::string msg = lib.last_error();
        unsigned byte = 0;
        unsigned long long read = 0;
        if (std::sscanf(msg.c_str(), "Unknown character in sequence: %u (read %llu)", &byte, &read) == 2)
            die("Unknown character in sequence: " + std::to_string(byte) + " (FASTQ record " + std::to_string(read + 1) +
                ")"); // utils/mod.rs:77-79
        die(msg);
    }
    const double t_stage = now_s();
    std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_stage - t_start);
    res.n = n;
    res.nb = nb;
    res.off.resize(nb + 1);
    res.kept.assign(n + 1, 0);
    res.root.assign(n + 1, 0);
    res.freq.resize(n + 1);
    res.rep.resize(n + 1);
    std::memset(&res.st, 0, sizeof(res.st));
    if (n) {
        uint8_t *d_kept = (uint8_t *)dev(n);
        uint32_t *d_root = (uint32_t *)dev(4 * n);
        if (lib.dedup_seqs_device(ctx, d_keys, any_n ? d_nmask : nullptr, n_words, d_freq, res.off.data(), blen.data(), nb,
                                  args.k, args.percentage, algo, 0 /* adjacency.rs:56 */, d_kept, d_root, nullptr,
                                  &res.st) != UMI_OK)
            die(lib.last_error());
        down(res.kept.data(), d_kept, n);
        down(res.root.data(), d_root, 4 * n);
        down(res.freq.data(), d_freq, 4 * n);
        std::vector<uint64_t> rep64(n);
        down(rep64.data(), d_rep, 8 * n);
        for (size_t e = 0; e < n; e++) res.rep[e] = (uint32_t)rep64[e];
        if (args.track_clusters) {
            res.entry_of_read.resize(n_reads);
            down(res.entry_of_read.data(), d_eor, 4 * n_reads);
        }
        if (args.consensus) { // everything it reads is resident; the consensus, its offsets and the counts come back
            size_t cap = 0;
            for (size_t i = 0; i < n_ok; i++) cap += len[i];
            uint8_t *d_cs = (uint8_t *)dev(cap), *d_cq = (uint8_t *)dev(cap);
            uint64_t *d_coff = (uint64_t *)dev(8 * n);
            uint32_t *d_cr = (uint32_t *)dev(4 * n);
            uint64_t cons_bytes = 0;
            if (lib.consensus_seqs_device(ctx, d_text, d_pos, d_pos + n_ok, d_len, n_ok, d_eor, d_freq, d_kept, d_root, n,
                                          res.off.data(), blen.data(), nb, d_cs, d_cq, d_coff, d_cr, &cons_bytes,
                                          nullptr) != UMI_OK)
                die(lib.last_error());
            res.cons_seq.resize(cons_bytes);
            res.cons_qual.resize(cons_bytes);
            res.cons_off.resize(n);
            res.cluster_reads.resize(n);
            down(res.cons_seq.data(), d_cs, cons_bytes);
            down(res.cons_qual.data(), d_cq, cons_bytes);
            down(res.cons_off.data(), d_coff, 8 * n);
            down(res.cluster_reads.data(), d_cr, 4 * n);
        }
    }
    const double t_gpu1 = now_s();
    res.t_staging = t_stage - t_init;
    res.t_init = t_init - t_read;
    res.t_hot = t_gpu1 - t_stage;
    res.gpu_staged = true;
    write_fastq(args, text, recs, res, t_start, t_read, t_gpu1);
}

// fastq mode's staging on the host: per read length a map sequence -> entry, then the entries in canonical
// order (bucket by bucket, freq descending, first appearance on ties)
struct FastqHostStaging {
    size_t n = 0, nb = 0;
    int n_words = 1;
    std::vector<uint64_t> keys, nmask, off;
    std::vector<int32_t> freq, blen, bucket_of_len;
    std::vector<uint32_t> rep;
    bool any_n = false;
    void stage(const Cli &args, int merge, const umi::bgzf::Bytes &text, const std::vector<umi::fastq::Record> &recs)
    {
        const uint8_t *d = text.data();
        const size_t n_reads = recs.size();
        // staging: per read length a map sequence -> entry, entries in first appearance
        struct Entry {
            uint32_t freq, rep;
            int32_t score;
        };
        struct Bucket {
            uint32_t len;
            std::vector<Entry> entries;
            std::unordered_map<std::string, uint32_t> index;
        };
        std::vector<Bucket> buckets;
        bucket_of_len.assign(UMI_MAX_SEQ_LEN + 1, -1);
        for (size_t i = 0; i < n_reads; i++) {
            const umi::fastq::Record &r = recs[i];
            const std::string len_problem = fastq_length_problem(args, i, r);
            if (!len_problem.empty()) die(len_problem);
            check_fastq_bases(d, i, r);
            int32_t &bi = bucket_of_len[r.len];
            if (bi < 0) {
                bi = (int32_t)buckets.size();
                buckets.push_back(Bucket{(uint32_t)r.len, {}, {}});
            }
            Bucket &bk = buckets[bi];
            const int32_t score = merge == 1 ? umi::fastq::avg_qual(d + r.qual, r.len) : 0;
            auto it = bk.index.emplace(std::string((const char *)d + r.seq, r.len), (uint32_t)bk.entries.size());
            if (it.second) {
                bk.entries.push_back(Entry{1, (uint32_t)i, score});
            } else {
                Entry &e = bk.entries[it.first->second];
                e.freq++;
                if (merge == 1 && !(e.score >= score)) { // merge/mod.rs:35: the kept read stays on ties
                    e.rep = (uint32_t)i;
                    e.score = score;
                }
            }
        }
        // entries in canonical order: bucket by bucket, freq descending, first appearance on ties
        for (const Bucket &bk : buckets) {
            n += bk.entries.size();
            n_words = std::max(n_words, (int)((3 * bk.len + 63) / 64));
        }
        nb = buckets.size();
        keys.assign(n * n_words + 1, 0);
        nmask.assign(n * n_words + 1, 0);
        off.assign(nb + 1, 0);
        freq.resize(n + 1);
        blen.resize(nb + 1);
        rep.resize(n + 1);
        {
            size_t e = 0;
            for (size_t b = 0; b < nb; b++) {
                Bucket &bk = buckets[b];
                std::vector<uint32_t> order(bk.entries.size());
                for (uint32_t j = 0; j < order.size(); j++) order[j] = j;
                std::stable_sort(order.begin(), order.end(),
                                 [&](uint32_t x, uint32_t y) { return bk.entries[x].freq > bk.entries[y].freq; });
                off[b] = e;
                blen[b] = (int32_t)bk.len;
                for (uint32_t j : order) {
                    const Entry &en = bk.entries[j];
                    const umi::fastq::Record &r = recs[en.rep];
                    freq[e] = (int32_t)en.freq;
                    rep[e] = en.rep;
                    uint64_t *kw = &keys[e * n_words], *mw = &nmask[e * n_words];
                    for (size_t p = 0; p < r.len; p++) { // to_bitset, utils/mod.rs:63-83; read.rs:23-31
                        uint64_t c = 0;
                        switch (d[r.seq + p]) {
                        case 'T': c = 5; break;
                        case 'C': c = 6; break;
                        case 'G': c = 3; break;
                        case 'N': c = 4; any_n = true; break;
                        default: break;
                        }
                        for (int q = 0; q < 3; q++) { // a base may straddle two words (bitset.rs:52-75)
                            const size_t bit = 3 * p + q;
                            if ((c >> q) & 1) kw[bit >> 6] |= 1ull << (bit & 63);
                            if (c == 4) mw[bit >> 6] |= 1ull << (bit & 63);
                        }
                    }
                    e++;
                }
                bk.index.clear();
            }
            off[nb] = e;
        }
    }
};

// ---- FASTQ mode (-m fastq).  The reference leaves it a TODO (src/main.rs:49-50); this build defines it
// after UMICollapse's fastq mode: the whole read sequence is the key.  One bucket per read length
// (first appearance), one entry per distinct sequence (freq, rep: the first read with --merge any, the
// highest average quality -- first on ties -- with avgqual), rank order inside, ONE umi_dedup_seqs call,
// survivors' rep reads written in file order (-u N trims N bases and quality characters from each).
// Staging on the device (--stage gpu, or auto): the inflated text goes up as it is, with every read's
// offsets and length; umi_stage_seqs_device leaves its output on the device for umi_dedup_seqs_device,
// and only what the writer needs comes back.  --stage host (and auto with --dump-staging or 2^30
// reads or more): the per-length hash maps below.
int run_fastq(const Cli &args, HipLib &lib, GpuWarmup &gpu)
{
    const double t_start = now_s();
    const int algo = args.algo_id, merge = args.merge_id;
    if (args.paired || args.remove_unpaired || args.remove_chimeric || args.keep_unmapped || args.two_pass)
        die("--paired, --remove-unpaired, --remove-chimeric, --keep-unmapped and --two-pass do not go with fastq mode");
    if (!args.umi_tag.empty() || args.cell_tag_given || args.per_cell)
        die("--umi-tag, --cell-tag and --per-cell do not go with fastq mode");
    check_stage(args);
    if (args.stage == "gpu" && !args.dump_staging.empty()) die("--stage gpu does not go with --dump-staging");
    if (args.devices.size() > 1) die("fastq mode runs on one GPU: --devices takes one id here");
    if (args.consensus && args.track_clusters) die("--consensus does not go with --tag (which writes every read as it is)");
    if (args.consensus && !args.dump_staging.empty()) die("--consensus does not go with --dump-staging (which stops before the GPU)");
    if (merge == 2) die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data);
    // the GPU is woken while the file is read (as in BAM mode: a tiny staging call and a tiny dedup call
    // load the library's code objects)
    const bool want_gpu_stage = args.stage != "host" && args.dump_staging.empty();
    if (want_gpu_stage) gpu.start(true, merge);
    umi::bgzf::Bytes text = umi::fastq::read_all(args.input, args.num_threads);
    std::vector<umi::fastq::Record> recs;
    const std::string perr = umi::fastq::parse(text.data(), text.size(), recs);
    if (!perr.empty()) die(perr);
    const double t_read = now_s();
    const uint8_t *d = text.data();
    const size_t n_reads = recs.size();
    if (want_gpu_stage && n_reads < (1ull << 30))
        run_fastq_gpu_stage(args, lib, gpu, text, recs, t_start, t_read); // (does not return)
    // (the BAM staging on the device, OnePass::stage_on_gpu, is unrelated: another key, another library call)
    FastqHostStaging hs;
    hs.stage(args, merge, text, recs);
    const size_t n = hs.n, nb = hs.nb;
    const double t_stage = now_s();
    std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_stage - t_start);
    if (!args.dump_staging.empty()) { // test hook: staged hot-path input, no GPU touched
        FILE *f = std::fopen(args.dump_staging.c_str(), "wb");
        if (!f) die("cannot open " + args.dump_staging);
        const uint64_t hdr[4] = {n, nb, 0, (uint64_t)hs.n_words};
        std::fwrite(hdr, 8, 4, f);
        std::fwrite(hs.keys.data(), 8, n * hs.n_words, f);
        std::fwrite(hs.nmask.data(), 8, n * hs.n_words, f);
        std::fwrite(hs.freq.data(), 4, n, f);
        std::fwrite(hs.rep.data(), 4, n, f);
        std::fwrite(hs.off.data(), 8, nb + 1, f);
        std::fwrite(hs.blen.data(), 4, nb, f);
        std::fclose(f);
        return 0;
    }
    std::vector<uint8_t> kept(n + 1, 0);
    std::vector<uint32_t> root(n + 1, 0);
    umi_stats st;
    std::memset(&st, 0, sizeof(st));
    double t_gpu0 = now_s(), t_gpu1 = t_gpu0;
    umi_ctx *ctx = nullptr;
    if (n) {
        ctx = gpu.get(); // (--stage auto with 2^30 reads or more: the context the start-up thread made)
        t_gpu0 = now_s();
        if (lib.dedup_seqs(ctx, hs.keys.data(), hs.any_n ? hs.nmask.data() : nullptr, hs.n_words, hs.freq.data(), hs.off.data(),
                           hs.blen.data(), nb, args.k, args.percentage, algo, 0 /* adjacency.rs:56 */, kept.data(),
                           root.data(), &st) != UMI_OK)
            die(lib.last_error());
        t_gpu1 = now_s();
    }
    FastqResult res{n, nb, std::move(hs.off), std::move(hs.freq), std::move(hs.rep), std::move(kept), std::move(root), {}, {}, {}, {}, {}, st,
                    t_stage - t_read, t_gpu0 - t_stage, t_gpu1 - t_gpu0, false};
    // entry of every read (--tag, --consensus): its sequence's, looked up again per bucket
    if (args.track_clusters || args.consensus) {
        res.entry_of_read.resize(n_reads);
        std::vector<std::unordered_map<std::string, uint32_t>> index(nb);
        for (size_t b = 0; b < nb; b++)
            for (uint64_t e = res.off[b]; e < res.off[b + 1]; e++)
                index[b].emplace(std::string((const char *)d + recs[res.rep[e]].seq, recs[res.rep[e]].len), (uint32_t)e);
        for (size_t i = 0; i < n_reads; i++) {
            const umi::fastq::Record &r = recs[i];
            res.entry_of_read[i] = index[hs.bucket_of_len[r.len]].at(std::string((const char *)d + r.seq, r.len));
        }
    }
    if (args.consensus && n) { // the text and the reads' offsets go up for this one call
        if (!lib.consensus_seqs) die("libumihip.so lacks umi_consensus_seqs");
        std::vector<uint64_t> pos(2 * n_reads);
        std::vector<uint32_t> len(n_reads);
        size_t cap = 0;
        for (size_t i = 0; i < n_reads; i++) {
            pos[i] = recs[i].seq;
            pos[n_reads + i] = recs[i].qual;
            len[i] = (uint32_t)recs[i].len;
            cap += recs[i].len;
        }
        res.cons_seq.resize(cap + 1);
        res.cons_qual.resize(cap + 1);
        res.cons_off.assign(n, 0);
        res.cluster_reads.assign(n, 0);
        uint64_t cons_bytes = 0;
        if (lib.consensus_seqs(ctx, d, pos.data(), pos.data() + n_reads, len.data(), n_reads, res.entry_of_read.data(),
                               res.freq.data(), res.kept.data(), res.root.data(), n, res.off.data(), hs.blen.data(), nb,
                               res.cons_seq.data(), res.cons_qual.data(), res.cons_off.data(), res.cluster_reads.data(),
                               &cons_bytes) != UMI_OK)
            die(lib.last_error());
        t_gpu1 = now_s();
        res.t_hot = t_gpu1 - t_gpu0;
    }
    write_fastq(args, text, recs, res, t_start, t_read, t_gpu1);
}

// the survivors (or with --tag every read) written, the summary printed; the process ends here
[[noreturn]] void write_fastq(const Cli &args, const umi::bgzf::Bytes &text, const std::vector<umi::fastq::Record> &recs,
                              const FastqResult &res, double t_start, double t_read, double t_gpu1)
{
    const uint8_t *d = text.data();
    const size_t n_reads = recs.size(), n = res.n, nb = res.nb;
    const std::vector<uint64_t> &off = res.off;
    const std::vector<int32_t> &freq = res.freq;
    const std::vector<uint32_t> &rep = res.rep, &root = res.root;
    const std::vector<uint8_t> &kept = res.kept;
    const umi_stats &st = res.st;
    // survivors in output order: their rep reads in file order
    std::vector<uint32_t> entry_of_rep(n_reads, UINT32_MAX);
    for (size_t e = 0; e < n; e++) entry_of_rep[rep[e]] = (uint32_t)e;
    const size_t trim = args.umi_length;
    std::string out;
    out.reserve(text.size() + (args.track_clusters ? n_reads * 48 : 0));
    auto put = [&](size_t p, size_t len) { out.append((const char *)d + p, len); };
    auto put_record = [&](const umi::fastq::Record &r, const std::string &extra) {
        put(r.head, r.head_len);
        out += extra;
        out += '\n';
        put(r.seq + trim, r.len - trim);
        out += '\n';
        put(r.plus, r.plus_len);
        out += '\n';
        put(r.qual + trim, r.len - trim);
        out += '\n';
    };
    size_t n_out = 0, n_below = 0;
    if (args.consensus) {
        // the same records in the same order, each with its cluster's consensus for sequence and quality
        std::vector<uint32_t> len_of(n + 1, 0);
        for (size_t b = 0; b < nb; b++)
            for (uint64_t e = off[b]; e < off[b + 1]; e++) len_of[e] = (uint32_t)recs[rep[e]].len;
        for (size_t i = 0; i < n_reads; i++) {
            const uint32_t e = entry_of_rep[i];
            if (e == UINT32_MAX || !kept[e]) continue;
            if (res.cluster_reads[e] < args.consensus_min_reads) {
                n_below++;
                continue;
            }
            const umi::fastq::Record &r = recs[i];
            const size_t at = res.cons_off[e], L = len_of[e];
            put(r.head, r.head_len);
            out += " cluster_size=" + std::to_string(res.cluster_reads[e]);
            out += '\n';
            out.append((const char *)res.cons_seq.data() + at + trim, L - trim);
            out += '\n';
            put(r.plus, r.plus_len);
            out += '\n';
            out.append((const char *)res.cons_qual.data() + at + trim, L - trim);
            out += '\n';
            n_out++;
        }
    } else if (!args.track_clusters) {
        for (size_t i = 0; i < n_reads; i++) {
            const uint32_t e = entry_of_rep[i];
            if (e == UINT32_MAX || !kept[e]) continue;
            put_record(recs[i], "");
            n_out++;
        }
    } else {
        // --tag: cluster_id = index of the cluster's root among the survivors in output order,
        // cluster_size = reads of the cluster (on the root's rep read), same_umi = reads of the sequence
        // (on every sequence's rep read)
        std::vector<uint32_t> cluster_id(n + 1, 0), cluster_reads(n + 1, 0);
        for (size_t i = 0; i < n_reads; i++) {
            const uint32_t e = entry_of_rep[i];
            if (e != UINT32_MAX && kept[e]) cluster_id[e] = (uint32_t)n_out++;
        }
        for (size_t e = 0; e < n; e++) cluster_reads[root[e]] += (uint32_t)freq[e];
        for (size_t i = 0; i < n_reads; i++) {
            const umi::fastq::Record &r = recs[i];
            const uint32_t e = res.entry_of_read[i];
            const uint32_t rt = root[e];
            std::string extra = " cluster_id=" + std::to_string(cluster_id[rt]);
            if (rep[rt] == i) extra += " cluster_size=" + std::to_string(cluster_reads[rt]);
            if (rep[e] == i) extra += " same_umi=" + std::to_string(freq[e]);
            put_record(r, extra);
        }
    }
    const std::string &o = args.output;
    if (o.size() >= 3 && o.compare(o.size() - 3, 3, ".gz") == 0) {
        umi::bgzf::compress_to_file(o, (const uint8_t *)out.data(), out.size(), args.num_threads, args.compress_level);
    } else {
        FILE *f = std::fopen(o.c_str(), "wb");
        if (!f) die("cannot open " + o);
        if (!out.empty() && std::fwrite(out.data(), 1, out.size(), f) != out.size()) die("cannot write " + o);
        if (std::fclose(f) != 0) die("cannot write " + o);
    }
    const double t_end = now_s();
    size_t max_bucket = 0;
    for (size_t b = 0; b < nb; b++) max_bucket = std::max<size_t>(max_bucket, off[b + 1] - off[b]);
    std::fprintf(stderr, "Number of input reads: %zu\n", n_reads);
    std::fprintf(stderr, "Number of read lengths: %zu\n", nb);
    std::fprintf(stderr, "Number of distinct sequences: %zu\n", n);
    std::fprintf(stderr, "Max number of distinct sequences of one length: %zu\n", max_bucket);
    std::fprintf(stderr, args.track_clusters ? "Number of groups of reads: %llu\n" : "Number of reads after deduplicating: %llu\n",
                 (unsigned long long)st.n_kept);
    if (args.consensus) std::fprintf(stderr, "Number of clusters below --consensus-min-reads: %zu\n", n_below);
    std::fprintf(stderr,
                 "phases: read+parse %.3f s, staging (%s) %.3f s, gpu init %.3f s, hot path (H2D+GPU+D2H) %.3f s "
                 "[%llu pairs, %llu evaluated], write %.3f s\n",
                 t_read - t_start, res.gpu_staged ? "gpu" : "host", res.t_staging, res.t_init, res.t_hot,
                 (unsigned long long)st.n_pairs, (unsigned long long)st.n_pairs_evaluated, t_end - t_gpu1);
    std::fprintf(stderr, "UMI collapsing finished in %.3f seconds\n", t_end - t_start); // main.rs:97-102
    std::fflush(stderr);
    std::_Exit(0); // (no static destructors: as the BAM path, the process ends without tearing HIP down)
}

} // namespace
