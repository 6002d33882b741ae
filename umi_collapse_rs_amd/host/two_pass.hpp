// --two-pass (the reference parses it and ignores it; UMICollapse's meaning): the input is read twice and
// never held.  Pass 1 counts, writes the kept unmapped reads and notes the last read of every alignment
// key; pass 2 holds a position's reads until its last one, deduplicates closed positions in windows of
// --two-pass-window reads (one batched library call each) and writes the survivors through a reorder
// buffer in the one-pass order.  Same decompressed output and summary lines as one pass, plus
// "two-pass: <W> windows, at most <R> reads held" (run_two_pass).  --dump-staging and
// --passthrough keep their one-pass behaviour with it.
#pragma once
#include <sys/stat.h>

#include "hiplib.hpp"
#include "staging.hpp"

namespace {

// ---- --two-pass: the file is read twice and never held.  Pass 1 (census) walks the
// records without keeping them: counters, the kept unmapped reads (written at once: they come first), the
// UMI length, and per alignment key the index of its last read (UMICollapse's `latest`).  Pass 2 reads
// the file again; a position's reads are held until its last one has been read, closed positions gather
// in a window that goes to the library as one batched call once it holds --two-pass-window reads, and a
// reorder buffer writes the survivors in the one-pass order (positions by first appearance).  Output and
// summary lines are those of the one-pass run; only the decompressed stream is equal, the BGZF block cut
// differs.

// Records of a BGZF-compressed BAM, one at a time (the checks of umi::bam::File::parse_behind); only
// the chunk being parsed and a record cut by its end are held.
class RecordStream
{
  public:
    RecordStream(const std::string &path, unsigned threads) : in_(path, threads) {}
    // the header (magic .. end of the reference list), verbatim
    umi::bgzf::Bytes header()
    {
        size_t q;
        while (!(q = header_len()))
            if (!more()) {
                if (buf_.size() >= 4 && std::memcmp(buf_.data(), "BAM\1", 4) != 0)
                    throw umi::bam::FormatError("Invalid input path: not a BAM file");
                throw umi::bam::FormatError("truncated BAM header");
            }
        umi::bgzf::Bytes h(buf_.begin(), buf_.begin() + (ptrdiff_t)q);
        pos_ = q;
        return h;
    }
    // the next record, valid until the next call; false at the end of the file
    bool next(umi::bam::Record &r)
    {
        while (true) {
            const size_t avail = buf_.size() - pos_;
            if (avail >= 4) {
                const uint8_t *p = buf_.data() + pos_;
                const int32_t bs = umi::bam::rd_i32(p);
                if (bs < 32) throw umi::bam::FormatError("Failed to parse record");
                if (avail - 4 >= (size_t)bs) {
                    const umi::bam::Record rec{p, p + 4 + (size_t)bs};
                    const int32_t l_seq = rec.l_seq();
                    if (l_seq < 0 || 32ull + rec.l_read_name() + 4ull * rec.n_cigar() + ((uint64_t)l_seq + 1) / 2 +
                                             (uint64_t)l_seq > (uint64_t)bs)
                        throw umi::bam::FormatError("Failed to parse record");
                    pos_ += 4 + (size_t)bs;
                    r = rec;
                    return true;
                }
            }
            if (!more()) {
                if (avail) throw umi::bam::FormatError("Failed to parse record");
                return false;
            }
        }
    }

  private:
    bool more()
    {
        buf_.erase(buf_.begin(), buf_.begin() + (ptrdiff_t)pos_);
        pos_ = 0;
        return in_.next(buf_);
    }
    // bytes of the header once they are all there, else 0
    size_t header_len() const
    {
        const uint8_t *p = buf_.data();
        const size_t size = buf_.size();
        if (size < 12) return 0;
        if (std::memcmp(p, "BAM\1", 4) != 0) throw umi::bam::FormatError("Invalid input path: not a BAM file");
        const int32_t l_text = umi::bam::rd_i32(p + 4);
        if (l_text < 0) throw umi::bam::FormatError("truncated BAM header");
        size_t q = 8 + (size_t)l_text;
        if (size < q + 4) return 0;
        const int32_t n_ref = umi::bam::rd_i32(p + q);
        if (n_ref < 0) throw umi::bam::FormatError("truncated BAM header");
        q += 4;
        for (int32_t r = 0; r < n_ref; r++) {
            if (size < q + 4) return 0;
            const int32_t l_name = umi::bam::rd_i32(p + q);
            if (l_name < 0) throw umi::bam::FormatError("truncated BAM header");
            q += 4 + (size_t)l_name + 4;
            if (size < q) return 0;
        }
        return q;
    }
    umi::bgzf::ChunkReader in_;
    umi::bgzf::Bytes buf_;
    size_t pos_ = 0;
};

struct TwoPass {
    const Cli &args;
    HipLib &lib;
    GpuWarmup &gpu;
    Clock &clock;
    const double t_start;
    const int algo = args.algo_id, merge = args.merge_id;
    const unsigned T = std::max(1u, args.num_threads);
    struct ReadRef {
        uint64_t off;    // of the record in its position's bytes
        uint32_t umi_at; // of the UMI in the read name
        int32_t score;
    };
    struct Bucket {
        uint64_t seq = 0, last = 0; // first-appearance rank; index of the last read
        std::vector<uint8_t> bytes;
        std::vector<ReadRef> reads;
    };
    struct Survivors { // a deduplicated position's written records, in rank order
        std::vector<uint8_t> bytes;
        uint64_t count = 0;
    };
    struct Mate {
        uint64_t ri;
        std::string key;
        std::vector<uint8_t> rec;
    };

    umi::bgzf::ChunkWriter out{args.output, T, args.compress_level};
    size_t umi_length = args.umi_length;
    Summary sum;
    std::unordered_map<AlignKey, uint64_t, KeyHash> latest; // alignment key -> index of its last read
    std::unordered_map<int32_t, uint64_t> last_mate_on;     // --paired: reference -> index of its last candidate second mate
    std::unordered_map<uint64_t, uint32_t> reg_count;       // --paired: hash of the (qname, mate ref, mate pos) a staged
                                                            // first mate registers -> first mates not yet written or dropped
    bool bad_char = false;
    // --umi-tag / --per-cell: reads without their tags are dropped in both passes; a barcode's id is its rank
    // of first appearance, as in one pass, and the positions are counted apart from the (position, cell) groups
    const bool by_tags = !args.umi_tag.empty() || args.per_cell;
    std::unordered_map<std::string, uint64_t> cell_ids;
    std::unordered_set<AlignKey, KeyHash> positions;
    double t_census = 0.0;
    bool gpu_stage = false;
    int n_words = 1;

    // ---- pass 2
    std::unordered_map<AlignKey, Bucket, KeyHash> open;
    std::vector<Bucket> window;
    std::unordered_map<uint64_t, Survivors> pending; // the reorder buffer
    std::unordered_map<int32_t, std::vector<Mate>> mates; // --paired: second mates by reference, file order
    std::unordered_set<std::string> waiting;
    uint64_t next_seq = 0, next_out = 0, n_windows = 0, done_upto = 0; // done_upto: records of pass 2 read so far
    bool pass2_done = false, have_ref = false, stalled = false;
    int32_t cur_ref = 0;
    uint64_t held_open = 0, held_window = 0, held_pending = 0, held_mates = 0, peak = 0;
    uint64_t n_pairs = 0;
    double t_hot = 0.0;

    TwoPass(const Cli &a, HipLib &l, GpuWarmup &g, Clock &c, double t0) : args(a), lib(l), gpu(g), clock(c), t_start(t0) {}
    static uint64_t reg_hash(const std::string &key) { return (uint64_t)std::hash<std::string>()(key); }
    static umi::bam::Record rec_at(const uint8_t *p) { return umi::bam::Record{p, p + 4 + (size_t)umi::bam::rd_i32(p)}; }
    void note_peak() { peak = std::max(peak, held_open + held_window + held_pending + held_mates); }

    // the (alignment, cell) key of a staged read, false if it lacks a tag (census: counted; err ends the run)
    bool staged_key(const umi::bam::Record &r, ReadTags &tg, AlignKey &key, bool census)
    {
        key = align_key(r, args.paired);
        if (!by_tags) return true;
        std::string err;
        const uint8_t miss = read_tags(args, r, tg, err);
        if (!err.empty()) die(err);
        if (miss) {
            if (census) {
                sum.no_umi_tag += (miss & MISS_UMI) ? 1 : 0;
                sum.no_cell += (miss & MISS_CELL) ? 1 : 0;
            }
            return false;
        }
        if (args.per_cell) {
            if (census) positions.insert(key);
            key.cell = census ? cell_ids.emplace(std::string(tg.cell), cell_ids.size()).first->second
                              : cell_ids.at(std::string(tg.cell));
        }
        return true;
    }

    void census()
    {
        {
            RecordStream rs(args.input, T);
            const umi::bgzf::Bytes h = rs.header();
            out.write(h.data(), h.size());
            umi::bam::Record r;
            UmiKey k, nm;
            for (uint64_t ri = 0; rs.next(r); ri++) {
                uint8_t up, ch;
                const uint8_t state = read_state(args, r, up, ch);
                if (state != 3) sum.total_read_count++;
                sum.unpaired += up;
                sum.chimeric += ch;
                if (args.paired && mate_candidate(r)) last_mate_on[r.tid()] = ri;
                if (state == 4) sum.unmapped++;
                if (state == 1) {
                    sum.unmapped++;
                    if (args.keep_unmapped) out.write(r.begin, (size_t)(r.end - r.begin)); // :104-106, ahead of every position
                }
                if (state != 0) continue;
                ReadTags tg;
                AlignKey key;
                if (!staged_key(r, tg, key, true)) continue;
                if (umi_length == 0) umi_length = detect_length(args, r, tg); // :154-156
                size_t at;
                const std::string err = umi_offset(args, r, tg, umi_length, at);
                if (!err.empty()) die(err);
                if (!bad_char && !encode_umi(r.qname() + at, umi_length, &k, &nm)) bad_char = true;
                latest[key] = ri;
                if (args.paired && r.is_paired()) reg_count[reg_hash(mate_key(r.qname(), r.qname_len(), r.mtid(), r.mpos()))]++;
            }
        }
        if (bad_char) die("Unknown character in UMI sequence");
        clock.lap("census");
        t_census = now_s();

        gpu_stage = args.stage != "host" && !args.paired && umi_length >= 1;
        if (args.stage == "gpu" && !gpu_stage) die("--stage gpu does not go with --paired, --tag or --dump-staging");
        n_words = umi_length ? (int)((3 * umi_length + 63) / 64) : 1;
        check_edit_length(args, umi_length, "this file's have");
    }

    void release(const umi::bam::Record &r)
    { // a staged first mate written or dropped
        if (!args.paired || !r.is_paired()) return;
        auto it = reg_count.find(reg_hash(mate_key(r.qname(), r.qname_len(), r.mtid(), r.mpos())));
        if (it != reg_count.end() && --it->second == 0) reg_count.erase(it);
    }

    // UcWriter::write_reversed (:382-459) over the held second mates of one reference (or all of them, at
    // the end) in file order; a mate no staged first mate can still register is let go
    void flush_mates(int32_t tid, bool all)
    {
        std::vector<Mate> cands;
        if (all) {
            for (auto &m : mates)
                for (Mate &x : m.second) cands.push_back(std::move(x));
            mates.clear();
            std::sort(cands.begin(), cands.end(), [](const Mate &a, const Mate &b) { return a.ri < b.ri; });
        } else {
            auto it = mates.find(tid);
            if (it == mates.end()) return;
            cands.swap(it->second);
            mates.erase(it);
        }
        std::vector<Mate> keep;
        for (Mate &m : cands) {
            auto w = waiting.find(m.key);
            if (w != waiting.end()) {
                out.write(m.rec.data(), m.rec.size());
                waiting.erase(w);
            } else if (!all && reg_count.count(reg_hash(m.key))) {
                keep.push_back(std::move(m));
            }
        }
        held_mates -= cands.size() - keep.size();
        if (!keep.empty()) mates[tid] = std::move(keep);
    }

    // write the deduplicated positions that are next in first-appearance order
    void pump()
    {
        stalled = false;
        for (auto it = pending.find(next_out); it != pending.end(); it = pending.find(++next_out)) {
            Survivors &sv = it->second;
            if (args.paired && sv.count) {
                const int32_t tid = rec_at(sv.bytes.data()).tid();
                if (have_ref && cur_ref != tid) {
                    auto lm = last_mate_on.find(cur_ref); // (every second mate of the reference must have been read)
                    if (!pass2_done && lm != last_mate_on.end() && lm->second >= done_upto) {
                        stalled = true;
                        return;
                    }
                    flush_mates(cur_ref, false);
                }
            }
            for (size_t o = 0; o < sv.bytes.size();) {
                const umi::bam::Record r = rec_at(sv.bytes.data() + o);
                const size_t len = (size_t)(r.end - r.begin);
                if (args.paired) {
                    have_ref = true;
                    cur_ref = r.tid();
                    if (r.is_paired()) waiting.insert(mate_key(r.qname(), r.qname_len(), r.mtid(), r.mpos())); // :395-401
                    release(r);
                }
                out.write(r.begin, len);
                o += len;
            }
            held_pending -= sv.count;
            pending.erase(it);
        }
    }

    // one batched library call for the closed positions of the window, in first-appearance order
    void run_window()
    {
        if (window.empty()) return;
        std::sort(window.begin(), window.end(), [](const Bucket &a, const Bucket &b) { return a.seq < b.seq; });
        const size_t nb = window.size();
        std::vector<uint64_t> read_base(nb + 1, 0);
        for (size_t b = 0; b < nb; b++) read_base[b + 1] = read_base[b] + window[b].reads.size();
        const size_t nr = read_base[nb];
        U64s keys(nr * n_words), nmask(nr * n_words), off(nr + 1), rep(nr);
        I32s freq(nr);
        auto umi_of = [&](const Bucket &bk, const ReadRef &rr) { return bk.bytes.data() + rr.off + 4 + 32 + rr.umi_at; };
        uint64_t ne = 0, nbk = 0;
        umi_ctx *ctx = gpu.get();
        const double t0 = now_s();
        if (gpu_stage) {
            // (the window's position rank is the alignment key: the reads go in position by position, file order inside)
            U64s akey(nr);
            umi::bgzf::Bytes umis(nr * umi_length);
            I32s sc(nr);
            for (size_t b = 0; b < nb; b++)
                for (size_t j = 0; j < window[b].reads.size(); j++) {
                    const size_t g = read_base[b] + j;
                    akey[g] = b;
                    std::memcpy(&umis[g * umi_length], umi_of(window[b], window[b].reads[j]), umi_length);
                    sc[g] = window[b].reads[j].score;
                }
            if (lib.stage_reads(ctx, akey.data(), bits_of(nb), umis.data(), sc.data(), nr, (int)umi_length, n_words, merge != 0 ? 1 : 0,
                                keys.data(), nmask.data(), freq.data(), rep.data(), off.data(), &ne, &nbk) != UMI_OK)
                die(lib.last_error());
            if (nbk != nb) die("device staging returned " + std::to_string(nbk) + " positions for " + std::to_string(nb));
        } else {
            // deduplicate_sam.rs:148-176 per position, then the stable freq-descending rank order
            UmiIndex idx;
            std::vector<Entry> ents;
            std::vector<uint32_t> members;
            size_t w = 0;
            off[0] = 0;
            for (size_t b = 0; b < nb; b++) {
                const Bucket &bk = window[b];
                idx.clear();
                ents.clear();
                members.clear();
                for (uint32_t j = 0; j < bk.reads.size(); j++) {
                    UmiKey k, nm;
                    encode_umi(umi_of(bk, bk.reads[j]), umi_length, &k, &nm); // (checked by the census)
                    add_read(idx, ents, members, k, nm, bk.reads[j].score, j, merge);
                }
                emit_position(ents, members, n_words, keys.data(), nmask.data(), freq.data(), w);
                for (const Entry &en : ents) rep[en.index] = read_base[b] + en.rep;
                off[b + 1] = w;
            }
            ne = w;
        }
        bool any_n = false;
        for (size_t i = 0; i < ne * n_words; i++) any_n |= nmask[i] != 0;
        std::vector<uint8_t> kept(ne + 1, 0);
        umi_stats st;
        std::memset(&st, 0, sizeof(st));
        if (lib.dedup(ctx, keys.data(), any_n ? nmask.data() : nullptr, n_words, freq.data(), off.data(), nb,
                      (int)umi_length, args.k, args.percentage, algo, 0 /* adjacency.rs:56 */, kept.data(), nullptr,
                      &st) != UMI_OK)
            die(lib.last_error());
        t_hot += now_s() - t0;
        sum.n += ne;
        sum.nb += nb;
        sum.n_kept += st.n_kept;
        n_pairs += st.n_pairs;
        std::vector<uint8_t> survivor;
        for (size_t b = 0; b < nb; b++) {
            Bucket &bk = window[b];
            sum.max_umi = std::max<size_t>(sum.max_umi, off[b + 1] - off[b]);
            Survivors sv;
            if (args.paired) survivor.assign(bk.reads.size(), 0);
            for (uint64_t e = off[b]; e < off[b + 1]; e++) {
                if (!kept[e]) continue;
                const uint64_t j = rep[e] - read_base[b];
                const umi::bam::Record r = rec_at(bk.bytes.data() + bk.reads[j].off);
                sv.bytes.insert(sv.bytes.end(), r.begin, r.end);
                sv.count++;
                if (args.paired) survivor[j] = 1;
            }
            if (args.paired) // the merged-away and removed first mates register nothing
                for (size_t j = 0; j < bk.reads.size(); j++)
                    if (!survivor[j]) release(rec_at(bk.bytes.data() + bk.reads[j].off));
            held_pending += sv.count;
            pending.emplace(bk.seq, std::move(sv));
        }
        note_peak();
        held_window = 0;
        window.clear();
        n_windows++;
        pump();
    }

    // (the paired writer here -- flush_mates over a stream, behind a reorder buffer -- and the one-pass
    // OnePass::select_paired, which walks the record indices of a file held in memory, are different algorithms)
    void pass2()
    {
        {
            RecordStream rs(args.input, T);
            (void)rs.header();
            umi::bam::Record r;
            for (uint64_t ri = 0; rs.next(r); ri++) {
                done_upto = ri + 1;
                uint8_t up, ch;
                const uint8_t state = read_state(args, r, up, ch);
                if (args.paired && mate_candidate(r)) {
                    std::string key = mate_key(r.qname(), r.qname_len(), r.tid(), r.pos());
                    if (waiting.count(key) || reg_count.count(reg_hash(key))) { // (else no first mate can ask for it)
                        mates[r.tid()].push_back(Mate{ri, std::move(key), std::vector<uint8_t>(r.begin, r.end)});
                        held_mates++;
                        note_peak();
                    }
                }
                ReadTags tg;
                AlignKey key;
                if (state == 0 && staged_key(r, tg, key, false)) {
                    auto it = open.find(key);
                    if (it == open.end()) {
                        it = open.emplace(key, Bucket()).first;
                        it->second.seq = next_seq++;
                        auto l = latest.find(key);
                        it->second.last = l->second;
                        latest.erase(l);
                    }
                    Bucket &bk = it->second;
                    size_t at;
                    (void)umi_offset(args, r, tg, umi_length, at); // (checked by the census)
                    bk.reads.push_back({bk.bytes.size(), (uint32_t)at, merge == 2 ? (int32_t)r.mapq() : r.avg_qual()});
                    bk.bytes.insert(bk.bytes.end(), r.begin, r.end);
                    held_open++;
                    note_peak();
                    if (ri == bk.last) { // the position is closed
                        held_open -= bk.reads.size();
                        held_window += bk.reads.size();
                        window.push_back(std::move(bk));
                        open.erase(it);
                        if (held_window >= args.two_pass_window) run_window();
                    }
                }
                if (stalled) pump();
            }
        }
        pass2_done = true;
        if (!open.empty()) die("two-pass: the input changed between the passes");
        run_window();
        pump();
        if (have_ref) flush_mates(0, true); // close(), :411-415
    }

    void finish()
    {
        clock.lap("pass-2");
        const double t_pass2 = now_s();
        out.close();
        clock.lap("write");
        const double t_end = now_s();

        sum.n_positions = args.per_cell ? positions.size() : sum.nb;
        std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_census - t_start);
        sum.print(args);
        std::fprintf(stderr, "two-pass: %llu windows, at most %llu reads held\n", (unsigned long long)n_windows,
                     (unsigned long long)peak);
        std::fprintf(stderr,
                     "phases: census %.3f s, pass 2 (staging %s) %.3f s, hot path (H2D+GPU+D2H) %.3f s [%llu pairs], write %.3f s\n",
                     t_census - t_start, gpu_stage ? "gpu" : "host", t_pass2 - t_census, t_hot, (unsigned long long)n_pairs,
                     t_end - t_pass2);
        std::fprintf(stderr, "UMI collapsing finished in %.3f seconds\n", t_end - t_start);
    }
};

void run_two_pass(const Cli &args, HipLib &lib, GpuWarmup &gpu, Clock &clock, double t_start)
{
    struct stat sb;
    if (::stat(args.input.c_str(), &sb) != 0) die("Invalid input path: " + args.input);
    if (!S_ISREG(sb.st_mode)) die("--two-pass reads the input twice: -i must be a regular file (" + args.input + ")");
    check_stage(args);
    TwoPass tp(args, lib, gpu, clock, t_start);
    tp.census();
    tp.pass2();
    tp.finish();
}

} // namespace
