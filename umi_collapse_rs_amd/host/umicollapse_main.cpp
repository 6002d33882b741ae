// `umicollapse`: the reference's command-line surface (src/cli.rs:7-77, src/main.rs:17-103)
// over the MI355X hot path.  BAM in -> read staging (src/deduplicate_sam.rs:93-177) ->
// ONE batched GPU call for every alignment position (replaces the loop :207-233) -> BAM out.
//
// "Next" rows N1/N2 of SURVEY.md 8f.  Deterministic where the reference is not: buckets and
// freq ties follow first appearance in the input (canonical determinisation).
// --paired (N4): template length joins the alignment key, second mates are skipped while
// staging and follow their surviving first mates into the output (UcWriter,
// deduplicate_sam.rs:339-459).
// --tag (N3): the reference stops after collecting its ClusterTrackers (the second pass is a
// TODO, deduplicate_sam.rs:236-239, so its output holds no deduplicated records at all).  Here
// the pass is finished from what the trackers hold (cluster_tracker.rs:76-103): every staged
// read is written, in file order, with MI:i = cluster id (offset + index of the cluster's root
// among the survivors), cs:i = reads in the cluster, su:i = reads with the same UMI at the same
// position.  Nothing in the reference to be in parity with: tests/bamio.py defines it.
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
// --two-pass (the reference parses it and ignores it; UMICollapse's meaning): the input is read twice and
// never held.  Pass 1 counts, writes the kept unmapped reads and notes the last read of every alignment
// key; pass 2 holds a position's reads until its last one, deduplicates closed positions in windows of
// --two-pass-window reads (one batched library call each) and writes the survivors through a reorder
// buffer in the one-pass order.  Same decompressed output and summary lines as one pass, plus
// "two-pass: <W> windows, at most <R> reads held" (run_two_pass).  --dump-staging and
// --passthrough keep their one-pass behaviour with it.
// --umi-tag XX (bam/sam mode; fgbio / umi_tools / single-cell convention, not the reference's): the UMI of a
// staged read is the value of its aux tag XX (type Z; -u N or the first staged read's length; another length
// ends the run naming the read, a byte outside ATCGN -- a duplex "-" included -- is "Unknown character";
// --umi_sep is ignored).  --per-cell: a position is (alignment, cell barcode) -- the value of --cell-tag
// (default CB, type Z), compared byte for byte -- so UMIs of different cells are never compared.  A staged
// read without its tags is dropped, not written, and counted ("Number of reads without a UMI tag / a cell
// barcode", each tag counted by itself); "Number of unique alignment positions" still counts alignments,
// "Number of (position, cell) groups" the buckets, which the average and maximum lines are over.  A
// barcode's id is the rank of its first appearance (per-thread tables made global); the device staging takes
// it as the group key of umi_stage_reads_grouped_wide.  Everything else -- merge, --paired (the first
// mate's tags), --tag, --two-pass, --devices, --stage -- as without the flags; --dump-staging appends every
// bucket's cell id.  A malformed aux block or a tag of another type ends the run with status 101.
// --umi-whitelist FILE (bam/sam mode, one pass; fgbio CorrectUmis / umi_tools whitelist, not the reference's):
// the UMIs of the reads that would be staged go through umi_correct_umis in one call, between the per-read
// pass and the staging.  A read whose UMI matches a listed one (at most --whitelist-max-mismatches away, the
// next best listed UMI at least --whitelist-min-distance further; both default 1) is staged with the listed
// UMI's bytes; any other is dropped like a read without its tag, not written, and counted ("Number of reads
// with a corrected UMI / an uncorrectable UMI", printed with the flag only).  Written records are the
// input's bytes.  The UMI length is the list's.  --whitelist-metrics FILE: umi, reads, exact, corrected per
// listed UMI.  Refused before the GPU is woken: fastq mode, --two-pass, --dump-staging, --passthrough, another
// -u, the other three flags alone, a list that is empty, of mixed lengths, with a byte outside ACGT, with a
// duplicate, or of more than 85 bases.
// --cell-whitelist FILE (with --per-cell; STARsolo's 1MM rule, not the reference's, tests/barcode_model.py defines
// it): the kit's cell barcodes, one per line, for files whose barcode tag is raw (--cell-tag CR).  The barcodes
// of the reads that would be staged go through umi_correct_barcodes in one call -- an indexed lookup of the
// barcode and its single substitutions, not a comparison with every entry -- after the per-read pass and
// before the barcodes are numbered: a listed barcode stands for itself, an unlisted one with exactly one
// listed barcode one substitution away (--cell-whitelist-max-mismatches 1, the default; 0: none) for that
// one, and a cell's id is the rank of first appearance of the corrected barcode.  Reads whose barcode is
// unlisted or ambiguous are dropped like reads without a barcode, not written, and counted ("Number of reads
// with a corrected / an unlisted / an ambiguous cell barcode", printed with the flag only).  The tag's value
// must have the list's length and bytes from ACGTN, else the run ends with status 101.  Written records are
// the input's bytes.  --cell-whitelist-metrics FILE: barcode, reads, exact, corrected per listed barcode that
// took a read.  Refused before the GPU is woken: without --per-cell, fastq mode, --two-pass, --dump-staging,
// --passthrough, the two other flags alone, a mismatch bound other than 0 or 1, a list that is empty, of mixed
// lengths, with a byte outside ACGT (Cell Ranger's "-1" suffix included), with a duplicate, or of more than 32
// bases.
// --call-consensus (bam/sam mode, one pass; not the reference's, tests/bam_consensus_model.py defines it): the
// same records in the same order, but of each kept record the sequence and the qualities are its cluster's
// consensus.  A cluster is a kept entry with every entry it removed, as for --tag; its voters are its reads
// whose l_seq and CIGAR (n_cigar_op and the op words) are the representative's and that have qualities (the
// reads of a position share strand and unclipped 5' end, so these line up column by column).  Per column the
// base (nibble 1, 2, 4, 8) with the greatest sum of min(quality, 93) over the voters, ties by their number and
// then the order ACGT, quality min(93, winner's sum - the others'), nibble 15 and quality 0 where nobody voted
// (umi_consensus_bam, include/umihip.h: one call, the inflated file and the voters' offsets go up for it).
// The record keeps everything else -- MAPQ, flags, its aux fields (an NM or MD may now be stale) -- and gets
// cD:i = voters, cs:i = reads of the cluster (--tag's cs), ce:i = base votes that lost, appended.  A cluster
// whose representative has no bases or no qualities is written unchanged, without the tags ("Number of
// clusters without a consensus").  --call-consensus-min-reads M (default 1) leaves out the clusters with a
// consensus of fewer than M voters ("Number of clusters below --call-consensus-min-reads").  Host staging,
// as --tag.  Refused with status 101: with fastq mode, --tag, --two-pass, --paired, --dump-staging or
// --passthrough; the second flag without the first or not a number >= 1; a staged read of more than 1024
// bases.
// --distance hamming|edit (bam/sam mode; not the reference's, tests/edit_model.py defines it): which distance -k
// bounds.  hamming, the default, is the reference's umi_dist and changes nothing.  edit is the Levenshtein
// distance over the UMI's letters -- substitution, insertion and deletion cost 1 each, N matches N only -- which
// sees the shift that a base lost or gained in synthesis leaves in a fixed-length UMI window: ACGTACGTACGT
// without its first base reads CGTACGTACGTx, Hamming distance ~9, edit distance 2.  Between UMIs of one length
// an indel costs 2 (one insertion and one deletion), the two distances agree wherever either is at most 1, and
// -k 0 / -k 1 therefore give the Hamming result: the flag matters from -k 2.  Only the batched library call
// differs (umi_dedup_batch_edit, include/umihip.h): -k, -p, --algo, --merge, --keep-unmapped, --paired, --tag,
// --umi-tag, --per-cell, --umi-whitelist, --call-consensus, --two-pass and both --stage values work as before;
// the summary gains "UMI distance: edit".  Refused with status 101: any other value, fastq mode, several
// --devices, a UMI length above 21 (-u, the whitelist's, or the first staged read's).
// Not implemented, as in the reference: --algo cc.
#include <algorithm>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <dlfcn.h>
#include <functional>
#include <future>
#include <sys/stat.h>
#include <string>
#include <string_view>
#include <unistd.h>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "../../include/umihip.h"
#include "bam.hpp"
#include "bgzf.hpp"
#include "fastq.hpp"

namespace {

struct Cli { // src/cli.rs:7-77 (same flags, same defaults)
    std::string mode = "bam", input, output, algo = "dir", merge, data = "ngrambktree";
    int k = 1;
    size_t umi_length = 0;
    float percentage = 0.5f;
    unsigned num_threads = 1;
    uint8_t umi_sep = '_';
    bool two_pass = false, paired = false, remove_unpaired = false, remove_chimeric = false,
         keep_unmapped = false, track_clusters = false;
    // development switches (not in the reference)
    std::string dump_staging; // write the staged hot-path input here and stop before the GPU
    bool passthrough = false; // write every mapped record back (codec round trip), no dedup
    std::vector<int> devices{0}; // --device <ID> or --devices <ID,ID,...>
    int compress_level = 1;      // --compress-level 0..9: deflate level of the output's BGZF blocks.  Parity is
                                 // defined on the decompressed stream (htslib's own level and backend are
                                 // not reproducible here), and level 1 deflates a third of level 6's time
    uint64_t two_pass_window = 1u << 21; // --two-pass-window <N>: reads per GPU call of --two-pass (see run_two_pass)
    std::string stage = "auto";  // --stage gpu|host|auto: where the reads are merged per (position, UMI) and
                                 // put in rank order (auto: on the GPU unless --paired or --tag need the
                                 // host's per-read bookkeeping)
    std::string umi_tag;         // --umi-tag XX: the UMI is the value of this aux tag, not the name's suffix
    std::string cell_tag = "CB"; // --cell-tag XX: the cell barcode's tag (--per-cell)
    bool per_cell = false, cell_tag_given = false; // --per-cell: positions are (alignment, cell barcode)
    bool consensus = false;           // --consensus (fastq mode): every cluster written as its consensus read
    uint64_t consensus_min_reads = 1; // --consensus-min-reads M: clusters of fewer members are left out
    bool consensus_min_given = false;
    bool call_consensus = false;           // --call-consensus (bam/sam mode): kept records carry their cluster's consensus
    uint64_t call_consensus_min_reads = 1; // --call-consensus-min-reads M: clusters of fewer voters are left out
    bool call_consensus_min_given = false;
    std::string umi_whitelist;     // --umi-whitelist FILE: every UMI is snapped to the nearest listed one first
    std::string whitelist_metrics; // --whitelist-metrics FILE: reads, exact, corrected per listed UMI
    int wl_max_mismatches = 1, wl_min_distance = 1; // --whitelist-max-mismatches, --whitelist-min-distance
    std::string cell_whitelist;         // --cell-whitelist FILE: cell barcodes are snapped to the kit's list first
    std::string cell_whitelist_metrics; // --cell-whitelist-metrics FILE: reads, exact, corrected per listed barcode
    int cell_wl_max_mismatches = 1;     // --cell-whitelist-max-mismatches: 0 or 1
    bool cell_wl_max_given = false;
    bool wl_max_given = false, wl_min_given = false;
    bool edit_distance = false; // --distance edit: -k bounds the Levenshtein distance (umi_dedup_batch_edit)
};

[[noreturn]] void die(const std::string &msg)
{ // the reference panics (panic = "abort")
    std::fprintf(stderr, "umicollapse: %s\n", msg.c_str());
    std::fflush(stderr);
    std::_Exit(101); // (no static destructors: the GPU's start-up thread may still be running)
}

// libumihip.so is opened by hand, on the side thread that wakes the GPU: mapping the library and
// the HIP runtime it brings along (static initialisers, the code objects' registration) takes
// ~0.15 s before main() of a process that otherwise lives 0.45 s, and the first thing the
// program does -- reading and inflating the input -- needs none of it.
struct HipLib {
    void *handle = nullptr;
    int (*ctx_create_multi)(const int *, int, umi_ctx **) = nullptr;
    int (*ctx_set_option)(umi_ctx *, const char *, int64_t) = nullptr;
    const char *(*last_error)(void) = nullptr;
    // (the forms for keys of any number of words: one word is the ordinary call behind them)
    int (*stage_reads)(umi_ctx *, const uint64_t *, int, const uint8_t *, const int32_t *, uint64_t, int, int, int,
                       uint64_t *, uint64_t *, int32_t *, uint64_t *, uint64_t *, uint64_t *, uint64_t *) = nullptr;
    // --per-cell: positions are (alignment, cell id) pairs
    int (*stage_reads_grouped)(umi_ctx *, const uint64_t *, int, const uint64_t *, int, const uint8_t *, const int32_t *,
                               uint64_t, int, int, int, uint64_t *, uint64_t *, int32_t *, uint64_t *, uint64_t *, uint64_t *,
                               uint64_t *) = nullptr;
    int (*dedup_batch)(umi_ctx *, const uint64_t *, const uint64_t *, int, const int32_t *, const uint64_t *, uint64_t,
                       int, int, float, int, int32_t, uint8_t *, uint32_t *, umi_stats *) = nullptr;
    int (*dedup_seqs)(umi_ctx *, const uint64_t *, const uint64_t *, int, const int32_t *, const uint64_t *,
                      const int32_t *, uint64_t, int, float, int, int32_t, uint8_t *, uint32_t *, umi_stats *) = nullptr;
    // fastq mode's device staging: its arrays stay on the device between the two calls
    int (*stage_seqs)(umi_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint64_t, int, int,
                      uint64_t *, uint64_t *, int32_t *, uint64_t *, uint32_t *, uint64_t *, int32_t *, uint64_t *,
                      uint64_t *, int *) = nullptr;
    int (*stage_seqs_device)(umi_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint64_t, int,
                             int, uint64_t *, uint64_t *, int32_t *, uint64_t *, uint32_t *, uint64_t *, int32_t *,
                             uint64_t *, uint64_t *, int *, void *) = nullptr;
    int (*dedup_seqs_device)(umi_ctx *, const uint64_t *, const uint64_t *, int, const int32_t *, const uint64_t *,
                             const int32_t *, uint64_t, int, float, int, int32_t, uint8_t *, uint32_t *, void *,
                             umi_stats *) = nullptr;
    // --distance edit: resolved only when the flag is given, like --consensus below; one-word keys only
    bool want_edit = false;
    int (*dedup_batch_edit)(umi_ctx *, const uint64_t *, const uint64_t *, const int32_t *, const uint64_t *, uint64_t, int, int,
                            float, int, int32_t, uint8_t *, uint32_t *, umi_stats *) = nullptr;
    // the batched call of the run: by the distance --distance names
    int dedup(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq, const uint64_t *off,
              uint64_t nb, int umi_len, int k, float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
              umi_stats *st) const
    {
        if (want_edit) // (n_words is 1: a UMI length above 21 has been refused)
            return dedup_batch_edit(ctx, keys, nmask, freq, off, nb, umi_len, k, percentage, algo, adj_max_freq, kept, root, st);
        return dedup_batch(ctx, keys, nmask, n_words, freq, off, nb, umi_len, k, percentage, algo, adj_max_freq, kept, root, st);
    }
    // --consensus: resolved only when the flag is given, so that a library without them serves every other run
    bool want_consensus = false;
    int (*consensus_seqs)(umi_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint64_t,
                          const uint32_t *, const int32_t *, const uint8_t *, const uint32_t *, uint64_t, const uint64_t *,
                          const int32_t *, uint64_t, uint8_t *, uint8_t *, uint64_t *, uint32_t *, uint64_t *) = nullptr;
    int (*consensus_seqs_device)(umi_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *, uint64_t,
                                 const uint32_t *, const int32_t *, const uint8_t *, const uint32_t *, uint64_t,
                                 const uint64_t *, const int32_t *, uint64_t, uint8_t *, uint8_t *, uint64_t *, uint32_t *,
                                 uint64_t *, void *) = nullptr;
    // --call-consensus: likewise
    bool want_consensus_bam = false;
    int (*consensus_bam)(umi_ctx *, const uint8_t *, const uint64_t *, const uint64_t *, const uint32_t *, const uint32_t *,
                         uint64_t, const uint32_t *, uint64_t, uint8_t *, uint8_t *, uint64_t *, uint64_t *, uint32_t *,
                         uint32_t *, uint64_t *, uint64_t *) = nullptr;
    // --umi-whitelist: resolved only when the flag is given, like --consensus
    bool want_correct = false;
    int (*correct_umis)(umi_ctx *, const uint8_t *, uint64_t, int, const uint8_t *, uint32_t, int, int, uint8_t *, int32_t *,
                        uint8_t *, uint8_t *, uint64_t *) = nullptr;
    // --cell-whitelist: likewise
    bool want_barcodes = false;
    int (*correct_barcodes)(umi_ctx *, const uint8_t *, uint64_t, int, const uint8_t *, uint32_t, int, int32_t *, uint8_t *,
                            uint64_t *) = nullptr;
    // (the HIP runtime the library brings along: device buffers for the arrays above)
    int (*hip_set_device)(int) = nullptr; // (the current device is per thread: the context was made on another)
    int (*hip_malloc)(void **, size_t) = nullptr;
    int (*hip_memcpy)(void *, const void *, size_t, int) = nullptr; // kind: 1 host to device, 2 device to host
    std::string error;
    bool load()
    {
        if (handle) return true;
        char exe[4096];
        const ssize_t n = readlink("/proc/self/exe", exe, sizeof(exe) - 1);
        std::string dir = n > 0 ? std::string(exe, (size_t)n) : std::string(".");
        dir = dir.substr(0, dir.find_last_of('/'));
        const std::string path = dir + "/../libumihip.so"; // bin/umicollapse beside the package's library
        handle = dlopen(path.c_str(), RTLD_NOW | RTLD_GLOBAL);
        if (!handle) {
            error = std::string("cannot load ") + path + ": " + dlerror() + " (there is no CPU path)";
            return false;
        }
        auto sym = [&](const char *name) {
            void *p = dlsym(handle, name);
            if (!p && error.empty()) error = std::string("libumihip.so lacks ") + name;
            return p;
        };
        ctx_create_multi = (decltype(ctx_create_multi))sym("umi_ctx_create_multi");
        ctx_set_option = (decltype(ctx_set_option))sym("umi_ctx_set_option");
        last_error = (decltype(last_error))sym("umi_last_error");
        stage_reads = (decltype(stage_reads))sym("umi_stage_reads_wide");
        // (looked up without a verdict: only --per-cell's GPU staging needs it, and says so if it is missing)
        stage_reads_grouped = (decltype(stage_reads_grouped))dlsym(handle, "umi_stage_reads_grouped_wide");
        dedup_batch = (decltype(dedup_batch))sym("umi_dedup_batch_wide");
        dedup_seqs = (decltype(dedup_seqs))sym("umi_dedup_seqs");
        stage_seqs = (decltype(stage_seqs))sym("umi_stage_seqs");
        stage_seqs_device = (decltype(stage_seqs_device))sym("umi_stage_seqs_device");
        dedup_seqs_device = (decltype(dedup_seqs_device))sym("umi_dedup_seqs_device");
        if (want_edit) dedup_batch_edit = (decltype(dedup_batch_edit))sym("umi_dedup_batch_edit");
        if (want_consensus) {
            consensus_seqs = (decltype(consensus_seqs))sym("umi_consensus_seqs");
            consensus_seqs_device = (decltype(consensus_seqs_device))sym("umi_consensus_seqs_device");
        }
        if (want_consensus_bam) consensus_bam = (decltype(consensus_bam))sym("umi_consensus_bam");
        if (want_correct) correct_umis = (decltype(correct_umis))sym("umi_correct_umis");
        if (want_barcodes) correct_barcodes = (decltype(correct_barcodes))sym("umi_correct_barcodes");
        hip_set_device = (decltype(hip_set_device))sym("hipSetDevice");
        hip_malloc = (decltype(hip_malloc))sym("hipMalloc");
        hip_memcpy = (decltype(hip_memcpy))sym("hipMemcpy");
        return error.empty();
    }
};

// A UMI key: BitSet.bits of the reference (src/utils/bitset.rs:9-27), up to 85 bases in four words
constexpr int MAX_WORDS = 4;
struct UmiKey {
    uint64_t w[MAX_WORDS];
    bool operator==(const UmiKey &o) const { return w[0] == o.w[0] && w[1] == o.w[1] && w[2] == o.w[2] && w[3] == o.w[3]; }
};
struct UmiKeyHash {
    size_t operator()(const UmiKey &k) const
    {
        uint64_t x = k.w[0] * 0x9E3779B97F4A7C15ull ^ (k.w[1] + 0x7F4A7C15u) * 0xD6E8FEB86659FD93ull ^ (k.w[2] << 7) ^ (k.w[3] >> 3);
        x ^= x >> 31;
        x *= 0xBF58476D1CE4E5B9ull;
        return (size_t)(x ^ (x >> 29));
    }
};

// src/utils/mod.rs:63-83 with the codes of src/utils/read.rs:23-31 (the library's umi_encode_umis[_wide],
// restated here so that the staging of the host path needs no library call); base b at bits
// 3b .. 3b+2 of the word string, bit by bit: a base may sit across two words (bitset.rs:52-75)
bool encode_umi(const uint8_t *u, size_t len, UmiKey *key, UmiKey *nmask)
{
    UmiKey k{{0, 0, 0, 0}}, nm{{0, 0, 0, 0}};
    for (size_t b = 0; b < len; b++) {
        uint64_t c;
        switch (u[b]) {
        case 'A': c = 0; break;
        case 'T': c = 5; break;
        case 'C': c = 6; break;
        case 'G': c = 3; break;
        case 'N': c = 4; break;
        default: return false;
        }
        for (int j = 0; j < 3; j++) {
            const size_t bit = 3 * b + j;
            if ((c >> j) & 1) k.w[bit >> 6] |= 1ull << (bit & 63);
            if (c == 4) nm.w[bit >> 6] |= 1ull << (bit & 63);
        }
    }
    *key = k;
    *nmask = nm;
    return true;
}

void usage()
{
    std::puts("Usage: umicollapse [OPTIONS] -i <INPUT_FILE> -o <OUITPUT_FILE>\n"
              "  -m, --mode <MODE>        Either fastq or SAM/BAM mode [default: bam]; fastq: whole reads\n"
              "                           (<= 256 bases) are the key, one bucket per read length\n"
              "  -k <K>                   Number of substitution edits to allow [default: 1]\n"
              "      --distance <D>       hamming or edit [default: hamming]: the distance -k bounds.  edit is the\n"
              "                           Levenshtein distance (substitution, insertion, deletion cost 1 each), which\n"
              "                           sees a UMI shifted by a lost or gained base; between UMIs of one length an\n"
              "                           indel costs 2, so -k 0 and -k 1 give the hamming result and the flag matters\n"
              "                           from -k 2 (bam/sam mode, one GPU, UMIs of at most 21 bases)\n"
              "  -u <UMI_LENGTH>          The UMI length [default: 0 = autodetect]; fastq: bases trimmed\n"
              "                           from the start of every written read\n"
              "  -p <PERCENTAGE>          Directional threshold percentage [default: 0.5]\n"
              "      --num-threads <N>    Threads used in reader/writer [default: 1]\n"
              "      --umi_sep <BYTE>     Separator byte value between UMI and read name [default: 95]\n"
              "      --algo <ALGO>        adj or dir [default: dir]\n"
              "      --merge <MERGE>      any, avgqual or mapqual [default: mapqual in bam mode, avgqual in fastq mode]\n"
              "      --data <DATA>        accepted; every value gives Naive's result (as in the reference)\n"
              "      --keep-unmapped      Keep unmapped reads\n"
              "      --paired             Paired-end mode: template length joins the alignment key,\n"
              "                           second mates follow their surviving first mates\n"
              "      --remove-unpaired    Remove unpaired reads (paired-end mode)\n"
              "      --remove-chimeric    Remove chimeric pairs (paired-end mode)\n"
              "      --tag                Write every read tagged with its cluster (MI, cs, su) instead of\n"
              "                           removing duplicates\n"
              "      --two-pass           Read the input twice and hold only the open positions: peak memory\n"
              "                           bounded for coordinate-sorted input, output identical to one pass\n"
              "                           (-i must be a regular file; not with --tag or fastq mode)\n"
              "      --two-pass-window <N> reads per GPU call with --two-pass [default: 2097152]\n"
              "      --compress-level <N> deflate level of the output BAM, 0..9 [default: 1]\n"
              "      --consensus          fastq mode: write every cluster as its consensus read -- each column the\n"
              "                           quality-weighted majority of all the cluster's reads -- in place of the kept\n"
              "                           read, the header with cluster_size=<reads> appended (not with --tag)\n"
              "      --consensus-min-reads <M> with --consensus: leave out clusters of fewer than M reads [default: 1]\n"
              "      --call-consensus     bam/sam mode: every kept record carries its cluster's consensus -- each column the\n"
              "                           quality-weighted majority of the cluster's reads with the kept read's length\n"
              "                           and CIGAR -- for sequence and qualities, with cD:i (voters), cs:i (reads of the\n"
              "                           cluster) and ce:i (base votes that lost) appended; everything else of the\n"
              "                           record stays (not with --tag, --paired, --two-pass)\n"
              "      --call-consensus-min-reads <M> with --call-consensus: leave out clusters of fewer than M voters\n"
              "                           [default: 1]\n"
              "      --stage <WHERE>      gpu, host or auto: where reads are merged per (position, UMI) [default: auto]\n"
              "      --umi-tag <XX>       the UMI is the value of aux tag XX (type Z, e.g. RX or UB) instead of the\n"
              "                           read name's suffix; reads without it are dropped (bam/sam mode)\n"
              "      --per-cell           deduplicate per cell: positions are (alignment, cell barcode); reads\n"
              "                           without a barcode are dropped (bam/sam mode)\n"
              "      --cell-tag <XX>      aux tag of the cell barcode, type Z [default: CB]\n"
              "      --umi-whitelist <FILE> the kit's UMIs, one per line (ACGT, all of one length; blank lines and\n"
              "                           lines starting with # skipped): every read's UMI is replaced, on the GPU, by\n"
              "                           the nearest listed one before the reads are grouped; reads that match none\n"
              "                           are dropped; written records keep their own bytes (bam/sam mode, one pass)\n"
              "      --whitelist-max-mismatches <M> a UMI matches a listed one at up to M mismatches [default: 1]\n"
              "      --whitelist-min-distance <D> ... if the next best listed UMI is at least D further away [default: 1]\n"
              "      --whitelist-metrics <FILE> write a table: umi, reads, exact, corrected per listed UMI, in list order\n"
              "      --cell-whitelist <FILE> with --per-cell: the kit's cell barcodes, one per line (ACGT, all of one\n"
              "                           length, at most 32 bases, no -1 suffix; blank lines and lines starting with #\n"
              "                           skipped): every read's barcode (--cell-tag CR for raw ones) is looked up in an\n"
              "                           index of the list on the GPU; an unlisted barcode one substitution from exactly\n"
              "                           one listed barcode counts as that one; reads with an unlisted or ambiguous\n"
              "                           barcode are dropped; written records keep their own bytes (bam/sam mode, one pass)\n"
              "      --cell-whitelist-max-mismatches <M> 0: listed barcodes only; 1: one substitution allowed [default: 1]\n"
              "      --cell-whitelist-metrics <FILE> write a table: barcode, reads, exact, corrected per listed barcode\n"
              "                           that took a read, in list order\n"
              "      --device <ID>        GPU to use [default: 0]\n"
              "      --devices <ID,..>    several GPUs of the node: alignment positions are sharded over them");
}

// a GPU id: decimal digits only (atoi would take "x" for device 0)
int device_id(const char *text)
{
    char *end = nullptr;
    const long v = std::strtol(text, &end, 10);
    if (end == text || *end != '\0' || v < 0 || v > 1023) die(std::string("not a GPU id: '") + text + "'");
    return (int)v;
}

Cli parse(int argc, char **argv)
{
    Cli c;
    auto need = [&](int &i) -> const char * {
        if (i + 1 >= argc) die(std::string("a value is required for '") + argv[i] + "'");
        return argv[++i];
    };
    for (int i = 1; i < argc; i++) {
        const std::string a = argv[i];
        if (a == "-m" || a == "--mode") c.mode = need(i);
        else if (a == "-i") c.input = need(i);
        else if (a == "-o") c.output = need(i);
        else if (a == "-k") c.k = std::atoi(need(i));
        else if (a == "-u") c.umi_length = (size_t)std::atol(need(i));
        else if (a == "-p") c.percentage = std::strtof(need(i), nullptr);
        else if (a == "--num-threads") c.num_threads = (unsigned)std::atoi(need(i));
        else if (a == "--umi_sep") c.umi_sep = (uint8_t)std::atoi(need(i)); // a number, cli.rs:31-32
        else if (a == "--algo") c.algo = need(i);
        else if (a == "--distance") {
            const std::string d = need(i);
            if (d != "hamming" && d != "edit") die("--distance wants hamming or edit: '" + d + "'");
            c.edit_distance = d == "edit";
        }
        else if (a == "--merge") c.merge = need(i);
        else if (a == "--data") c.data = need(i);
        else if (a == "--two-pass") c.two_pass = true;
        else if (a == "--two-pass-window") {
            const char *v = need(i);
            char *end = nullptr;
            const long long w = std::strtoll(v, &end, 10);
            if (end == v || *end != '\0' || w < 1) die("--two-pass-window wants a number of reads, 1 or more");
            c.two_pass_window = (uint64_t)w;
        }
        else if (a == "--paired") c.paired = true;
        else if (a == "--remove-unpaired") c.remove_unpaired = true;
        else if (a == "--remove-chimeric") c.remove_chimeric = true;
        else if (a == "--keep-unmapped") c.keep_unmapped = true;
        else if (a == "--tag") c.track_clusters = true;
        else if (a == "--dump-staging") c.dump_staging = need(i);
        else if (a == "--passthrough") c.passthrough = true;
        else if (a == "--stage") c.stage = need(i);
        else if (a == "--umi-tag" || a == "--cell-tag") {
            const std::string t = need(i);
            auto alpha = [](char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
            if (t.size() != 2 || !alpha(t[0]) || !(alpha(t[1]) || (t[1] >= '0' && t[1] <= '9'))) // SAM spec
                die(a + " wants a tag name of two characters, [A-Za-z][A-Za-z0-9]: '" + t + "'");
            if (a == "--umi-tag") c.umi_tag = t;
            else { c.cell_tag = t; c.cell_tag_given = true; }
        }
        else if (a == "--per-cell") c.per_cell = true;
        else if (a == "--umi-whitelist") c.umi_whitelist = need(i);
        else if (a == "--whitelist-metrics") c.whitelist_metrics = need(i);
        else if (a == "--whitelist-max-mismatches" || a == "--whitelist-min-distance") {
            const char *v = need(i);
            char *end = nullptr;
            const long long m = std::strtoll(v, &end, 10);
            if (end == v || *end != '\0' || m < 0 || m > INT32_MAX) die(a + " wants a number, 0 or more");
            if (a == "--whitelist-max-mismatches") { c.wl_max_mismatches = (int)m; c.wl_max_given = true; }
            else { c.wl_min_distance = (int)m; c.wl_min_given = true; }
        }
        else if (a == "--cell-whitelist") c.cell_whitelist = need(i);
        else if (a == "--cell-whitelist-metrics") c.cell_whitelist_metrics = need(i);
        else if (a == "--cell-whitelist-max-mismatches") {
            const std::string v = need(i);
            if (v != "0" && v != "1") die(a + " wants 0 or 1: '" + v + "'");
            c.cell_wl_max_mismatches = v == "1";
            c.cell_wl_max_given = true;
        }
        else if (a == "--consensus") c.consensus = true;
        else if (a == "--consensus-min-reads") {
            const char *v = need(i);
            char *end = nullptr;
            const long long m = std::strtoll(v, &end, 10);
            if (end == v || *end != '\0' || m < 1) die("--consensus-min-reads wants a number of reads, 1 or more");
            c.consensus_min_reads = (uint64_t)m;
            c.consensus_min_given = true;
        }
        else if (a == "--call-consensus") c.call_consensus = true;
        else if (a == "--call-consensus-min-reads") {
            const char *v = need(i);
            char *end = nullptr;
            const long long m = std::strtoll(v, &end, 10);
            if (end == v || *end != '\0' || m < 1) die("--call-consensus-min-reads wants a number of reads, 1 or more");
            c.call_consensus_min_reads = (uint64_t)m;
            c.call_consensus_min_given = true;
        }
        else if (a == "--compress-level") {
            c.compress_level = std::atoi(need(i));
            if (c.compress_level < 0 || c.compress_level > 9) die("--compress-level wants 0..9");
        }
        else if (a == "--device") c.devices.assign(1, device_id(need(i)));
        else if (a == "--devices") { // the GPUs of the node the position buckets are sharded over
            c.devices.clear();
            std::string list = need(i);
            for (size_t p = 0; p <= list.size();) {
                const size_t q = std::min(list.find(',', p), list.size());
                if (q == p) die("--devices wants a comma separated list of GPU ids");
                c.devices.push_back(device_id(list.substr(p, q - p).c_str()));
                p = q + 1;
            }
        }
        else if (a == "-h" || a == "--help") { usage(); std::exit(0); }
        else die("unexpected argument '" + a + "'");
    }
    if (c.input.empty() || c.output.empty()) { usage(); die("-i and -o are required"); }
    return c;
}

struct Entry { // one (alignment key, UMI): ReadFreq of src/utils/read_freq.rs + its key
    UmiKey key, nmask;
    int32_t freq;
    int32_t score;  // avg qual or mapq of the representative
    uint32_t rep;   // record index of the representative read
    uint32_t bucket;
};

// Align (deduplicate_sam.rs:478-481): Alignment{strand, coord, ref} or, with --paired,
// PairedAlignment{strand, coord, ref, tlen} (:547-553); ref as tid (equal names <=> equal tid)
struct AlignKey {
    uint64_t coord, ref_strand, tlen;
    uint64_t cell = 0; // --per-cell: the barcode's dense id (first-appearance rank); 0 otherwise
    bool operator==(const AlignKey &o) const
    {
        return coord == o.coord && ref_strand == o.ref_strand && tlen == o.tlen && cell == o.cell;
    }
};

struct KeyHash {
    size_t operator()(const AlignKey &k) const
    {
        uint64_t x = k.coord * 0x9E3779B97F4A7C15ull ^ (k.ref_strand + 0x7F4A7C15u) ^ (k.tlen * 0xD6E8FEB86659FD93ull) ^
                     (k.cell * 0x94D049BB133111EBull);
        x ^= x >> 29;
        x *= 0xBF58476D1CE4E5B9ull;
        return (size_t)(x ^ (x >> 32));
    }
};

// ReverseRead (deduplicate_sam.rs:272-286): the mate a written paired record is waiting for
std::string mate_key(const uint8_t *qname, size_t n, int32_t tid, int32_t pos)
{
    std::string s((const char *)qname, n);
    s.append((const char *)&tid, 4);
    s.append((const char *)&pos, 4);
    return s;
}

// UcSAMRead::get_umi_length (read.rs:65-75,87-94): first separator followed by a base
// (caseless [ATCGN]), length of that run.
size_t detect_umi_length(const uint8_t *q, size_t n, uint8_t sep)
{
    auto is_base = [](uint8_t ch) {
        switch (ch | 0x20) { case 'a': case 't': case 'c': case 'g': case 'n': return true; default: return false; }
    };
    for (size_t i = 0; i + 1 < n; i++)
        if (q[i] == sep && is_base(q[i + 1])) {
            size_t j = i + 1;
            while (j < n && is_base(q[j])) j++;
            return j - i - 1;
        }
    die("No UMI group found in pattern match");
}

// The filters of the read loop (deduplicate_sam.rs:95-129), shared by the one-pass staging and both
// passes of --two-pass.  Returns the read's state: 0 staged, 1 unmapped, 3 second mate (not counted),
// 4 mate unmapped, 5 filtered (--remove-unpaired / --remove-chimeric); 2 (error) is set by the caller.
uint8_t read_state(const Cli &args, const umi::bam::Record &r, uint8_t &is_unpaired, uint8_t &is_chimeric)
{
    is_unpaired = is_chimeric = 0;
    if (args.paired && r.is_paired() && r.is_last_in_template()) return 3; // :95-97
    if (r.is_unmapped()) return 1;                                         // :102-108
    if (args.paired && !args.passthrough) {                                // :110-129
        if (!r.is_paired()) {
            is_unpaired = 1;
            if (args.remove_unpaired) return 5;
        }
        if (r.is_paired() && r.is_mate_unmapped()) return 4;
        if (r.is_paired() && r.tid() != r.mtid()) {
            is_chimeric = 1;
            if (args.remove_chimeric) return 5;
        }
    }
    return 0;
}

// Alignment{strand, coord, ref} (:141-145) or, with --paired, PairedAlignment (:138, :547-553) of a
// staged read; equality on tid == equality on the reference name
AlignKey align_key(const umi::bam::Record &r, bool paired)
{
    return AlignKey{(uint64_t)r.unclipped_pos(), ((uint64_t)(uint32_t)r.tid() << 1) | (r.is_reverse() ? 1u : 0u),
                    paired ? (uint64_t)(int64_t)r.tlen() : 0};
}

// where a staged read's UMI starts in its name (read.rs:100), or the reference's message
const char *find_umi(const umi::bam::Record &r, uint8_t sep, size_t umi_length, size_t &at)
{
    const uint8_t *q = r.qname();
    const size_t qn = r.qname_len();
    const uint8_t *sp = (const uint8_t *)std::memchr(q, sep, qn);
    at = sp ? (size_t)(sp - q) + 1 : 0;
    if (!sp) return "failed to get the umi";
    if (umi_length == 0) return "Empty UMI sequence extracted";
    if (umi_length > UMI_MAX_WIDE_UMI_LEN) return "UMIs of more than 85 bases are not handled";
    if (at + umi_length > qn) return "UMI runs past the end of the read name";
    return nullptr;
}

// --umi-tag / --per-cell: the aux tags a staged read is looked up by.  Returns the bits of the ones it
// lacks (MISS_UMI, MISS_CELL: the read is dropped, not written, and counted); err: the message that ends
// the run (a malformed aux block, a tag that is not of type Z).
enum : uint8_t { MISS_UMI = 1, MISS_CELL = 2 };
struct ReadTags {
    const uint8_t *umi = nullptr; // --umi-tag: the value
    size_t umi_len = 0;
    std::string_view cell;        // --per-cell: the barcode, an opaque byte string
};
uint8_t read_tags(const Cli &args, const umi::bam::Record &r, ReadTags &t, std::string &err)
{
    auto look = [&](const std::string &tag, umi::bam::AuxField &f) -> bool {
        const umi::bam::AuxFind got = umi::bam::find_aux(r, tag.c_str(), &f);
        const std::string name((const char *)r.qname(), r.qname_len());
        if (got == umi::bam::AuxFind::malformed) err = "malformed aux block in read " + name;
        else if (got == umi::bam::AuxFind::found && f.type != 'Z')
            err = "tag " + tag + " of read " + name + " is of type " + std::string(1, f.type) + ", not Z";
        return got == umi::bam::AuxFind::found && err.empty();
    };
    uint8_t miss = 0;
    umi::bam::AuxField f;
    if (!args.umi_tag.empty()) {
        if (look(args.umi_tag, f)) {
            t.umi = f.value;
            t.umi_len = f.len;
        } else {
            miss |= MISS_UMI;
        }
        if (!err.empty()) return 0;
    }
    if (args.per_cell) {
        if (look(args.cell_tag, f)) t.cell = std::string_view((const char *)f.value, f.len);
        else miss |= MISS_CELL;
    }
    return miss;
}

// where the UMI of a read with all its tags starts, as an offset from its name: after --umi_sep in the
// name (find_umi), or the --umi-tag value, which must be umi_length bases; empty, or the message that
// ends the run
std::string umi_offset(const Cli &args, const umi::bam::Record &r, const ReadTags &t, size_t umi_length, size_t &at)
{
    if (args.umi_tag.empty()) {
        const char *err = find_umi(r, args.umi_sep, umi_length, at);
        return err ? err : "";
    }
    at = (size_t)(t.umi - r.qname());
    if (umi_length == 0) return "Empty UMI sequence extracted";
    if (umi_length > UMI_MAX_WIDE_UMI_LEN) return "UMIs of more than 85 bases are not handled";
    if (t.umi_len != umi_length)
        return "UMI tag " + args.umi_tag + " of read " + std::string((const char *)r.qname(), r.qname_len()) + " holds " +
               std::to_string(t.umi_len) + " bases, not " + std::to_string(umi_length);
    return "";
}

// the UMI length of the first staged read (src: :154-156): the name's UMI group, or the --umi-tag value's length
size_t detect_length(const Cli &args, const umi::bam::Record &r, const ReadTags &t)
{
    return args.umi_tag.empty() ? detect_umi_length(r.qname(), r.qname_len(), args.umi_sep) : t.umi_len;
}

// --umi-whitelist: the listed UMIs back to back; their length in umi_len.  One UMI per line, blank lines and
// lines that start with # skipped; anything a kit's list cannot be ends the run.
// (--cell-whitelist reads its list the same way: `list_name` and `item` are what the messages call them)
std::vector<uint8_t> read_whitelist(const std::string &path, size_t &umi_len, const std::string &list_name = "UMI whitelist",
                                    const std::string &item = "UMI", size_t max_len = UMI_MAX_WIDE_UMI_LEN)
{
    FILE *f = std::fopen(path.c_str(), "rb");
    if (!f) die("cannot open the " + list_name + " " + path);
    std::string text;
    char buf[1 << 16];
    for (size_t got; (got = std::fread(buf, 1, sizeof(buf), f)) > 0;) text.append(buf, got);
    std::fclose(f);
    std::vector<uint8_t> list;
    std::unordered_set<std::string> seen;
    umi_len = 0;
    size_t line_no = 0;
    for (size_t p = 0; p < text.size();) {
        size_t q = text.find('\n', p);
        if (q == std::string::npos) q = text.size();
        std::string line = text.substr(p, q - p);
        p = q + 1;
        line_no++;
        while (!line.empty() && (line.back() == '\r' || line.back() == ' ' || line.back() == '\t')) line.pop_back();
        if (line.empty() || line[0] == '#') continue;
        const std::string where = list_name + " " + path + ", line " + std::to_string(line_no) + ": ";
        if (line.size() > max_len) die(where + std::to_string(line.size()) + " bases, more than " + std::to_string(max_len));
        for (char ch : line)
            if (ch != 'A' && ch != 'C' && ch != 'G' && ch != 'T')
                die(where + "a character outside ACGT: " + std::to_string((unsigned)(uint8_t)ch));
        if (umi_len && line.size() != umi_len)
            die(where + std::to_string(line.size()) + " bases, the " + item + "s before it have " + std::to_string(umi_len));
        if (!seen.insert(line).second) die(where + "duplicate entry " + line);
        umi_len = line.size();
        list.insert(list.end(), line.begin(), line.end());
    }
    if (list.empty()) die("the " + list_name + " " + path + " holds no " + item);
    return list;
}

int bits_of(uint64_t v)
{
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// a second mate the paired writer may look for (:425-429)
bool mate_candidate(const umi::bam::Record &r)
{
    return !r.is_unmapped() && r.is_paired() && r.is_last_in_template() && !r.is_mate_unmapped();
}

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

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

// fastq mode with the staging on the device.  The checks of the host staging come in the same order and
// with the same messages: per record in file order its length (over 256, under -u), then its characters.
// A file with a length problem is an error either way: the reads before it are checked for characters
// on the host and the earlier problem is named, no GPU needed.  Otherwise the device checks the
// characters and reports the first bad read.
[[noreturn]] void run_fastq_gpu_stage(const Cli &args, int algo, int merge, HipLib &lib, const umi::bgzf::Bytes &text,
                                      const std::vector<umi::fastq::Record> &recs, std::future<umi_ctx *> &warm,
                                      const std::string &warm_error, double t_start, double t_read)
{
    const size_t n_reads = recs.size();
    size_t n_ok = n_reads; // reads before the first length problem
    std::string len_problem;
    for (size_t i = 0; i < n_reads && n_ok == n_reads; i++) {
        const umi::fastq::Record &r = recs[i];
        if (r.len > UMI_MAX_SEQ_LEN)
            len_problem = "FASTQ record " + std::to_string(i + 1) + ": " + std::to_string(r.len) + " bases, more than " +
                          std::to_string(UMI_MAX_SEQ_LEN);
        else if (r.len < args.umi_length)
            len_problem = "FASTQ record " + std::to_string(i + 1) + ": " + std::to_string(r.len) +
                          " bases, shorter than -u " + std::to_string(args.umi_length);
        if (!len_problem.empty()) n_ok = i;
    }
    if (!len_problem.empty()) {
        for (size_t i = 0; i < n_ok; i++)
            for (size_t b = 0; b < recs[i].len; b++) {
                const uint8_t c = text[recs[i].seq + b];
                if (c != 'A' && c != 'T' && c != 'C' && c != 'G' && c != 'N')
                    die("Unknown character in sequence: " + std::to_string((unsigned)c) + " (FASTQ record " +
                        std::to_string(i + 1) + ")"); // utils/mod.rs:77-79
            }
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
    umi_ctx *ctx = warm.get();
    if (!ctx) die(warm_error);
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

// ---- FASTQ mode (-m fastq).  The reference leaves it a TODO (src/main.rs:49-50); this build defines it
// after UMICollapse's fastq mode: the whole read sequence is the key.  One bucket per read length
// (first appearance), one entry per distinct sequence (freq, rep: the first read with --merge any, the
// highest average quality -- first on ties -- with avgqual), rank order inside, ONE umi_dedup_seqs call,
// survivors' rep reads written in file order (-u N trims N bases and quality characters from each).
// Staging on the device (--stage gpu, or auto): the inflated text goes up as it is, with every read's
// offsets and length; umi_stage_seqs_device leaves its output on the device for umi_dedup_seqs_device,
// and only what the writer needs comes back.  --stage host (and auto with --dump-staging or 2^30
// reads or more): the per-length hash maps below.
int run_fastq(const Cli &args, int algo, int merge, HipLib &lib)
{
    const double t_start = now_s();
    if (args.paired || args.remove_unpaired || args.remove_chimeric || args.keep_unmapped || args.two_pass)
        die("--paired, --remove-unpaired, --remove-chimeric, --keep-unmapped and --two-pass do not go with fastq mode");
    if (!args.umi_tag.empty() || args.cell_tag_given || args.per_cell)
        die("--umi-tag, --cell-tag and --per-cell do not go with fastq mode");
    if (args.stage != "auto" && args.stage != "gpu" && args.stage != "host") die("--stage wants gpu, host or auto");
    if (args.stage == "gpu" && !args.dump_staging.empty()) die("--stage gpu does not go with --dump-staging");
    if (args.devices.size() > 1) die("fastq mode runs on one GPU: --devices takes one id here");
    if (args.consensus && args.track_clusters) die("--consensus does not go with --tag (which writes every read as it is)");
    if (args.consensus && !args.dump_staging.empty()) die("--consensus does not go with --dump-staging (which stops before the GPU)");
    lib.want_consensus = args.consensus;
    if (merge == 2) die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data);
    // the GPU is woken while the file is read (as in BAM mode: a tiny staging call and a tiny dedup call
    // load the library's code objects)
    const bool want_gpu_stage = args.stage != "host" && args.dump_staging.empty();
    std::future<umi_ctx *> warm;
    std::string warm_error;
    if (want_gpu_stage)
        warm = std::async(std::launch::async, [&]() -> umi_ctx * {
            umi_ctx *c = nullptr;
            if (!lib.load()) {
                warm_error = lib.error;
                return nullptr;
            }
            if (lib.ctx_create_multi(args.devices.data(), 1, &c) != UMI_OK) {
                warm_error = lib.last_error();
                return nullptr;
            }
            const uint8_t txt[8] = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'A'};
            const uint64_t pos[2] = {0, 4};
            const uint32_t len[2] = {4, 4};
            uint64_t k[2], nm[2], rp[2], off[3], ne = 0, nbk = 0;
            int32_t fr[2], bl[2];
            int an = 0;
            uint8_t kept[2];
            umi_stats wst;
            if (lib.stage_seqs(c, txt, pos, pos, len, 2, 1, merge, k, nm, fr, rp, nullptr, off, bl, &ne, &nbk, &an) != UMI_OK ||
                lib.dedup_seqs(c, k, nullptr, 1, fr, off, bl, nbk, 1, 0.5f, UMI_ALGO_DIRECTIONAL, 0, kept, nullptr, &wst) != UMI_OK)
                warm_error = lib.last_error(); // (reported when the real call fails the same way)
            return c;
        });
    umi::bgzf::Bytes text = umi::fastq::read_all(args.input, args.num_threads);
    std::vector<umi::fastq::Record> recs;
    const std::string perr = umi::fastq::parse(text.data(), text.size(), recs);
    if (!perr.empty()) die(perr);
    const double t_read = now_s();
    const uint8_t *d = text.data();
    const size_t n_reads = recs.size();
    if (want_gpu_stage && n_reads < (1ull << 30))
        run_fastq_gpu_stage(args, algo, merge, lib, text, recs, warm, warm_error, t_start, t_read);
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
    std::vector<int32_t> bucket_of_len(UMI_MAX_SEQ_LEN + 1, -1);
    for (size_t i = 0; i < n_reads; i++) {
        const umi::fastq::Record &r = recs[i];
        if (r.len > UMI_MAX_SEQ_LEN)
            die("FASTQ record " + std::to_string(i + 1) + ": " + std::to_string(r.len) + " bases, more than " +
                std::to_string(UMI_MAX_SEQ_LEN));
        if (r.len < args.umi_length)
            die("FASTQ record " + std::to_string(i + 1) + ": " + std::to_string(r.len) + " bases, shorter than -u " +
                std::to_string(args.umi_length));
        for (size_t b = 0; b < r.len; b++) {
            const uint8_t c = d[r.seq + b];
            if (c != 'A' && c != 'T' && c != 'C' && c != 'G' && c != 'N')
                die("Unknown character in sequence: " + std::to_string((unsigned)c) + " (FASTQ record " +
                    std::to_string(i + 1) + ")"); // utils/mod.rs:77-79
        }
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
    size_t n = 0;
    int n_words = 1;
    for (const Bucket &bk : buckets) {
        n += bk.entries.size();
        n_words = std::max(n_words, (int)((3 * bk.len + 63) / 64));
    }
    const size_t nb = buckets.size();
    std::vector<uint64_t> keys(n * n_words + 1, 0), nmask(n * n_words + 1, 0), off(nb + 1, 0);
    std::vector<int32_t> freq(n + 1), blen(nb + 1);
    std::vector<uint32_t> rep(n + 1);
    bool any_n = false;
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
    const double t_stage = now_s();
    std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_stage - t_start);
    if (!args.dump_staging.empty()) { // test hook: staged hot-path input, no GPU touched
        FILE *f = std::fopen(args.dump_staging.c_str(), "wb");
        if (!f) die("cannot open " + args.dump_staging);
        const uint64_t hdr[4] = {n, nb, 0, (uint64_t)n_words};
        std::fwrite(hdr, 8, 4, f);
        std::fwrite(keys.data(), 8, n * n_words, f);
        std::fwrite(nmask.data(), 8, n * n_words, f);
        std::fwrite(freq.data(), 4, n, f);
        std::fwrite(rep.data(), 4, n, f);
        std::fwrite(off.data(), 8, nb + 1, f);
        std::fwrite(blen.data(), 4, nb, f);
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
        if (warm.valid()) { // (--stage auto with 2^30 reads or more: the context the start-up thread made)
            ctx = warm.get();
            if (!ctx) die(warm_error);
        } else {
            if (!lib.load()) die(lib.error);
            if (!lib.dedup_seqs) die("libumihip.so lacks umi_dedup_seqs");
            if (lib.ctx_create_multi(args.devices.data(), 1, &ctx) != UMI_OK) die(lib.last_error());
        }
        t_gpu0 = now_s();
        if (lib.dedup_seqs(ctx, keys.data(), any_n ? nmask.data() : nullptr, n_words, freq.data(), off.data(),
                           blen.data(), nb, args.k, args.percentage, algo, 0 /* adjacency.rs:56 */, kept.data(),
                           root.data(), &st) != UMI_OK)
            die(lib.last_error());
        t_gpu1 = now_s();
    }
    FastqResult res{n, nb, std::move(off), std::move(freq), std::move(rep), std::move(kept), std::move(root), {}, {}, {}, {}, {}, st,
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
            res.entry_of_read[i] = index[bucket_of_len[r.len]].at(std::string((const char *)d + r.seq, r.len));
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
                               res.freq.data(), res.kept.data(), res.root.data(), n, res.off.data(), blen.data(), nb,
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

void run_two_pass(const Cli &args, int algo, int merge, HipLib &lib, const std::function<umi_ctx *()> &get_ctx,
                  const std::function<void(const char *)> &lap, double t_start)
{
    struct stat sb;
    if (::stat(args.input.c_str(), &sb) != 0) die("Invalid input path: " + args.input);
    if (!S_ISREG(sb.st_mode)) die("--two-pass reads the input twice: -i must be a regular file (" + args.input + ")");
    if (args.stage != "auto" && args.stage != "gpu" && args.stage != "host") die("--stage wants gpu, host or auto");
    const unsigned T = std::max(1u, args.num_threads);
    auto reg_hash = [](const std::string &key) { return (uint64_t)std::hash<std::string>()(key); };

    // ---- pass 1: census
    umi::bgzf::ChunkWriter out(args.output, T, args.compress_level);
    size_t umi_length = args.umi_length;
    size_t total_read_count = 0, unmapped = 0, unpaired = 0, chimeric = 0;
    std::unordered_map<AlignKey, uint64_t, KeyHash> latest; // alignment key -> index of its last read
    std::unordered_map<int32_t, uint64_t> last_mate_on;     // --paired: reference -> index of its last candidate second mate
    std::unordered_map<uint64_t, uint32_t> reg_count;       // --paired: hash of the (qname, mate ref, mate pos) a staged
                                                            // first mate registers -> first mates not yet written or dropped
    bool bad_char = false;
    uint64_t n_records = 0;
    // --umi-tag / --per-cell: reads without their tags are dropped in both passes; a barcode's id is its rank
    // of first appearance, as in one pass, and the positions are counted apart from the (position, cell) groups
    const bool by_tags = !args.umi_tag.empty() || args.per_cell;
    size_t no_umi_tag = 0, no_cell = 0;
    std::unordered_map<std::string, uint64_t> cell_ids;
    std::unordered_set<AlignKey, KeyHash> positions;
    // the (alignment, cell) key of a staged read, false if it lacks a tag (census: counted; err ends the run)
    auto staged_key = [&](const umi::bam::Record &r, ReadTags &tg, AlignKey &key, bool census) -> bool {
        key = align_key(r, args.paired);
        if (!by_tags) return true;
        std::string err;
        const uint8_t miss = read_tags(args, r, tg, err);
        if (!err.empty()) die(err);
        if (miss) {
            if (census) {
                no_umi_tag += (miss & MISS_UMI) ? 1 : 0;
                no_cell += (miss & MISS_CELL) ? 1 : 0;
            }
            return false;
        }
        if (args.per_cell) {
            if (census) positions.insert(key);
            key.cell = census ? cell_ids.emplace(std::string(tg.cell), cell_ids.size()).first->second
                              : cell_ids.at(std::string(tg.cell));
        }
        return true;
    };
    {
        RecordStream rs(args.input, T);
        const umi::bgzf::Bytes h = rs.header();
        out.write(h.data(), h.size());
        umi::bam::Record r;
        UmiKey k, nm;
        for (uint64_t ri = 0; rs.next(r); ri++, n_records++) {
            uint8_t up, ch;
            const uint8_t state = read_state(args, r, up, ch);
            if (state != 3) total_read_count++;
            unpaired += up;
            chimeric += ch;
            if (args.paired && mate_candidate(r)) last_mate_on[r.tid()] = ri;
            if (state == 4) unmapped++;
            if (state == 1) {
                unmapped++;
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
    lap("census");
    const double t_census = now_s();

    const bool gpu_stage = args.stage != "host" && !args.paired && umi_length >= 1;
    if (args.stage == "gpu" && !gpu_stage) die("--stage gpu does not go with --paired, --tag or --dump-staging");
    const int n_words = umi_length ? (int)((3 * umi_length + 63) / 64) : 1;
    if (args.edit_distance && umi_length > UMI_MAX_UMI_LEN)
        die("--distance edit takes UMIs of at most 21 bases (this file's have " + std::to_string(umi_length) + ")");

    // ---- pass 2
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
    auto rec_at = [](const uint8_t *p) {
        return umi::bam::Record{p, p + 4 + (size_t)umi::bam::rd_i32(p)};
    };
    std::unordered_map<AlignKey, Bucket, KeyHash> open;
    std::vector<Bucket> window;
    std::unordered_map<uint64_t, Survivors> pending; // the reorder buffer
    std::unordered_map<int32_t, std::vector<Mate>> mates; // --paired: second mates by reference, file order
    std::unordered_set<std::string> waiting;
    uint64_t next_seq = 0, next_out = 0, n_windows = 0, done_upto = 0; // done_upto: records of pass 2 read so far
    bool pass2_done = false, have_ref = false, stalled = false;
    int32_t cur_ref = 0;
    uint64_t held_open = 0, held_window = 0, held_pending = 0, held_mates = 0, peak = 0;
    auto note_peak = [&]() { peak = std::max(peak, held_open + held_window + held_pending + held_mates); };
    size_t n_total = 0, nb_total = 0, max_umi = 0;
    uint64_t n_kept = 0, n_pairs = 0;
    double t_hot = 0.0;
    umi_ctx *ctx = nullptr;

    auto release = [&](const umi::bam::Record &r) { // a staged first mate written or dropped
        if (!args.paired || !r.is_paired()) return;
        auto it = reg_count.find(reg_hash(mate_key(r.qname(), r.qname_len(), r.mtid(), r.mpos())));
        if (it != reg_count.end() && --it->second == 0) reg_count.erase(it);
    };
    // UcWriter::write_reversed (:382-459) over the held second mates of one reference (or all of them, at
    // the end) in file order; a mate no staged first mate can still register is let go
    auto flush_mates = [&](int32_t tid, bool all) {
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
    };
    // write the deduplicated positions that are next in first-appearance order
    auto pump = [&]() {
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
    };
    // one batched library call for the closed positions of the window, in first-appearance order
    auto run_window = [&]() {
        if (window.empty()) return;
        std::sort(window.begin(), window.end(), [](const Bucket &a, const Bucket &b) { return a.seq < b.seq; });
        const size_t nb = window.size();
        std::vector<uint64_t> read_base(nb + 1, 0);
        for (size_t b = 0; b < nb; b++) read_base[b + 1] = read_base[b] + window[b].reads.size();
        const size_t nr = read_base[nb];
        std::vector<uint64_t, umi::bgzf::default_init_allocator<uint64_t>> keys(nr * n_words), nmask(nr * n_words),
            off(nr + 1), rep(nr);
        std::vector<int32_t, umi::bgzf::default_init_allocator<int32_t>> freq(nr);
        auto umi_of = [&](const Bucket &bk, const ReadRef &rr) { return bk.bytes.data() + rr.off + 4 + 32 + rr.umi_at; };
        uint64_t ne = 0, nbk = 0;
        if (!ctx) ctx = get_ctx();
        const double t0 = now_s();
        if (gpu_stage) {
            // (the window's position rank is the alignment key: the reads go in position by position, file order inside)
            std::vector<uint64_t, umi::bgzf::default_init_allocator<uint64_t>> akey(nr);
            umi::bgzf::Bytes umis(nr * umi_length);
            std::vector<int32_t, umi::bgzf::default_init_allocator<int32_t>> sc(nr);
            for (size_t b = 0; b < nb; b++)
                for (size_t j = 0; j < window[b].reads.size(); j++) {
                    const size_t g = read_base[b] + j;
                    akey[g] = b;
                    std::memcpy(&umis[g * umi_length], umi_of(window[b], window[b].reads[j]), umi_length);
                    sc[g] = window[b].reads[j].score;
                }
            int bits = 1;
            while (bits < 64 && (nb >> bits)) bits++;
            if (lib.stage_reads(ctx, akey.data(), bits, umis.data(), sc.data(), nr, (int)umi_length, n_words, merge != 0 ? 1 : 0,
                                keys.data(), nmask.data(), freq.data(), rep.data(), off.data(), &ne, &nbk) != UMI_OK)
                die(lib.last_error());
            if (nbk != nb) die("device staging returned " + std::to_string(nbk) + " positions for " + std::to_string(nb));
        } else {
            // deduplicate_sam.rs:148-176 per position, then the stable freq-descending rank order
            std::unordered_map<UmiKey, uint32_t, UmiKeyHash> idx;
            std::vector<Entry> ents;
            std::vector<uint32_t> order;
            off[0] = 0;
            for (size_t b = 0; b < nb; b++) {
                const Bucket &bk = window[b];
                idx.clear();
                ents.clear();
                for (uint32_t j = 0; j < bk.reads.size(); j++) {
                    const ReadRef &rr = bk.reads[j];
                    UmiKey k, nm;
                    encode_umi(umi_of(bk, rr), umi_length, &k, &nm); // (checked by the census)
                    auto e = idx.find(k);
                    if (e == idx.end()) {
                        idx.emplace(k, (uint32_t)ents.size());
                        ents.push_back({k, nm, 1, rr.score, j, (uint32_t)b});
                    } else {
                        Entry &en = ents[e->second];
                        en.freq += 1;
                        if (merge != 0 && !(en.score >= rr.score)) { en.rep = j; en.score = rr.score; } // merge/mod.rs:21,35,49
                    }
                }
                order.resize(ents.size());
                for (uint32_t j = 0; j < order.size(); j++) order[j] = j;
                std::stable_sort(order.begin(), order.end(), [&](uint32_t x, uint32_t y) { return ents[y].freq < ents[x].freq; });
                for (uint32_t j : order) {
                    const Entry &en = ents[j];
                    for (int q = 0; q < n_words; q++) {
                        keys[ne * n_words + q] = en.key.w[q];
                        nmask[ne * n_words + q] = en.nmask.w[q];
                    }
                    freq[ne] = en.freq;
                    rep[ne] = read_base[b] + en.rep;
                    ne++;
                }
                off[b + 1] = ne;
            }
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
        n_total += ne;
        nb_total += nb;
        n_kept += st.n_kept;
        n_pairs += st.n_pairs;
        std::vector<uint8_t> survivor;
        for (size_t b = 0; b < nb; b++) {
            Bucket &bk = window[b];
            max_umi = std::max<size_t>(max_umi, off[b + 1] - off[b]);
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
    };

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
    lap("pass-2");
    const double t_pass2 = now_s();
    out.close();
    lap("write");
    const double t_end = now_s();

    std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_census - t_start);
    std::fprintf(stderr, "Number of input reads: %zu\n", total_read_count);
    std::fprintf(stderr, "Number of removed unmapped reads: %zu\n", unmapped);
    if (args.paired) {
        std::fprintf(stderr, "Number of unpaired reads: %zu\n", unpaired);
        std::fprintf(stderr, "Number of chimeric reads: %zu\n", chimeric);
    }
    if (!args.umi_tag.empty()) std::fprintf(stderr, "Number of reads without a UMI tag: %zu\n", no_umi_tag);
    if (args.per_cell) std::fprintf(stderr, "Number of reads without a cell barcode: %zu\n", no_cell);
    std::fprintf(stderr, "Number of unique alignment positions: %zu\n", args.per_cell ? positions.size() : nb_total);
    if (args.per_cell) std::fprintf(stderr, "Number of (position, cell) groups: %zu\n", nb_total);
    std::fprintf(stderr, "Number of UMIs: %zu\n", n_total);
    std::fprintf(stderr, "Average number of UMIs per alignment position: %g\n", nb_total ? (double)n_total / (double)nb_total : 0.0);
    std::fprintf(stderr, "Max number of UMIs over all alignment positions: %zu\n", max_umi);
    std::fprintf(stderr, "Number of reads after deduplicating: %llu\n", (unsigned long long)n_kept);
    if (args.edit_distance) std::fprintf(stderr, "UMI distance: edit\n");
    std::fprintf(stderr, "two-pass: %llu windows, at most %llu reads held\n", (unsigned long long)n_windows,
                 (unsigned long long)peak);
    std::fprintf(stderr,
                 "phases: census %.3f s, pass 2 (staging %s) %.3f s, hot path (H2D+GPU+D2H) %.3f s [%llu pairs], write %.3f s\n",
                 t_census - t_start, gpu_stage ? "gpu" : "host", t_pass2 - t_census, t_hot, (unsigned long long)n_pairs,
                 t_end - t_pass2);
    std::fprintf(stderr, "UMI collapsing finished in %.3f seconds\n", t_end - t_start);
}

} // namespace

int main(int argc, char **argv)
{
    const double t_main_realtime = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    Cli args = parse(argc, argv);
    const double t_start = now_s();
    if (args.merge.empty()) args.merge = args.mode == "fastq" ? "avgqual" : "mapqual"; // main.rs:33-39
    // --call-consensus: everything about it that can be refused is, before the GPU is woken
    if (args.call_consensus_min_given && !args.call_consensus) die("--call-consensus-min-reads goes with --call-consensus only");
    if (args.call_consensus) {
        if (args.mode == "fastq") die("--call-consensus is defined in bam/sam mode only (fastq mode has --consensus)");
        if (args.track_clusters) die("--call-consensus does not go with --tag (which writes every read as it is)");
        if (args.two_pass) die("--call-consensus does not go with --two-pass (a cluster's reads are not held there)");
        if (args.paired) die("--call-consensus does not go with --paired");
        if (!args.dump_staging.empty() || args.passthrough) die("--call-consensus does not go with --dump-staging or --passthrough");
    }
    if (args.track_clusters && args.two_pass) die("Cannot track clusters with the two pass algorithm!");
    if (args.paired && args.keep_unmapped) die("Cannot keep unmapped reads with paired-end reads!");
    if (args.consensus_min_given && !args.consensus) die("--consensus-min-reads goes with --consensus only");
    if (args.consensus && args.mode != "fastq") die("--consensus is defined in fastq mode only (-m fastq)");
    if (args.umi_whitelist.empty() && (args.wl_max_given || args.wl_min_given || !args.whitelist_metrics.empty()))
        die("--whitelist-max-mismatches, --whitelist-min-distance and --whitelist-metrics go with --umi-whitelist only");
    if (args.mode != "bam" && args.mode != "sam" && args.mode != "fastq") return 0; // main.rs:49-95: nothing happens
    // --distance edit: everything about it that can be refused is, before the GPU is woken
    if (args.edit_distance) {
        if (args.mode == "fastq") die("--distance edit is defined in bam/sam mode only (whole reads are the key in fastq mode)");
        if (args.devices.size() > 1) die("--distance edit runs on one GPU: --devices takes one id with it");
        if (args.umi_length > UMI_MAX_UMI_LEN) die("--distance edit takes UMIs of at most 21 bases (-u " + std::to_string(args.umi_length) + ")");
    }
    // --umi-whitelist: everything about it that can be refused is, before the GPU is woken
    std::vector<uint8_t> whitelist;
    if (!args.umi_whitelist.empty()) {
        if (args.mode == "fastq") die("--umi-whitelist does not go with fastq mode (whole reads are the key there)");
        if (args.two_pass) die("--umi-whitelist does not go with --two-pass (its census would need the correction too)");
        if (!args.dump_staging.empty() || args.passthrough) die("--umi-whitelist does not go with --dump-staging or --passthrough");
        size_t wl_len = 0;
        whitelist = read_whitelist(args.umi_whitelist, wl_len);
        if (args.umi_length != 0 && args.umi_length != wl_len)
            die("-u " + std::to_string(args.umi_length) + " does not go with a whitelist of UMIs of " + std::to_string(wl_len) +
                " bases");
        if (args.edit_distance && wl_len > UMI_MAX_UMI_LEN)
            die("--distance edit takes UMIs of at most 21 bases (the whitelist's have " + std::to_string(wl_len) + ")");
        args.umi_length = wl_len; // (a read whose UMI is of another length ends the run, as with -u)
    }
    // --cell-whitelist: likewise
    if (args.cell_whitelist.empty() && (args.cell_wl_max_given || !args.cell_whitelist_metrics.empty()))
        die("--cell-whitelist-max-mismatches and --cell-whitelist-metrics go with --cell-whitelist only");
    std::vector<uint8_t> cell_list;
    size_t cell_len = 0;
    if (!args.cell_whitelist.empty()) {
        if (args.mode == "fastq") die("--cell-whitelist does not go with fastq mode (there are no tags there)");
        if (!args.per_cell) die("--cell-whitelist goes with --per-cell only");
        if (args.two_pass) die("--cell-whitelist does not go with --two-pass (its census would need the correction too)");
        if (!args.dump_staging.empty() || args.passthrough) die("--cell-whitelist does not go with --dump-staging or --passthrough");
        cell_list = read_whitelist(args.cell_whitelist, cell_len, "cell barcode whitelist", "barcode", 32);
    }
    if (args.track_clusters && args.paired) die("--tag with --paired is not implemented (the reference never reaches its tagging pass)");
    int algo, merge;
    if (args.algo == "dir") algo = UMI_ALGO_DIRECTIONAL;
    else if (args.algo == "adj") algo = UMI_ALGO_ADJACENCY;
    else die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data); // main.rs:86-91
    if (args.merge == "any") merge = 0;
    else if (args.merge == "avgqual") merge = 1;
    else if (args.merge == "mapqual") merge = 2;
    else die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data);
    if (args.mode == "fastq") { // (this build's definition, see run_fastq)
        HipLib fq_lib;
        try {
            return run_fastq(args, algo, merge, fq_lib);
        } catch (const std::exception &e) {
            die(e.what());
        }
    }

    // The GPU is woken while the file is read: context creation and the first launch of the
    // library's kernels (their code objects are loaded then) take ~0.1 s of a process that lives
    // half a second, none of it on the device.  A tiny staging call and a tiny batch go through;
    // whoever needs the context first waits for this thread.
    HipLib lib;
    lib.want_correct = !whitelist.empty();
    lib.want_barcodes = !cell_list.empty();
    lib.want_consensus_bam = args.call_consensus;
    lib.want_edit = args.edit_distance;
    std::future<umi_ctx *> warm;
    std::string warm_error;
    if (!args.passthrough && args.dump_staging.empty())
        warm = std::async(std::launch::async, [&]() -> umi_ctx * {
            umi_ctx *c = nullptr;
            if (!lib.load()) {
                warm_error = lib.error;
                return nullptr;
            }
            if (lib.ctx_create_multi(args.devices.data(), (int)args.devices.size(), &c) != UMI_OK) {
                warm_error = lib.last_error();
                return nullptr;
            }
            const uint64_t akey[2] = {0, 0};
            const uint8_t umis[8] = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'A'};
            uint64_t k[2], nm[2], rp[2], off[3], ne = 0, nbk = 0;
            int32_t fr[2];
            uint8_t kept[2];
            umi_stats wst;
            if (lib.stage_reads(c, akey, 1, umis, nullptr, 2, 4, 1, 0, k, nm, fr, rp, off, &ne, &nbk) != UMI_OK ||
                lib.dedup_batch(c, k, nullptr, 1, fr, off, nbk, 4, 1, 0.5f, UMI_ALGO_DIRECTIONAL, 0, kept, nullptr, &wst) != UMI_OK)
                warm_error = lib.last_error(); // (reported when the real call fails the same way)
            return c;
        });

    // finer split of the program's time, printed with UMICOLLAPSE_CLOCK (tools/e2e_probe.py)
    std::vector<std::pair<const char *, double>> laps;
    double t_lap = now_s();
    auto lap = [&](const char *what) {
        const double t = now_s();
        laps.emplace_back(what, t - t_lap);
        t_lap = t;
    };
    auto leave = [&]() {
        if (warm.valid()) warm.wait(); // (a file without staged reads: the start-up thread may still be at it)
        if (std::getenv("UMICOLLAPSE_CLOCK")) { // (for tools/e2e_probe.py: what lies before main and after _Exit)
            std::fprintf(stderr, "laps:");
            for (const auto &l : laps) std::fprintf(stderr, " %s %.3f", l.first, l.second);
            std::fprintf(stderr, "\nclock: main at %.6f, exit at %.6f (realtime)\n", t_main_realtime,
                         std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count());
        }
        std::fflush(nullptr);
        std::_Exit(0); // the output file is closed; device memory and the runtime go with the process
    };
    if (args.two_pass && !args.passthrough && args.dump_staging.empty()) { // (those two keep the one-pass behaviour)
        try {
            run_two_pass(args, algo, merge, lib, [&]() -> umi_ctx * {
                umi_ctx *c = warm.get();
                if (!c) die(warm_error);
                return c;
            }, lap, t_start);
        } catch (const std::exception &e) {
            die(e.what());
        }
        leave();
    }
    try {
        // ---- read: BGZF inflate (threaded) + BAM parse
        umi::bam::File in;
        // (the compressed bytes are not given back before the process ends: unmapping 0.1 GB takes 6 ms)
        static umi::bgzf::Bytes raw;
        raw = umi::bgzf::read_file(args.input, args.num_threads);
        lap("read");
        {
            umi::bgzf::Inflater inflater(raw, args.num_threads); // (the parse walks behind the inflate threads)
            in.data.swap(inflater.out);                          // (same storage: the threads write through their pointer)
            in.parse_behind([&](size_t upto) { inflater.wait(upto); });
            inflater.finish();
        }
        lap("inflate+parse");
        const double t_read = now_s();

        // ---- staging: deduplicate_sam.rs:93-177, in three passes so that --num-threads helps:
        //  A (parallel over records)  alignment key, UMI key, merge score of every read
        //  B (parallel over shards of the alignment-key hash; every shard walks the reads in
        //     file order)              per-bucket UMI maps with the reference's merge rule
        //  C (sequential)             buckets in order of first appearance, entries in rank order
        const uint32_t n_rec = (uint32_t)in.records.size();
        const unsigned T = std::max(1u, args.num_threads);
        size_t umi_length = args.umi_length;
        // the filters of the read loop (:95-129); returns ReadInfo::state
        auto classify = [&](const umi::bam::Record &r, uint8_t &is_unpaired, uint8_t &is_chimeric) -> uint8_t {
            return read_state(args, r, is_unpaired, is_chimeric);
        };
        if (umi_length == 0 && !args.passthrough) // autodetect on the first staged read (:154-156)
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                uint8_t u, c;
                if (classify(in.records[ri], u, c) == 0) {
                    ReadTags tg;
                    std::string err;
                    const uint8_t miss = read_tags(args, in.records[ri], tg, err); // (a read without its tags is not staged)
                    if (!err.empty()) die(err);
                    if (miss) continue;
                    umi_length = detect_length(args, in.records[ri], tg);
                    break;
                }
            }
        // (where the reads are merged per (position, UMI): on the GPU unless something needs the host's
        // per-read bookkeeping -- decided here because the per-read pass only encodes UMIs for the host path)
        if (args.stage != "auto" && args.stage != "gpu" && args.stage != "host") die("--stage wants gpu, host or auto");
        const bool need_clusters = args.track_clusters || args.call_consensus; // every read's entry, every entry's root
        bool gpu_stage = args.stage != "host" && !args.passthrough && !args.paired && !need_clusters &&
                         args.dump_staging.empty() && umi_length >= 1;
        if (args.stage == "gpu" && !gpu_stage)
            die("--stage gpu does not go with --paired, --tag, --call-consensus or --dump-staging");
        struct ReadInfo {
            uint64_t coord, ref_strand, tlen;
            int32_t score;
            uint8_t state; // 0 staged, 1 unmapped, 2 error, 3 second mate (not counted),
                           // 4 mate unmapped, 5 filtered (--remove-unpaired / --remove-chimeric),
                           // 6 dropped: it lacks a tag of --umi-tag / --per-cell (`missing` says which)
                           // 7 dropped: its UMI matches no listed one (--umi-whitelist)
                           // 8 dropped: its cell barcode is unlisted or ambiguous (--cell-whitelist)
            uint8_t unpaired, chimeric, missing;
            uint32_t umi_at; // offset of the UMI from the read name (a --umi-tag value lies behind it)
            uint32_t cell;   // --per-cell: the barcode's id, the thread's own during the per-read pass
        };
        std::vector<ReadInfo> info(n_rec);
        umi::bgzf::Bytes wl_umis;      // --umi-whitelist: per record, the listed UMI a staged read was snapped to
        std::vector<UmiKey> rkey, rnm; // per read: its UMI key and N mask (host staging only: the device encodes its own)
        auto encode_all = [&]() {       // utils/mod.rs:63-83 for every staged read; the first bad character ends the run
            rkey.resize(n_rec);
            rnm.resize(n_rec);
            std::vector<uint32_t> bad(T, UINT32_MAX);
            const uint32_t per = (n_rec + T - 1) / T;
            umi::bgzf::parallel_for(T, T, [&](size_t t) {
                for (uint32_t ri = (uint32_t)t * per; ri < std::min(n_rec, ((uint32_t)t + 1) * per); ri++)
                    if (info[ri].state == 0 && !args.passthrough &&
                        !encode_umi(wl_umis.empty() ? in.records[ri].qname() + info[ri].umi_at : &wl_umis[(size_t)ri * umi_length],
                                    umi_length, &rkey[ri], &rnm[ri]) &&
                        bad[t] == UINT32_MAX)
                        bad[t] = ri;
            });
            for (unsigned t = 0; t < T; t++)
                if (bad[t] != UINT32_MAX) die("Unknown character in UMI sequence");
        };
        // GPU staging: what the device wants of a read -- alignment key, UMI text, score -- is written by the
        // per-read pass itself, at the read's own index (closed up afterwards if some reads are not staged)
        using U64s = std::vector<uint64_t, umi::bgzf::default_init_allocator<uint64_t>>;
        using I32s = std::vector<int32_t, umi::bgzf::default_init_allocator<int32_t>>;
        U64s akey, rep64;
        umi::bgzf::Bytes umis;
        I32s sc;
        std::vector<uint8_t> fits(T, 1);
        std::vector<int64_t> c_min(T, INT64_MAX), c_max(T, INT64_MIN); // coordinates and (ref, strand) codes seen, per thread
        std::vector<uint64_t> rs_max(T, 0);
        if (gpu_stage) {
            akey.resize(n_rec);
            umis.resize((size_t)n_rec * umi_length);
            sc.resize(n_rec);
        }
        std::vector<std::string> errors(T);
        std::vector<uint32_t> first_error(T, UINT32_MAX);
        const uint32_t chunk = (n_rec + T - 1) / T;
        // --per-cell: every thread numbers the barcodes of its reads in order of appearance; the numbers are
        // made global (first appearance in the file) below.  A few thousand to 10^5 barcodes: the tables stay
        // in cache.
        umi::bgzf::Bytes cell_raw; // --cell-whitelist: per record, a staged read's barcode as the tag has it
        if (!cell_list.empty()) cell_raw.resize((size_t)n_rec * cell_len);
        std::vector<std::unordered_map<std::string_view, uint32_t>> cell_ids(args.per_cell ? T : 0);
        std::vector<std::vector<std::string_view>> cell_seen(args.per_cell ? T : 0);
        U64s gkey; // GPU staging with --per-cell: every read's cell id, the group key
        if (gpu_stage && args.per_cell) gkey.resize(n_rec);
        umi::bgzf::parallel_for(T, T, [&](size_t t) {
            const uint32_t lo = (uint32_t)t * chunk, hi = std::min(n_rec, lo + chunk);
            // (the thread's extremes in locals: sixteen threads updating neighbours of one cache line
            // per read made this pass 0.27 s instead of 0.02)
            int64_t my_c_min = INT64_MAX, my_c_max = INT64_MIN;
            uint64_t my_rs_max = 0;
            for (uint32_t ri = lo; ri < hi; ri++) {
                const umi::bam::Record &r = in.records[ri];
                ReadInfo &ii = info[ri];
                ii.tlen = 0;
                ii.missing = 0;
                ii.cell = 0;
                ii.state = classify(r, ii.unpaired, ii.chimeric);
                if (ii.state != 0 || args.passthrough) continue;
                const AlignKey ak = align_key(r, args.paired);
                ii.coord = ak.coord;
                ii.ref_strand = ak.ref_strand;
                ii.tlen = ak.tlen;
                const uint8_t *q = r.qname();
                size_t at = 0;
                std::string err;
                ReadTags tg;
                if (!args.umi_tag.empty() || args.per_cell) {
                    ii.missing = read_tags(args, r, tg, err);
                    if (ii.missing && err.empty()) {
                        ii.state = 6;
                        continue;
                    }
                }
                if (err.empty()) err = umi_offset(args, r, tg, umi_length, at);
                if (!err.empty()) {
                    ii.state = 2;
                    if (first_error[t] == UINT32_MAX) { first_error[t] = ri; errors[t] = err; }
                    continue;
                }
                if (!cell_list.empty()) { // (numbered after the correction, below)
                    bool acgtn = tg.cell.size() == cell_len;
                    for (const char ch : tg.cell) acgtn = acgtn && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'N');
                    if (!acgtn) {
                        ii.state = 2;
                        if (first_error[t] == UINT32_MAX) {
                            first_error[t] = ri;
                            const std::string name((const char *)r.qname(), r.qname_len());
                            errors[t] = tg.cell.size() != cell_len
                                            ? "cell barcode tag " + args.cell_tag + " of read " + name + " holds " +
                                                  std::to_string(tg.cell.size()) + " bases, not " + std::to_string(cell_len)
                                            : "Unknown character in cell barcode tag " + args.cell_tag + " of read " + name;
                        }
                        continue;
                    }
                    std::memcpy(&cell_raw[(size_t)ri * cell_len], tg.cell.data(), cell_len);
                } else if (args.per_cell) {
                    const auto id = cell_ids[t].emplace(tg.cell, (uint32_t)cell_seen[t].size());
                    if (id.second) cell_seen[t].push_back(tg.cell);
                    ii.cell = id.first->second;
                }
                ii.score = merge == 2 ? (int32_t)r.mapq() : r.avg_qual();
                ii.umi_at = (uint32_t)at;
                if (gpu_stage) {
                    // Alignment{strand, coord, ref} in 64 bits: ref id (31) | strand (1) | coordinate (32)
                    const int64_t c = (int64_t)ii.coord;
                    if (c < INT32_MIN || c > INT32_MAX) fits[t] = 0;
                    my_c_min = std::min(my_c_min, c);
                    my_c_max = std::max(my_c_max, c);
                    my_rs_max = std::max(my_rs_max, ii.ref_strand);
                    akey[ri] = (ii.ref_strand << 32) | (uint64_t)(uint32_t)(int32_t)c; // (packed tighter below)
                    std::memcpy(&umis[(size_t)ri * umi_length], q + at, umi_length);
                    sc[ri] = ii.score;
                }
            }
            c_min[t] = my_c_min;
            c_max[t] = my_c_max;
            rs_max[t] = my_rs_max;
        });
        for (unsigned t = 0; t < T; t++) // the reference panics at the first offending read
            if (first_error[t] != UINT32_MAX) die(errors[t]);
        size_t n_cells = 0;
        umi_ctx *ctx = nullptr;
        double t_init = 0.0;
        auto need_ctx = [&]() { // (t_init: what of the GPU's start-up was left to wait for)
            if (ctx) return;
            const double t0 = now_s();
            if (warm.valid()) {
                ctx = warm.get();
                if (!ctx) die(warm_error);
            } else {
                if (!lib.load()) die(lib.error);
                if (lib.ctx_create_multi(args.devices.data(), (int)args.devices.size(), &ctx) != UMI_OK) die(lib.last_error());
            }
            t_init += now_s() - t0;
        };
        // --cell-whitelist: the barcodes of the reads that would be staged, looked up in the list's index in one
        // call; a read whose barcode is unlisted or ambiguous is dropped like one without the tag, and the
        // others are numbered by their corrected barcode (rank of first appearance in the file)
        uint64_t cb_counts[4] = {0, 0, 0, 0};
        if (!cell_list.empty()) {
            std::vector<uint32_t> cand;
            for (uint32_t ri = 0; ri < n_rec; ri++)
                if (info[ri].state == 0) cand.push_back(ri);
            const size_t nc = cand.size(), L = cell_len, n_wl = cell_list.size() / L;
            umi::bgzf::Bytes raw(nc * L);
            const size_t per = (nc + T - 1) / T;
            umi::bgzf::parallel_for(T, T, [&](size_t t) {
                for (size_t j = t * per; j < std::min(nc, (t + 1) * per); j++)
                    std::memcpy(&raw[j * L], &cell_raw[(size_t)cand[j] * L], L);
            });
            std::vector<int32_t> cb_match(nc);
            std::vector<uint8_t> cb_status(nc);
            if (nc) {
                need_ctx();
                if (lib.correct_barcodes(ctx, raw.data(), nc, (int)L, cell_list.data(), (uint32_t)n_wl, args.cell_wl_max_mismatches,
                                         cb_match.data(), cb_status.data(), cb_counts) != UMI_OK)
                    die(lib.last_error());
            }
            std::vector<uint32_t> id_of(n_wl, UINT32_MAX); // listed barcode -> cell id
            uint32_t next_id = 0;
            for (size_t j = 0; j < nc; j++) {
                ReadInfo &ii = info[cand[j]];
                if (cb_match[j] < 0) {
                    ii.state = 8;
                    continue;
                }
                uint32_t &id = id_of[(size_t)cb_match[j]];
                if (id == UINT32_MAX) id = next_id++;
                ii.cell = id;
                if (gpu_stage) gkey[cand[j]] = id;
            }
            n_cells = next_id;
            if (!args.cell_whitelist_metrics.empty()) { // per listed barcode that took a read, in list order
                std::vector<uint64_t> exact(n_wl, 0), corrected(n_wl, 0);
                for (size_t j = 0; j < nc; j++)
                    if (cb_match[j] >= 0) (cb_status[j] == 0 ? exact : corrected)[(size_t)cb_match[j]]++;
                FILE *f = std::fopen(args.cell_whitelist_metrics.c_str(), "wb");
                if (!f) die("cannot open " + args.cell_whitelist_metrics);
                std::fprintf(f, "barcode\treads\texact\tcorrected\n");
                for (size_t w = 0; w < n_wl; w++)
                    if (exact[w] + corrected[w])
                        std::fprintf(f, "%.*s\t%llu\t%llu\t%llu\n", (int)L, (const char *)&cell_list[w * L],
                                     (unsigned long long)(exact[w] + corrected[w]), (unsigned long long)exact[w],
                                     (unsigned long long)corrected[w]);
                if (std::fclose(f) != 0) die("cannot write " + args.cell_whitelist_metrics);
            }
            lap("cell whitelist");
        }
        if (args.per_cell && cell_list.empty()) { // the threads' barcode numbers -> ranks of first appearance in the file
            std::unordered_map<std::string_view, uint32_t> global;
            std::vector<std::vector<uint32_t>> to_global(T);
            for (unsigned t = 0; t < T; t++)
                for (const std::string_view &bc : cell_seen[t])
                    to_global[t].push_back(global.emplace(bc, (uint32_t)global.size()).first->second);
            n_cells = global.size();
            umi::bgzf::parallel_for(T, T, [&](size_t t) {
                const uint32_t lo = (uint32_t)t * chunk, hi = std::min(n_rec, lo + chunk);
                for (uint32_t ri = lo; ri < hi; ri++)
                    if (info[ri].state == 0) {
                        info[ri].cell = to_global[t][info[ri].cell];
                        if (gpu_stage) gkey[ri] = info[ri].cell;
                    }
            });
        }
        // --umi-whitelist: the UMIs of the reads that would be staged, snapped to the list in one call; a read
        // that matches no listed UMI is dropped like one without its tag, the others go on with the listed
        // UMI's bytes in place of their own (either staging below sees only those)
        uint64_t wl_counts[3] = {0, 0, 0};
        std::vector<int32_t> wl_match;    // per staged read, in file order
        if (!whitelist.empty()) {
            std::vector<uint32_t> cand;
            for (uint32_t ri = 0; ri < n_rec; ri++)
                if (info[ri].state == 0) cand.push_back(ri);
            const size_t nc = cand.size(), L = umi_length;
            umi::bgzf::Bytes raw_umis(nc * L), fixed(nc * L);
            const size_t per = (nc + T - 1) / T;
            umi::bgzf::parallel_for(T, T, [&](size_t t) {
                for (size_t j = t * per; j < std::min(nc, (t + 1) * per); j++)
                    std::memcpy(&raw_umis[j * L], in.records[cand[j]].qname() + info[cand[j]].umi_at, L);
            });
            wl_match.resize(nc);
            std::vector<uint8_t> wl_best(args.whitelist_metrics.empty() ? 0 : nc);
            if (nc) {
                need_ctx();
                if (lib.correct_umis(ctx, raw_umis.data(), nc, (int)L, whitelist.data(), (uint32_t)(whitelist.size() / L),
                                     args.wl_max_mismatches, args.wl_min_distance, fixed.data(), wl_match.data(),
                                     wl_best.empty() ? nullptr : wl_best.data(), nullptr, wl_counts) != UMI_OK)
                    die(lib.last_error());
                wl_umis.resize((size_t)n_rec * L);
                umi::bgzf::parallel_for(T, T, [&](size_t t) {
                    for (size_t j = t * per; j < std::min(nc, (t + 1) * per); j++) {
                        const uint32_t ri = cand[j];
                        if (wl_match[j] < 0) {
                            info[ri].state = 7;
                            continue;
                        }
                        std::memcpy(&wl_umis[(size_t)ri * L], &fixed[j * L], L);
                        if (gpu_stage) std::memcpy(&umis[(size_t)ri * L], &fixed[j * L], L);
                    }
                });
            }
            if (!args.whitelist_metrics.empty()) { // per listed UMI, in list order: the reads it took, exact and corrected
                const size_t n_wl = whitelist.size() / L;
                std::vector<uint64_t> exact(n_wl, 0), corrected(n_wl, 0);
                for (size_t j = 0; j < nc; j++)
                    if (wl_match[j] >= 0) (wl_best[j] == 0 ? exact : corrected)[(size_t)wl_match[j]]++;
                FILE *f = std::fopen(args.whitelist_metrics.c_str(), "wb");
                if (!f) die("cannot open " + args.whitelist_metrics);
                std::fprintf(f, "umi\treads\texact\tcorrected\n");
                for (size_t w = 0; w < n_wl; w++)
                    std::fprintf(f, "%.*s\t%llu\t%llu\t%llu\n", (int)L, (const char *)&whitelist[w * L],
                                 (unsigned long long)(exact[w] + corrected[w]), (unsigned long long)exact[w],
                                 (unsigned long long)corrected[w]);
                if (std::fclose(f) != 0) die("cannot write " + args.whitelist_metrics);
            }
            lap("whitelist");
        }
        lap("per-read");
        if (!gpu_stage && !args.passthrough) encode_all();

        size_t total_read_count = 0, unmapped = 0, unpaired = 0, chimeric = 0, no_umi_tag = 0, no_cell = 0;
        std::vector<uint32_t> out_records; // records written before dedup (--keep-unmapped, :104-106)
        for (uint32_t ri = 0; ri < n_rec; ri++) {
            if (info[ri].state != 3) total_read_count++; // :99
            if (info[ri].state == 6) {
                no_umi_tag += (info[ri].missing & MISS_UMI) ? 1 : 0;
                no_cell += (info[ri].missing & MISS_CELL) ? 1 : 0;
            }
            unpaired += info[ri].unpaired;
            chimeric += info[ri].chimeric;
            if (info[ri].state == 4) unmapped++; // :118-121
            if (info[ri].state == 1) {
                unmapped++;
                if (args.keep_unmapped || args.passthrough) out_records.push_back(ri);
            } else if (args.passthrough) {
                out_records.push_back(ri);
            }
        }

        // ---- staging: reads -> unique (position, UMI) entries in canonical order (:148-176 and the
        // rank order of directional.rs:67-72).  On the GPU (umi_stage_reads: sorts and a segmented
        // merge) where the alignment key packs into 64 bits and nothing needs the per-read
        // bookkeeping of the host version below; both give the same arrays.
        size_t n = 0, nb = 0, max_umi = 0;
        bool any_n = false;
        const int n_words = umi_length ? (int)((3 * umi_length + 63) / 64) : 1; // words per key (bitset.rs:17-18)
        if (args.edit_distance && umi_length > UMI_MAX_UMI_LEN)
            die("--distance edit takes UMIs of at most 21 bases (this file's have " + std::to_string(umi_length) + ")");
        // (not zeroed when sized: the staging call writes them)
        std::vector<uint64_t, umi::bgzf::default_init_allocator<uint64_t>> keys, nmask, off; // keys / nmask: n_words words per entry
        std::vector<int32_t, umi::bgzf::default_init_allocator<int32_t>> freq;
        std::vector<uint32_t> rep;
        std::vector<std::vector<uint32_t>> global_of;
        std::vector<uint32_t> entry_of;
        KeyHash hasher;
        if (gpu_stage) {
            // the staged reads closed up (nothing moves while every read so far is staged)
            std::vector<uint32_t> staged; // staged[j] = record of the j-th staged read, once a read has been left out
            bool moved = false;
            size_t ns = 0;
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                if (info[ri].state != 0) {
                    if (!moved) {
                        moved = true;
                        staged.reserve(n_rec);
                        for (uint32_t j = 0; j < ri; j++) staged.push_back(j);
                    }
                    continue;
                }
                if (moved) {
                    akey[ns] = akey[ri];
                    if (!gkey.empty()) gkey[ns] = gkey[ri];
                    std::memmove(&umis[ns * umi_length], &umis[(size_t)ri * umi_length], umi_length);
                    sc[ns] = sc[ri];
                    staged.push_back(ri);
                }
                ns++;
            }
            rep64.resize(ns);
            for (uint8_t f : fits) gpu_stage = gpu_stage && f;
            // The alignment key in as few bits as the file needs -- (ref, strand) code above the coordinate
            // counted from the smallest one -- so that with the UMI it fits the device sort's one 64-bit key
            // (a human genome: 6 + 28 bits, and 28 more for 12 bases)
            int akey_bits = 64;
            if (gpu_stage && ns) {
                const int64_t lo = *std::min_element(c_min.begin(), c_min.end()), hi = *std::max_element(c_max.begin(), c_max.end());
                const uint64_t rs_hi = *std::max_element(rs_max.begin(), rs_max.end());
                auto bits_of = [](uint64_t v) { int b = 1; while (b < 64 && (v >> b)) b++; return b; };
                const int cbits = bits_of((uint64_t)(hi - lo)), rbits = bits_of(rs_hi);
                if (cbits + rbits < 64) {
                    akey_bits = cbits + rbits;
                    const size_t per = (ns + T - 1) / T;
                    umi::bgzf::parallel_for(T, T, [&](size_t t) {
                        for (size_t j = t * per; j < std::min(ns, (t + 1) * per); j++) {
                            const uint64_t a = akey[j];
                            akey[j] = ((a >> 32) << cbits) | (uint64_t)((int64_t)(int32_t)(uint32_t)a - lo);
                        }
                    });
                }
            }
            lap("fill");
            if (!gpu_stage) encode_all(); // (a coordinate beyond 32 bits: the host staging takes the file)
            if (gpu_stage) {
                need_ctx();
                lap("wait-gpu");
                keys.resize(ns * n_words); nmask.resize(ns * n_words); freq.resize(ns); off.resize(ns + 1);
                uint64_t ne = 0, nbk = 0;
                if (args.per_cell && !lib.stage_reads_grouped) die("libumihip.so lacks umi_stage_reads_grouped_wide");
                const int rc = args.per_cell
                                   ? lib.stage_reads_grouped(ctx, akey.data(), akey_bits, gkey.data(), bits_of(n_cells), umis.data(),
                                                             sc.data(), ns, (int)umi_length, n_words, merge != 0 ? 1 : 0,
                                                             keys.data(), nmask.data(), freq.data(), rep64.data(), off.data(),
                                                             &ne, &nbk)
                                   : lib.stage_reads(ctx, akey.data(), akey_bits, umis.data(), sc.data(), ns, (int)umi_length,
                                                     n_words, merge != 0 ? 1 : 0, keys.data(), nmask.data(), freq.data(),
                                                     rep64.data(), off.data(), &ne, &nbk);
                if (rc != UMI_OK) die(lib.last_error());
                lap("stage-call");
                n = (size_t)ne;
                nb = (size_t)nbk;
                keys.resize(n * n_words); nmask.resize(n * n_words); freq.resize(n); off.resize(nb + 1);
                rep.resize(n);
                for (size_t i = 0; i < n; i++) rep[i] = moved ? staged[rep64[i]] : (uint32_t)rep64[i];
                for (uint64_t m : nmask) any_n |= m != 0;
                for (size_t b = 0; b < nb; b++) max_umi = std::max<size_t>(max_umi, off[b + 1] - off[b]);
                lap("after-stage");
            }
        }
        if (!gpu_stage) {
        struct Shard {
            std::unordered_map<AlignKey, uint32_t, KeyHash> bucket_of; // Align -> local bucket
            std::vector<std::unordered_map<UmiKey, uint32_t, UmiKeyHash>> umi_index;          // key -> local entry
            std::vector<std::vector<uint32_t>> bucket_entries;
            std::vector<uint32_t> bucket_first; // first read of the bucket
            std::vector<Entry> entries;
        };
        std::vector<Shard> shards(args.passthrough ? 0 : T);
        entry_of.assign(need_clusters ? n_rec : 0, 0); // read -> entry of its shard (--tag, --call-consensus)
        umi::bgzf::parallel_for(shards.size(), T, [&](size_t t) {
            Shard &sh = shards[t];
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                const ReadInfo &ii = info[ri];
                if (ii.state != 0) continue;
                const AlignKey akey{ii.coord, ii.ref_strand, ii.tlen, ii.cell};
                if (hasher(akey) % T != t) continue;
                auto it = sh.bucket_of.find(akey);
                uint32_t b;
                if (it == sh.bucket_of.end()) {
                    b = (uint32_t)sh.bucket_entries.size();
                    sh.bucket_of.emplace(akey, b);
                    sh.bucket_entries.emplace_back();
                    sh.umi_index.emplace_back();
                    sh.bucket_first.push_back(ri);
                } else {
                    b = it->second;
                }
                auto &idx = sh.umi_index[b];
                auto e = idx.find(rkey[ri]);
                if (need_clusters) entry_of[ri] = e == idx.end() ? (uint32_t)sh.entries.size() : e->second;
                if (e == idx.end()) { // Vacant :161-163
                    idx.emplace(rkey[ri], (uint32_t)sh.entries.size());
                    sh.bucket_entries[b].push_back((uint32_t)sh.entries.size());
                    sh.entries.push_back({rkey[ri], rnm[ri], 1, ii.score, ri, b});
                } else { // Occupied :164-175
                    Entry &en = sh.entries[e->second];
                    const bool keep_existing = merge == 0 ? true : en.score >= ii.score; // merge/mod.rs:21,35,49
                    en.freq += 1;
                    if (!keep_existing) { en.rep = ri; en.score = ii.score; }
                }
            }
        });

        // buckets in order of first appearance; inside a bucket the stable freq-descending order
        // of directional.rs:67-72 (creation order of a bucket's entries = first appearance)
        struct BucketRef { uint32_t first, shard, local; };
        std::vector<BucketRef> order;
        for (uint32_t t = 0; t < shards.size(); t++) {
            n += shards[t].entries.size();
            for (uint32_t b = 0; b < shards[t].bucket_entries.size(); b++)
                order.push_back({shards[t].bucket_first[b], t, b});
        }
        std::sort(order.begin(), order.end(), [](const BucketRef &x, const BucketRef &y) { return x.first < y.first; });
        nb = order.size();
        keys.assign(n * n_words, 0); nmask.assign(n * n_words, 0); off.assign(nb + 1, 0);
        freq.assign(n, 0);
        rep.assign(n, 0);
        size_t w = 0;
        global_of.assign(need_clusters ? shards.size() : 0, {}); // (shard, entry) -> index
        for (size_t t = 0; t < global_of.size(); t++) global_of[t].resize(shards[t].entries.size());
        for (size_t b = 0; b < nb; b++) {
            Shard &sh = shards[order[b].shard];
            auto &v = sh.bucket_entries[order[b].local];
            std::stable_sort(v.begin(), v.end(), [&](uint32_t x, uint32_t y) { return sh.entries[y].freq < sh.entries[x].freq; });
            for (uint32_t ei : v) {
                const Entry &en = sh.entries[ei];
                if (need_clusters) global_of[order[b].shard][ei] = (uint32_t)w;
                for (int q = 0; q < n_words; q++) {
                    keys[w * n_words + q] = en.key.w[q];
                    nmask[w * n_words + q] = en.nmask.w[q];
                    any_n |= en.nmask.w[q] != 0;
                }
                freq[w] = en.freq; rep[w] = en.rep;
                w++;
            }
            off[b + 1] = w;
            max_umi = std::max(max_umi, v.size());
        }
        }
        // --per-cell: a bucket is a (position, cell) group; the positions are counted as ever, and every
        // group's cell id (the rank of the barcode's first appearance) is what --dump-staging adds
        size_t n_positions = nb;
        std::vector<uint32_t> bucket_cell;
        if (args.per_cell && !args.passthrough) {
            std::unordered_set<AlignKey, KeyHash> positions;
            bucket_cell.resize(nb);
            for (size_t b = 0; b < nb; b++) {
                const ReadInfo &ii = info[rep[off[b]]];
                positions.insert(AlignKey{ii.coord, ii.ref_strand, ii.tlen});
                bucket_cell[b] = ii.cell;
            }
            n_positions = positions.size();
        }
        const double t_stage0 = now_s();
        std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_stage0 - t_start); // :178-183
        if (!args.dump_staging.empty()) { // test hook: staged hot-path input, no GPU touched
            FILE *f = std::fopen(args.dump_staging.c_str(), "wb");
            if (!f) die("cannot open " + args.dump_staging);
            const uint64_t hdr[4] = {n, nb, umi_length, (uint64_t)n_words};
            std::fwrite(hdr, 8, 4, f);
            std::fwrite(keys.data(), 8, n * n_words, f); std::fwrite(nmask.data(), 8, n * n_words, f);
            std::fwrite(freq.data(), 4, n, f); std::fwrite(rep.data(), 4, n, f);
            std::fwrite(off.data(), 8, nb + 1, f);
            if (args.per_cell) std::fwrite(bucket_cell.data(), 4, nb, f); // (--per-cell: every bucket's cell id)
            std::fclose(f);
            if (!args.umi_tag.empty()) std::fprintf(stderr, "Number of reads without a UMI tag: %zu\n", no_umi_tag);
            if (args.per_cell) {
                std::fprintf(stderr, "Number of reads without a cell barcode: %zu\n", no_cell);
                std::fprintf(stderr, "Number of unique alignment positions: %zu\n", n_positions);
                std::fprintf(stderr, "Number of (position, cell) groups: %zu\n", nb);
            }
            return 0;
        }

        // ---- the hot path: one batched call replaces the bucket loop :207-233
        lap("to-hot-path");
        std::vector<uint8_t> kept(n + 1, 0);
        std::vector<uint32_t> root(need_clusters ? n + 1 : 0);
        umi_stats st;
        std::memset(&st, 0, sizeof(st));
        double t_gpu0 = now_s(), t_gpu1 = t_gpu0;
        if (!args.passthrough && n) {
            need_ctx();
            // The reference accepts every --data value and always runs Naive
            // (deduplicate_sam.rs:210-213): the result -- and here the path -- is the same for all of them.
            t_gpu0 = now_s();
            if (lib.dedup(ctx, keys.data(), any_n ? nmask.data() : nullptr, n_words, freq.data(), off.data(), nb,
                          (int)umi_length, args.k, args.percentage, algo, 0 /* adjacency.rs:56 */,
                          kept.data(), need_clusters ? root.data() : nullptr, &st) != UMI_OK)
                die(lib.last_error());
            t_gpu1 = now_s();
        }
        // (the context is not put away: tearing the HIP runtime down costs a process that lives half
        // a second another 0.1 s, and the process ends below without running destructors)
        // --tag: cluster id / size per entry from the root of every entry.  Survivors in index
        // order are the roots in the order ClusterTracker::track sees them (bucket by bucket,
        // rank order inside), so offset + idx (cluster_tracker.rs:88-100, deduplicate_sam.rs:215)
        // is the running survivor count.
        std::vector<uint32_t> cluster_id, cluster_reads;
        std::vector<uint32_t> tagged; // staged reads in file order
        if (args.track_clusters) {
            cluster_id.assign(n, 0);
            cluster_reads.assign(n, 0);
            uint32_t next = 0;
            for (size_t i = 0; i < n; i++)
                if (kept[i]) cluster_id[i] = next++;
            for (size_t i = 0; i < n; i++) cluster_reads[root[i]] += (uint32_t)freq[i]; // temp_freq, :83-85
            for (uint32_t ri = 0; ri < n_rec; ri++)
                if (info[ri].state == 0) tagged.push_back(ri);
        } else if (!args.paired) {
            for (size_t i = 0; i < n; i++)
                if (kept[i]) out_records.push_back(rep[i]); // :227-231, in rank order per bucket
        } else {
            // UcWriter (:382-459): every written paired record leaves (qname, mate ref, mate pos)
            // in a set; when the reference name of the written records changes, and once at the
            // end, the input is scanned again in file order and the second mates found in the set
            // are written.  The file is in memory here, so the scans walk record indices (per
            // reference for the partial passes).  The reference's set hashes the coordinate but
            // compares only names (:288-296); here the coordinate is part of the identity.
            std::unordered_map<int32_t, std::vector<uint32_t>> mates_on; // tid -> second mates, file order
            std::vector<uint32_t> mates_all;
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                const umi::bam::Record &r = in.records[ri];
                if (mate_candidate(r)) { // :425-429
                    mates_on[r.tid()].push_back(ri);
                    mates_all.push_back(ri);
                }
            }
            std::unordered_set<std::string> waiting;
            auto write_reversed = [&](const std::vector<uint32_t> &cands) {
                for (uint32_t ri : cands) {
                    if (waiting.empty()) break;
                    const umi::bam::Record &r = in.records[ri];
                    auto it = waiting.find(mate_key(r.qname(), r.qname_len(), r.tid(), r.pos()));
                    if (it != waiting.end()) {
                        out_records.push_back(ri);
                        waiting.erase(it);
                    }
                }
            };
            bool have_ref = false;
            int32_t cur_ref = 0;
            for (size_t i = 0; i < n; i++) {
                if (!kept[i]) continue;
                const umi::bam::Record &r = in.records[rep[i]];
                if (!have_ref) {
                    have_ref = true;
                } else if (cur_ref != r.tid()) {
                    auto m = mates_on.find(cur_ref);
                    if (m != mates_on.end()) write_reversed(m->second); // write_reversed(false), :390-393
                }
                cur_ref = r.tid();
                if (r.is_paired()) waiting.insert(mate_key(r.qname(), r.qname_len(), r.mtid(), r.mpos())); // :395-401
                out_records.push_back(rep[i]);
            }
            if (have_ref) write_reversed(mates_all); // close(), :411-415
        }

        // --call-consensus: the clusters numbered in order of kept entry (as cluster_id above), every staged read a
        // voter of its cluster or of none, one call, then the kept records rebuilt around what came back
        struct ConsensusOut {
            std::vector<uint32_t> entry_of_out; // per written record: its kept entry, UINT32_MAX for the others
            std::vector<uint32_t> cluster_id, cluster_reads, clen, depth, disagree;
            std::vector<uint64_t> seq_off, qual_off;
            umi::bgzf::Bytes seq, qual;
            size_t n_below = 0, n_without = 0;
        } cons;
        if (args.call_consensus) {
            cons.entry_of_out.assign(out_records.size(), UINT32_MAX);
            cons.cluster_id.assign(n, 0);
            cons.cluster_reads.assign(n, 0);
            uint32_t nc = 0;
            {
                size_t o = out_records.size();
                for (size_t i = n; i-- > 0;)
                    if (kept[i]) cons.entry_of_out[--o] = (uint32_t)i; // (the kept entries are the last records written)
            }
            for (size_t i = 0; i < n; i++)
                if (kept[i]) cons.cluster_id[i] = nc++;
            for (size_t i = 0; i < n; i++) cons.cluster_reads[root[i]] += (uint32_t)freq[i];
            cons.clen.assign(nc, 0);
            for (size_t i = 0; i < n; i++) {
                if (!kept[i]) continue;
                const umi::bam::Record &rr = in.records[rep[i]];
                const bool can = rr.l_seq() > 0 && rr.qual()[0] != 0xFF;
                cons.clen[cons.cluster_id[i]] = can ? (uint32_t)rr.l_seq() : 0u;
                if (!can) cons.n_without++;
            }
            std::vector<uint64_t> pos;   // seq_pos, then qual_pos, of the staged reads
            std::vector<uint32_t> rlen, rcluster;
            std::vector<uint32_t> staged_reads;
            for (uint32_t ri = 0; ri < n_rec; ri++)
                if (info[ri].state == 0) staged_reads.push_back(ri);
            const size_t ns = staged_reads.size();
            pos.resize(2 * ns);
            rlen.resize(ns);
            rcluster.resize(ns);
            const uint8_t *base = in.data.data();
            for (size_t j = 0; j < ns; j++) {
                const uint32_t ri = staged_reads[j];
                const umi::bam::Record &r = in.records[ri];
                if (r.l_seq() > UMI_MAX_CONS_LEN)
                    die("--call-consensus: read " + std::string((const char *)r.qname(), r.qname_len()) + " has " +
                        std::to_string(r.l_seq()) + " bases, more than " + std::to_string(UMI_MAX_CONS_LEN));
                const AlignKey akey{info[ri].coord, info[ri].ref_strand, info[ri].tlen, info[ri].cell};
                const uint32_t e = global_of[hasher(akey) % T][entry_of[ri]];
                const uint32_t rt = root[e];
                const umi::bam::Record &rr = in.records[rep[rt]];
                const uint32_t c = cons.cluster_id[rt];
                const bool votes = cons.clen[c] != 0 && r.l_seq() == rr.l_seq() && r.n_cigar() == rr.n_cigar() &&
                                   std::memcmp(r.cigar(), rr.cigar(), 4 * (size_t)r.n_cigar()) == 0 && r.qual()[0] != 0xFF;
                pos[j] = (uint64_t)(r.seq() - base);
                pos[ns + j] = (uint64_t)(r.qual() - base);
                rlen[j] = (uint32_t)r.l_seq();
                rcluster[j] = votes ? c : UMI_NO_CLUSTER;
            }
            size_t cap_s = 0, cap_q = 0;
            for (uint32_t L : cons.clen) {
                cap_s += (L + 1) / 2;
                cap_q += L;
            }
            cons.seq.resize(cap_s + 1);
            cons.qual.resize(cap_q + 1);
            cons.seq_off.assign(nc + 1, 0);
            cons.qual_off.assign(nc + 1, 0);
            cons.depth.assign(nc + 1, 0);
            cons.disagree.assign(nc + 1, 0);
            if (nc) {
                need_ctx();
                if (!lib.consensus_bam) die("libumihip.so lacks umi_consensus_bam");
                // (a --devices context shards positions; the vote is one device's work: the first one's)
                umi_ctx *cctx = ctx;
                if (args.devices.size() > 1 &&
                    lib.ctx_create_multi(args.devices.data(), 1, &cctx) != UMI_OK)
                    die(lib.last_error());
                uint64_t sb = 0, qb = 0;
                if (lib.consensus_bam(cctx, base, pos.data(), pos.data() + ns, rlen.data(), rcluster.data(), ns, cons.clen.data(),
                                      nc, cons.seq.data(), cons.qual.data(), cons.seq_off.data(), cons.qual_off.data(),
                                      cons.depth.data(), cons.disagree.data(), &sb, &qb) != UMI_OK)
                    die(lib.last_error());
            }
            lap("consensus");
        }

        // ---- write: header verbatim (Header::from_template :357-362) + surviving records verbatim
        constexpr size_t TAG_BYTES = 3 * 7; // three int32 aux fields
        lap("hot-path+select");
        if (args.call_consensus) {
            size_t out_len = in.header_len;
            for (uint32_t ri : out_records) out_len += (size_t)(in.records[ri].end - in.records[ri].begin) + TAG_BYTES;
            umi::bgzf::Bytes out(out_len);
            std::memcpy(out.data(), in.data.data(), in.header_len);
            size_t o = in.header_len;
            for (size_t j = 0; j < out_records.size(); j++) {
                const umi::bam::Record &r = in.records[out_records[j]];
                const size_t len = (size_t)(r.end - r.begin);
                const uint32_t e = cons.entry_of_out[j];
                const uint32_t c = e == UINT32_MAX ? 0u : cons.cluster_id[e];
                if (e == UINT32_MAX || cons.clen[c] == 0) { // (a kept unmapped read; a cluster without a consensus)
                    std::memcpy(out.data() + o, r.begin, len);
                    o += len;
                    continue;
                }
                if (cons.depth[c] < args.call_consensus_min_reads) {
                    cons.n_below++;
                    continue;
                }
                const size_t head = (size_t)(r.seq() - r.begin), ls = (size_t)r.l_seq(), sbytes = (ls + 1) / 2;
                const size_t aux_len = (size_t)(r.end - r.aux());
                std::memcpy(out.data() + o, r.begin, head);
                const int32_t block_size = (int32_t)(len - 4 + TAG_BYTES);
                std::memcpy(out.data() + o, &block_size, 4);
                std::memcpy(out.data() + o + head, cons.seq.data() + cons.seq_off[c], sbytes);
                std::memcpy(out.data() + o + head + sbytes, cons.qual.data() + cons.qual_off[c], ls);
                std::memcpy(out.data() + o + head + sbytes + ls, r.aux(), aux_len);
                o += len;
                const struct { const char *tag; int32_t v; } aux[3] = {
                    {"cD", (int32_t)cons.depth[c]}, {"cs", (int32_t)cons.cluster_reads[e]}, {"ce", (int32_t)cons.disagree[c]}};
                for (const auto &a : aux) {
                    out[o++] = (uint8_t)a.tag[0];
                    out[o++] = (uint8_t)a.tag[1];
                    out[o++] = 'i';
                    std::memcpy(out.data() + o, &a.v, 4);
                    o += 4;
                }
            }
            umi::bgzf::compress_to_file(args.output, out.data(), o, args.num_threads, args.compress_level);
        } else if (tagged.empty()) {
            // the stream as pieces of the input (neighbouring survivors are one piece): the compressor
            // gathers each block's 64 KB itself, nothing is copied together first
            std::vector<umi::bgzf::Piece> pieces;
            pieces.reserve(out_records.size() / 2 + 2);
            pieces.push_back({in.data.data(), in.header_len});
            for (uint32_t ri : out_records) {
                const uint8_t *rb = in.records[ri].begin;
                const size_t len = (size_t)(in.records[ri].end - rb);
                if (pieces.back().p + pieces.back().len == rb) pieces.back().len += len;
                else pieces.push_back({rb, len});
            }
            umi::bgzf::compress_pieces_to_file(args.output, pieces, args.num_threads, args.compress_level);
        } else {
        size_t out_len = in.header_len;
        for (uint32_t ri : out_records) out_len += (size_t)(in.records[ri].end - in.records[ri].begin);
        for (uint32_t ri : tagged) out_len += (size_t)(in.records[ri].end - in.records[ri].begin) + TAG_BYTES;
        umi::bgzf::Bytes out(out_len);
        std::memcpy(out.data(), in.data.data(), in.header_len);
        size_t o = in.header_len;
        for (uint32_t ri : out_records) {
            const size_t len = (size_t)(in.records[ri].end - in.records[ri].begin);
            std::memcpy(out.data() + o, in.records[ri].begin, len);
            o += len;
        }
        for (uint32_t ri : tagged) {
            const size_t len = (size_t)(in.records[ri].end - in.records[ri].begin);
            std::memcpy(out.data() + o, in.records[ri].begin, len);
            const int32_t block_size = (int32_t)(len - 4 + TAG_BYTES);
            std::memcpy(out.data() + o, &block_size, 4);
            o += len;
            const AlignKey akey{info[ri].coord, info[ri].ref_strand, info[ri].tlen, info[ri].cell};
            const uint32_t e = global_of[hasher(akey) % T][entry_of[ri]];
            const uint32_t r = root[e];
            const struct { const char *tag; int32_t v; } aux[3] = {
                {"MI", (int32_t)cluster_id[r]}, {"cs", (int32_t)cluster_reads[r]}, {"su", freq[e]}};
            for (const auto &a : aux) {
                out[o++] = (uint8_t)a.tag[0];
                out[o++] = (uint8_t)a.tag[1];
                out[o++] = 'i';
                std::memcpy(out.data() + o, &a.v, 4);
                o += 4;
            }
        }
        umi::bgzf::compress_to_file(args.output, out.data(), out.size(), args.num_threads, args.compress_level);
        }
        lap("write");
        const double t_end = now_s();

        // counters of deduplicate_sam.rs:243-268
        std::fprintf(stderr, "Number of input reads: %zu\n", total_read_count);
        std::fprintf(stderr, "Number of removed unmapped reads: %zu\n", unmapped);
        if (args.paired) {
            std::fprintf(stderr, "Number of unpaired reads: %zu\n", unpaired);
            std::fprintf(stderr, "Number of chimeric reads: %zu\n", chimeric);
        }
        if (!args.umi_tag.empty()) std::fprintf(stderr, "Number of reads without a UMI tag: %zu\n", no_umi_tag);
        if (args.per_cell) std::fprintf(stderr, "Number of reads without a cell barcode: %zu\n", no_cell);
        if (!cell_list.empty()) {
            std::fprintf(stderr, "Number of reads with a corrected cell barcode: %llu\n", (unsigned long long)cb_counts[1]);
            std::fprintf(stderr, "Number of reads with an unlisted cell barcode: %llu\n", (unsigned long long)cb_counts[2]);
            std::fprintf(stderr, "Number of reads with an ambiguous cell barcode: %llu\n", (unsigned long long)cb_counts[3]);
        }
        if (!whitelist.empty()) {
            std::fprintf(stderr, "Number of reads with a corrected UMI: %llu\n", (unsigned long long)wl_counts[1]);
            std::fprintf(stderr, "Number of reads with an uncorrectable UMI: %llu\n", (unsigned long long)wl_counts[2]);
        }
        std::fprintf(stderr, "Number of unique alignment positions: %zu\n", n_positions);
        if (args.per_cell) std::fprintf(stderr, "Number of (position, cell) groups: %zu\n", nb);
        std::fprintf(stderr, "Number of UMIs: %zu\n", n);
        std::fprintf(stderr, "Average number of UMIs per alignment position: %g\n", nb ? (double)n / (double)nb : 0.0);
        std::fprintf(stderr, "Max number of UMIs over all alignment positions: %zu\n", max_umi);
        std::fprintf(stderr, args.track_clusters ? "Number of groups of reads: %llu\n" : "Number of reads after deduplicating: %llu\n",
                     (unsigned long long)st.n_kept); // :259-266
        if (args.edit_distance) std::fprintf(stderr, "UMI distance: edit\n");
        if (args.call_consensus) {
            std::fprintf(stderr, "Number of clusters below --call-consensus-min-reads: %zu\n", cons.n_below);
            std::fprintf(stderr, "Number of clusters without a consensus: %zu\n", cons.n_without);
        }
        std::fprintf(stderr,
                     "phases: read+inflate %.3f s, staging (%s) %.3f s, gpu init %.3f s, hot path (H2D+GPU+D2H) %.3f s [%llu pairs], write %.3f s\n",
                     t_read - t_start, gpu_stage ? "gpu" : "host", t_stage0 - t_read - (gpu_stage ? t_init : 0.0), t_init,
                     t_gpu1 - t_gpu0, (unsigned long long)st.n_pairs, t_end - t_gpu1);
        std::fprintf(stderr, "UMI collapsing finished in %.3f seconds\n", t_end - t_start); // main.rs:97-102
        leave(); // (from inside the scope of the file's buffers: they go with the process, unmapped by nobody)
    } catch (const std::exception &e) {
        die(e.what());
    }
    leave();
}
