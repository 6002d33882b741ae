// libumihip.so as the program uses it: the entry points resolved by hand (HipLib), the thread that wakes the
// GPU while the input is read (GpuWarmup) and the program's clock (Clock).
//
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
//
// --count-matrix DIR (with --per-gene): umi_count_matrix, the one library call behind the flag, is resolved only
// when the flag is given, so that a library without it serves every other run.
//
// --output-stats PREFIX: likewise umi_dedup_stats.
//
// --cell-whitelist-multi: likewise umi_correct_barcodes_multi, in umi_correct_barcodes' place.
//
// --umi-filtering multi-gene: likewise umi_filter_multigene.
//
// --cell-filter RULE (with --count-matrix): likewise umi_call_cells.
//
// --gene-annotation FILE: likewise umi_assign_genes.
//
// --gene-introns exon-first|all: likewise umi_assign_genes_introns, in umi_assign_genes' place.
// --gene-rule transcript: likewise umi_assign_genes_transcripts, in umi_assign_genes' place.
//
// --velocity: likewise umi_assign_genes_classes, in umi_assign_genes_introns' place, and umi_velocity_matrix.
//
// --transcript-introns exon-first|all (with --gene-rule transcript): likewise umi_assign_genes_transcripts_classes, in
// umi_assign_genes_transcripts' place; with --velocity it tells the classes too, and umi_assign_genes_classes is not asked for.
//
// --saturation-curve FILE: likewise umi_saturation_curve.
//
// --junction-matrix: likewise umi_junction_matrix.
#pragma once
#include <chrono>
#include <dlfcn.h>
#include <future>
#include <unistd.h>

#include "cli.hpp"

namespace {

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// libumihip.so is opened by hand, on the side thread that wakes the GPU: mapping the library and
// the HIP runtime it brings along (static initialisers, the code objects' registration) takes
// ~0.15 s before main() of a process that otherwise lives 0.45 s, and the first thing the
// program does -- reading and inflating the input -- needs none of it.
struct HipLib {
    void *handle = nullptr;
    // (every entry point with the type include/umihip.h declares it with)
    decltype(&umi_ctx_create_multi) ctx_create_multi = nullptr;
    decltype(&umi_ctx_set_option) ctx_set_option = nullptr;
    decltype(&umi_last_error) last_error = nullptr;
    // (the forms for keys of any number of words: one word is the ordinary call behind them)
    decltype(&umi_stage_reads_wide) stage_reads = nullptr;
    decltype(&umi_stage_reads_grouped_wide) stage_reads_grouped = nullptr; // --per-cell: positions are (alignment, cell id) pairs
    decltype(&umi_dedup_batch_wide) dedup_batch = nullptr;
    decltype(&umi_dedup_seqs) dedup_seqs = nullptr;
    // fastq mode's device staging: its arrays stay on the device between the two calls
    decltype(&umi_stage_seqs) stage_seqs = nullptr;
    decltype(&umi_stage_seqs_device) stage_seqs_device = nullptr;
    decltype(&umi_dedup_seqs_device) dedup_seqs_device = nullptr;
    // --distance edit: resolved only when the flag is given, like --consensus below; one-word keys only
    bool want_edit = false;
    decltype(&umi_dedup_batch_edit) dedup_batch_edit = nullptr;
    // --algo cr: likewise; one-word keys only, no -k and no -p
    bool want_cr = false;
    decltype(&umi_dedup_batch_cr) dedup_batch_cr = nullptr;
    // the batched call of the run: by the rule --algo names and the distance --distance names
    int dedup(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq, const uint64_t *off,
              uint64_t nb, int umi_len, int k, float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
              umi_stats *st) const
    {
        if (want_cr) // (n_words is 1: a UMI length above 21 has been refused)
            return dedup_batch_cr(ctx, keys, nmask, freq, off, nb, umi_len, kept, root, nullptr, st);
        if (want_edit) // (n_words is 1: a UMI length above 21 has been refused)
            return dedup_batch_edit(ctx, keys, nmask, freq, off, nb, umi_len, k, percentage, algo, adj_max_freq, kept, root, st);
        return dedup_batch(ctx, keys, nmask, n_words, freq, off, nb, umi_len, k, percentage, algo, adj_max_freq, kept, root, st);
    }
    // --consensus: resolved only when the flag is given, so that a library without them serves every other run
    bool want_consensus = false;
    decltype(&umi_consensus_seqs) consensus_seqs = nullptr;
    decltype(&umi_consensus_seqs_device) consensus_seqs_device = nullptr;
    // --call-consensus: likewise
    bool want_consensus_bam = false;
    decltype(&umi_consensus_bam) consensus_bam = nullptr;
    // --umi-whitelist: resolved only when the flag is given, like --consensus
    bool want_correct = false;
    decltype(&umi_correct_umis) correct_umis = nullptr;
    // --cell-whitelist: likewise
    bool want_barcodes = false;
    decltype(&umi_correct_barcodes) correct_barcodes = nullptr;
    // --cell-whitelist-multi: likewise, in its place
    bool want_barcodes_multi = false;
    decltype(&umi_correct_barcodes_multi) correct_barcodes_multi = nullptr;
    // --count-matrix: likewise
    bool want_count = false;
    decltype(&umi_count_matrix) count_matrix = nullptr;
    // --output-stats: likewise
    bool want_stats = false;
    decltype(&umi_dedup_stats) dedup_stats = nullptr;
    // --umi-filtering multi-gene: likewise
    bool want_multigene = false;
    decltype(&umi_filter_multigene) filter_multigene = nullptr;
    // --cell-filter: likewise
    bool want_cells = false;
    decltype(&umi_call_cells) call_cells = nullptr;
    // --gene-annotation: likewise
    bool want_genes = false;
    decltype(&umi_assign_genes) assign_genes = nullptr;
    // --gene-rule transcript: likewise, in its place
    bool want_transcripts = false;
    decltype(&umi_assign_genes_transcripts) assign_genes_transcripts = nullptr;
    // --transcript-introns exon-first|all: likewise, in its place
    bool want_transcript_classes = false;
    decltype(&umi_assign_genes_transcripts_classes) assign_genes_transcripts_classes = nullptr;
    // --gene-introns exon-first|all: likewise, in its place
    bool want_introns = false;
    decltype(&umi_assign_genes_introns) assign_genes_introns = nullptr;
    // --velocity: likewise, in its place (not under --transcript-introns, whose call tells the classes), and the three layers' call
    bool want_velocity = false, want_gene_classes = false;
    decltype(&umi_assign_genes_classes) assign_genes_classes = nullptr;
    decltype(&umi_velocity_matrix) velocity_matrix = nullptr;
    // --saturation-curve: likewise
    bool want_saturation = false;
    decltype(&umi_saturation_curve) saturation_curve = nullptr;
    // --junction-matrix: likewise
    bool want_junctions = false;
    decltype(&umi_junction_matrix) junction_matrix = nullptr;
    // (the HIP runtime the library brings along: device buffers for the arrays above)
    int (*hip_set_device)(int) = nullptr; // (the current device is per thread: the context was made on another)
    int (*hip_malloc)(void **, size_t) = nullptr;
    int (*hip_memcpy)(void *, const void *, size_t, int) = nullptr; // kind: 1 host to device, 2 device to host
    std::string error;
    explicit HipLib(const Cli &args)
        : want_edit(args.edit_distance), want_cr(args.algo_cr), want_consensus(args.consensus), want_consensus_bam(args.call_consensus),
          want_correct(!args.whitelist.empty()), want_barcodes(!args.cell_list.empty() && !args.cell_wl_multi),
          want_barcodes_multi(!args.cell_list.empty() && args.cell_wl_multi),
          want_count(!args.count_matrix.empty()), want_stats(!args.output_stats.empty()),
          want_multigene(args.filter_multigene), want_cells(args.cell_filter_given),
          want_genes(args.gene_annotation_given && args.gene_introns_mode == UMI_INTRONS_OFF && !args.gene_rule_transcript),
          want_transcripts(args.gene_annotation_given && args.gene_rule_transcript && args.transcript_introns_mode == UMI_INTRONS_OFF),
          want_transcript_classes(args.gene_annotation_given && args.gene_rule_transcript && args.transcript_introns_mode != UMI_INTRONS_OFF),
          want_introns(args.gene_annotation_given && args.gene_introns_mode != UMI_INTRONS_OFF && !args.velocity),
          want_velocity(args.velocity), want_gene_classes(args.velocity && args.transcript_introns_mode == UMI_INTRONS_OFF),
          want_saturation(!args.saturation_curve.empty()), want_junctions(args.junction_matrix)
    {
    }
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
        if (want_cr) dedup_batch_cr = (decltype(dedup_batch_cr))sym("umi_dedup_batch_cr");
        if (want_consensus) {
            consensus_seqs = (decltype(consensus_seqs))sym("umi_consensus_seqs");
            consensus_seqs_device = (decltype(consensus_seqs_device))sym("umi_consensus_seqs_device");
        }
        if (want_consensus_bam) consensus_bam = (decltype(consensus_bam))sym("umi_consensus_bam");
        if (want_correct) correct_umis = (decltype(correct_umis))sym("umi_correct_umis");
        if (want_barcodes) correct_barcodes = (decltype(correct_barcodes))sym("umi_correct_barcodes");
        if (want_barcodes_multi) correct_barcodes_multi = (decltype(correct_barcodes_multi))sym("umi_correct_barcodes_multi");
        if (want_count) count_matrix = (decltype(count_matrix))sym("umi_count_matrix");
        if (want_stats) dedup_stats = (decltype(dedup_stats))sym("umi_dedup_stats");
        if (want_multigene) filter_multigene = (decltype(filter_multigene))sym("umi_filter_multigene");
        if (want_cells) call_cells = (decltype(call_cells))sym("umi_call_cells");
        if (want_genes) assign_genes = (decltype(assign_genes))sym("umi_assign_genes");
        if (want_transcripts) assign_genes_transcripts = (decltype(assign_genes_transcripts))sym("umi_assign_genes_transcripts");
        if (want_transcript_classes)
            assign_genes_transcripts_classes = (decltype(assign_genes_transcripts_classes))sym("umi_assign_genes_transcripts_classes");
        if (want_introns) assign_genes_introns = (decltype(assign_genes_introns))sym("umi_assign_genes_introns");
        if (want_velocity) {
            if (want_gene_classes) assign_genes_classes = (decltype(assign_genes_classes))sym("umi_assign_genes_classes");
            velocity_matrix = (decltype(velocity_matrix))sym("umi_velocity_matrix");
        }
        if (want_saturation) saturation_curve = (decltype(saturation_curve))sym("umi_saturation_curve");
        if (want_junctions) junction_matrix = (decltype(junction_matrix))sym("umi_junction_matrix");
        hip_set_device = (decltype(hip_set_device))sym("hipSetDevice");
        hip_malloc = (decltype(hip_malloc))sym("hipMalloc");
        hip_memcpy = (decltype(hip_memcpy))sym("hipMemcpy");
        return error.empty();
    }
};

// The GPU is woken while the file is read: context creation and the first launch of the
// library's kernels (their code objects are loaded then) take ~0.1 s of a process that lives
// half a second, none of it on the device.  A tiny staging call and a tiny batch go through;
// whoever needs the context first waits for this thread.
struct GpuWarmup {
    HipLib &lib;
    const std::vector<int> &devices;
    std::future<umi_ctx *> warm;
    std::string error;
    umi_ctx *ctx = nullptr;
    double t_init = 0.0; // what of the GPU's start-up was left to wait for
    GpuWarmup(HipLib &l, const std::vector<int> &d) : lib(l), devices(d) {}
    // fastq mode's tiny calls are umi_stage_seqs / umi_dedup_seqs with the run's merge, BAM mode's
    // umi_stage_reads_wide / umi_dedup_batch_wide
    void start(bool fastq, int merge)
    {
        warm = std::async(std::launch::async, [this, fastq, merge]() -> umi_ctx * {
            umi_ctx *c = nullptr;
            if (!lib.load()) {
                error = lib.error;
                return nullptr;
            }
            if (lib.ctx_create_multi(devices.data(), (int)devices.size(), &c) != UMI_OK) {
                error = lib.last_error();
                return nullptr;
            }
            const uint8_t umis[8] = {'A', 'C', 'G', 'T', 'A', 'C', 'G', 'A'};
            const uint64_t akey[2] = {0, 0}, pos[2] = {0, 4};
            const uint32_t len[2] = {4, 4};
            uint64_t k[2], nm[2], rp[2], off[3], ne = 0, nbk = 0;
            int32_t fr[2], bl[2];
            int an = 0;
            uint8_t kept[2];
            umi_stats wst;
            const bool ok =
                fastq ? lib.stage_seqs(c, umis, pos, pos, len, 2, 1, merge, k, nm, fr, rp, nullptr, off, bl, &ne, &nbk, &an) == UMI_OK &&
                            lib.dedup_seqs(c, k, nullptr, 1, fr, off, bl, nbk, 1, 0.5f, UMI_ALGO_DIRECTIONAL, 0, kept, nullptr, &wst) == UMI_OK
                      : lib.stage_reads(c, akey, 1, umis, nullptr, 2, 4, 1, 0, k, nm, fr, rp, off, &ne, &nbk) == UMI_OK &&
                            lib.dedup_batch(c, k, nullptr, 1, fr, off, nbk, 4, 1, 0.5f, UMI_ALGO_DIRECTIONAL, 0, kept, nullptr, &wst) == UMI_OK;
            if (!ok) error = lib.last_error(); // (reported when the real call fails the same way)
            return c;
        });
    }
    // the context: the start-up thread's, or one made here if the thread was never started
    umi_ctx *get()
    {
        if (ctx) return ctx;
        const double t0 = now_s();
        if (warm.valid()) {
            ctx = warm.get();
            if (!ctx) die(error);
        } else {
            if (!lib.load()) die(lib.error);
            if (lib.ctx_create_multi(devices.data(), (int)devices.size(), &ctx) != UMI_OK) die(lib.last_error());
        }
        t_init += now_s() - t0;
        return ctx;
    }
    void wait()
    {
        if (warm.valid()) warm.wait(); // (a file without staged reads: the start-up thread may still be at it)
    }
};

// finer split of the program's time, printed with UMICOLLAPSE_CLOCK (tools/e2e_probe.py)
struct Clock {
    const double t_main_realtime;
    std::vector<std::pair<const char *, double>> laps;
    double t_lap = now_s();
    explicit Clock(double t_main) : t_main_realtime(t_main) {}
    void lap(const char *what)
    {
        const double t = now_s();
        laps.emplace_back(what, t - t_lap);
        t_lap = t;
    }
    [[noreturn]] void leave(GpuWarmup &gpu)
    {
        gpu.wait();
        if (std::getenv("UMICOLLAPSE_CLOCK")) { // (for tools/e2e_probe.py: what lies before main and after _Exit)
            std::fprintf(stderr, "laps:");
            for (const auto &l : laps) std::fprintf(stderr, " %s %.3f", l.first, l.second);
            std::fprintf(stderr, "\nclock: main at %.6f, exit at %.6f (realtime)\n", t_main_realtime,
                         std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count());
        }
        std::fflush(nullptr);
        std::_Exit(0); // the output file is closed; device memory and the runtime go with the process
    }
};
} // namespace
