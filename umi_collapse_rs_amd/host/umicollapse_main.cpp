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
// --cell-whitelist-multi (with --cell-whitelist; after STARsolo's 1MM_multi and Cell Ranger, tests/
// barcode_multi_model.py defines it; cli.hpp has the flags): the one call is umi_correct_barcodes_multi, which
// also takes the barcodes' qualities -- the value of --cell-quality-tag (CY), gathered beside the barcode; every
// read with a barcode must carry it, type Z, of the barcode's length, bytes 33..126, else the run ends with status
// 101 -- and decides a barcode with several listed neighbours by their exact reads and the quality at the
// mismatch.  Resolved reads are numbered and grouped like corrected ones; the summary gains "Number of reads with
// a resolved cell barcode", "... an ambiguous cell barcode" counts what stayed ambiguous, and the metrics table
// gains the column `resolved`.  Without the flag every output and summary line is as before.
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
// --per-gene [--gene-tag XX] (bam/sam mode, one pass; not the reference's, tests/gene_model.py defines it): the
// reads are grouped by gene -- with --per-cell by (cell, gene) -- and not by alignment position (staging.hpp has
// the rule for a read's gene and for the reads that are dropped).  The genes are numbered after the two
// whitelists have dropped their reads, by first appearance among the reads that are staged (number_genes); both
// stagings, the collapse and the records written are as without the flag.  Goes with --umi-tag, --per-cell /
// --cell-tag, --cell-whitelist, --umi-whitelist, -k, -p, --algo, --merge, --distance edit, --num-threads,
// --devices and every --stage; refused with status 101: see cli.hpp.
// --count-matrix DIR (with --per-gene): after the collapse one call to umi_count_matrix (include/umihip.h) sums
// kept[] and freq[] over the buckets, row = the bucket's gene, column = its cell (one column without
// --per-cell), and four files are written to DIR, uncompressed, lines ended by \n: features.tsv, a line
// "<gene>\t<gene>\tGene Expression" per gene in id order; barcodes.tsv, a line per cell in id order -- the tag's
// bytes, with --cell-whitelist the listed barcode, without --per-cell the one line "all"; matrix.mtx,
// "%%MatrixMarket matrix coordinate integer general", then "G C NNZ", then NNZ lines "row col molecules", counted
// from 1, by column and then row; reads.mtx, the same with the reads.  The molecules add up to "Number of reads
// after deduplicating".
// --output-stats PREFIX [--output-stats-seed S]: three tables on what the deduplication did, from one call to
// umi_dedup_stats after the collapse (cli.hpp has the flag's definition and its refusals; output_stats() below).
// --umi-filtering multi-gene (with --per-gene; cli.hpp has the flag's definition and its refusals): after the collapse
// one call to umi_filter_multigene, group = the bucket's cell (one group without --per-cell); what it leaves --
// kept_out, and freq_out for the matrix -- is what the records written, "Number of reads after deduplicating" and
// --count-matrix see, which leaves out the pairs without a molecule; --output-stats sees the collapse's own kept[]
// (filter_multigene() below).
// --cell-filter RULE (with --per-cell --per-gene --count-matrix DIR; cli.hpp has the flag's definition, its files and
// its refusals): after umi_count_matrix one call to umi_call_cells over the triplets matrix.mtx holds; DIR/filtered/,
// DIR/cells.tsv and eight summary lines are added, everything else stays byte for byte (call_cells() below).
// --gene-annotation FILE (with --per-gene; annotation.hpp has the flags' definition, the file's reader and the
// refusals): one call to umi_assign_genes over every mapped read, after the file is read and before the per-read
// pass, which takes its verdict in the gene tag's place (assign_genes() below).
// --gene-rule transcript (with --gene-annotation; annotation.hpp): that one call is umi_assign_genes_transcripts.
// --transcript-introns exon-first|all (with --gene-rule transcript; annotation.hpp): that one call is
// umi_assign_genes_transcripts_classes -- a read that fits no transcript falls back to the gene bodies -- and with
// --velocity its classes feed umi_velocity_matrix.
// --gene-introns exon-first|all (with --gene-annotation; annotation.hpp): that one call is umi_assign_genes_introns,
// whose gene and status are used alike; its counts by tier go into the summary, the tier of a read goes nowhere.
// --velocity (with --gene-introns exon-first|all and --count-matrix DIR; annotation.hpp has the rule and the files): that
// one call is umi_assign_genes_classes, whose gene, status and counts are umi_assign_genes_introns' and whose class per
// read is kept; the reads are staged on the host, which keeps every read's entry as for --tag; after umi_count_matrix one
// call to umi_velocity_matrix over the reads' entries and classes, the surviving mask, root[] and the buckets' gene and
// cell gives the three layers of the same triplets, written to DIR/velocity/ (and, for the called cells, to
// DIR/velocity/filtered/); everything else stays byte for byte what --stage host writes without the flag.
// --saturation-curve FILE (with --per-gene --count-matrix DIR; cli.hpp has the rule and the file): the reads are staged on
// the host, which keeps every read's entry as for --velocity; after umi_count_matrix, and after umi_call_cells where
// --cell-filter is given, one call to umi_saturation_curve over the reads' entries, the surviving mask, root[], the buckets'
// gene and cell and the called cells gives every depth's row of FILE; everything else stays byte for byte what --stage
// host writes without the flag.
// --junction-matrix (with --per-gene --count-matrix DIR; cli.hpp has the rule and the files): the reads are staged on the
// host likewise; behind the calls above one call to umi_junction_matrix over the staged reads' reference, position, CIGAR
// words and entry, the surviving mask, root[] and the buckets' cell gives the junction table and its triplets, written to
// DIR/junctions/ (and, for the called cells, to DIR/junctions/filtered/); everything else stays byte for byte likewise.
// --algo cluster: connected components of "within -k" (cli.hpp); every pipeline here only forwards the algorithm
// to the library, so it goes with every flag --algo dir goes with.
// --algo cr: Cell Ranger's one-mismatch correction (cli.hpp; include/umihip.h has the rule, tests/cr_model.py defines
// it): the one-pass bam/sam pipeline's batched call is umi_dedup_batch_cr (HipLib::dedup), whose kept[] and root[] keep
// the contract of the other algorithms, so everything behind the collapse -- the matrix, the filters, the statistics,
// --tag, --call-consensus -- runs as it is.  -k 1 only, -p plays no part; the summary gains "UMI correction: cr".
// Refused before the GPU is woken: fastq mode, --two-pass, several --devices, --distance edit, UMIs of more than 21 bases.
// Not implemented, as in the reference: --algo cc (that spelling stays refused; `cluster` is the mode's name).
#include "annotation.hpp"
#include "fastq_mode.hpp"
#include "hiplib.hpp"
#include "staging.hpp"
#include "two_pass.hpp"

namespace {

struct ReadInfo {
    uint64_t coord, ref_strand, tlen;
    int32_t score;
    uint8_t state; // 0 staged, 1 unmapped, 2 error, 3 second mate (not counted),
                   // 4 mate unmapped, 5 filtered (--remove-unpaired / --remove-chimeric),
                   // 6 dropped: it lacks a tag of --umi-tag / --per-cell (`missing` says which)
                   // 7 dropped: its UMI matches no listed one (--umi-whitelist)
                   // 8 dropped: its cell barcode is unlisted or ambiguous (--cell-whitelist)
                   // 9 dropped: its gene tag names several genes (--per-gene)
    uint8_t unpaired, chimeric, missing;
    uint32_t umi_at; // offset of the UMI from the read name (a --umi-tag value lies behind it)
    uint32_t cell;   // --per-cell: the barcode's id, the thread's own during the per-read pass
    uint32_t gene;   // --per-gene: the gene's id, likewise (until number_genes)
};

// three int32 aux fields appended to a record that has been copied to `out` and ends at o; returns the new end
constexpr size_t TAG_BYTES = 3 * 7;
struct IntTag {
    const char *tag;
    int32_t v;
};
size_t append_int_tags(umi::bgzf::Bytes &out, size_t o, const IntTag (&aux)[3])
{
    for (const IntTag &a : aux) {
        out[o++] = (uint8_t)a.tag[0];
        out[o++] = (uint8_t)a.tag[1];
        out[o++] = 'i';
        std::memcpy(out.data() + o, &a.v, 4);
        o += 4;
    }
    return o;
}

// ---- the one-pass BAM pipeline: the file is held in memory, every stage a member function, the data that
// flows between them the fields
struct OnePass {
    const Cli &args;
    HipLib &lib;
    GpuWarmup &gpu;
    Clock &clock;
    const double t_start;
    const int algo = args.algo_id, merge = args.merge_id;
    const unsigned T = std::max(1u, args.num_threads);
    const bool need_clusters = args.track_clusters || args.call_consensus; // every read's entry, every entry's root
    const bool need_entries = need_clusters || args.velocity || !args.saturation_curve.empty() || args.junction_matrix; // every read's entry: the host staging keeps it
    const bool need_root = need_entries || !args.output_stats.empty() || args.filter_multigene; // root[] of the collapse (no host
                                                                                                // staging for it alone)

    umi::bam::File in;
    uint32_t n_rec = 0, chunk = 0; // records; records per thread of the per-read passes
    size_t umi_length = args.umi_length;
    bool gpu_stage = false; // where the reads are merged per (position, UMI)
    double t_read = 0.0, t_stage0 = 0.0, t_gpu0 = 0.0, t_gpu1 = 0.0;
    umi_ctx *ctx = nullptr;
    Summary sum;

    // the per-read pass
    std::vector<ReadInfo> info;
    umi::bgzf::Bytes wl_umis;      // --umi-whitelist: per record, the listed UMI a staged read was snapped to
    std::vector<UmiKey> rkey, rnm; // per read: its UMI key and N mask (host staging only: the device encodes its own)
    // GPU staging: what the device wants of a read -- alignment key, UMI text, score -- is written by the
    // per-read pass itself, at the read's own index (closed up afterwards if some reads are not staged)
    U64s akey, rep64;
    umi::bgzf::Bytes umis;
    I32s sc;
    std::vector<uint8_t> fits;
    std::vector<int64_t> c_min, c_max; // coordinates and (ref, strand) codes seen, per thread
    std::vector<uint64_t> rs_max;
    umi::bgzf::Bytes cell_raw; // --cell-whitelist: per record, a staged read's barcode as the tag has it
    umi::bgzf::Bytes cell_qual; // --cell-whitelist-multi: ... and its qualities
    std::vector<std::vector<std::string_view>> cell_seen; // --per-cell: per thread, its barcodes in order of appearance
    U64s gkey; // GPU staging with --per-cell: every read's cell id, the group key
    size_t n_cells = 0;
    std::vector<std::string_view> cell_names; // --count-matrix: what barcodes.tsv calls every cell, in id order
    std::vector<std::vector<std::string_view>> gene_seen; // --per-gene: per thread, its genes in order of appearance
    std::vector<std::string_view> gene_names;             // ... and all of them in id order
    // --gene-annotation: per record what umi_assign_genes made of it (a record the call did not see: none), the id
    // of every gene of the call, and what features.tsv calls a gene beside its id (its gene_name where it has one)
    std::vector<uint8_t> assigned_status;
    std::vector<int32_t> assigned_gene;
    std::vector<uint8_t> assigned_class; // --velocity: per record its UMI_READ_CLASS_*
    std::vector<std::string_view> annotation_ids;
    std::unordered_map<std::string_view, std::string_view> gene_display;
    const AssignedGene *assigned(uint32_t ri, AssignedGene &a) const
    {
        if (!args.gene_annotation_given) return nullptr;
        a.status = assigned_status[ri];
        a.id = a.status == UMI_GENE_ASSIGNED ? annotation_ids[(size_t)assigned_gene[ri]] : std::string_view();
        return &a;
    }
    // features.tsv: "<gene>\t<name>\tGene Expression" per gene in id order, the name being the id without an annotation
    std::string features_text() const
    {
        std::string text;
        for (const std::string_view &g : gene_names) {
            const auto d = gene_display.find(g);
            text.append(g).append("\t").append(d == gene_display.end() ? g : d->second).append("\tGene Expression\n");
        }
        return text;
    }
    std::vector<uint32_t> out_records; // the records to write, in order; first those written before dedup (--keep-unmapped, :104-106)

    // the staged arrays: unique (position, UMI) entries in canonical order
    size_t n = 0, nb = 0, max_umi = 0;
    bool any_n = false;
    int n_words = 1; // words per key (bitset.rs:17-18)
    U64s keys, nmask, off; // keys / nmask: n_words words per entry (not zeroed when sized: the staging call writes them)
    I32s freq;
    std::vector<uint32_t> rep;
    std::vector<uint32_t> entry_of;    // host staging, --tag / --call-consensus / --velocity: every staged read's entry
    std::vector<uint32_t> bucket_cell; // --per-cell: every bucket's cell id
    std::vector<uint32_t> bucket_gene; // --per-gene: every bucket's gene id

    // the collapse and what is made of it
    std::vector<uint8_t> kept;
    std::vector<uint32_t> root;
    umi_stats st;
    // --umi-filtering multi-gene: what the filter leaves of kept[] and freq[]; `survivors` is the mask everything
    // behind the collapse but --output-stats reads (kept[] itself without the flag)
    std::vector<uint8_t> kept_filtered;
    I32s freq_filtered;
    uint64_t n_survivors = 0;
    const std::vector<uint8_t> &survivors() const { return args.filter_multigene ? kept_filtered : kept; }
    std::vector<uint32_t> cluster_id, cluster_reads; // per entry (of its root): --tag, --call-consensus
    uint32_t n_clusters = 0;
    std::vector<uint32_t> staged_reads; // the staged reads in file order (with the two)
    struct ConsensusOut {
        std::vector<uint32_t> entry_of_out; // per written record: its kept entry, UINT32_MAX for the others
        std::vector<uint32_t> clen, depth, disagree;
        std::vector<uint64_t> seq_off, qual_off;
        umi::bgzf::Bytes seq, qual;
    } cons;

    OnePass(const Cli &a, HipLib &l, GpuWarmup &g, Clock &c, double t0) : args(a), lib(l), gpu(g), clock(c), t_start(t0) {}
    void lap(const char *what) { clock.lap(what); }
    void need_ctx() { ctx = gpu.get(); }

    // the reads that would be staged, in file order
    std::vector<uint32_t> candidates() const
    {
        std::vector<uint32_t> cand;
        for (uint32_t ri = 0; ri < n_rec; ri++)
            if (info[ri].state == 0) cand.push_back(ri);
        return cand;
    }
    // L bytes of each of them, from where `at` finds a read's, back to back
    umi::bgzf::Bytes gather(const std::vector<uint32_t> &cand, size_t L, const std::function<const uint8_t *(uint32_t)> &at) const
    {
        const size_t nc = cand.size(), per = (nc + T - 1) / T;
        umi::bgzf::Bytes packed(nc * L);
        umi::bgzf::parallel_for(T, T, [&](size_t t) {
            for (size_t j = t * per; j < std::min(nc, (t + 1) * per); j++) std::memcpy(&packed[j * L], at(cand[j]), L);
        });
        return packed;
    }

    // the pipeline; returns only from the --dump-staging exit
    int run()
    {
        read_input();
        if (args.gene_annotation_given) assign_genes();
        choose_staging();
        per_read_pass();
        if (!args.cell_list.empty()) correct_cells();
        else if (args.per_cell && !args.passthrough) number_cells(); // (--passthrough reads no tags)
        if (!args.whitelist.empty()) correct_umis();
        if (args.per_gene) number_genes();
        lap("per-read");
        if (!gpu_stage && !args.passthrough) encode_all();
        count_reads();
        n_words = umi_length ? (int)((3 * umi_length + 63) / 64) : 1;
        check_edit_length(args, umi_length, "this file's have");
        if (gpu_stage) stage_on_gpu(); // (gives the file to the host staging if a coordinate does not fit)
        if (!gpu_stage) stage_on_host();
        count_positions();
        if (!args.dump_staging.empty()) {
            dump_staging();
            return 0;
        }
        collapse();
        if (args.filter_multigene) filter_multigene();
        if (!args.count_matrix.empty()) count_matrix();
        if (!args.output_stats.empty()) output_stats();
        if (need_clusters) number_clusters();
        select_records();
        if (args.call_consensus) call_consensus();
        write_output();
        print_summary();
        clock.leave(gpu); // (from inside the scope of the file's buffers: they go with the process, unmapped by nobody)
    }

    // ---- read: BGZF inflate (threaded) + BAM parse
    void read_input()
    {
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
        t_read = now_s();
        n_rec = (uint32_t)in.records.size();
        chunk = (n_rec + T - 1) / T;
    }

    // --gene-annotation: the file's lines on the BAM's references, every mapped read's reference, position, strand
    // and CIGAR words gathered (the walk is the device's), one call; what it made of a read is what read_tags sees
    // in the gene tag's place
    void assign_genes()
    {
        const Cli::Annotation &an = args.annotation;
        // the BAM header's reference names -> ids (parse() has checked the lengths)
        std::unordered_map<std::string_view, int32_t> tid_of;
        {
            const uint8_t *p = in.data.data();
            size_t q = 8 + (size_t)umi::bam::rd_i32(p + 4) + 4;
            for (int32_t r = 0; r < in.n_ref; r++) {
                const size_t l_name = (size_t)umi::bam::rd_i32(p + q);
                std::string_view name((const char *)p + q + 4, l_name);
                if (!name.empty() && name.back() == '\0') name.remove_suffix(1);
                tid_of.emplace(name, r); // (a name that occurs twice: its first id, as a lookup by name would give)
                q += 4 + l_name + 4;
            }
        }
        std::vector<int32_t> tid_of_ref(an.refs.size());
        for (size_t r = 0; r < an.refs.size(); r++) {
            const auto it = tid_of.find(an.refs[r]);
            tid_of_ref[r] = it == tid_of.end() ? -1 : it->second;
        }
        // the lines on known references, their genes numbered anew by first appearance among them
        std::vector<int32_t> x_ref, x_start, x_end, x_gene, new_gene(an.gene_ids.size(), -1);
        std::vector<int32_t> x_tr, new_tr(an.n_transcripts, -1); // --gene-rule transcript: the lines' transcripts, numbered likewise
        std::vector<uint8_t> x_strand;
        for (size_t i = 0; i < an.gene.size(); i++) {
            const int32_t tid = tid_of_ref[an.ref_name[i]];
            if (tid < 0) {
                sum.annotation_unknown++;
                continue;
            }
            int32_t &g = new_gene[(size_t)an.gene[i]];
            if (g < 0) {
                g = (int32_t)annotation_ids.size();
                const std::string &id = an.gene_ids[(size_t)an.gene[i]], &name = an.gene_names[(size_t)an.gene[i]];
                annotation_ids.emplace_back(id);
                gene_display.emplace(id, name.empty() ? std::string_view(id) : std::string_view(name));
            }
            x_ref.push_back(tid);
            x_start.push_back(an.start[i]);
            x_end.push_back(an.end[i]);
            x_strand.push_back(an.strand[i]);
            x_gene.push_back(g);
            if (args.gene_rule_transcript) {
                int32_t &t = new_tr[(size_t)an.transcript[i]];
                if (t < 0) t = (int32_t)sum.annotation_transcripts++;
                x_tr.push_back(t);
            }
        }
        sum.annotation_genes = annotation_ids.size();
        sum.annotation_features = x_gene.size();
        // the reads the call sees: mapped, on a reference
        std::vector<uint32_t> cand;
        std::vector<uint64_t> c_off(1, 0);
        for (uint32_t ri = 0; ri < n_rec; ri++) {
            const umi::bam::Record &r = in.records[ri];
            if (r.is_unmapped() || r.tid() < 0) continue;
            cand.push_back(ri);
            c_off.push_back(c_off.back() + r.n_cigar());
        }
        const size_t nc = cand.size(), per = (nc + T - 1) / T;
        std::vector<int32_t> r_ref(nc), r_pos(nc), r_gene(nc);
        std::vector<uint8_t> r_rev(nc), r_status(nc);
        std::vector<uint32_t> words((size_t)c_off.back() + 1);
        umi::bgzf::parallel_for(T, T, [&](size_t t) {
            for (size_t j = t * per; j < std::min(nc, (t + 1) * per); j++) {
                const umi::bam::Record &r = in.records[cand[j]];
                r_ref[j] = r.tid();
                r_pos[j] = r.pos();
                r_rev[j] = r.is_reverse() ? 1 : 0;
                std::memcpy(&words[(size_t)c_off[j]], r.cigar(), 4 * (size_t)r.n_cigar());
            }
        });
        assigned_status.assign(n_rec, UMI_GENE_NONE);
        assigned_gene.assign(n_rec, -1);
        uint64_t counts[3] = {0, 0, 0};
        if (args.velocity) assigned_class.assign(n_rec, UMI_READ_CLASS_NONE);
        if (nc && args.transcript_introns_mode != UMI_INTRONS_OFF) { // --transcript-introns: transcripts first, bodies behind; --velocity: the classes too
            need_ctx();
            if (!lib.assign_genes_transcripts_classes) die("libumihip.so lacks umi_assign_genes_transcripts_classes");
            std::vector<uint8_t> r_tier(nc), r_class(args.velocity ? nc : 0);
            uint64_t by_tier[4] = {0, 0, 0, 0};
            if (lib.assign_genes_transcripts_classes(ctx, x_ref.data(), x_start.data(), x_end.data(), x_strand.data(), x_gene.data(),
                                                     x_tr.data(), x_gene.size(), (uint32_t)annotation_ids.size(),
                                                     (uint32_t)sum.annotation_transcripts, args.gene_strand_mode,
                                                     args.transcript_introns_mode, r_ref.data(), r_pos.data(), r_rev.data(), words.data(),
                                                     c_off.data(), nc, r_gene.data(), r_status.data(), r_tier.data(),
                                                     args.velocity ? r_class.data() : nullptr, by_tier,
                                                     args.velocity ? sum.class_counts : nullptr) != UMI_OK)
                die(lib.last_error());
            sum.by_exon = by_tier[0];
            sum.by_intron = by_tier[1];
            if (args.velocity)
                for (size_t j = 0; j < nc; j++) assigned_class[cand[j]] = r_class[j];
        } else if (nc && args.velocity) { // --velocity: the call that tells the classes too, in the two-tier call's place
            need_ctx();
            if (!lib.assign_genes_classes) die("libumihip.so lacks umi_assign_genes_classes");
            std::vector<uint8_t> r_tier(nc), r_class(nc);
            uint64_t by_tier[4] = {0, 0, 0, 0};
            if (lib.assign_genes_classes(ctx, x_ref.data(), x_start.data(), x_end.data(), x_strand.data(), x_gene.data(),
                                         x_gene.size(), (uint32_t)annotation_ids.size(), args.gene_strand_mode,
                                         args.gene_introns_mode, r_ref.data(), r_pos.data(), r_rev.data(), words.data(),
                                         c_off.data(), nc, r_gene.data(), r_status.data(), r_tier.data(), r_class.data(), by_tier,
                                         sum.class_counts) != UMI_OK)
                die(lib.last_error());
            sum.by_exon = by_tier[0];
            sum.by_intron = by_tier[1];
            for (size_t j = 0; j < nc; j++) assigned_class[cand[j]] = r_class[j];
        } else if (nc && args.gene_introns_mode != UMI_INTRONS_OFF) { // --gene-introns: the two-tier call in the plain one's place
            need_ctx();
            if (!lib.assign_genes_introns) die("libumihip.so lacks umi_assign_genes_introns");
            std::vector<uint8_t> r_tier(nc);
            uint64_t by_tier[4] = {0, 0, 0, 0};
            if (lib.assign_genes_introns(ctx, x_ref.data(), x_start.data(), x_end.data(), x_strand.data(), x_gene.data(),
                                         x_gene.size(), (uint32_t)annotation_ids.size(), args.gene_strand_mode,
                                         args.gene_introns_mode, r_ref.data(), r_pos.data(), r_rev.data(), words.data(),
                                         c_off.data(), nc, r_gene.data(), r_status.data(), r_tier.data(), by_tier) != UMI_OK)
                die(lib.last_error());
            sum.by_exon = by_tier[0];
            sum.by_intron = by_tier[1];
        } else if (nc && args.gene_rule_transcript) { // --gene-rule transcript: the transcript-model call in the plain one's place
            need_ctx();
            if (!lib.assign_genes_transcripts) die("libumihip.so lacks umi_assign_genes_transcripts");
            if (lib.assign_genes_transcripts(ctx, x_ref.data(), x_start.data(), x_end.data(), x_strand.data(), x_gene.data(), x_tr.data(),
                                             x_gene.size(), (uint32_t)annotation_ids.size(), (uint32_t)sum.annotation_transcripts,
                                             args.gene_strand_mode, r_ref.data(), r_pos.data(), r_rev.data(), words.data(), c_off.data(),
                                             nc, r_gene.data(), r_status.data(), counts) != UMI_OK)
                die(lib.last_error());
        } else if (nc) {
            need_ctx();
            if (!lib.assign_genes) die("libumihip.so lacks umi_assign_genes");
            if (lib.assign_genes(ctx, x_ref.data(), x_start.data(), x_end.data(), x_strand.data(), x_gene.data(), x_gene.size(),
                                 (uint32_t)annotation_ids.size(), args.gene_strand_mode, r_ref.data(), r_pos.data(), r_rev.data(),
                                 words.data(), c_off.data(), nc, r_gene.data(), r_status.data(), counts) != UMI_OK)
                die(lib.last_error());
        }
        for (size_t j = 0; j < nc; j++) {
            assigned_status[cand[j]] = r_status[j];
            assigned_gene[cand[j]] = r_gene[j];
        }
        lap("gene annotation");
    }

    // the UMI length, and where the reads are staged
    void choose_staging()
    {
        if (umi_length == 0 && !args.passthrough) // autodetect on the first staged read (:154-156)
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                uint8_t u, c;
                if (read_state(args, in.records[ri], u, c) == 0) {
                    ReadTags tg;
                    std::string err;
                    AssignedGene ag;
                    const uint8_t miss = read_tags(args, in.records[ri], tg, err, assigned(ri, ag)); // (a read without its tags is not staged)
                    if (!err.empty()) die(err);
                    if (miss || tg.several_genes) continue;
                    umi_length = detect_length(args, in.records[ri], tg);
                    break;
                }
            }
        // (where the reads are merged per (position, UMI): on the GPU unless something needs the host's
        // per-read bookkeeping -- decided here because the per-read pass only encodes UMIs for the host path)
        check_stage(args);
        gpu_stage = args.stage != "host" && !args.passthrough && !args.paired && !need_entries &&
                    args.dump_staging.empty() && umi_length >= 1;
        if (args.stage == "gpu" && !gpu_stage)
            die("--stage gpu does not go with --paired, --tag, --call-consensus, --velocity or --dump-staging");
    }

    // utils/mod.rs:63-83 for every staged read; the first bad character ends the run
    void encode_all()
    {
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
    }

    // ---- staging: deduplicate_sam.rs:93-177, in three passes so that --num-threads helps:
    //  A (parallel over records)  alignment key, UMI key, merge score of every read
    //  B (parallel over shards of the alignment-key hash; every shard walks the reads in
    //     file order)              per-bucket UMI maps with the reference's merge rule
    //  C (sequential)             buckets in order of first appearance, entries in rank order
    void per_read_pass()
    {
        info.resize(n_rec);
        fits.assign(T, 1);
        c_min.assign(T, INT64_MAX);
        c_max.assign(T, INT64_MIN);
        rs_max.assign(T, 0);
        if (gpu_stage) {
            akey.resize(n_rec);
            umis.resize((size_t)n_rec * umi_length);
            sc.resize(n_rec);
        }
        std::vector<std::string> errors(T);
        std::vector<uint32_t> first_error(T, UINT32_MAX);
        if (!args.cell_list.empty()) cell_raw.resize((size_t)n_rec * args.cell_len);
        if (args.cell_wl_multi) cell_qual.resize((size_t)n_rec * args.cell_len);
        // --per-cell: every thread numbers the barcodes of its reads in order of appearance; the numbers are
        // made global (first appearance in the file) below.  A few thousand to 10^5 barcodes: the tables stay
        // in cache.
        std::vector<std::unordered_map<std::string_view, uint32_t>> cell_ids(args.per_cell ? T : 0);
        cell_seen.assign(args.per_cell ? T : 0, {});
        std::vector<std::unordered_map<std::string_view, uint32_t>> gene_ids(args.per_gene ? T : 0); // --per-gene: likewise
        gene_seen.assign(args.per_gene ? T : 0, {});
        if (gpu_stage && (args.per_cell || args.per_gene)) gkey.resize(n_rec);
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
                ii.gene = 0;
                ii.state = read_state(args, r, ii.unpaired, ii.chimeric);
                if (ii.state != 0 || args.passthrough) continue;
                const AlignKey ak = args.per_gene ? AlignKey{0, 0, 0} : align_key(r, args.paired); // (--per-gene: no part)
                ii.coord = ak.coord;
                ii.ref_strand = ak.ref_strand;
                ii.tlen = ak.tlen;
                const uint8_t *q = r.qname();
                size_t at = 0;
                std::string err;
                ReadTags tg;
                if (!args.umi_tag.empty() || args.per_cell || args.per_gene) {
                    AssignedGene ag;
                    ii.missing = read_tags(args, r, tg, err, assigned(ri, ag));
                    if (ii.missing && err.empty()) {
                        ii.state = 6;
                        continue;
                    }
                    if (tg.several_genes && err.empty()) {
                        ii.state = 9;
                        continue;
                    }
                }
                if (err.empty()) err = umi_offset(args, r, tg, umi_length, at);
                if (!err.empty()) {
                    ii.state = 2;
                    if (first_error[t] == UINT32_MAX) { first_error[t] = ri; errors[t] = err; }
                    continue;
                }
                if (!args.cell_list.empty()) { // (numbered after the correction, below)
                    bool acgtn = tg.cell.size() == args.cell_len;
                    for (const char ch : tg.cell) acgtn = acgtn && (ch == 'A' || ch == 'C' || ch == 'G' || ch == 'T' || ch == 'N');
                    if (!acgtn) {
                        ii.state = 2;
                        if (first_error[t] == UINT32_MAX) {
                            first_error[t] = ri;
                            const std::string name((const char *)r.qname(), r.qname_len());
                            errors[t] = tg.cell.size() != args.cell_len
                                            ? "cell barcode tag " + args.cell_tag + " of read " + name + " holds " +
                                                  std::to_string(tg.cell.size()) + " bases, not " + std::to_string(args.cell_len)
                                            : "Unknown character in cell barcode tag " + args.cell_tag + " of read " + name;
                        }
                        continue;
                    }
                    std::memcpy(&cell_raw[(size_t)ri * args.cell_len], tg.cell.data(), args.cell_len);
                    if (args.cell_wl_multi) { // the qualities beside it: of the barcode's length, bytes 33..126
                        bool phred = tg.cell_qual.size() == args.cell_len;
                        for (const char ch : tg.cell_qual) phred = phred && (uint8_t)ch >= 33 && (uint8_t)ch <= 126;
                        if (!phred) {
                            ii.state = 2;
                            if (first_error[t] == UINT32_MAX) {
                                first_error[t] = ri;
                                const std::string name((const char *)r.qname(), r.qname_len());
                                errors[t] = tg.cell_qual.size() != args.cell_len
                                                ? "cell quality tag " + args.cell_qual_tag + " of read " + name + " holds " +
                                                      std::to_string(tg.cell_qual.size()) + " bytes, not " + std::to_string(args.cell_len)
                                                : "Unknown character in cell quality tag " + args.cell_qual_tag + " of read " + name;
                            }
                            continue;
                        }
                        std::memcpy(&cell_qual[(size_t)ri * args.cell_len], tg.cell_qual.data(), args.cell_len);
                    }
                } else if (args.per_cell) {
                    const auto id = cell_ids[t].emplace(tg.cell, (uint32_t)cell_seen[t].size());
                    if (id.second) cell_seen[t].push_back(tg.cell);
                    ii.cell = id.first->second;
                }
                if (args.per_gene) {
                    const auto id = gene_ids[t].emplace(tg.gene, (uint32_t)gene_seen[t].size());
                    if (id.second) gene_seen[t].push_back(tg.gene);
                    ii.gene = id.first->second;
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
    }

    // --cell-whitelist: the barcodes of the reads that would be staged, looked up in the list's index in one
    // call; a read whose barcode is unlisted or ambiguous is dropped like one without the tag, and the
    // others are numbered by their corrected barcode (rank of first appearance in the file)
    void correct_cells()
    {
        const std::vector<uint32_t> cand = candidates();
        const size_t nc = cand.size(), L = args.cell_len, n_wl = args.cell_list.size() / L;
        const umi::bgzf::Bytes raw = gather(cand, L, [&](uint32_t ri) { return &cell_raw[(size_t)ri * L]; });
        std::vector<int32_t> cb_match(nc);
        std::vector<uint8_t> cb_status(nc);
        if (nc && args.cell_wl_multi) { // ambiguous barcodes weighed by their candidates' exact reads and the qualities
            const umi::bgzf::Bytes qual = gather(cand, L, [&](uint32_t ri) { return &cell_qual[(size_t)ri * L]; });
            need_ctx();
            if (lib.correct_barcodes_multi(ctx, raw.data(), qual.data(), nc, (int)L, args.cell_list.data(), (uint32_t)n_wl,
                                           args.cell_wl_min_posterior, args.cell_wl_pseudocount, cb_match.data(), cb_status.data(),
                                           nullptr, sum.cb_counts) != UMI_OK)
                die(lib.last_error());
        } else if (nc) {
            need_ctx();
            if (lib.correct_barcodes(ctx, raw.data(), nc, (int)L, args.cell_list.data(), (uint32_t)n_wl, args.cell_wl_max_mismatches,
                                     cb_match.data(), cb_status.data(), sum.cb_counts) != UMI_OK)
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
            if (id == UINT32_MAX) {
                id = next_id++;
                cell_names.emplace_back((const char *)&args.cell_list[(size_t)cb_match[j] * L], L); // (the listed barcode)
            }
            ii.cell = id;
            if (gpu_stage) gkey[cand[j]] = id;
        }
        n_cells = next_id;
        if (!args.cell_whitelist_metrics.empty()) // per listed barcode that took a read, in list order
            write_list_metrics(args.cell_whitelist_metrics, "barcode", args.cell_list, L, cb_match, cb_status, true, args.cell_wl_multi);
        lap("cell whitelist");
    }

    // --per-cell without a list: the threads' barcode numbers -> ranks of first appearance in the file
    void number_cells()
    {
        std::unordered_map<std::string_view, uint32_t> global;
        std::vector<std::vector<uint32_t>> to_global(T);
        for (unsigned t = 0; t < T; t++)
            for (const std::string_view &bc : cell_seen[t])
                to_global[t].push_back(global.emplace(bc, (uint32_t)global.size()).first->second);
        n_cells = global.size();
        cell_names.resize(n_cells);
        for (const auto &g : global) cell_names[g.second] = g.first;
        umi::bgzf::parallel_for(T, T, [&](size_t t) {
            const uint32_t lo = (uint32_t)t * chunk, hi = std::min(n_rec, lo + chunk);
            for (uint32_t ri = lo; ri < hi; ri++)
                if (info[ri].state == 0) {
                    info[ri].cell = to_global[t][info[ri].cell];
                    if (gpu_stage) gkey[ri] = info[ri].cell;
                }
        });
    }

    // --per-gene: the threads' gene numbers -> ranks of first appearance among the reads that are staged (the
    // whitelists have dropped theirs), the threads' reads walked in file order; the device staging's group key is
    // cell | gene << bits_of(n_cells)
    void number_genes()
    {
        std::unordered_map<std::string_view, uint32_t> global;
        const int cell_bits = bits_of(n_cells);
        for (unsigned t = 0; t < T; t++) {
            std::vector<uint32_t> to_global(gene_seen[t].size(), UINT32_MAX);
            const uint32_t lo = t * chunk, hi = std::min(n_rec, lo + chunk);
            for (uint32_t ri = lo; ri < hi; ri++) {
                ReadInfo &ii = info[ri];
                if (ii.state != 0) continue;
                uint32_t &g = to_global[ii.gene];
                if (g == UINT32_MAX) {
                    const auto id = global.emplace(gene_seen[t][ii.gene], (uint32_t)gene_names.size());
                    if (id.second) gene_names.push_back(id.first->first);
                    g = id.first->second;
                }
                ii.gene = g;
                if (gpu_stage) gkey[ri] = (uint64_t)ii.cell | ((uint64_t)g << cell_bits);
            }
        }
        sum.n_genes = gene_names.size();
    }

    // --umi-whitelist: the UMIs of the reads that would be staged, snapped to the list in one call; a read
    // that matches no listed UMI is dropped like one without its tag, the others go on with the listed
    // UMI's bytes in place of their own (either staging below sees only those)
    void correct_umis()
    {
        const std::vector<uint32_t> cand = candidates();
        const size_t nc = cand.size(), L = umi_length;
        const umi::bgzf::Bytes raw_umis = gather(cand, L, [&](uint32_t ri) { return in.records[ri].qname() + info[ri].umi_at; });
        umi::bgzf::Bytes fixed(nc * L);
        const size_t per = (nc + T - 1) / T;
        std::vector<int32_t> wl_match(nc); // per staged read, in file order
        std::vector<uint8_t> wl_best(args.whitelist_metrics.empty() ? 0 : nc);
        if (nc) {
            need_ctx();
            if (lib.correct_umis(ctx, raw_umis.data(), nc, (int)L, args.whitelist.data(), (uint32_t)(args.whitelist.size() / L),
                                 args.wl_max_mismatches, args.wl_min_distance, fixed.data(), wl_match.data(),
                                 wl_best.empty() ? nullptr : wl_best.data(), nullptr, sum.wl_counts) != UMI_OK)
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
        if (!args.whitelist_metrics.empty()) // per listed UMI, in list order: the reads it took, exact and corrected
            write_list_metrics(args.whitelist_metrics, "umi", args.whitelist, L, wl_match, wl_best, false);
        lap("whitelist");
    }

    void count_reads()
    {
        for (uint32_t ri = 0; ri < n_rec; ri++) {
            if (info[ri].state != 3) sum.total_read_count++; // :99
            if (info[ri].state == 6) {
                sum.no_umi_tag += (info[ri].missing & MISS_UMI) ? 1 : 0;
                sum.no_cell += (info[ri].missing & MISS_CELL) ? 1 : 0;
                sum.no_gene += (info[ri].missing & MISS_GENE) ? 1 : 0;
            }
            if (info[ri].state == 9) sum.several_genes++;
            sum.unpaired += info[ri].unpaired;
            sum.chimeric += info[ri].chimeric;
            if (info[ri].state == 4) sum.unmapped++; // :118-121
            if (info[ri].state == 1) {
                sum.unmapped++;
                if (args.keep_unmapped || args.passthrough) out_records.push_back(ri);
            } else if (args.passthrough) {
                out_records.push_back(ri);
            }
        }
    }

    // ---- staging: reads -> unique (position, UMI) entries in canonical order (:148-176 and the
    // rank order of directional.rs:67-72).  On the GPU (umi_stage_reads: sorts and a segmented
    // merge) where the alignment key packs into 64 bits and nothing needs the per-read
    // bookkeeping of the host version below; both give the same arrays.
    void stage_on_gpu()
    {
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
        int akey_bits = args.per_gene ? 1 : 64; // (--per-gene: the alignment key is the constant 0, and the call refuses 0 bits)
        if (gpu_stage && ns && !args.per_gene) {
            const int64_t lo = *std::min_element(c_min.begin(), c_min.end()), hi = *std::max_element(c_max.begin(), c_max.end());
            const uint64_t rs_hi = *std::max_element(rs_max.begin(), rs_max.end());
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
        if (!gpu_stage) { // (a coordinate beyond 32 bits: the host staging takes the file)
            encode_all();
            return;
        }
        need_ctx();
        lap("wait-gpu");
        keys.resize(ns * n_words); nmask.resize(ns * n_words); freq.resize(ns); off.resize(ns + 1);
        uint64_t ne = 0, nbk = 0;
        const bool grouped = args.per_cell || args.per_gene;
        if (grouped && !lib.stage_reads_grouped) die("libumihip.so lacks umi_stage_reads_grouped_wide");
        const int group_bits = bits_of(n_cells) + (args.per_gene ? bits_of(sum.n_genes) : 0);
        const int rc = grouped
                           ? lib.stage_reads_grouped(ctx, akey.data(), akey_bits, gkey.data(), group_bits, umis.data(),
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
        for (size_t b = 0; b < nb; b++) max_umi = std::max<size_t>(max_umi, off[b + 1] - off[b]);
        lap("after-stage");
    }

    // the same arrays made on the host: deduplicate_sam.rs:148-176 per shard of the alignment-key hash
    void stage_on_host()
    {
        struct Shard {
            std::unordered_map<AlignKey, uint32_t, KeyHash> bucket_of; // Align -> local bucket
            std::vector<UmiIndex> umi_index;                           // per bucket: key -> entry of the shard
            std::vector<std::vector<uint32_t>> bucket_entries;
            std::vector<uint32_t> bucket_first; // first read of the bucket
            std::vector<Entry> entries;
        };
        std::vector<Shard> shards(args.passthrough ? 0 : T);
        entry_of.assign(need_entries ? n_rec : 0, 0); // read -> its entry (--tag, --call-consensus, --velocity): its shard's number first
        const KeyHash hasher;
        auto key_of = [&](const ReadInfo &ii) { return AlignKey{ii.coord, ii.ref_strand, ii.tlen, ii.cell, ii.gene}; };
        umi::bgzf::parallel_for(shards.size(), T, [&](size_t t) {
            Shard &sh = shards[t];
            for (uint32_t ri = 0; ri < n_rec; ri++) {
                const ReadInfo &ii = info[ri];
                if (ii.state != 0) continue;
                const AlignKey key = key_of(ii);
                if (hasher(key) % T != t) continue;
                auto it = sh.bucket_of.find(key);
                uint32_t b;
                if (it == sh.bucket_of.end()) {
                    b = (uint32_t)sh.bucket_entries.size();
                    sh.bucket_of.emplace(key, b);
                    sh.bucket_entries.emplace_back();
                    sh.umi_index.emplace_back();
                    sh.bucket_first.push_back(ri);
                } else {
                    b = it->second;
                }
                const uint32_t e = add_read(sh.umi_index[b], sh.entries, sh.bucket_entries[b], rkey[ri], rnm[ri], ii.score, ri, merge);
                if (need_entries) entry_of[ri] = e;
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
        for (size_t b = 0; b < nb; b++) {
            Shard &sh = shards[order[b].shard];
            std::vector<uint32_t> &v = sh.bucket_entries[order[b].local];
            emit_position(sh.entries, v, n_words, keys.data(), nmask.data(), freq.data(), w);
            for (uint32_t ei : v) rep[sh.entries[ei].index] = sh.entries[ei].rep;
            off[b + 1] = w;
            max_umi = std::max(max_umi, v.size());
        }
        // read -> entry: the shard's number becomes the entry's place in the arrays, once and for every later stage
        if (need_entries && !shards.empty())
            umi::bgzf::parallel_for(T, T, [&](size_t t) {
                for (uint32_t ri = (uint32_t)t * chunk; ri < std::min(n_rec, ((uint32_t)t + 1) * chunk); ri++)
                    if (info[ri].state == 0) entry_of[ri] = shards[hasher(key_of(info[ri])) % T].entries[entry_of[ri]].index;
            });
    }

    // --per-cell: a bucket is a (position, cell) group; the positions are counted as ever, and every
    // group's cell id (the rank of the barcode's first appearance) is what --dump-staging adds
    void count_positions()
    {
        for (size_t i = 0; i < n * n_words; i++) any_n |= nmask[i] != 0;
        sum.n = n;
        sum.nb = sum.n_positions = nb;
        sum.max_umi = max_umi;
        if (args.per_cell && !args.passthrough) {
            std::unordered_set<AlignKey, KeyHash> positions;
            bucket_cell.resize(nb);
            for (size_t b = 0; b < nb; b++) {
                const ReadInfo &ii = info[rep[off[b]]];
                positions.insert(AlignKey{ii.coord, ii.ref_strand, ii.tlen});
                bucket_cell[b] = ii.cell;
            }
            sum.n_positions = positions.size();
        }
        if (args.per_gene) {
            bucket_gene.resize(nb);
            for (size_t b = 0; b < nb; b++) bucket_gene[b] = info[rep[off[b]]].gene;
        }
        t_stage0 = now_s();
        std::fprintf(stderr, "UMI collapsing reading finished in %.3f seconds\n", t_stage0 - t_start); // :178-183
    }

    // test hook: staged hot-path input, no GPU touched
    void dump_staging()
    {
        FILE *f = std::fopen(args.dump_staging.c_str(), "wb");
        if (!f) die("cannot open " + args.dump_staging);
        const uint64_t hdr[4] = {n, nb, umi_length, (uint64_t)n_words};
        std::fwrite(hdr, 8, 4, f);
        if (n) { // (without entries data() may be null, which fwrite is not to be given)
            std::fwrite(keys.data(), 8, n * n_words, f); std::fwrite(nmask.data(), 8, n * n_words, f);
            std::fwrite(freq.data(), 4, n, f); std::fwrite(rep.data(), 4, n, f);
        }
        std::fwrite(off.data(), 8, nb + 1, f);
        if (args.per_cell) std::fwrite(bucket_cell.data(), 4, nb, f); // (--per-cell: every bucket's cell id)
        if (args.per_gene) std::fwrite(bucket_gene.data(), 4, nb, f); // (--per-gene: every bucket's gene id)
        std::fclose(f);
        sum.print(args, true);
    }

    // ---- the hot path: one batched call replaces the bucket loop :207-233
    void collapse()
    {
        lap("to-hot-path");
        kept.assign(n + 1, 0);
        root.resize(need_root ? n + 1 : 0);
        std::memset(&st, 0, sizeof(st));
        t_gpu0 = t_gpu1 = now_s();
        if (!args.passthrough && n) {
            need_ctx();
            // The reference accepts every --data value and always runs Naive
            // (deduplicate_sam.rs:210-213): the result -- and here the path -- is the same for all of them.
            t_gpu0 = now_s();
            if (lib.dedup(ctx, keys.data(), any_n ? nmask.data() : nullptr, n_words, freq.data(), off.data(), nb,
                          (int)umi_length, args.k, args.percentage, algo, 0 /* adjacency.rs:56 */,
                          kept.data(), need_root ? root.data() : nullptr, &st) != UMI_OK)
                die(lib.last_error());
            t_gpu1 = now_s();
        }
        // (the context is not put away: tearing the HIP runtime down costs a process that lives half
        // a second another 0.1 s, and the process ends below without running destructors)
    }

    // --umi-filtering multi-gene: the molecules of one cell that share their UMI across its genes, decided in one call
    // over the staged keys and freq and the collapse's kept[] and root[]
    void filter_multigene()
    {
        kept_filtered.assign(n + 1, 0);
        freq_filtered.assign(n + 1, 0);
        if (n) {
            need_ctx();
            if (!lib.filter_multigene) die("libumihip.so lacks umi_filter_multigene");
            const std::vector<uint32_t> one_group(args.per_cell ? 0 : nb, 0u);
            if (lib.filter_multigene(ctx, keys.data(), n_words, (int)umi_length, freq.data(), kept.data(), root.data(), off.data(), nb,
                                     args.per_cell ? bucket_cell.data() : one_group.data(), args.per_cell ? (uint32_t)n_cells : 1u,
                                     kept_filtered.data(), freq_filtered.data(), sum.mg_counts) != UMI_OK)
                die(lib.last_error());
        }
        n_survivors = st.n_kept - sum.mg_counts[1];
        lap("multi-gene filter");
    }

    // --count-matrix: molecules and reads per (cell, gene) in one call over the collapse's kept[] and the staged
    // freq[] (with --umi-filtering multi-gene: what the filter left of both, and only the pairs that still hold a
    // molecule), then the four files
    void count_matrix()
    {
        const uint32_t n_rows = (uint32_t)sum.n_genes, n_cols = args.per_cell ? (uint32_t)n_cells : 1u;
        std::vector<uint32_t> out_row(nb + 1), out_col(nb + 1), molecules(nb + 1);
        std::vector<uint64_t> reads(nb + 1);
        uint64_t nnz = 0;
        if (nb) {
            need_ctx();
            if (!lib.count_matrix) die("libumihip.so lacks umi_count_matrix");
            const std::vector<uint32_t> one_column(args.per_cell ? 0 : nb, 0u);
            if (lib.count_matrix(ctx, survivors().data(), args.filter_multigene ? freq_filtered.data() : freq.data(), off.data(), nb,
                                 bucket_gene.data(), args.per_cell ? bucket_cell.data() : one_column.data(), n_rows, n_cols,
                                 out_row.data(), out_col.data(), molecules.data(), reads.data(), &nnz) != UMI_OK)
                die(lib.last_error());
        }
        auto write = [&](const char *name, const std::string &text) {
            const std::string path = args.count_matrix + "/" + name;
            FILE *f = std::fopen(path.c_str(), "wb");
            if (!f) die("cannot open " + path);
            const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
            if (std::fclose(f) != 0 || !ok) die("cannot write " + path);
        };
        std::string text = features_text();
        write("features.tsv", text);
        text.clear();
        if (!args.per_cell) text = "all\n";
        for (size_t c = 0; c < n_cols && args.per_cell; c++) text.append(cell_names[c]).append("\n");
        write("barcodes.tsv", text);
        uint64_t lines = nnz;
        if (args.filter_multigene) lines = (uint64_t)std::count_if(molecules.begin(), molecules.begin() + nnz, [](uint32_t m) { return m != 0; });
        const std::string head = "%%MatrixMarket matrix coordinate integer general\n" + std::to_string(n_rows) + " " +
                                 std::to_string(n_cols) + " " + std::to_string(lines) + "\n";
        std::string mol = head, rd = head;
        for (uint64_t i = 0; i < nnz; i++) {
            if (args.filter_multigene && molecules[i] == 0) continue; // (a pair whose molecules were all removed)
            const std::string at = std::to_string(out_row[i] + 1) + " " + std::to_string(out_col[i] + 1) + " ";
            mol.append(at).append(std::to_string(molecules[i])).append("\n");
            rd.append(at).append(std::to_string(reads[i])).append("\n");
        }
        write("matrix.mtx", mol);
        write("reads.mtx", rd);
        lap("count matrix");
        std::vector<uint32_t> v_row, v_col, layer[3];
        uint64_t v_nnz = 0;
        if (args.velocity) velocity_matrix(n_rows, n_cols, v_row, v_col, layer, v_nnz, write);
        if (args.cell_filter_given) {
            if (args.filter_multigene) { // (what matrix.mtx holds: the pairs that still have a molecule)
                uint64_t w = 0;
                for (uint64_t i = 0; i < nnz; i++) {
                    if (molecules[i] == 0) continue;
                    out_row[w] = out_row[i], out_col[w] = out_col[i], molecules[w] = molecules[i], reads[w] = reads[i];
                    w++;
                }
                nnz = w;
            }
            call_cells(n_rows, n_cols, out_row, out_col, molecules, reads, nnz, write);
            if (args.velocity) { // the layers of the called cells, their columns renumbered as DIR/filtered's
                uint64_t w = 0;
                for (uint64_t i = 0; i < v_nnz; i++) {
                    if (called_col[v_col[i]] == UINT32_MAX) continue;
                    v_row[w] = v_row[i], v_col[w] = called_col[v_col[i]];
                    for (auto &l : layer) l[w] = l[i];
                    w++;
                }
                write_layers("velocity/filtered/", n_rows, (uint32_t)sum.cell_counts[1], v_row, v_col, layer, w, write);
            }
        }
        if (!args.saturation_curve.empty()) saturation_curve(n_rows, n_cols);
        if (args.junction_matrix) junction_matrix(n_cols, write);
    }

    // --junction-matrix: molecules and reads per (cell, junction) in one call over the staged reads' reference, position,
    // CIGAR words and entry, the mask the matrix was counted from, root[] and the buckets' cell; then DIR/junctions' four
    // files and, for the called cells, DIR/junctions/filtered's (cli.hpp has the rule and the files)
    void junction_matrix(uint32_t n_cols, const std::function<void(const char *, const std::string &)> &write)
    {
        std::vector<uint32_t> cand;
        std::vector<uint64_t> c_off(1, 0);
        uint64_t capacity = 0; // the N words among them: no read has more junctions than N words
        for (uint32_t ri = 0; ri < n_rec; ri++) {
            const umi::bam::Record &r = in.records[ri];
            if (info[ri].state != 0 || r.is_unmapped() || r.tid() < 0) continue;
            cand.push_back(ri);
            c_off.push_back(c_off.back() + r.n_cigar());
        }
        const size_t nc = cand.size();
        std::vector<int32_t> r_ref(nc + 1), r_pos(nc + 1);
        std::vector<uint32_t> r_entry(nc + 1), words((size_t)c_off.back() + 1);
        for (size_t j = 0; j < nc; j++) {
            const umi::bam::Record &r = in.records[cand[j]];
            r_ref[j] = r.tid();
            r_pos[j] = r.pos();
            r_entry[j] = entry_of[cand[j]];
            std::memcpy(&words[(size_t)c_off[j]], r.cigar(), 4 * (size_t)r.n_cigar());
            for (uint64_t w = c_off[j]; w < c_off[j + 1]; w++) capacity += (words[(size_t)w] & 15u) == 3u;
        }
        const size_t cap = (size_t)capacity + 1;
        std::vector<int32_t> jn_ref(cap), jn_start(cap), jn_end(cap);
        std::vector<uint32_t> o_jn(cap), o_col(cap), o_mol(cap);
        std::vector<uint64_t> o_reads(cap);
        uint64_t *counts = sum.junction_counts;
        if (nb && nc) {
            need_ctx();
            if (!lib.junction_matrix) die("libumihip.so lacks umi_junction_matrix");
            const std::vector<uint32_t> one_column(args.per_cell ? 0 : nb, 0u);
            if (lib.junction_matrix(ctx, r_ref.data(), r_pos.data(), words.data(), c_off.data(), r_entry.data(), nc, survivors().data(),
                                    root.data(), off.data(), nb, args.per_cell ? bucket_cell.data() : one_column.data(), n_cols, capacity,
                                    jn_ref.data(), jn_start.data(), jn_end.data(), o_jn.data(), o_col.data(), o_mol.data(),
                                    o_reads.data(), counts) != UMI_OK)
                die(lib.last_error());
        }
        // the references' names, from the header
        std::vector<std::string_view> ref_names;
        {
            const uint8_t *p = in.data.data();
            size_t q = 8 + (size_t)umi::bam::rd_i32(p + 4) + 4;
            for (int32_t r = 0; r < in.n_ref; r++) {
                const size_t l_name = (size_t)umi::bam::rd_i32(p + q);
                std::string_view name((const char *)p + q + 4, l_name);
                if (!name.empty() && name.back() == '\0') name.remove_suffix(1);
                ref_names.push_back(name);
                q += 4 + l_name + 4;
            }
        }
        // a directory's four files: the junctions `rows` of the table in this order, the triplets [0, nnz) with their
        // junctions numbered by `row_of`
        auto files = [&](const std::string &dir, const std::vector<uint32_t> &rows, const std::vector<uint32_t> &row_of, uint32_t cols,
                         bool filtered, uint64_t nnz) {
            std::string text;
            for (const uint32_t j : rows) {
                const int32_t ref = jn_ref[j];
                text.append(ref < (int32_t)ref_names.size() ? ref_names[(size_t)ref] : std::string_view("*")).append("\t");
                text.append(std::to_string((int64_t)jn_start[j] + 1)).append("\t").append(std::to_string(jn_end[j])).append("\n");
            }
            write((dir + "features.tsv").c_str(), text);
            text.clear();
            if (!args.per_cell) text = "all\n";
            for (size_t c = 0; c < cell_names.size() && args.per_cell; c++)
                if (!filtered || called_col[c] != UINT32_MAX) text.append(cell_names[c]).append("\n");
            write((dir + "barcodes.tsv").c_str(), text);
            const std::string head = "%%MatrixMarket matrix coordinate integer general\n" + std::to_string(rows.size()) + " " +
                                     std::to_string(cols) + " " + std::to_string(nnz) + "\n";
            std::string mol = head, rd = head;
            for (uint64_t i = 0; i < nnz; i++) {
                const std::string at = std::to_string(row_of[o_jn[i]] + 1) + " " + std::to_string(o_col[i] + 1) + " ";
                mol.append(at).append(std::to_string(o_mol[i])).append("\n");
                rd.append(at).append(std::to_string(o_reads[i])).append("\n");
            }
            write((dir + "matrix.mtx").c_str(), mol);
            write((dir + "reads.mtx").c_str(), rd);
        };
        const size_t n_jn = (size_t)counts[2];
        std::vector<uint32_t> rows(n_jn), row_of(n_jn + 1, 0);
        for (size_t j = 0; j < n_jn; j++) rows[j] = row_of[j] = (uint32_t)j;
        files("junctions/", rows, row_of, n_cols, false, counts[3]);
        if (args.cell_filter_given) { // the called cells: their columns as DIR/filtered's, the junctions they still have
            std::vector<uint8_t> used(n_jn + 1, 0);
            uint64_t w = 0;
            for (uint64_t i = 0; i < counts[3]; i++) {
                if (o_col[i] >= called_col.size() || called_col[o_col[i]] == UINT32_MAX) continue;
                o_jn[w] = o_jn[i], o_col[w] = called_col[o_col[i]], o_mol[w] = o_mol[i], o_reads[w] = o_reads[i];
                used[o_jn[w]] = 1;
                w++;
            }
            rows.clear();
            for (size_t j = 0; j < n_jn; j++)
                if (used[j]) {
                    row_of[j] = (uint32_t)rows.size();
                    rows.push_back((uint32_t)j);
                }
            files("junctions/filtered/", rows, row_of, (uint32_t)sum.cell_counts[1], true, w);
        }
        lap("junction matrix");
    }

    // --saturation-curve: reads, molecules, pairs and the medians of the selected cells at every depth, in one call over
    // every read's entry (as --velocity builds it: a read's index is its record's number), the mask the matrix was
    // counted from, root[] and the buckets' gene and cell; the selected cells are --cell-filter's called ones, and
    // without that flag every column with a molecule.  Then FILE (cli.hpp has its layout)
    void saturation_curve(uint32_t n_rows, uint32_t n_cols)
    {
        const int L = args.saturation_points;
        std::vector<uint64_t> curve((size_t)L * 8, 0);
        if (nb) {
            need_ctx();
            if (!lib.saturation_curve) die("libumihip.so lacks umi_saturation_curve");
            std::vector<uint32_t> read_entry(n_rec);
            for (uint32_t ri = 0; ri < n_rec; ri++) read_entry[ri] = info[ri].state == 0 ? entry_of[ri] : UMI_READ_UNSTAGED;
            const std::vector<uint32_t> one_column(args.per_cell ? 0 : nb, 0u);
            std::vector<uint8_t> cell_mask;
            if (args.cell_filter_given) {
                cell_mask.assign((size_t)n_cols + 1, 0);
                for (size_t c = 0; c < called_col.size() && c < n_cols; c++) cell_mask[c] = called_col[c] != UINT32_MAX;
            }
            if (lib.saturation_curve(ctx, read_entry.data(), n_rec, survivors().data(), root.data(), off.data(), nb, bucket_gene.data(),
                                     args.per_cell ? bucket_cell.data() : one_column.data(), n_rows, n_cols, args.saturation_seed, L,
                                     args.cell_filter_given ? cell_mask.data() : nullptr, curve.data()) != UMI_OK)
                die(lib.last_error());
        }
        std::string text = "depth\treads\tmolecules\tsaturation\tpairs\tcells\tmolecules_in_cells\tpairs_in_cells\tmedian_molecules\tmedian_genes\n";
        for (int j = 0; j < L; j++) {
            const uint64_t *c = &curve[(size_t)j * 8];
            text.append(std::to_string(j + 1)).append("/").append(std::to_string(L)).append("\t");
            text.append(std::to_string(c[0])).append("\t").append(std::to_string(c[1])).append("\t");
            text.append(Summary::saturation_text(c[0], c[1]));
            for (int k = 2; k < 8; k++) text.append("\t").append(std::to_string(c[k]));
            text.append("\n");
        }
        FILE *f = std::fopen(args.saturation_curve.c_str(), "wb");
        if (!f) die("cannot open " + args.saturation_curve);
        const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
        if (std::fclose(f) != 0 || !ok) die("cannot write " + args.saturation_curve);
        sum.saturation_reads = curve[(size_t)(L - 1) * 8];
        sum.saturation_molecules = curve[(size_t)(L - 1) * 8 + 1];
        lap("saturation curve");
    }

    // --velocity: the three layers of the matrix's triplets in one call over every read's entry and class, the mask
    // the matrix was counted from, root[] and the buckets' gene and cell; then DIR/velocity's five files
    using Write = std::function<void(const char *, const std::string &)>;
    std::vector<uint32_t> called_col; // --cell-filter: per column its number among the called cells, UINT32_MAX: not called
    void velocity_matrix(uint32_t n_rows, uint32_t n_cols, std::vector<uint32_t> &v_row, std::vector<uint32_t> &v_col,
                         std::vector<uint32_t> (&layer)[3], uint64_t &v_nnz, const Write &write)
    {
        v_row.assign(nb + 1, 0);
        v_col.assign(nb + 1, 0);
        for (auto &l : layer) l.assign(nb + 1, 0);
        if (nb) {
            need_ctx();
            if (!lib.velocity_matrix) die("libumihip.so lacks umi_velocity_matrix");
            std::vector<uint32_t> read_entry(n_rec);
            for (uint32_t ri = 0; ri < n_rec; ri++) read_entry[ri] = info[ri].state == 0 ? entry_of[ri] : UMI_READ_UNSTAGED;
            const std::vector<uint32_t> one_column(args.per_cell ? 0 : nb, 0u);
            if (lib.velocity_matrix(ctx, read_entry.data(), assigned_class.data(), n_rec, survivors().data(), root.data(), off.data(), nb,
                                    bucket_gene.data(), args.per_cell ? bucket_cell.data() : one_column.data(), n_rows, n_cols,
                                    v_row.data(), v_col.data(), layer[0].data(), layer[1].data(), layer[2].data(), &v_nnz) != UMI_OK)
                die(lib.last_error());
        }
        for (int k = 0; k < 3; k++)
            for (uint64_t i = 0; i < v_nnz; i++) sum.layers[k] += layer[k][i];
        write_layers("velocity/", n_rows, n_cols, v_row, v_col, layer, v_nnz, write);
        lap("velocity matrix");
    }

    // features.tsv and barcodes.tsv as their directory's parent has them, and a layer per file, each with its non-zero entries alone
    void write_layers(const std::string &dir, uint32_t n_rows, uint32_t n_cols, const std::vector<uint32_t> &row,
                      const std::vector<uint32_t> &col, const std::vector<uint32_t> (&layer)[3], uint64_t nnz, const Write &write)
    {
        const bool filtered = dir != "velocity/";
        write((dir + "features.tsv").c_str(), features_text());
        std::string text;
        if (!args.per_cell) text = "all\n";
        for (size_t c = 0; c < cell_names.size() && args.per_cell; c++)
            if (!filtered || called_col[c] != UINT32_MAX) text.append(cell_names[c]).append("\n");
        write((dir + "barcodes.tsv").c_str(), text);
        const char *names[3] = {"spliced.mtx", "unspliced.mtx", "ambiguous.mtx"};
        for (int k = 0; k < 3; k++) {
            const uint64_t lines = (uint64_t)std::count_if(layer[k].begin(), layer[k].begin() + nnz, [](uint32_t m) { return m != 0; });
            text = "%%MatrixMarket matrix coordinate integer general\n" + std::to_string(n_rows) + " " + std::to_string(n_cols) + " " +
                   std::to_string(lines) + "\n";
            for (uint64_t i = 0; i < nnz; i++)
                if (layer[k][i])
                    text.append(std::to_string(row[i] + 1)).append(" ").append(std::to_string(col[i] + 1)).append(" ")
                        .append(std::to_string(layer[k][i])).append("\n");
            write((dir + names[k]).c_str(), text);
        }
    }

    // --cell-filter: which cells of the matrix are called, in one call over its triplets, then DIR/filtered/'s four
    // files and DIR/cells.tsv
    void call_cells(uint32_t n_rows, uint32_t n_cols, const std::vector<uint32_t> &row, const std::vector<uint32_t> &col,
                    const std::vector<uint32_t> &molecules, const std::vector<uint64_t> &reads, uint64_t nnz,
                    const std::function<void(const char *, const std::string &)> &write)
    {
        std::vector<uint64_t> cell_molecules(n_cols + 1, 0), cell_reads(n_cols + 1, 0), f_reads(nnz + 1);
        std::vector<uint32_t> cell_genes(n_cols + 1, 0), new_col(n_cols + 1, UINT32_MAX), f_row(nnz + 1), f_col(nnz + 1), f_mol(nnz + 1);
        std::vector<uint8_t> called(n_cols + 1, 0);
        uint64_t f_nnz = 0;
        if (nnz) {
            need_ctx();
            if (!lib.call_cells) die("libumihip.so lacks umi_call_cells");
            if (lib.call_cells(ctx, row.data(), col.data(), molecules.data(), reads.data(), nnz, n_rows, n_cols, args.cell_filter_rule,
                               args.expect_cells, args.cell_filter_permille, args.cell_filter_ratio, args.cell_min_molecules,
                               cell_molecules.data(), cell_reads.data(), cell_genes.data(), called.data(), new_col.data(), f_row.data(),
                               f_col.data(), f_mol.data(), f_reads.data(), &f_nnz, sum.cell_counts) != UMI_OK)
                die(lib.last_error());
        }
        std::string text = features_text();
        write("filtered/features.tsv", text);
        text.clear();
        std::string table = "barcode\treads\tmolecules\tgenes\tcalled\n";
        for (size_t c = 0; c < n_cols; c++) {
            if (called[c]) text.append(cell_names[c]).append("\n");
            if (cell_molecules[c] == 0) continue; // (no candidate)
            table.append(cell_names[c]).append("\t").append(std::to_string(cell_reads[c])).append("\t");
            table.append(std::to_string(cell_molecules[c])).append("\t").append(std::to_string(cell_genes[c]));
            table.append(called[c] ? "\t1\n" : "\t0\n");
        }
        write("filtered/barcodes.tsv", text);
        write("cells.tsv", table);
        const std::string head = "%%MatrixMarket matrix coordinate integer general\n" + std::to_string(n_rows) + " " +
                                 std::to_string(sum.cell_counts[1]) + " " + std::to_string(f_nnz) + "\n";
        std::string mol = head, rd = head;
        for (uint64_t i = 0; i < f_nnz; i++) {
            const std::string at = std::to_string(f_row[i] + 1) + " " + std::to_string(f_col[i] + 1) + " ";
            mol.append(at).append(std::to_string(f_mol[i])).append("\n");
            rd.append(at).append(std::to_string(f_reads[i])).append("\n");
        }
        write("filtered/matrix.mtx", mol);
        write("filtered/reads.mtx", rd);
        called_col.assign(new_col.begin(), new_col.begin() + n_cols);
        for (size_t c = 0; c < n_cols; c++)
            if (!called[c]) called_col[c] = UINT32_MAX;
        lap("cell filter");
    }

    // --output-stats: family sizes, UMI distances and UMI usage in one call over the staged keys and freq and the
    // collapse's kept[] and root[], then the three files
    void output_stats()
    {
        const size_t L = umi_length;
        uint64_t most = 0; // the largest bucket's reads: no total is larger
        for (size_t b = 0; b < nb; b++) {
            uint64_t reads = 0;
            for (uint64_t i = off[b]; i < off[b + 1]; i++) reads += (uint64_t)freq[i];
            most = std::max(most, reads);
        }
        const uint32_t bins = (uint32_t)std::min<uint64_t>(1u << 22, 2 + most);
        std::vector<uint64_t> count_pre(bins, 0), count_post(bins, 0), dist(4 * (L + 2), 0), reads_pre(n + 1), reads_post(n + 1);
        std::vector<uint32_t> umi_entry(n + 1), times_pre(n + 1), times_post(n + 1);
        uint64_t rows = 0;
        if (n) {
            need_ctx();
            if (!lib.dedup_stats) die("libumihip.so lacks umi_dedup_stats");
            if (lib.dedup_stats(ctx, keys.data(), n_words, freq.data(), kept.data(), root.data(), off.data(), nb, (int)L,
                                args.output_stats_seed, bins, count_pre.data(), count_post.data(), dist.data(), umi_entry.data(),
                                times_pre.data(), reads_pre.data(), times_post.data(), reads_post.data(), &rows) != UMI_OK)
                die(lib.last_error());
        }
        const std::vector<std::string> paths = output_stats_paths(args);
        auto write = [&](const std::string &path, const std::string &text) {
            FILE *f = std::fopen(path.c_str(), "wb");
            if (!f) die("cannot open " + path);
            const bool ok = std::fwrite(text.data(), 1, text.size(), f) == text.size();
            if (std::fclose(f) != 0 || !ok) die("cannot write " + path);
        };
        std::string text = "counts\tinstances_pre\tinstances_post\n";
        for (uint32_t c = 0; c < bins; c++)
            if (count_pre[c] || count_post[c])
                text.append(std::to_string(c)).append(c == bins - 1 ? "+" : "").append("\t").append(std::to_string(count_pre[c]))
                    .append("\t").append(std::to_string(count_post[c])).append("\n");
        write(paths[0], text);
        text = "edit_distance\tunique\tunique_null\t" + args.algo + "\t" + args.algo + "_null\n";
        for (size_t j = 0; j < L + 2; j++) {
            text.append(j <= L ? std::to_string(j) : std::string("Single_UMI"));
            for (size_t r = 0; r < 4; r++) text.append("\t").append(std::to_string(dist[r * (L + 2) + j]));
            text.append("\n");
        }
        write(paths[1], text);
        text = "UMI\ttimes_observed_pre\ttotal_counts_pre\ttimes_observed_post\ttotal_counts_post\n";
        for (uint64_t j = 0; j < rows; j++) {
            const uint64_t *k = &keys[(size_t)umi_entry[j] * n_words];
            for (size_t b = 0; b < L; b++) { // the 3-bit code at bits [3b, 3b + 3) of the key as one little-endian integer
                const size_t w = 3 * b / 64, sh = 3 * b % 64;
                uint64_t c = k[w] >> sh;
                if (sh > 61 && w + 1 < (size_t)n_words) c |= k[w + 1] << (64 - sh);
                text.push_back("A??GNTC?"[c & 7]);
            }
            text.append("\t").append(std::to_string(times_pre[j])).append("\t").append(std::to_string(reads_pre[j])).append("\t")
                .append(std::to_string(times_post[j])).append("\t").append(std::to_string(reads_post[j])).append("\n");
        }
        write(paths[2], text);
        lap("output stats");
    }

    // --tag, --call-consensus: cluster id / size per entry from the root of every entry.  Survivors in index
    // order are the roots in the order ClusterTracker::track sees them (bucket by bucket,
    // rank order inside), so offset + idx (cluster_tracker.rs:88-100, deduplicate_sam.rs:215)
    // is the running survivor count.
    void number_clusters()
    {
        cluster_id.assign(n, 0);
        cluster_reads.assign(n, 0);
        for (size_t i = 0; i < n; i++)
            if (kept[i]) cluster_id[i] = n_clusters++;
        for (size_t i = 0; i < n; i++) cluster_reads[root[i]] += (uint32_t)freq[i]; // temp_freq, :83-85
        staged_reads = candidates();
    }

    // the records to write, in output order; --tag writes every staged read instead (write_tagged)
    void select_records()
    {
        if (args.track_clusters) return;
        if (args.paired) return select_paired();
        const std::vector<uint8_t> &mask = survivors();
        for (size_t i = 0; i < n; i++)
            if (mask[i]) out_records.push_back(rep[i]); // :227-231, in rank order per bucket
    }

    // UcWriter (:382-459): every written paired record leaves (qname, mate ref, mate pos)
    // in a set; when the reference name of the written records changes, and once at the
    // end, the input is scanned again in file order and the second mates found in the set
    // are written.  The file is in memory here, so the scans walk record indices (per
    // reference for the partial passes).  The reference's set hashes the coordinate but
    // compares only names (:288-296); here the coordinate is part of the identity.
    // (--two-pass writes its pairs otherwise -- TwoPass::flush_mates, over a stream and behind a reorder buffer:
    // a different algorithm, not a copy of this one)
    void select_paired()
    {
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
    void call_consensus()
    {
        cons.entry_of_out.assign(out_records.size(), UINT32_MAX);
        const uint32_t nc = n_clusters;
        {
            size_t o = out_records.size();
            for (size_t i = n; i-- > 0;)
                if (kept[i]) cons.entry_of_out[--o] = (uint32_t)i; // (the kept entries are the last records written)
        }
        cons.clen.assign(nc, 0);
        for (size_t i = 0; i < n; i++) {
            if (!kept[i]) continue;
            const umi::bam::Record &rr = in.records[rep[i]];
            const bool can = rr.l_seq() > 0 && rr.qual()[0] != 0xFF;
            cons.clen[cluster_id[i]] = can ? (uint32_t)rr.l_seq() : 0u;
            if (!can) sum.n_without++;
        }
        std::vector<uint64_t> pos;   // seq_pos, then qual_pos, of the staged reads
        std::vector<uint32_t> rlen, rcluster;
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
            const uint32_t rt = root[entry_of[ri]];
            const umi::bam::Record &rr = in.records[rep[rt]];
            const uint32_t c = cluster_id[rt];
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
    void write_output()
    {
        lap("hot-path+select");
        if (args.call_consensus) write_consensus();
        else if (!args.track_clusters || args.passthrough || staged_reads.empty()) write_pieces(); // (--passthrough: as they are)
        else write_tagged();
        lap("write");
    }

    // --call-consensus: the kept records rebuilt around their cluster's consensus
    void write_consensus()
    {
        size_t out_len = in.header_len;
        for (uint32_t ri : out_records) out_len += (size_t)(in.records[ri].end - in.records[ri].begin) + TAG_BYTES;
        umi::bgzf::Bytes out(out_len);
        std::memcpy(out.data(), in.data.data(), in.header_len);
        size_t o = in.header_len;
        for (size_t j = 0; j < out_records.size(); j++) {
            const umi::bam::Record &r = in.records[out_records[j]];
            const size_t len = (size_t)(r.end - r.begin);
            const uint32_t e = cons.entry_of_out[j];
            const uint32_t c = e == UINT32_MAX ? 0u : cluster_id[e];
            if (e == UINT32_MAX || cons.clen[c] == 0) { // (a kept unmapped read; a cluster without a consensus)
                std::memcpy(out.data() + o, r.begin, len);
                o += len;
                continue;
            }
            if (cons.depth[c] < args.call_consensus_min_reads) {
                sum.n_below++;
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
            o = append_int_tags(out, o,
                                {{"cD", (int32_t)cons.depth[c]}, {"cs", (int32_t)cluster_reads[e]}, {"ce", (int32_t)cons.disagree[c]}});
        }
        umi::bgzf::compress_to_file(args.output, out.data(), o, args.num_threads, args.compress_level);
    }

    void write_pieces()
    {
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
    }

    // --tag: what was written before the deduplication, then every staged read with its cluster's tags
    void write_tagged()
    {
        size_t out_len = in.header_len;
        for (uint32_t ri : out_records) out_len += (size_t)(in.records[ri].end - in.records[ri].begin);
        for (uint32_t ri : staged_reads) out_len += (size_t)(in.records[ri].end - in.records[ri].begin) + TAG_BYTES;
        umi::bgzf::Bytes out(out_len);
        std::memcpy(out.data(), in.data.data(), in.header_len);
        size_t o = in.header_len;
        for (uint32_t ri : out_records) {
            const size_t len = (size_t)(in.records[ri].end - in.records[ri].begin);
            std::memcpy(out.data() + o, in.records[ri].begin, len);
            o += len;
        }
        for (uint32_t ri : staged_reads) {
            const size_t len = (size_t)(in.records[ri].end - in.records[ri].begin);
            std::memcpy(out.data() + o, in.records[ri].begin, len);
            const int32_t block_size = (int32_t)(len - 4 + TAG_BYTES);
            std::memcpy(out.data() + o, &block_size, 4);
            o += len;
            const uint32_t e = entry_of[ri], r = root[e];
            o = append_int_tags(out, o, {{"MI", (int32_t)cluster_id[r]}, {"cs", (int32_t)cluster_reads[r]}, {"su", freq[e]}});
        }
        umi::bgzf::compress_to_file(args.output, out.data(), out.size(), args.num_threads, args.compress_level);
    }

    void print_summary()
    {
        const double t_end = now_s();
        sum.n_kept = args.filter_multigene ? n_survivors : st.n_kept;
        sum.print(args);
        std::fprintf(stderr,
                     "phases: read+inflate %.3f s, staging (%s) %.3f s, gpu init %.3f s, hot path (H2D+GPU+D2H) %.3f s [%llu pairs], write %.3f s\n",
                     t_read - t_start, gpu_stage ? "gpu" : "host", t_stage0 - t_read - (gpu_stage ? gpu.t_init : 0.0), gpu.t_init,
                     t_gpu1 - t_gpu0, (unsigned long long)st.n_pairs, t_end - t_gpu1);
        std::fprintf(stderr, "UMI collapsing finished in %.3f seconds\n", t_end - t_start); // main.rs:97-102
    }
};

} // namespace

int main(int argc, char **argv)
{
    const double t_main_realtime = std::chrono::duration<double>(std::chrono::system_clock::now().time_since_epoch()).count();
    Cli args = parse(argc, argv);
    const double t_start = now_s();
    if (!validate(args)) return 0;
    HipLib lib(args);
    GpuWarmup gpu(lib, args.devices);
    try {
        if (args.mode == "fastq") return run_fastq(args, lib, gpu); // (this build's definition, see run_fastq)
        // (the warm-up thread starts before the input is read, and opens libumihip.so itself)
        if (!args.passthrough && args.dump_staging.empty()) gpu.start(false, 0);
        Clock clock(t_main_realtime);
        if (args.two_pass && !args.passthrough && args.dump_staging.empty()) { // (those two keep the one-pass behaviour)
            run_two_pass(args, lib, gpu, clock, t_start);
            clock.leave(gpu);
        }
        return OnePass(args, lib, gpu, clock, t_start).run();
    } catch (const std::exception &e) {
        die(e.what());
    }
}
