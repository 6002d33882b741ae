// `umicollapse`'s command line: the flags (Cli, parse, usage), the refusals that need no input file
// (validate) and the lists the flags name (read_whitelist).
//
// --algo cluster (every mode that takes --algo; umi_tools' --method cluster, STARsolo's 1MM_All at -k 1, what the
// reference's help calls `cc` and its main() refuses): one UMI per connected component of "within -k", the
// component's first in rank order; -p is accepted and plays no part (UMI_ALGO_CLUSTER, include/umihip.h).  `cc`
// itself stays refused with the reference's message.
// --per-gene [--gene-tag XX] (bam/sam mode, one pass; umi_tools --per-gene / STARsolo's grouping, not the
// reference's, tests/gene_model.py defines it): reads are grouped by gene -- with --per-cell by (cell, gene) --
// and not by alignment position (staging.hpp has the rule, umicollapse_main.cpp the pipeline).
// --count-matrix DIR (with --per-gene): the molecules per cell and gene, written to DIR as features.tsv,
// barcodes.tsv, matrix.mtx and reads.mtx.  DIR is made here, while the flags are looked at (its parent must be
// there; a directory that is there is used).  Refused with status 101 before the GPU is woken, each with a
// message of its own: --per-gene with fastq mode, --two-pass, --paired, --keep-unmapped, --tag, --call-consensus
// or --passthrough; --gene-tag without --per-gene, or not a tag name of two characters; --count-matrix without
// --per-gene, with --dump-staging, or a DIR that cannot be made.
// --output-stats PREFIX [--output-stats-seed S] (bam/sam mode, one pass; umi_tools dedup --output-stats, not the
// reference's, tests/stats_model.py defines it): after the collapse one call to umi_dedup_stats (include/umihip.h)
// over the staged keys and freq and the collapse's kept[] and root[] -- asked of the collapse for the flag, which alone
// does not move --stage auto to the host -- and three tab-separated files, uncompressed, lines ended by \n:
// PREFIX_per_umi_per_position.tsv ("counts instances_pre instances_post": how many entries had that many reads before,
// how many kept entries stand for that many after; a row per count with a non-zero instance, ascending; hist_bins is
// min(2^22, 2 + the largest bucket's reads), so below 2^22 nothing reaches the last bin, whose row would read
// "<hist_bins-1>+"), PREFIX_edit_distance.tsv ("edit_distance unique unique_null <algo> <algo>_null" with --algo's
// value: per bucket the mean pair distance of its UMIs before and after, rounded up, against a null drawn from the
// file's UMI usage with seed S [default 0]; rows 0..umi_len, all of them, then Single_UMI) and PREFIX_per_umi.tsv
// ("UMI times_observed_pre total_counts_pre times_observed_post total_counts_post", a row per distinct UMI in the
// library's order).  The distances are letter distances whatever --distance says; with a whitelist the corrected UMI
// is what is counted; with --devices the call runs on the first.  The three files are made here, while the flags
// are looked at and after every other refusal, so a prefix that cannot be written ends the run with status 101 before
// the GPU is woken.  Refused likewise, each with a message of its own: fastq mode, --two-pass (its windows never hold
// the file's UMI usage), --dump-staging, --passthrough, --output-stats-seed without --output-stats or not a whole
// number in 0..2^64-1.  The output BAM and the summary lines are as without the flag.
// --umi-filtering none|multi-gene (with --per-gene; Cell Ranger's rule and STARsolo's --soloUMIfiltering
// MultiGeneUMI_CR, not the reference's, tests/multigene_model.py defines it): none, the default, changes nothing.
// multi-gene: after every (cell, gene) group has been collapsed, a UMI that one cell -- without --per-cell: the one
// cell `all` -- still shows under two or more genes is a chimera or a mis-assignment; only the gene with the most reads
// keeps it, none where the top count is shared.  One call to umi_filter_multigene (include/umihip.h) after the
// collapse, over the staged keys and freq and the collapse's kept[] and root[] (asked of the collapse for the flag,
// as --output-stats does); the records written, "Number of reads after deduplicating" and --count-matrix (which
// leaves out a pair that lost all its molecules) follow the filtered mask, --output-stats keeps describing the
// collapse.  With --devices the call runs on the first.  The summary gains "UMI filtering: multi-gene" and three
// counts.  Refused with status 101 before the GPU is woken: any other value, multi-gene without --per-gene, the flag
// given twice with different values.
// --cell-whitelist-multi [--cell-quality-tag XX] [--cell-whitelist-min-posterior P] [--cell-whitelist-pseudocount N]
// (with --cell-whitelist; after STARsolo's 1MM_multi[_pseudocounts] and Cell Ranger, tests/barcode_multi_model.py
// defines it): a barcode one substitution from two or more listed ones is not dropped but weighed -- every
// candidate by the reads that carry it exactly and by the base quality at the mismatched position, from the tag XX
// [default: CY] -- and the heaviest is taken where it holds P of the weight [default: 0.975]; N [default: 0, 0..1000]
// is added to every candidate's reads.  P is read from its text as per-mille and never as a float: 0 or 1, or 0. / 1.
// and at most three decimals, 0..1.  Refused with status 101 before the GPU is woken, each with a message of its own:
// any of the four flags without --cell-whitelist, a companion flag without --cell-whitelist-multi,
// --cell-whitelist-max-mismatches 0 with it, a tag name that is not two characters, a malformed P or N.
// --cell-filter cr2.2|top-cells|min-molecules [--expect-cells N] [--cell-filter-percentile P] [--cell-filter-ratio R]
// [--cell-min-molecules T] (with --per-cell --per-gene --count-matrix DIR and everything those go with; STARsolo's
// --soloCellFilter CellRanger2.2 N P R and TopCells N, not the reference's, tests/cells_model.py defines it): which of
// the matrix's columns are cells.  A cell's total is its molecules over all genes; the candidates are the cells with
// a molecule, S their totals in descending order, and every rule yields one threshold t: a candidate with a total of
// t or more is called, a tie at t whole.  cr2.2: m = S[min(n - 1, floor(N (1 - P)))], t = max(1, m / R rounded half
// up) [N 3000, P 0.99, R 10]; top-cells: t = S[min(n - 1, N - 1)], N required; min-molecules: t = T, required.  P is
// read from its text as per-mille like --cell-whitelist-min-posterior.  One call to umi_call_cells (include/umihip.h)
// after umi_count_matrix, over the triplets matrix.mtx holds; the four raw files, the BAM and the summary lines
// before it are as without the flag.  Added: DIR/filtered/ with features.tsv (as raw), barcodes.tsv (the called cells
// in id order), matrix.mtx and reads.mtx (raw's layout, columns renumbered); DIR/cells.tsv, "barcode reads molecules
// genes called" tab-separated, a line per candidate cell in id order; and the summary lines "Cell filter", "Number of
// candidate cells", "Number of cells called", "Molecule threshold", "Number of molecules in called cells", "Number of
// reads in called cells", "Median molecules per called cell", "Median genes per called cell" (lower medians).
// DIR/filtered is made here, after DIR.  Refused with status 101 before the GPU is woken and with nothing written,
// each with a message that names the flag: --cell-filter without --per-cell, --per-gene or --count-matrix, or given
// twice with different values; an unknown rule; a companion flag without --cell-filter or with a rule that does not
// read it; top-cells without --expect-cells, min-molecules without --cell-min-molecules; N, R or T below 1; P outside
// 0..1 or with more than three decimals; a DIR/filtered that cannot be made.
// --gene-annotation FILE [--annotation-feature F] [--annotation-attribute A] [--gene-strand S] (with --per-gene): a
// read's gene comes from a GTF, decided on the GPU, and not from a tag (annotation.hpp has the flags' definition, the
// file's reader and every refusal; the flags and the file are looked at here, in validate(), before the GPU is woken).
// --gene-introns off|exon-first|all (with --gene-annotation) [off]: reads in a gene's introns count too, by
// umi_assign_genes_introns (annotation.hpp has the rule, the summary lines and the refusals).
// --gene-rule overlap|transcript [--annotation-transcript-attribute A] (with --gene-annotation) [overlap]: transcript: a
// read's gene is the one gene with a transcript the read fits, by umi_assign_genes_transcripts (annotation.hpp has the
// rule, the summary lines, the refusals and what is not built).
// --transcript-introns off|exon-first|all (with --gene-rule transcript, and with everything that goes with it) [off;
// tests/transcript_intron_model.py defines it]: exon-first: a read that fits a transcript of one gene is that gene's, and
// a read that fits none falls back to the gene bodies (Cell Ranger 7's counting with introns); all: the bodies decide, and
// the fit names the tier; off: the run without the flag, byte for byte.  The one call is
// umi_assign_genes_transcripts_classes.  The summary gains, in "Gene introns"' place, "Transcript introns: <mode>",
// "Number of reads assigned by a transcript" and "Number of reads assigned by a gene body".  With exon-first or all,
// --velocity goes with --gene-rule transcript: a read's class comes from the same call (a read that fits is a junction
// read where it has two blocks, else exonic; a read a body assigned is classed by the cover of its gene's exons), the
// staging is the host's as ever, and the layers are umi_velocity_matrix's, unchanged.
// Refused with status 101 before the GPU is woken: the flag without --gene-rule transcript; a value other than the
// three; the flag twice with different values; the flag together with --gene-introns (whose tiers are the overlap
// rule's: another rule).
// --velocity (with --per-gene --gene-annotation FILE --gene-introns exon-first|all --count-matrix DIR; tests/velocity_model.py
// defines it): the molecules of the matrix in three layers, spliced, unspliced and ambiguous, as STARsolo's --soloFeatures
// Velocyto, velocyto and alevin-fry's USA mode write them -- but by a gene-level rule, not by their transcript models
// (with --gene-rule transcript the classes come by transcript model, under --transcript-introns exon-first|all, above;
// annotation.hpp has the rule, the files, the summary lines and what is not built).
// Refused with status 101 before the GPU is woken: --velocity without --count-matrix, without --gene-annotation, with
// --gene-introns absent or off (with --gene-rule transcript: --transcript-introns absent or off), or with --stage gpu (a
// read's entry is kept by the host staging alone).
// --saturation-curve FILE [--saturation-points L] [--saturation-seed S] (with --per-gene --count-matrix DIR, with or
// without --per-cell -- without it there is the one column "all" -- and with everything those go with;
// tests/saturation_model.py defines it, include/umihip.h has the same rule) [L 10, S 0]: sequencing saturation and the
// median genes and molecules per cell as a function of depth, as Cell Ranger plots them, by nested read subsampling on
// the GPU.  Read i -- its record's number in the input -- has the hash h = splitmix64(S, i) >> 32 of umihip.h and the
// level (h * L) >> 32; depth j of 1..L is the reads of a level below j, so a read of one depth is in every deeper one,
// and depth L is the whole file.  A molecule is there at a depth when one of its reads is; a (cell, gene) pair when one
// of its molecules is.  The collapse is the full-depth one: the molecules are those of the run, and nothing is
// collapsed again per depth (what Cell Ranger does from its molecule table).  Reads under a UMI that --umi-filtering
// multi-gene removed count nowhere.  One call to umi_saturation_curve on the first device, after the matrix and after
// --cell-filter's call, over every read's entry as --velocity builds it, the mask the matrix was counted from, root[]
// and the buckets' gene and cell.  The selected cells of the medians and the "in cells" columns are --cell-filter's
// called cells; without that flag every column with a molecule.
// FILE: tab-separated, uncompressed, the header "depth reads molecules saturation pairs cells molecules_in_cells
// pairs_in_cells median_molecules median_genes" and a line per depth; depth is the text j/L; saturation is
// floor(10000 (reads - molecules) / reads) printed as 0.dddd, 0.0000 where reads is 0, computed in integers; the medians
// are lower medians over all selected cells, those with nothing at the depth as 0.  The summary gains "Saturation
// curve: <L> points, seed <S>" and "Sequencing saturation: 0.dddd" (the last line's).  The BAM, every matrix file,
// cells.tsv, velocity/ and the other summary lines are byte for byte what --stage host writes without the flag.  The
// flag stages on the host, as --velocity does: --stage auto goes to the host.
// Refused with status 101 before the GPU is woken: the flag without --count-matrix or with --stage gpu;
// --saturation-points or --saturation-seed without the flag; L that is not a number in 1..32; S that is not a number in
// 0..2^64-1; any of the three given twice with different values; a FILE that cannot be created (its parent must exist).
// --junction-matrix (no argument; with --per-gene --count-matrix DIR, with or without --per-cell -- without it there is the
// one column "all" -- and with everything those go with: GX tags or --gene-annotation under any rule, --umi-filtering
// multi-gene, --cell-filter, --velocity, --saturation-curve, --output-stats, both whitelists, -k, --algo, --distance edit,
// --devices; tests/junction_model.py defines it, include/umihip.h has the same rule): a count matrix whose rows are splice
// junctions instead of genes, what STARsolo's --soloFeatures SJ writes.  A junction of a read is the stretch between two
// consecutive non-empty blocks of its CIGAR (blocks as --gene-rule transcript walks them: M, =, X and D extend a block,
// an N of any length closes it, I, S, H and P consume nothing), where it is at least one base long and ends at or
// before 2^31 - 1: several N with only I, S, H or P between them are one junction, a leading, trailing or zero-length
// N gives none, a D never makes one.  Its identity is (reference, start, end); it has no strand, because there is no
// genome here to read a motif from.  A molecule of the run -- a surviving UMI of a (cell, gene) -- supports a junction
// when one of its reads has it.  The collapse is the run's own: nothing is collapsed again per junction, which is not
// what STARsolo's SJ does (it dedups UMIs per cell and junction).  Reads the run did not stage (no gene, several genes,
// no barcode, no UMI) contribute no junction, and reads under a UMI that --umi-filtering multi-gene removed count
// nowhere.  One call to umi_junction_matrix on the first device, after the matrix and after --cell-filter's call, over
// the staged reads' reference, position, CIGAR words and entry (as --velocity builds it), the mask the matrix was
// counted from, root[] and the buckets' cell; its capacity is the number of N words among those reads, an upper bound.
// DIR/junctions/: features.tsv, a line "<reference name>\t<start + 1>\t<end>" per junction -- the intron's first and
// last base, 1-based -- sorted by (reference id, start, end); barcodes.tsv, the raw file's bytes; matrix.mtx, the
// molecules, laid out like the raw matrix.mtx, "junction cell count" sorted by cell, then junction; reads.mtx, the
// reads under surviving UMIs that have the junction.  With --cell-filter also DIR/junctions/filtered/, the same four
// files for the called cells: columns renumbered as in DIR/filtered/, junctions with no entry left dropped and the rest
// renumbered; the cells are called from the gene matrix exactly as without the flag.  The summary gains, behind every
// other line, "Junction matrix: on", "Number of spliced reads counted", "Number of junction occurrences", "Number of
// distinct junctions" and "Number of (cell, junction) pairs".  The BAM, every other file and the other summary lines are
// byte for byte what --stage host writes without the flag.  The flag stages on the host, as --velocity does: --stage auto
// goes to the host.
// Refused with status 101 before the GPU is woken: the flag without --count-matrix or with --stage gpu; a DIR/junctions
// or DIR/junctions/filtered that cannot be made.  Not built: junction strand and motif, an annotated / novel column
// from the GTF, junctions of reads outside every gene, per-junction UMI collapse as STARsolo does it, --two-pass,
// --paired, a read's entry from the GPU staging.
#pragma once
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <unordered_set>
#include <utility>
#include <vector>

#include <cerrno>
#include <sys/stat.h>

#include "../../include/umihip.h"

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
    bool cell_wl_multi = false;         // --cell-whitelist-multi: ambiguous barcodes are decided by posterior
    std::string cell_qual_tag = "CY";   // --cell-quality-tag XX: the barcode's base qualities
    int cell_wl_min_posterior = 975;    // --cell-whitelist-min-posterior P, per-mille
    int cell_wl_pseudocount = 0;        // --cell-whitelist-pseudocount N
    bool cell_qual_tag_given = false, cell_wl_min_posterior_given = false, cell_wl_pseudocount_given = false;
    bool wl_max_given = false, wl_min_given = false;
    bool per_gene = false, gene_tag_given = false; // --per-gene: a bucket is a gene, with --per-cell a (cell, gene) pair
    std::string gene_tag = "GX";                   // --gene-tag XX: the gene's tag
    std::string count_matrix;                      // --count-matrix DIR: molecules per cell and gene, MatrixMarket files
    std::string output_stats;        // --output-stats PREFIX: three tables on what the deduplication did
    uint64_t output_stats_seed = 0;  // --output-stats-seed S: the seed of the tables' null
    bool output_stats_seed_given = false;
    std::string umi_filtering;       // --umi-filtering none|multi-gene: what is done to the collapsed UMIs across genes
    bool umi_filtering_given = false, filter_multigene = false; // ... multi-gene (filled in by validate())
    std::string cell_filter;         // --cell-filter cr2.2|top-cells|min-molecules: which columns of the matrix are cells
    bool cell_filter_given = false;
    int cell_filter_rule = UMI_CELLS_CR22;  // ... as UMI_CELLS_* (filled in by validate())
    long long expect_cells = 3000;          // --expect-cells N
    int cell_filter_permille = 990;         // --cell-filter-percentile P, per-mille
    long long cell_filter_ratio = 10;       // --cell-filter-ratio R
    long long cell_min_molecules = 1;       // --cell-min-molecules T
    bool expect_cells_given = false, cell_filter_percentile_given = false, cell_filter_ratio_given = false,
         cell_min_molecules_given = false;
    // --gene-annotation FILE: a read's gene is decided from this GTF (annotation.hpp), not read from --gene-tag
    std::string gene_annotation, annotation_feature = "exon", annotation_attribute = "gene_id", gene_strand = "forward";
    bool gene_annotation_given = false, annotation_feature_given = false, annotation_attribute_given = false, gene_strand_given = false;
    int gene_strand_mode = UMI_STRAND_FORWARD; // --gene-strand as UMI_STRAND_* (filled in by validate())
    // --gene-introns M: off, exon-first or all (annotation.hpp); off and no flag are the same run
    std::string gene_introns = "off";
    bool gene_introns_given = false;
    int gene_introns_mode = UMI_INTRONS_OFF; // as UMI_INTRONS_* (filled in by validate())
    // --transcript-introns M (with --gene-rule transcript): off, exon-first or all; off and no flag are the same run
    std::string transcript_introns = "off";
    bool transcript_introns_given = false;
    int transcript_introns_mode = UMI_INTRONS_OFF; // as UMI_INTRONS_* (filled in by validate())
    bool velocity = false; // --velocity: spliced, unspliced and ambiguous matrices beside --count-matrix's
    bool junction_matrix = false;  // --junction-matrix: molecules per cell and splice junction beside --count-matrix's
    std::string saturation_curve;  // --saturation-curve FILE: saturation and medians per depth (the rule is at the top)
    int saturation_points = 10;    // --saturation-points L
    uint64_t saturation_seed = 0;  // --saturation-seed S
    std::string saturation_points_text, saturation_seed_text; // ... as given, for "given twice"
    // --gene-rule overlap|transcript (annotation.hpp); overlap and no flag are the same run
    std::string gene_rule = "overlap", annotation_transcript_attribute = "transcript_id";
    bool gene_rule_given = false, annotation_transcript_attribute_given = false;
    bool gene_rule_transcript = false; // ... transcript (filled in by validate())
    struct Annotation { // the file's taken lines (filled in by validate(): read_annotation)
        std::vector<std::string> refs;      // the reference names of column 1, in order of first appearance
        std::vector<uint32_t> ref_name;     // per taken line: its reference, an index into refs
        std::vector<int32_t> start, end;    // ... half-open, 0-based
        std::vector<uint8_t> strand;        // ... + - or .
        std::vector<int32_t> gene;          // ... an index into gene_ids
        std::vector<int32_t> transcript;    // ... its transcript, numbered by first appearance (--gene-rule transcript alone)
        uint32_t n_transcripts = 0;
        std::vector<std::string> gene_ids;  // the genes in order of first appearance
        std::vector<std::string> gene_names; // ... and the gene_name of each one's first taken line (empty: none)
    } annotation;
    bool edit_distance = false; // --distance edit: -k bounds the Levenshtein distance (umi_dedup_batch_edit)
    bool algo_cr = false;       // --algo cr: Cell Ranger's one-mismatch correction (umi_dedup_batch_cr); filled in by validate()
    // filled in by validate(): --algo as UMI_ALGO_*, --merge as 0 any, 1 avgqual, 2 mapqual, and the two lists
    int algo_id = 0, merge_id = 0;
    std::vector<uint8_t> whitelist, cell_list; // the listed UMIs / barcodes back to back
    size_t cell_len = 0;
};

[[noreturn]] void die(const std::string &msg)
{ // the reference panics (panic = "abort")
    std::fprintf(stderr, "umicollapse: %s\n", msg.c_str());
    std::fflush(stderr);
    std::_Exit(101); // (no static destructors: the GPU's start-up thread may still be running)
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
              "      --algo <ALGO>        adj, dir or cluster [default: dir], or cr; cluster: one UMI per connected component of\n"
              "                           \"within k\" (umi_tools' cluster, STARsolo's 1MM_All at -k 1); -p plays no part;\n"
              "                           cr: Cell Ranger's one-mismatch correction (STARsolo's 1MM_CR) -- every UMI goes to\n"
              "                           the best of itself and its one-mismatch neighbours by (reads, string), every target\n"
              "                           is a molecule, nothing is transitive; -k 1 only, -p plays no part (bam/sam mode,\n"
              "                           one pass, one GPU, UMIs of at most 21 bases)\n"
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
              "                           that took a read, in list order (with --cell-whitelist-multi also: resolved)\n"
              "      --cell-whitelist-multi with --cell-whitelist: a barcode one substitution from two or more listed ones\n"
              "                           is weighed, not dropped: every candidate by its exact reads and by the base\n"
              "                           quality at the mismatched position; the heaviest is taken where it holds the\n"
              "                           minimum posterior (STARsolo 1MM_multi, Cell Ranger)\n"
              "      --cell-quality-tag <XX> aux tag of the barcode's qualities, type Z, Phred + 33 [default: CY]\n"
              "      --cell-whitelist-min-posterior <P> 0..1, at most three decimals [default: 0.975]\n"
              "      --cell-whitelist-pseudocount <N> added to every candidate's exact reads, 0..1000 [default: 0]\n"
              "      --per-gene           deduplicate per gene: reads are grouped by gene (with --per-cell by cell and\n"
              "                           gene) and not by alignment position, so a molecule fragmented at two places\n"
              "                           is kept once; reads without a gene, or assigned to several, are dropped\n"
              "                           (bam/sam mode, one pass; not with --paired, --tag, --keep-unmapped,\n"
              "                           --call-consensus)\n"
              "      --gene-tag <XX>      aux tag of the gene, type Z [default: GX]; no tag, an empty value, -, or a value\n"
              "                           starting with __ or Unassigned: no gene; a value with ; or , : several genes\n"
              "      --gene-annotation <FILE> with --per-gene: a read's gene comes from this GTF (plain or gzip) and not from\n"
              "                           a tag: the one gene whose features share a base with the read's aligned blocks\n"
              "                           (the CIGAR's M = X D stretches between its N), on an admissible strand; no gene\n"
              "                           or several: the read is dropped (featureCounts' default rule, decided on the\n"
              "                           GPU); features.tsv names a gene by its gene_name where the file has one (not\n"
              "                           with --gene-tag, --dump-staging)\n"
              "      --annotation-feature <F> the lines taken: column 3 equals F [default: exon]; gene: whole gene bodies,\n"
              "                           introns included (single-nucleus runs)\n"
              "      --annotation-attribute <A> the attribute of column 9 that names the gene [default: gene_id]\n"
              "      --gene-strand <S>    forward, reverse or unstranded [default: forward]: a feature is admissible on the\n"
              "                           read's strand, on the opposite one, or on either (featureCounts -s 1, 2, 0)\n"
              "      --gene-introns <M>   off, exon-first or all [default: off], with --gene-annotation: a gene's body runs\n"
              "                           from its first taken line to its last, per reference and strand.  exon-first: a\n"
              "                           read that hits no exon goes to the one gene whose body it shares a base with\n"
              "                           (STARsolo's GeneFull_ExonOverIntron, Cell Ranger 7's default); all: every read\n"
              "                           goes by the bodies alone (GeneFull); no body or several: dropped\n"
              "      --gene-rule <R>      overlap or transcript [default: overlap], with --gene-annotation.  transcript: a read\n"
              "                           belongs to a gene when it fits one of the gene's transcripts: every block inside\n"
              "                           an exon, every N from one exon's end to the next one's start (STARsolo's Gene,\n"
              "                           Cell Ranger's transcriptome-compatible reads); no such gene or several: dropped\n"
              "                           (not with --gene-introns exon-first|all; with --velocity only under\n"
              "                           --transcript-introns exon-first|all)\n"
              "      --transcript-introns <M> off, exon-first or all [default: off], with --gene-rule transcript.  exon-first:\n"
              "                           a read that fits no transcript falls back to the gene bodies; all: the bodies\n"
              "                           decide, the fit names the tier.  Makes --velocity go with --gene-rule transcript:\n"
              "                           a read's class comes by transcript model (not with --gene-introns)\n"
              "      --annotation-transcript-attribute <A> with --gene-rule transcript: the attribute of column 9 that names\n"
              "                           a line's transcript [default: transcript_id]\n"
              "      --velocity           with --gene-annotation, --gene-introns exon-first|all and --count-matrix: write the\n"
              "                           matrix's molecules in three layers to DIR/velocity (spliced.mtx, unspliced.mtx,\n"
              "                           ambiguous.mtx, features.tsv, barcodes.tsv) by a gene-level rule: a molecule with a\n"
              "                           read that skips an intron is spliced, with a read in an intron or over an exon's\n"
              "                           edge unspliced, with both or neither ambiguous (host staging; not with --stage gpu)\n"
              "      --saturation-curve <FILE> with --per-gene --count-matrix: write sequencing saturation and the median genes\n"
              "                           and molecules per cell at L depths to FILE (tab-separated), by nested subsampling\n"
              "                           of the reads on the GPU; the molecules are the run's own, nothing is collapsed\n"
              "                           again per depth (host staging; not with --stage gpu)\n"
              "      --junction-matrix    with --per-gene --count-matrix: write the molecules per cell and splice junction to\n"
              "                           DIR/junctions (features.tsv: reference, first and last base of the intron;\n"
              "                           barcodes.tsv, matrix.mtx, reads.mtx); junctions come from the CIGARs of the reads\n"
              "                           the run staged, have no strand, and nothing is collapsed again per junction\n"
              "                           (host staging; not with --stage gpu)\n"
              "      --saturation-points <L> with --saturation-curve: depths, 1..32 [default: 10]\n"
              "      --saturation-seed <S> with --saturation-curve: seed of the reads' hash, 0..2^64-1 [default: 0]\n"
              "      --count-matrix <DIR> with --per-gene: write the molecules per cell and gene to DIR (made if it is\n"
              "                           not there) as features.tsv, barcodes.tsv, matrix.mtx (molecules) and reads.mtx\n"
              "                           (reads), MatrixMarket coordinate files sorted by cell, then gene, counted on the GPU\n"
              "      --output-stats <PREFIX> write three tables, counted on the GPU (umi_tools dedup --output-stats):\n"
              "                           PREFIX_per_umi_per_position.tsv (reads per UMI and position, before and after),\n"
              "                           PREFIX_edit_distance.tsv (mean UMI distance per position before and after, each\n"
              "                           against a null drawn from the file's UMI usage; letter distances also with\n"
              "                           --distance edit) and PREFIX_per_umi.tsv (how every UMI sequence is used)\n"
              "                           (bam/sam mode, one pass; not with --dump-staging, --passthrough)\n"
              "      --output-stats-seed <S> with --output-stats: seed of the null, 0..2^64-1 [default: 0]\n"
              "      --umi-filtering <F>  none or multi-gene [default: none]; multi-gene, with --per-gene: a UMI that a cell\n"
              "                           shows under several genes after the collapse is kept by the gene with the most\n"
              "                           reads only, by none where the top count is shared (Cell Ranger, STARsolo's\n"
              "                           MultiGeneUMI_CR); the records, the summary and --count-matrix follow, decided on\n"
              "                           the GPU\n"
              "      --cell-filter <RULE> cr2.2, top-cells or min-molecules, with --per-cell --per-gene --count-matrix: call\n"
              "                           cells on the GPU by their molecule totals and write DIR/filtered/ (the matrix of\n"
              "                           the called cells) and DIR/cells.tsv; cr2.2: Cell Ranger 2.2's knee (STARsolo\n"
              "                           CellRanger2.2 N P R): the total at rank N (1 - P), divided by R; top-cells: the\n"
              "                           total at rank N (STARsolo TopCells); min-molecules: T; ties at the threshold\n"
              "                           are called whole\n"
              "      --expect-cells <N>   with --cell-filter cr2.2 [default: 3000] or top-cells (required), 1 or more\n"
              "      --cell-filter-percentile <P> with cr2.2: 0..1, at most three decimals [default: 0.99]\n"
              "      --cell-filter-ratio <R> with cr2.2: 1 or more [default: 10]\n"
              "      --cell-min-molecules <T> with --cell-filter min-molecules (required): 1 or more\n"
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
    // a flag's value as a whole decimal number from `least` to `most`, or the flag's message
    auto number = [&](int &i, const std::string &msg, long long least, long long most = INT64_MAX) -> long long {
        const char *v = need(i);
        char *end = nullptr;
        const long long w = std::strtoll(v, &end, 10);
        if (end == v || *end != '\0' || w < least || w > most) die(msg);
        return w;
    };
    // a flag's value in 0..1 as per-mille, from the text and never as a float: [01] or [01].d{1,3}, at most 1
    auto permille = [&](int &i, const std::string &a) -> int {
        const std::string v = need(i);
        bool ok = !v.empty() && (v[0] == '0' || v[0] == '1') && (v.size() == 1 || (v[1] == '.' && v.size() >= 3 && v.size() <= 5));
        int pm = ok ? (v[0] - '0') * 1000 : 0;
        for (size_t d = 2, unit = 100; ok && d < v.size(); d++, unit /= 10) {
            ok = v[d] >= '0' && v[d] <= '9';
            pm += (v[d] - '0') * (int)unit;
        }
        if (!ok || pm > 1000) die(a + " wants a number in 0..1 with at most three decimals: '" + v + "'");
        return pm;
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
        else if (a == "--two-pass-window")
            c.two_pass_window = (uint64_t)number(i, "--two-pass-window wants a number of reads, 1 or more", 1);
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
        else if (a == "--per-gene") c.per_gene = true;
        else if (a == "--gene-tag") { c.gene_tag = need(i); c.gene_tag_given = true; } // (looked at by validate)
        else if (a == "--gene-annotation" || a == "--annotation-feature" || a == "--annotation-attribute" || a == "--gene-strand") {
            const std::string v = need(i);
            std::string &value = a == "--gene-annotation" ? c.gene_annotation : a == "--annotation-feature" ? c.annotation_feature
                                 : a == "--annotation-attribute" ? c.annotation_attribute : c.gene_strand;
            bool &given = a == "--gene-annotation" ? c.gene_annotation_given : a == "--annotation-feature" ? c.annotation_feature_given
                          : a == "--annotation-attribute" ? c.annotation_attribute_given : c.gene_strand_given;
            if (given && value != v) die(a + " given twice with different values: '" + value + "' and '" + v + "'");
            value = v;
            given = true;
        }
        else if (a == "--gene-introns") {
            const std::string v = need(i);
            if (c.gene_introns_given && c.gene_introns != v)
                die(a + " given twice with different values: '" + c.gene_introns + "' and '" + v + "'");
            c.gene_introns = v;
            c.gene_introns_given = true;
        }
        else if (a == "--transcript-introns") {
            const std::string v = need(i);
            if (c.transcript_introns_given && c.transcript_introns != v)
                die(a + " given twice with different values: '" + c.transcript_introns + "' and '" + v + "'");
            c.transcript_introns = v;
            c.transcript_introns_given = true;
        }
        else if (a == "--velocity") c.velocity = true;
        else if (a == "--junction-matrix") c.junction_matrix = true;
        else if (a == "--gene-rule" || a == "--annotation-transcript-attribute") {
            const std::string v = need(i);
            std::string &value = a == "--gene-rule" ? c.gene_rule : c.annotation_transcript_attribute;
            bool &given = a == "--gene-rule" ? c.gene_rule_given : c.annotation_transcript_attribute_given;
            if (given && value != v) die(a + " given twice with different values: '" + value + "' and '" + v + "'");
            value = v;
            given = true;
        }
        else if (a == "--saturation-curve" || a == "--saturation-points" || a == "--saturation-seed") {
            const std::string v = need(i);
            std::string &value = a == "--saturation-curve" ? c.saturation_curve : a == "--saturation-points" ? c.saturation_points_text
                                                                                                           : c.saturation_seed_text;
            if (!value.empty() && value != v) die(a + " given twice with different values: '" + value + "' and '" + v + "'");
            if (v.empty()) die(a + " wants a value");
            value = v;
            const bool digits = v.find_first_not_of("0123456789") == std::string::npos;
            errno = 0;
            const unsigned long long w = digits ? std::strtoull(v.c_str(), nullptr, 10) : 0ull;
            if (a == "--saturation-points") {
                if (!digits || errno == ERANGE || w < 1 || w > 32) die("--saturation-points wants a whole number in 1..32: '" + v + "'");
                c.saturation_points = (int)w;
            } else if (a == "--saturation-seed") {
                if (!digits || errno == ERANGE) die("--saturation-seed wants a whole number in 0..2^64-1: '" + v + "'");
                c.saturation_seed = (uint64_t)w;
            }
        }
        else if (a == "--count-matrix") c.count_matrix = need(i);
        else if (a == "--output-stats") c.output_stats = need(i);
        else if (a == "--output-stats-seed") {
            const std::string v = need(i);
            errno = 0;
            char *end = nullptr;
            const unsigned long long w = std::strtoull(v.c_str(), &end, 10);
            const bool digits = !v.empty() && v.find_first_not_of("0123456789") == std::string::npos;
            if (!digits || *end != '\0' || errno == ERANGE) die("--output-stats-seed wants a whole number in 0..2^64-1: '" + v + "'");
            c.output_stats_seed = (uint64_t)w;
            c.output_stats_seed_given = true;
        }
        else if (a == "--umi-filtering") {
            const std::string v = need(i);
            if (c.umi_filtering_given && c.umi_filtering != v)
                die("--umi-filtering given twice with different values: '" + c.umi_filtering + "' and '" + v + "'");
            c.umi_filtering = v;
            c.umi_filtering_given = true;
        }
        else if (a == "--umi-whitelist") c.umi_whitelist = need(i);
        else if (a == "--whitelist-metrics") c.whitelist_metrics = need(i);
        else if (a == "--whitelist-max-mismatches" || a == "--whitelist-min-distance") {
            const long long m = number(i, a + " wants a number, 0 or more", 0, INT32_MAX);
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
        else if (a == "--cell-whitelist-multi") c.cell_wl_multi = true;
        else if (a == "--cell-quality-tag") {
            const std::string t = need(i);
            auto alpha = [](char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
            if (t.size() != 2 || !alpha(t[0]) || !(alpha(t[1]) || (t[1] >= '0' && t[1] <= '9')))
                die(a + " wants a tag name of two characters, [A-Za-z][A-Za-z0-9]: '" + t + "'");
            c.cell_qual_tag = t;
            c.cell_qual_tag_given = true;
        }
        else if (a == "--cell-whitelist-min-posterior") {
            c.cell_wl_min_posterior = permille(i, a);
            c.cell_wl_min_posterior_given = true;
        }
        else if (a == "--cell-filter") {
            const std::string v = need(i);
            if (c.cell_filter_given && c.cell_filter != v)
                die("--cell-filter given twice with different values: '" + c.cell_filter + "' and '" + v + "'");
            c.cell_filter = v;
            c.cell_filter_given = true;
        }
        else if (a == "--expect-cells") {
            c.expect_cells = number(i, "--expect-cells wants a number of cells, 1 or more", 1);
            c.expect_cells_given = true;
        }
        else if (a == "--cell-filter-percentile") {
            c.cell_filter_permille = permille(i, a);
            c.cell_filter_percentile_given = true;
        }
        else if (a == "--cell-filter-ratio") {
            c.cell_filter_ratio = number(i, "--cell-filter-ratio wants a number, 1 or more", 1);
            c.cell_filter_ratio_given = true;
        }
        else if (a == "--cell-min-molecules") {
            c.cell_min_molecules = number(i, "--cell-min-molecules wants a number of molecules, 1 or more", 1);
            c.cell_min_molecules_given = true;
        }
        else if (a == "--cell-whitelist-pseudocount") {
            const std::string v = need(i);
            const bool digits = !v.empty() && v.size() <= 4 && v.find_first_not_of("0123456789") == std::string::npos;
            if (!digits || std::atoi(v.c_str()) > 1000) die(a + " wants a whole number in 0..1000: '" + v + "'");
            c.cell_wl_pseudocount = std::atoi(v.c_str());
            c.cell_wl_pseudocount_given = true;
        }
        else if (a == "--consensus") c.consensus = true;
        else if (a == "--consensus-min-reads") {
            c.consensus_min_reads = (uint64_t)number(i, "--consensus-min-reads wants a number of reads, 1 or more", 1);
            c.consensus_min_given = true;
        }
        else if (a == "--call-consensus") c.call_consensus = true;
        else if (a == "--call-consensus-min-reads") {
            c.call_consensus_min_reads = (uint64_t)number(i, "--call-consensus-min-reads wants a number of reads, 1 or more", 1);
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

// --gene-annotation: the file's taken lines into args.annotation, or the message that ends the run (annotation.hpp)
void read_annotation(Cli &args);

// the one spelling of --stage's values (each mode asks at its own place among its refusals)
void check_stage(const Cli &args)
{
    if (args.stage != "auto" && args.stage != "gpu" && args.stage != "host") die("--stage wants gpu, host or auto");
}

// --distance edit: one-word keys only; `whose` says where the length came from
void check_edit_length(const Cli &args, size_t umi_length, const std::string &whose)
{
    if (args.edit_distance && umi_length > UMI_MAX_UMI_LEN)
        die("--distance edit takes UMIs of at most 21 bases (" + whose + " " + std::to_string(umi_length) + ")");
    if (args.algo_cr && umi_length > UMI_MAX_UMI_LEN) // (--algo cr: one-word keys as well)
        die("--algo cr takes UMIs of at most 21 bases (" + whose + " " + std::to_string(umi_length) + ")");
}

// --output-stats: its three files (none without the flag)
std::vector<std::string> output_stats_paths(const Cli &args)
{
    if (args.output_stats.empty()) return {};
    return {args.output_stats + "_per_umi_per_position.tsv", args.output_stats + "_edit_distance.tsv", args.output_stats + "_per_umi.tsv"};
}

// The refusals that need nothing but the command line and the lists it names, in the order that decides
// which message wins when two apply; fills in the defaults and the decoded --algo / --merge.  False: a
// --mode that is none of bam, sam, fastq, for which nothing happens.
bool validate(Cli &args)
{
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
    if (args.mode != "bam" && args.mode != "sam" && args.mode != "fastq") return false; // main.rs:49-95: nothing happens
    // --per-gene, --count-matrix: likewise (the directory is made last, once nothing else refuses the run)
    if (args.gene_tag_given && !args.per_gene) die("--gene-tag goes with --per-gene only");
    if (!args.count_matrix.empty() && !args.per_gene) die("--count-matrix goes with --per-gene only");
    if (args.per_gene) {
        if (args.mode == "fastq") die("--per-gene is defined in bam/sam mode only (there are no tags in fastq mode)");
        if (args.two_pass) die("--per-gene does not go with --two-pass (its census is by position)");
        if (args.paired) die("--per-gene does not go with --paired");
        if (args.keep_unmapped) die("--per-gene does not go with --keep-unmapped (an unmapped read has no gene)");
        if (args.track_clusters) die("--per-gene does not go with --tag");
        if (args.call_consensus) die("--per-gene does not go with --call-consensus (the reads of a gene do not line up)");
        if (args.passthrough) die("--per-gene does not go with --passthrough");
        const std::string &t = args.gene_tag;
        auto alpha = [](char ch) { return (ch >= 'A' && ch <= 'Z') || (ch >= 'a' && ch <= 'z'); };
        if (t.size() != 2 || !alpha(t[0]) || !(alpha(t[1]) || (t[1] >= '0' && t[1] <= '9')))
            die("--gene-tag wants a tag name of two characters, [A-Za-z][A-Za-z0-9]: '" + t + "'");
        if (!args.count_matrix.empty() && !args.dump_staging.empty()) die("--count-matrix does not go with --dump-staging");
    }
    // --gene-annotation: likewise, the file included
    if (!args.gene_annotation_given) {
        for (const auto &f : {std::make_pair(args.annotation_feature_given, "--annotation-feature"),
                              std::make_pair(args.annotation_attribute_given, "--annotation-attribute"),
                              std::make_pair(args.gene_strand_given, "--gene-strand")})
            if (f.first) die(std::string(f.second) + " goes with --gene-annotation only");
        if (args.gene_introns_given) die("--gene-introns goes with --gene-annotation only");
        if (args.gene_rule_given) die("--gene-rule goes with --gene-annotation only");
        if (args.annotation_transcript_attribute_given) die("--annotation-transcript-attribute goes with --gene-rule transcript only");
        if (args.transcript_introns_given) die("--transcript-introns goes with --gene-rule transcript only");
    } else {
        if (args.gene_rule != "overlap" && args.gene_rule != "transcript") die("--gene-rule wants overlap or transcript: '" + args.gene_rule + "'");
        args.gene_rule_transcript = args.gene_rule == "transcript";
        if (args.annotation_transcript_attribute_given && !args.gene_rule_transcript)
            die("--annotation-transcript-attribute goes with --gene-rule transcript only");
        if (args.annotation_transcript_attribute.empty()) die("--annotation-transcript-attribute wants an attribute name");
        if (args.gene_introns == "off") args.gene_introns_mode = UMI_INTRONS_OFF;
        else if (args.gene_introns == "exon-first") args.gene_introns_mode = UMI_INTRONS_EXON_FIRST;
        else if (args.gene_introns == "all") args.gene_introns_mode = UMI_INTRONS_ALL;
        else die("--gene-introns wants off, exon-first or all: '" + args.gene_introns + "'");
        if (args.transcript_introns_given && !args.gene_rule_transcript) die("--transcript-introns goes with --gene-rule transcript only");
        if (args.transcript_introns == "off") args.transcript_introns_mode = UMI_INTRONS_OFF;
        else if (args.transcript_introns == "exon-first") args.transcript_introns_mode = UMI_INTRONS_EXON_FIRST;
        else if (args.transcript_introns == "all") args.transcript_introns_mode = UMI_INTRONS_ALL;
        else die("--transcript-introns wants off, exon-first or all: '" + args.transcript_introns + "'");
        if (args.transcript_introns_given && args.gene_introns_given)
            die("--transcript-introns does not go with --gene-introns (the one falls back from the transcript models, the other from the "
                "overlap rule's exons: two rules)");
        if (args.gene_rule_transcript && args.gene_introns_mode != UMI_INTRONS_OFF)
            die("--gene-rule transcript does not go with --gene-introns " + args.gene_introns + " (the gene bodies behind the transcript "
                "models are --transcript-introns " + args.gene_introns + "). Not built: the overlap rule's exon tier beside the transcript models");
        if (args.gene_rule_transcript && args.velocity && args.transcript_introns_mode == UMI_INTRONS_OFF)
            die("--gene-rule transcript does not go with --velocity unless --transcript-introns exon-first or all is given. Not built: read "
                "classes by transcript model without the gene bodies behind it");
        if (!args.per_gene) die("--gene-annotation goes with --per-gene only");
        if (args.gene_tag_given) die("--gene-annotation does not go with --gene-tag (the gene comes from the file, not from a tag)");
        if (!args.dump_staging.empty()) die("--gene-annotation does not go with --dump-staging (which stops before the GPU)");
        if (args.gene_strand == "forward") args.gene_strand_mode = UMI_STRAND_FORWARD;
        else if (args.gene_strand == "reverse") args.gene_strand_mode = UMI_STRAND_REVERSE;
        else if (args.gene_strand == "unstranded") args.gene_strand_mode = UMI_STRAND_UNSTRANDED;
        else die("--gene-strand wants forward, reverse or unstranded: '" + args.gene_strand + "'");
        if (args.annotation_feature.empty()) die("--annotation-feature wants a feature type");
        if (args.annotation_attribute.empty()) die("--annotation-attribute wants an attribute name");
        read_annotation(args);
    }
    // --velocity: likewise (its directories are made last, behind --cell-filter's)
    if (args.velocity) {
        if (args.count_matrix.empty()) die("--velocity goes with --count-matrix DIR only");
        if (!args.gene_annotation_given) die("--velocity goes with --gene-annotation only (a read's class comes from the file's exons)");
        if (args.gene_introns_mode == UMI_INTRONS_OFF && args.transcript_introns_mode == UMI_INTRONS_OFF)
            die("--velocity goes with --gene-introns exon-first or all only");
        if (args.stage == "gpu") die("--stage gpu does not go with --paired, --tag, --call-consensus, --velocity or --dump-staging");
    }
    // --saturation-curve: likewise (its file is made last)
    if (args.saturation_curve.empty()) {
        if (!args.saturation_points_text.empty()) die("--saturation-points goes with --saturation-curve only");
        if (!args.saturation_seed_text.empty()) die("--saturation-seed goes with --saturation-curve only");
    } else {
        if (args.count_matrix.empty()) die("--saturation-curve goes with --count-matrix DIR only");
        if (args.stage == "gpu")
            die("--stage gpu does not go with --saturation-curve (a read's entry is kept by the host staging alone)");
    }
    // --junction-matrix: likewise (its directories are made last)
    if (args.junction_matrix) {
        if (args.count_matrix.empty()) die("--junction-matrix goes with --count-matrix DIR only");
        if (args.stage == "gpu") die("--stage gpu does not go with --junction-matrix");
    }
    // --umi-filtering: likewise
    if (args.umi_filtering_given &&args.umi_filtering != "none" && args.umi_filtering != "multi-gene")
        die("--umi-filtering wants none or multi-gene: '" + args.umi_filtering + "'");
    args.filter_multigene = args.umi_filtering == "multi-gene";
    if (args.filter_multigene && !args.per_gene) die("--umi-filtering multi-gene goes with --per-gene only");
    // --cell-filter: likewise (its directory is made last, behind --count-matrix's)
    if (!args.cell_filter_given) {
        for (const auto &f : {std::make_pair(args.expect_cells_given, "--expect-cells"),
                              std::make_pair(args.cell_filter_percentile_given, "--cell-filter-percentile"),
                              std::make_pair(args.cell_filter_ratio_given, "--cell-filter-ratio"),
                              std::make_pair(args.cell_min_molecules_given, "--cell-min-molecules")})
            if (f.first) die(std::string(f.second) + " goes with --cell-filter only");
    } else {
        const std::string &r = args.cell_filter;
        if (r == "cr2.2") args.cell_filter_rule = UMI_CELLS_CR22;
        else if (r == "top-cells") args.cell_filter_rule = UMI_CELLS_TOP;
        else if (r == "min-molecules") args.cell_filter_rule = UMI_CELLS_MIN;
        else die("--cell-filter wants cr2.2, top-cells or min-molecules: '" + r + "'");
        if (!args.per_cell || !args.per_gene || args.count_matrix.empty())
            die("--cell-filter goes with --per-cell --per-gene --count-matrix DIR only");
        if (args.expect_cells_given && r == "min-molecules") die("--expect-cells does not go with --cell-filter min-molecules");
        if (args.cell_filter_percentile_given && r != "cr2.2") die("--cell-filter-percentile goes with --cell-filter cr2.2 only");
        if (args.cell_filter_ratio_given && r != "cr2.2") die("--cell-filter-ratio goes with --cell-filter cr2.2 only");
        if (args.cell_min_molecules_given && r != "min-molecules") die("--cell-min-molecules goes with --cell-filter min-molecules only");
        if (r == "top-cells" && !args.expect_cells_given) die("--cell-filter top-cells wants --expect-cells N");
        if (r == "min-molecules" && !args.cell_min_molecules_given) die("--cell-filter min-molecules wants --cell-min-molecules T");
    }
    // --algo cr: everything about it that can be refused is, before the GPU is woken
    args.algo_cr = args.algo == "cr";
    if (args.algo_cr) {
        if (args.mode == "fastq") die("--algo cr is defined in bam/sam mode only (whole reads are the key in fastq mode)");
        if (args.two_pass) die("--algo cr does not go with --two-pass");
        if (args.devices.size() > 1) die("--algo cr runs on one GPU: --devices takes one id with it");
        if (args.edit_distance) die("--algo cr does not go with --distance edit (its distance is one substitution)");
        if (args.k != 1) die("--algo cr corrects at one mismatch: -k " + std::to_string(args.k) + " does not go with it");
        check_edit_length(args, args.umi_length, "-u");
    }
    // --distance edit: everything about it that can be refused is, before the GPU is woken
    if (args.edit_distance) {
        if (args.mode == "fastq") die("--distance edit is defined in bam/sam mode only (whole reads are the key in fastq mode)");
        if (args.devices.size() > 1) die("--distance edit runs on one GPU: --devices takes one id with it");
        check_edit_length(args, args.umi_length, "-u");
    }
    // --umi-whitelist: everything about it that can be refused is, before the GPU is woken
    if (!args.umi_whitelist.empty()) {
        if (args.mode == "fastq") die("--umi-whitelist does not go with fastq mode (whole reads are the key there)");
        if (args.two_pass) die("--umi-whitelist does not go with --two-pass (its census would need the correction too)");
        if (!args.dump_staging.empty() || args.passthrough) die("--umi-whitelist does not go with --dump-staging or --passthrough");
        size_t wl_len = 0;
        args.whitelist = read_whitelist(args.umi_whitelist, wl_len);
        if (args.umi_length != 0 && args.umi_length != wl_len)
            die("-u " + std::to_string(args.umi_length) + " does not go with a whitelist of UMIs of " + std::to_string(wl_len) +
                " bases");
        check_edit_length(args, wl_len, "the whitelist's have");
        args.umi_length = wl_len; // (a read whose UMI is of another length ends the run, as with -u)
    }
    // --cell-whitelist: likewise
    if (args.cell_whitelist.empty() && (args.cell_wl_max_given || !args.cell_whitelist_metrics.empty()))
        die("--cell-whitelist-max-mismatches and --cell-whitelist-metrics go with --cell-whitelist only");
    const bool multi_companion = args.cell_qual_tag_given || args.cell_wl_min_posterior_given || args.cell_wl_pseudocount_given;
    if (args.cell_whitelist.empty() && (args.cell_wl_multi || multi_companion))
        die("--cell-whitelist-multi, --cell-quality-tag, --cell-whitelist-min-posterior and --cell-whitelist-pseudocount go with "
            "--cell-whitelist only");
    if (multi_companion && !args.cell_wl_multi)
        die("--cell-quality-tag, --cell-whitelist-min-posterior and --cell-whitelist-pseudocount go with --cell-whitelist-multi only");
    if (args.cell_wl_multi && args.cell_wl_max_mismatches == 0)
        die("--cell-whitelist-multi does not go with --cell-whitelist-max-mismatches 0 (nothing is ambiguous then)");
    if (!args.cell_whitelist.empty()) {
        if (args.mode == "fastq") die("--cell-whitelist does not go with fastq mode (there are no tags there)");
        if (!args.per_cell) die("--cell-whitelist goes with --per-cell only");
        if (args.two_pass) die("--cell-whitelist does not go with --two-pass (its census would need the correction too)");
        if (!args.dump_staging.empty() || args.passthrough) die("--cell-whitelist does not go with --dump-staging or --passthrough");
        args.cell_list = read_whitelist(args.cell_whitelist, args.cell_len, "cell barcode whitelist", "barcode", 32);
    }
    // --output-stats: likewise (its files are made last, once nothing else refuses the run)
    if (args.output_stats_seed_given && args.output_stats.empty()) die("--output-stats-seed goes with --output-stats only");
    if (!args.output_stats.empty()) {
        if (args.mode == "fastq") die("--output-stats is defined in bam/sam mode only");
        if (args.two_pass) die("--output-stats does not go with --two-pass (its windows never hold the file's UMI usage)");
        if (!args.dump_staging.empty()) die("--output-stats does not go with --dump-staging");
        if (args.passthrough) die("--output-stats does not go with --passthrough");
    }
    if (args.track_clusters && args.paired) die("--tag with --paired is not implemented (the reference never reaches its tagging pass)");
    if (args.algo == "dir") args.algo_id = UMI_ALGO_DIRECTIONAL;
    else if (args.algo == "adj") args.algo_id = UMI_ALGO_ADJACENCY;
    else if (args.algo == "cluster") args.algo_id = UMI_ALGO_CLUSTER; // (not `cc`: that name stays refused, as below)
    else if (args.algo_cr) args.algo_id = UMI_ALGO_DIRECTIONAL; // (a call of its own, HipLib::dedup: the id plays no part)
    else die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data); // main.rs:86-91
    if (args.merge == "any") args.merge_id = 0;
    else if (args.merge == "avgqual") args.merge_id = 1;
    else if (args.merge == "mapqual") args.merge_id = 2;
    else die("Invalid algorithm combination: " + args.algo + " , " + args.merge + " and " + args.data);
    if (!args.count_matrix.empty() && mkdir(args.count_matrix.c_str(), 0777) != 0) {
        const int why = errno;
        struct stat sb;
        if (why != EEXIST || stat(args.count_matrix.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
            die("cannot make the directory " + args.count_matrix + " for --count-matrix: " + std::strerror(why));
    }
    if (args.cell_filter_given) {
        const std::string dir = args.count_matrix + "/filtered";
        if (mkdir(dir.c_str(), 0777) != 0) {
            const int why = errno;
            struct stat sb;
            if (why != EEXIST || stat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
                die("cannot make the directory " + dir + " for --cell-filter: " + std::strerror(why));
        }
    }
    if (args.velocity) {
        std::vector<std::string> dirs{args.count_matrix + "/velocity"};
        if (args.cell_filter_given) dirs.push_back(args.count_matrix + "/velocity/filtered");
        for (const std::string &dir : dirs)
            if (mkdir(dir.c_str(), 0777) != 0) {
                const int why = errno;
                struct stat sb;
                if (why != EEXIST || stat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
                    die("cannot make the directory " + dir + " for --velocity: " + std::strerror(why));
            }
    }
    if (args.junction_matrix) {
        std::vector<std::string> dirs{args.count_matrix + "/junctions"};
        if (args.cell_filter_given) dirs.push_back(args.count_matrix + "/junctions/filtered");
        for (const std::string &dir : dirs)
            if (mkdir(dir.c_str(), 0777) != 0) {
                const int why = errno;
                struct stat sb;
                if (why != EEXIST || stat(dir.c_str(), &sb) != 0 || !S_ISDIR(sb.st_mode))
                    die("cannot make the directory " + dir + " for --junction-matrix: " + std::strerror(why));
            }
    }
    for (const std::string &path : output_stats_paths(args)) {
        FILE *f = std::fopen(path.c_str(), "wb");
        if (!f) die("cannot make " + path + " for --output-stats: " + std::strerror(errno));
        std::fclose(f);
    }
    if (!args.saturation_curve.empty()) {
        FILE *f = std::fopen(args.saturation_curve.c_str(), "wb");
        if (!f) die("cannot make " + args.saturation_curve + " for --saturation-curve: " + std::strerror(errno));
        std::fclose(f);
    }
    return true;
}

} // namespace
