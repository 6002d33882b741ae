// --gene-annotation FILE (with --per-gene; bam/sam mode, one pass; featureCounts' default rule, not the reference's,
// tests/annotation_model.py defines it): a read's gene is decided from an annotation file, on the GPU, and not read
// from a tag -- for files from STAR without solo, minimap2, bowtie2 or any bulk aligner, which write no GX, and in
// place of the featureCounts -R BAM pass, the sort and the index that umi_tools asks of their users.
//
// The rule: a read's blocks are the stretches of its CIGAR's M, =, X and D from its position on, an N closing one
// and skipping its length (I, S, H, P consume nothing); a gene hits the read when one of its features lies on the
// read's reference, on an admissible strand, and shares at least one base with a block.  --gene-strand forward (the
// default: 10x 3' chemistry, featureCounts -s 1): the feature's strand is the read's (- where flag 0x10 is set);
// reverse (-s 2): the opposite; unstranded (-s 0): any; a feature on '.' is admissible always.  Exactly one gene:
// the read is that gene's.  None: dropped like a read without a gene tag ("Number of reads outside every gene" takes
// that line's place).  Two or more: dropped like a read whose tag names several ("Number of reads assigned to several
// genes").  Overlapping features of one gene are one gene.  One call, umi_assign_genes (include/umihip.h), over every
// mapped read, after the file is read and before the per-read pass, which then takes the call's verdict where it
// took the tag's value (staging.hpp, read_tags): the tag is not looked at, and everything behind the gene's id --
// numbering by first appearance among the staged reads, buckets, collapse, matrix, filters -- is --per-gene's,
// unchanged.  With --devices the call runs on the first.
//
// The file: a GTF, plain or gzip (by its magic bytes), nine tab-separated columns; lines that start with # and
// empty lines are skipped.  The lines taken are those whose column 3 equals --annotation-feature (default exon;
// `gene` counts reads over whole gene bodies, introns included, as single-nucleus runs do); the others are skipped
// silently.  Columns 4 and 5 are 1-based and inclusive, column 7 is the strand.  The gene is the value of
// --annotation-attribute (default gene_id) in column 9, `key "value";`; features.tsv's second column is the value of
// gene_name on the gene's first taken line where there is one, else the gene's id.  Column 1 is matched to the BAM
// header's reference names; lines on a reference the BAM does not have are skipped and counted.  The summary gains
// "Gene annotation: <genes> genes, <features> features" (those on the BAM's references), "Gene strand: <mode>" and
// "Number of annotation lines on unknown references".
//
// Refused with status 101 before the GPU is woken: without --per-gene; with --gene-tag or --dump-staging; a
// companion flag without --gene-annotation; an unknown --gene-strand; any of the four flags given twice with
// different values; a file that cannot be read; a line of fewer than nine columns; on a taken line a start or end
// that is not a number, a start below 1, an end below the start or above 2^31 - 1, a strand other than + - ., no
// such attribute, an empty value, or a value with a byte outside 0x21..0x7e or a ; or , (the bytes --per-gene
// reserves); a file without a taken line.  Everything --per-gene refuses stays refused.
//
// Transcript-level containment (STARsolo's Gene: a read inside one transcript's exons) is --gene-rule transcript,
// below.  Not built: --paired, fractional assignment of a read among several genes, a minimum overlap above 1.
//
// --gene-rule overlap|transcript (with --gene-annotation; default overlap; tests/transcript_model.py defines transcript):
// how a read gets its gene from the file.  overlap: the rule above; the run is the run without the flag, byte for byte.
// transcript (STARsolo's default feature Gene, Cell Ranger's transcriptome-compatible reads, velocyto's models): a read
// belongs to a gene when it fits one of that gene's transcripts.  A taken line's transcript is the value of
// --annotation-transcript-attribute (default transcript_id) in column 9; a transcript's identity is (gene, that value,
// reference, strand as written), so an id that recurs on chrX and chrY, as in older GENCODE PAR entries, is two
// transcripts.  A transcript's lines are taken in ascending order whatever order the file has them in (minus-strand
// GTFs list them descending), and lines that overlap or abut are united: exons x_1 < ... < x_n, a base or more between
// neighbours.  The read's blocks b_1 .. b_m are the rule's above (a zero-length N closes a block too; empty blocks are
// left out).  The read fits the transcript when the transcript is on its reference and on an admissible strand
// (--gene-strand's rule; a . transcript always), m >= 1, and there is a j with b_i inside x_{j+i-1} for every i, and for
// every i < m the block ends where its exon ends and the next block starts where the next exon starts.  A D never
// splits a block, so a deletion across an intron fits nothing; a read with more blocks than the transcript has exons
// left does not fit it; a block before 0 or beyond 2^31 - 1 lies in nothing.  G: the genes with a transcript the read
// fits.  One gene: the read is that gene's.  None: "Number of reads outside every gene".  Two or more: "Number of reads
// assigned to several genes".  Two fitting transcripts of one gene are one gene.  G is a subset of the overlap rule's
// genes: a read that hangs one base into an exon from an intron is dropped here and counted there, and a read that fits
// a transcript of gene A and grazes an exon of an overlapping gene B is A's here and "several" there.  The one call is
// umi_assign_genes_transcripts in umi_assign_genes' place; everything behind the gene's id is --per-gene's, unchanged.
// The summary gains, behind "Number of annotation lines on unknown references": "Gene rule: transcript" and "Number of
// transcripts" (those with a line on the BAM's references).  Refused with status 101 before the GPU is woken: the flag
// without --gene-annotation; a value other than overlap, transcript; the flag given twice with different values;
// --annotation-transcript-attribute without --gene-rule transcript; on a taken line no such attribute, an empty value,
// or a value with a byte outside 0x21..0x7e or a ; or , ; --gene-rule transcript with --gene-introns exon-first|all, or
// with --velocity and no --transcript-introns exon-first|all.  Not built: --paired.
//
// --transcript-introns off|exon-first|all (with --gene-rule transcript; default off; tests/transcript_intron_model.py
// defines it): the gene bodies behind the transcript models, as Cell Ranger 7 counts with introns, and read classes by
// transcript model.  G is --gene-rule transcript's set, B --gene-introns' (the bodies derived from the same lines); G is
// in B.  exon-first: one gene in G: that gene, by a transcript; two or more: several; G empty: one gene in B: that gene,
// by a gene body; none: none; two or more: several.  all: one gene in B: that gene, by a transcript where G is not
// empty, else by a body; none: none; two or more: several.  off: the run without the flag, byte for byte.  It is another
// rule than --gene-introns, whose first tier is the overlap set E: a read that hangs a base into an exon is "by an exon"
// there and "by a gene body" here.  With --velocity the class of an assigned read comes from the same call: by a
// transcript: junction where the read has two blocks or more, else exonic; by a body: intronic where no base of its
// blocks lies in one of its gene's lines, exon-intron where some do, and where all do, junction where a stretch an N
// skipped is not covered whole by the gene's own lines (a splice the annotation does not have), else exonic.  So a read
// spliced over an intron that another isoform retains is a junction read here, and exonic under the gene-level rule.
// Stated after velocyto and STARsolo's Velocyto, not claimed equal to them: no intron validation, no per-model logic
// across a molecule's reads.  The one call is umi_assign_genes_transcripts_classes in umi_assign_genes_transcripts'
// place; molecules, layers and files are --velocity's, unchanged.  The summary gains, in "Gene introns"' place:
// "Transcript introns: <mode>", "Number of reads assigned by a transcript", "Number of reads assigned by a gene body".
// Refused with status 101 before the GPU is woken: the flag without --gene-rule transcript; a value other than off,
// exon-first, all; the flag given twice with different values; the flag together with --gene-introns.
// Not built: --paired, Ex50pAS, antisense counting, --two-pass.
//
// --gene-introns off|exon-first|all (with --gene-annotation; default off; tests/intron_model.py defines it): reads in
// a gene's introns count too, as Cell Ranger 7 counts them by default and as single-nucleus runs need.  A gene's body:
// its taken lines grouped by reference and strand as written (+, - or .), each group one body from the group's
// smallest start to its largest end, which may come from different lines; no `gene` or `transcript` line is needed,
// and bodies come from whatever --annotation-feature takes.  B: the genes with a body on the read's reference, on an
// admissible strand (the features' rule; a . body always), that shares a base with a block; E, the genes that hit by a
// feature, is a subset of B.  exon-first (STARsolo's GeneFull_ExonOverIntron, with this program's overlap of one
// base): one gene in E: that gene, by an exon; two or more: several; E empty: one gene in B: that gene, by an
// intron; none: none; two or more: several.  all (GeneFull on derived bodies): one gene in B: that gene, by an exon
// where E is not empty, else by an intron; none: none; two or more: several.  off: the run without the flag, byte
// for byte.  The minimum overlap is 1 throughout: a block that starts in an exon and runs on into the intron is
// assigned by the exon.  The one call is umi_assign_genes_introns in umi_assign_genes' place; everything behind the
// gene's id is --per-gene's, unchanged.  The summary gains, behind "Number of annotation lines on unknown
// references": "Gene introns: <mode>", "Number of reads assigned by an exon", "Number of reads assigned by an
// intron" (over every mapped read the call saw).  Refused with status 101 before the GPU is woken: the flag without
// --gene-annotation; a value other than off, exon-first, all; the flag given twice with different values.
// Not built: STARsolo's Ex50pAS half-of-the-read rule, antisense counting, --paired.
//
// --velocity (with --gene-annotation, --gene-introns exon-first|all and --count-matrix DIR; tests/velocity_model.py
// defines it): the matrix's molecules in three layers -- spliced, unspliced, ambiguous -- what STARsolo's --soloFeatures
// Velocyto, velocyto and alevin-fry's USA mode give scVelo and its kin.  The rule is at gene level and in exact integers;
// it is NOT velocyto's or STARsolo's transcript-model rule (classes by transcript model: --transcript-introns, above).  A read's
// gene, status and tier are --gene-introns', unchanged.  The class of an assigned read with gene g: its blocks are cut
// to [0, 2^31) and the empty ones left out; the cover of a stretch is the number of its bases in one of g's taken lines
// on the read's reference and an admissible strand.  Assigned by an intron: intronic.  By an exon: where the blocks are
// not covered whole, exon-intron (the read leaves the exons, into an intron or past the gene's end); else, where a
// stretch that an N skipped between two blocks is not covered whole, junction (the read skips an intron); else exonic.
// A molecule is a kept entry; its reads are the staged reads whose entry's root it is.  With a junction read and no
// exon-intron or intronic read it is spliced; with an exon-intron or intronic read and no junction read, unspliced;
// with both kinds, or with exonic reads alone (alevin-fry's A), ambiguous.  A molecule --umi-filtering multi-gene removed
// counts nowhere.  The classes are relative to the lines taken: under --annotation-feature gene the lines are whole genes, no read
// is intronic, and every assigned read that stays inside its gene is exonic; this is documented, not refused.
// The one call over the reads is umi_assign_genes_classes in umi_assign_genes_introns' place (the same gene, status,
// tier and counts, and a class per read); the flag stages on the host, as --tag does, because the host staging keeps
// every read's entry; after umi_count_matrix one call to umi_velocity_matrix gives the layers of that matrix's
// triplets.  Written: DIR/velocity/features.tsv and barcodes.tsv (the raw ones' bytes) and spliced.mtx, unspliced.mtx,
// ambiguous.mtx, matrix.mtx's layout, each with its non-zero entries alone and its own line count in the header; the
// three add up to matrix.mtx pair by pair.  With --cell-filter the same five files under DIR/velocity/filtered/ for the
// called cells, columns renumbered as in DIR/filtered/; the cells are called from the total matrix, as without the flag.
// The summary gains "Velocity: on", "Number of exonic reads", "Number of junction reads", "Number of exon-intron reads",
// "Number of intronic reads" (over every mapped read the call saw) and "Number of spliced molecules", "Number of
// unspliced molecules", "Number of ambiguous molecules" (together "Number of reads after deduplicating").  The BAM, the
// four raw files, filtered/, cells.tsv and the other summary lines are what --stage host writes without the flag.
// Refused with status 101 before the GPU is woken: --velocity without --count-matrix, without --gene-annotation, with
// --gene-introns absent or off (with --gene-rule transcript: --transcript-introns absent or off), with --stage gpu.  Not
// built: velocyto's or STARsolo's own rules, a read's entry from the GPU staging, --two-pass, --paired.
#pragma once
#include <unordered_map>

#include "cli.hpp"
#include "fastq.hpp"

namespace {

// the value of `key` among column 9's attributes, `key "value";` (a bare value is taken up to the ;): false where
// the key is absent
bool gtf_attribute(std::string_view attrs, std::string_view key, std::string_view &value)
{
    size_t p = 0;
    while (p < attrs.size()) {
        while (p < attrs.size() && (attrs[p] == ' ' || attrs[p] == ';')) p++;
        const size_t k0 = p;
        while (p < attrs.size() && attrs[p] != ' ' && attrs[p] != ';') p++;
        const std::string_view k = attrs.substr(k0, p - k0);
        while (p < attrs.size() && attrs[p] == ' ') p++;
        std::string_view v;
        if (p < attrs.size() && attrs[p] == '"') {
            const size_t v0 = ++p;
            while (p < attrs.size() && attrs[p] != '"') p++;
            v = attrs.substr(v0, p - v0);
            if (p < attrs.size()) p++;
        } else {
            const size_t v0 = p;
            while (p < attrs.size() && attrs[p] != ';') p++;
            size_t v1 = p;
            while (v1 > v0 && attrs[v1 - 1] == ' ') v1--;
            v = attrs.substr(v0, v1 - v0);
        }
        if (!k.empty() && k == key) {
            value = v;
            return true;
        }
    }
    return false;
}

void read_annotation(Cli &args)
{
    umi::bgzf::Bytes text;
    try {
        text = umi::fastq::read_all(args.gene_annotation, args.num_threads);
    } catch (const std::exception &e) {
        die("cannot read the gene annotation " + args.gene_annotation + ": " + e.what());
    }
    Cli::Annotation &an = args.annotation;
    std::unordered_map<std::string, uint32_t> ref_of;
    std::unordered_map<std::string, int32_t> gene_of, transcript_of;
    const std::string_view all((const char *)text.data(), text.size());
    size_t line_no = 0;
    for (size_t p = 0; p < all.size();) {
        size_t q = all.find('\n', p);
        if (q == std::string_view::npos) q = all.size();
        std::string_view line = all.substr(p, q - p);
        p = q + 1;
        line_no++;
        if (!line.empty() && line.back() == '\r') line.remove_suffix(1);
        if (line.empty() || line[0] == '#') continue;
        const std::string where = "gene annotation " + args.gene_annotation + ", line " + std::to_string(line_no) + ": ";
        std::string_view col[9];
        size_t c = 0, at = 0;
        for (; c < 9; c++) {
            const size_t tab = c < 8 ? line.find('\t', at) : std::string_view::npos;
            col[c] = line.substr(at, tab == std::string_view::npos ? std::string_view::npos : tab - at);
            if (tab == std::string_view::npos) break;
            at = tab + 1;
        }
        if (c < 8) die(where + "fewer than nine tab-separated columns");
        if (col[2] != args.annotation_feature) continue;
        long long se[2];
        for (int i = 0; i < 2; i++) {
            const std::string v(col[3 + i]);
            const bool digits = !v.empty() && v.size() <= 10 && v.find_first_not_of("0123456789") == std::string::npos;
            if (!digits) die(where + (i ? "the end '" : "the start '") + v + "' is not a number");
            se[i] = std::atoll(v.c_str());
        }
        if (se[0] < 1) die(where + "a start below 1");
        if (se[1] < se[0]) die(where + "the end " + std::to_string(se[1]) + " lies before the start " + std::to_string(se[0]));
        if (se[1] > INT32_MAX) die(where + "the end " + std::to_string(se[1]) + " lies beyond 2^31 - 1");
        if (col[6] != "+" && col[6] != "-" && col[6] != ".") die(where + "the strand '" + std::string(col[6]) + "' is none of + - .");
        std::string_view id, name;
        if (!gtf_attribute(col[8], args.annotation_attribute, id)) die(where + "no attribute " + args.annotation_attribute);
        if (id.empty()) die(where + "the attribute " + args.annotation_attribute + " is empty");
        for (const char ch : id)
            if ((uint8_t)ch < 0x21 || (uint8_t)ch > 0x7e || ch == ';' || ch == ',')
                die(where + "the attribute " + args.annotation_attribute + " holds a byte that a gene's name cannot: " +
                    std::to_string((unsigned)(uint8_t)ch));
        const auto g = gene_of.emplace(std::string(id), (int32_t)an.gene_ids.size());
        if (g.second) {
            an.gene_ids.emplace_back(id);
            an.gene_names.emplace_back(gtf_attribute(col[8], "gene_name", name) ? name : std::string_view());
        }
        const auto r = ref_of.emplace(std::string(col[0]), (uint32_t)an.refs.size());
        if (r.second) an.refs.emplace_back(col[0]);
        an.ref_name.push_back(r.first->second);
        an.start.push_back((int32_t)(se[0] - 1));
        an.end.push_back((int32_t)se[1]);
        an.strand.push_back((uint8_t)col[6][0]);
        an.gene.push_back(g.first->second);
        if (!args.gene_rule_transcript) continue;
        // the line's transcript: (gene, the attribute's value, reference, strand as written)
        const std::string &ta = args.annotation_transcript_attribute;
        std::string_view tv;
        if (!gtf_attribute(col[8], ta, tv)) die(where + "no attribute " + ta);
        if (tv.empty()) die(where + "the attribute " + ta + " is empty");
        for (const char ch : tv)
            if ((uint8_t)ch < 0x21 || (uint8_t)ch > 0x7e || ch == ';' || ch == ',')
                die(where + "the attribute " + ta + " holds a byte that a transcript's name cannot: " + std::to_string((unsigned)(uint8_t)ch));
        std::string key = std::to_string(g.first->second) + '\t' + std::to_string(r.first->second) + '\t' + col[6][0] + '\t';
        key.append(tv);
        const auto t = transcript_of.emplace(std::move(key), (int32_t)transcript_of.size());
        an.transcript.push_back(t.first->second);
    }
    an.n_transcripts = (uint32_t)transcript_of.size();
    if (an.gene.empty())
        die("the gene annotation " + args.gene_annotation + " holds no line of feature type " + args.annotation_feature);
}

} // namespace
