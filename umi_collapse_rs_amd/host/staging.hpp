// What BAM mode's staging is made of, shared by the one-pass pipeline and --two-pass: UMI and alignment keys,
// the filters of the read loop, the tags a read is looked up by, the host staging of one position and the
// summary lines.
//
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
//
// --per-gene (bam/sam mode, one pass; umi_tools --per-gene, Cell Ranger, STARsolo; tests/gene_model.py defines it):
// a staged read's gene is the value of --gene-tag (default GX, type Z), compared byte for byte, and a bucket is
// (gene) -- with --per-cell (cell, gene) -- whatever the alignment: strand, unclipped position, reference and
// template length play no part, so one molecule fragmented at two places is one entry.  A tag of another type, a
// malformed aux block or a value with a byte below 0x21 or above 0x7e ends the run with status 101.  A read
// without the tag, with an empty value, the value "-", or a value that starts with "__" or "Unassigned" has no
// gene (MISS_GENE: dropped like a read without its UMI tag, "Number of reads without a gene tag"); one whose
// value holds ';' or ',' is assigned to several and dropped too ("Number of reads assigned to several genes").
// A gene's id is the rank of its first appearance among the staged reads in file order.  In the host staging
// the key's coord / ref_strand / tlen are zero and `gene` tells the buckets apart; the device staging gets a
// constant alignment key of one bit and cell | gene << bits_of(n_cells) as the group key.  Bucket and entry
// order, the merge rule and what is written are as ever.  The summary gains the two lines, "Number of genes"
// and "Number of (cell, gene) groups" ("Number of gene groups" without --per-cell) and loses "Number of unique
// alignment positions"; --dump-staging appends every bucket's gene id behind the cell ids.
//
// --gene-annotation (annotation.hpp): the gene is what umi_assign_genes made of the read (AssignedGene below) and
// the tag is not looked at; a read outside every gene is dropped like one without the tag ("Number of reads outside
// every gene" in that line's place), one in several genes like one whose tag names several.
//
// --cell-whitelist-multi (cli.hpp has the flags, umicollapse_main.cpp the call): a read with the cell barcode tag
// must carry --cell-quality-tag (default CY, type Z) as well -- a read with the one and without the other ends the
// run with status 101, as a tag of another type does; its length and bytes (33..126) are looked at where the
// barcode's are.  The summary gains "Number of reads with a resolved cell barcode" after the corrected ones, and
// write_list_metrics the column `resolved`.
#pragma once
#include <string_view>
#include <unordered_map>

#include "bam.hpp"
#include "bgzf.hpp"
#include "cli.hpp"

namespace {

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

struct Entry { // one (alignment key, UMI): ReadFreq of src/utils/read_freq.rs + its key
    UmiKey key, nmask;
    int32_t freq;
    int32_t score;  // avg qual or mapq of the representative
    uint32_t rep;   // record index of the representative read
    uint32_t index; // its place in the canonical order, once its position has been emitted
};

// Align (deduplicate_sam.rs:478-481): Alignment{strand, coord, ref} or, with --paired,
// PairedAlignment{strand, coord, ref, tlen} (:547-553); ref as tid (equal names <=> equal tid)
struct AlignKey {
    uint64_t coord, ref_strand, tlen;
    uint64_t cell = 0; // --per-cell: the barcode's dense id (first-appearance rank); 0 otherwise
    uint64_t gene = 0; // --per-gene: the gene's dense id (the three alignment fields are then 0); 0 otherwise
    bool operator==(const AlignKey &o) const
    {
        return coord == o.coord && ref_strand == o.ref_strand && tlen == o.tlen && cell == o.cell && gene == o.gene;
    }
};

struct KeyHash {
    size_t operator()(const AlignKey &k) const
    {
        uint64_t x = k.coord * 0x9E3779B97F4A7C15ull ^ (k.ref_strand + 0x7F4A7C15u) ^ (k.tlen * 0xD6E8FEB86659FD93ull) ^
                     (k.cell * 0x94D049BB133111EBull) ^ (k.gene * 0xC2B2AE3D27D4EB4Full);
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

// --umi-tag / --per-cell / --per-gene: the aux tags a staged read is looked up by.  Returns the bits of the ones
// it lacks (MISS_UMI, MISS_CELL, MISS_GENE: the read is dropped, not written, and counted); err: the message
// that ends the run (a malformed aux block, a tag that is not of type Z, a gene with a byte that is not a
// printable character).
enum : uint8_t { MISS_UMI = 1, MISS_CELL = 2, MISS_GENE = 4 };
struct ReadTags {
    const uint8_t *umi = nullptr; // --umi-tag: the value
    size_t umi_len = 0;
    std::string_view cell;        // --per-cell: the barcode, an opaque byte string
    std::string_view cell_qual;   // --cell-whitelist-multi: its qualities (--cell-quality-tag)
    std::string_view gene;        // --per-gene: the gene, likewise
    bool several_genes = false;   // ... its value lists more than one (';' or ','): the read is dropped
};
// --gene-annotation: what umi_assign_genes made of a read (UMI_GENE_*), and the gene's id where it is assigned
struct AssignedGene {
    uint8_t status = UMI_GENE_NONE;
    std::string_view id;
};
uint8_t read_tags(const Cli &args, const umi::bam::Record &r, ReadTags &t, std::string &err, const AssignedGene *assigned = nullptr)
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
        if (!err.empty()) return 0;
        if (args.cell_wl_multi && !(miss & MISS_CELL)) { // a read with a barcode carries its qualities
            if (look(args.cell_qual_tag, f)) t.cell_qual = std::string_view((const char *)f.value, f.len);
            else if (err.empty())
                err = "read " + std::string((const char *)r.qname(), r.qname_len()) + " has the cell barcode tag " + args.cell_tag +
                      " without the quality tag " + args.cell_qual_tag;
            if (!err.empty()) return 0;
        }
    }
    if (args.per_gene && assigned) { // --gene-annotation: the tag is not looked at
        if (assigned->status == UMI_GENE_NONE) miss |= MISS_GENE;
        t.gene = assigned->id;
        t.several_genes = assigned->status == UMI_GENE_SEVERAL;
    } else if (args.per_gene) {
        std::string_view g;
        if (look(args.gene_tag, f)) g = std::string_view((const char *)f.value, f.len);
        if (!err.empty()) return 0;
        for (const char ch : g)
            if ((uint8_t)ch < 0x21 || (uint8_t)ch > 0x7e) {
                err = "tag " + args.gene_tag + " of read " + std::string((const char *)r.qname(), r.qname_len()) +
                      " holds a byte that is not a printable character: " + std::to_string((unsigned)(uint8_t)ch);
                return 0;
            }
        if (g.empty() || g == "-" || g.substr(0, 2) == "__" || g.substr(0, 10) == "Unassigned") miss |= MISS_GENE;
        t.gene = g;
        t.several_genes = g.find_first_of(";,") != std::string_view::npos;
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

// ---- the host staging of one position (deduplicate_sam.rs:148-176), shared by the one-pass shards and the
// windows of --two-pass.  `index` maps the position's UMIs to their entries in `entries` (which may hold other
// positions' too), `members` lists the position's entries in order of first appearance.
using UmiIndex = std::unordered_map<UmiKey, uint32_t, UmiKeyHash>;
using U64s = std::vector<uint64_t, umi::bgzf::default_init_allocator<uint64_t>>; // (not zeroed when sized)
using I32s = std::vector<int32_t, umi::bgzf::default_init_allocator<int32_t>>;

// a read joins its position: a new entry, or one more read of an entry that keeps the better representative.
// Returns the entry.
uint32_t add_read(UmiIndex &index, std::vector<Entry> &entries, std::vector<uint32_t> &members, const UmiKey &key,
                  const UmiKey &nmask, int32_t score, uint32_t read, int merge)
{
    const auto e = index.find(key);
    if (e == index.end()) { // Vacant :161-163
        const uint32_t ei = (uint32_t)entries.size();
        index.emplace(key, ei);
        members.push_back(ei);
        entries.push_back({key, nmask, 1, score, read, 0});
        return ei;
    }
    Entry &en = entries[e->second]; // Occupied :164-175
    const bool keep_existing = merge == 0 ? true : en.score >= score; // merge/mod.rs:21,35,49
    en.freq += 1;
    if (!keep_existing) { en.rep = read; en.score = score; }
    return e->second;
}

// a position's entries go out in the stable freq-descending order of directional.rs:67-72 (creation order of
// a position's entries = first appearance): n_words key and mask words and the frequency of each, from entry
// `w` of the arrays on; every entry learns its index, `members` is left in that order
void emit_position(std::vector<Entry> &entries, std::vector<uint32_t> &members, int n_words, uint64_t *keys, uint64_t *nmask,
                   int32_t *freq, size_t &w)
{
    std::stable_sort(members.begin(), members.end(), [&](uint32_t x, uint32_t y) { return entries[y].freq < entries[x].freq; });
    for (uint32_t ei : members) {
        Entry &en = entries[ei];
        for (int q = 0; q < n_words; q++) {
            keys[w * n_words + q] = en.key.w[q];
            nmask[w * n_words + q] = en.nmask.w[q];
        }
        freq[w] = en.freq;
        en.index = (uint32_t)w++;
    }
}

// --whitelist-metrics / --cell-whitelist-metrics: per listed item, in list order, the reads it took, exact and
// corrected (status 0: exact); `used_only` leaves out the items that took none.  `with_resolved`
// (--cell-whitelist-multi): a fifth column, the reads of status UMI_BARCODE_RESOLVED, counted among `reads` too
void write_list_metrics(const std::string &path, const char *item, const std::vector<uint8_t> &list, size_t L,
                        const std::vector<int32_t> &match, const std::vector<uint8_t> &status, bool used_only,
                        bool with_resolved = false)
{
    const size_t n_wl = list.size() / L;
    std::vector<uint64_t> exact(n_wl, 0), corrected(n_wl, 0), resolved(n_wl, 0);
    for (size_t j = 0; j < match.size(); j++)
        if (match[j] >= 0)
            (status[j] == 0 ? exact : with_resolved && status[j] == UMI_BARCODE_RESOLVED ? resolved : corrected)[(size_t)match[j]]++;
    FILE *f = std::fopen(path.c_str(), "wb");
    if (!f) die("cannot open " + path);
    std::fprintf(f, with_resolved ? "%s\treads\texact\tcorrected\tresolved\n" : "%s\treads\texact\tcorrected\n", item);
    for (size_t w = 0; w < n_wl; w++)
        if (!used_only || exact[w] + corrected[w] + resolved[w]) {
            std::fprintf(f, "%.*s\t%llu\t%llu\t%llu", (int)L, (const char *)&list[w * L],
                         (unsigned long long)(exact[w] + corrected[w] + resolved[w]), (unsigned long long)exact[w],
                         (unsigned long long)corrected[w]);
            if (with_resolved) std::fprintf(f, "\t%llu", (unsigned long long)resolved[w]);
            std::fputc('\n', f);
        }
    if (std::fclose(f) != 0) die("cannot write " + path);
}

// counters of deduplicate_sam.rs:243-268 and this build's own, printed by one pass, --two-pass and (the lines
// about tags and cells only) the --dump-staging exit
struct Summary {
    size_t total_read_count = 0, unmapped = 0, unpaired = 0, chimeric = 0, no_umi_tag = 0, no_cell = 0;
    size_t no_gene = 0, several_genes = 0, n_genes = 0; // --per-gene
    size_t annotation_genes = 0, annotation_features = 0, annotation_unknown = 0; // --gene-annotation: on the file's references
    size_t annotation_transcripts = 0; // --gene-rule transcript: the transcripts of the lines on the BAM's references
    uint64_t by_exon = 0, by_intron = 0; // --gene-introns exon-first|all: the call's reads assigned by either tier
    uint64_t class_counts[5] = {0, 0, 0, 0, 0}; // --velocity: the call's reads by class (UMI_READ_CLASS_*)
    uint64_t layers[3] = {0, 0, 0};             // ... and the molecules: spliced, unspliced, ambiguous
    uint64_t cb_counts[5] = {0, 0, 0, 0, 0}; // --cell-whitelist: exact, corrected, unlisted, ambiguous, (-multi) resolved
    uint64_t wl_counts[3] = {0, 0, 0};    // --umi-whitelist: exact, corrected, uncorrectable
    size_t n_positions = 0, nb = 0, n = 0, max_umi = 0;
    uint64_t n_kept = 0;
    size_t n_below = 0, n_without = 0; // --call-consensus
    uint64_t mg_counts[3] = {0, 0, 0}; // --umi-filtering multi-gene: UMIs in several genes of a cell, molecules removed, their reads
    uint64_t cell_counts[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0}; // --cell-filter: umi_call_cells' counts
    uint64_t saturation_reads = 0, saturation_molecules = 0; // --saturation-curve: the full depth's counted reads and molecules
    uint64_t junction_counts[4] = {0, 0, 0, 0}; // --junction-matrix: umi_junction_matrix' counts
    // floor(10000 (reads - molecules) / reads) as 0.dddd, in integers; 0.0000 for no reads (--saturation-curve)
    static std::string saturation_text(uint64_t reads, uint64_t molecules)
    {
        const unsigned long long v = reads ? (unsigned long long)((unsigned __int128)10000 * (reads - molecules) / reads) : 0ull;
        char text[32];
        std::snprintf(text, sizeof text, "%llu.%04llu", v / 10000ull, v % 10000ull);
        return text;
    }
    void print(const Cli &args, bool dump_exit = false) const
    {
        if (!dump_exit) {
            std::fprintf(stderr, "Number of input reads: %zu\n", total_read_count);
            std::fprintf(stderr, "Number of removed unmapped reads: %zu\n", unmapped);
            if (args.paired) {
                std::fprintf(stderr, "Number of unpaired reads: %zu\n", unpaired);
                std::fprintf(stderr, "Number of chimeric reads: %zu\n", chimeric);
            }
        }
        if (!args.umi_tag.empty()) std::fprintf(stderr, "Number of reads without a UMI tag: %zu\n", no_umi_tag);
        if (args.per_cell) std::fprintf(stderr, "Number of reads without a cell barcode: %zu\n", no_cell);
        if (args.per_gene) {
            std::fprintf(stderr, "Number of reads %s: %zu\n", args.gene_annotation_given ? "outside every gene" : "without a gene tag", no_gene);
            std::fprintf(stderr, "Number of reads assigned to several genes: %zu\n", several_genes);
            if (args.gene_annotation_given) {
                std::fprintf(stderr, "Gene annotation: %zu genes, %zu features\n", annotation_genes, annotation_features);
                std::fprintf(stderr, "Gene strand: %s\n", args.gene_strand.c_str());
                std::fprintf(stderr, "Number of annotation lines on unknown references: %zu\n", annotation_unknown);
                if (args.gene_rule_transcript) {
                    std::fprintf(stderr, "Gene rule: transcript\n");
                    std::fprintf(stderr, "Number of transcripts: %zu\n", annotation_transcripts);
                }
                if (args.transcript_introns_mode != UMI_INTRONS_OFF) {
                    std::fprintf(stderr, "Transcript introns: %s\n", args.transcript_introns.c_str());
                    std::fprintf(stderr, "Number of reads assigned by a transcript: %llu\n", (unsigned long long)by_exon);
                    std::fprintf(stderr, "Number of reads assigned by a gene body: %llu\n", (unsigned long long)by_intron);
                }
                if (args.gene_introns_mode != UMI_INTRONS_OFF) {
                    std::fprintf(stderr, "Gene introns: %s\n", args.gene_introns.c_str());
                    std::fprintf(stderr, "Number of reads assigned by an exon: %llu\n", (unsigned long long)by_exon);
                    std::fprintf(stderr, "Number of reads assigned by an intron: %llu\n", (unsigned long long)by_intron);
                }
            }
        }
        if (!args.cell_list.empty()) {
            std::fprintf(stderr, "Number of reads with a corrected cell barcode: %llu\n", (unsigned long long)cb_counts[1]);
            if (args.cell_wl_multi)
                std::fprintf(stderr, "Number of reads with a resolved cell barcode: %llu\n", (unsigned long long)cb_counts[4]);
            std::fprintf(stderr, "Number of reads with an unlisted cell barcode: %llu\n", (unsigned long long)cb_counts[2]);
            std::fprintf(stderr, "Number of reads with an ambiguous cell barcode: %llu\n", (unsigned long long)cb_counts[3]);
        }
        if (!args.whitelist.empty()) {
            std::fprintf(stderr, "Number of reads with a corrected UMI: %llu\n", (unsigned long long)wl_counts[1]);
            std::fprintf(stderr, "Number of reads with an uncorrectable UMI: %llu\n", (unsigned long long)wl_counts[2]);
        }
        if (args.per_gene) { // (positions play no part)
            std::fprintf(stderr, "Number of genes: %zu\n", n_genes);
            std::fprintf(stderr, args.per_cell ? "Number of (cell, gene) groups: %zu\n" : "Number of gene groups: %zu\n", nb);
        } else {
            if (!dump_exit || args.per_cell) std::fprintf(stderr, "Number of unique alignment positions: %zu\n", n_positions);
            if (args.per_cell) std::fprintf(stderr, "Number of (position, cell) groups: %zu\n", nb);
        }
        if (dump_exit) return;
        std::fprintf(stderr, "Number of UMIs: %zu\n", n);
        std::fprintf(stderr, "Average number of UMIs per alignment position: %g\n", nb ? (double)n / (double)nb : 0.0);
        std::fprintf(stderr, "Max number of UMIs over all alignment positions: %zu\n", max_umi);
        std::fprintf(stderr, args.track_clusters ? "Number of groups of reads: %llu\n" : "Number of reads after deduplicating: %llu\n",
                     (unsigned long long)n_kept); // :259-266
        if (args.edit_distance) std::fprintf(stderr, "UMI distance: edit\n");
        if (args.algo_cr) std::fprintf(stderr, "UMI correction: cr\n");
        if (args.filter_multigene) {
            std::fprintf(stderr, "UMI filtering: multi-gene\n");
            std::fprintf(stderr, "Number of UMIs seen in several genes of a cell: %llu\n", (unsigned long long)mg_counts[0]);
            std::fprintf(stderr, "Number of molecules removed as multi-gene UMIs: %llu\n", (unsigned long long)mg_counts[1]);
            std::fprintf(stderr, "Number of reads in removed molecules: %llu\n", (unsigned long long)mg_counts[2]);
        }
        if (args.cell_filter_given) {
            const unsigned long long *c = (const unsigned long long *)cell_counts;
            std::fprintf(stderr, "Cell filter: %s\n", args.cell_filter.c_str());
            std::fprintf(stderr, "Number of candidate cells: %llu\n", c[0]);
            std::fprintf(stderr, "Number of cells called: %llu\n", c[1]);
            std::fprintf(stderr, "Molecule threshold: %llu\n", c[2]);
            std::fprintf(stderr, "Number of molecules in called cells: %llu\n", c[4]);
            std::fprintf(stderr, "Number of reads in called cells: %llu\n", c[5]);
            std::fprintf(stderr, "Median molecules per called cell: %llu\n", c[8]);
            std::fprintf(stderr, "Median genes per called cell: %llu\n", c[9]);
        }
        if (args.velocity) {
            std::fprintf(stderr, "Velocity: on\n");
            std::fprintf(stderr, "Number of exonic reads: %llu\n", (unsigned long long)class_counts[UMI_READ_CLASS_EXONIC]);
            std::fprintf(stderr, "Number of junction reads: %llu\n", (unsigned long long)class_counts[UMI_READ_CLASS_JUNCTION]);
            std::fprintf(stderr, "Number of exon-intron reads: %llu\n", (unsigned long long)class_counts[UMI_READ_CLASS_SPANNING]);
            std::fprintf(stderr, "Number of intronic reads: %llu\n", (unsigned long long)class_counts[UMI_READ_CLASS_INTRONIC]);
            std::fprintf(stderr, "Number of spliced molecules: %llu\n", (unsigned long long)layers[0]);
            std::fprintf(stderr, "Number of unspliced molecules: %llu\n", (unsigned long long)layers[1]);
            std::fprintf(stderr, "Number of ambiguous molecules: %llu\n", (unsigned long long)layers[2]);
        }
        if (!args.saturation_curve.empty()) {
            std::fprintf(stderr, "Saturation curve: %d points, seed %llu\n", args.saturation_points, (unsigned long long)args.saturation_seed);
            std::fprintf(stderr, "Sequencing saturation: %s\n", saturation_text(saturation_reads, saturation_molecules).c_str());
        }
        if (args.call_consensus) {
            std::fprintf(stderr, "Number of clusters below --call-consensus-min-reads: %zu\n", n_below);
            std::fprintf(stderr, "Number of clusters without a consensus: %zu\n", n_without);
        }
        if (args.junction_matrix) {
            std::fprintf(stderr, "Junction matrix: on\n");
            std::fprintf(stderr, "Number of spliced reads counted: %llu\n", (unsigned long long)junction_counts[0]);
            std::fprintf(stderr, "Number of junction occurrences: %llu\n", (unsigned long long)junction_counts[1]);
            std::fprintf(stderr, "Number of distinct junctions: %llu\n", (unsigned long long)junction_counts[2]);
            std::fprintf(stderr, "Number of (cell, junction) pairs: %llu\n", (unsigned long long)junction_counts[3]);
        }
    }
};
} // namespace
