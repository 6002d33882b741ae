/*
 * umihip.h -- C ABI of the MI355X (gfx950) UMI-collapse hot path.
 *
 * This is the drop-in boundary for tkob-vh/umi-collapse-rs.  The reference has
 * no FFI of its own; the seam is its pair of generic traits
 *     trait Algorithm  { fn apply(..) }                    src/algo/mod.rs:13-20
 *     trait DataStruct { new / remove_near / contains }    src/data/mod.rs:11-17
 * called from the bucket loop src/deduplicate_sam.rs:207-233.  Every entry point
 * below names the reference interface it replaces.  Plain pointers and sizes
 * only; nothing here throws or unwinds (the reference builds with panic=abort,
 * Cargo.toml:19): failures come back as a negative status and a thread-local
 * message from umi_last_error().
 *
 * Key format (all entry points): one uint64 per UMI = BitSet.bits[0] of the
 * reference (src/utils/bitset.rs:9-14) for umi_len <= 21, i.e. base i occupies
 * bits 3i..3i+2 with A=000 T=101 C=110 G=011 N=100 (src/utils/read.rs:23-31,
 * src/utils/mod.rs:38-41); nmask = BitSet.n_bits[0] (bits 3i..3i+2 set where
 * base i is N; src/utils/mod.rs:45-50), NULL when no UMI holds an N.
 */
#ifndef UMIHIP_H
#define UMIHIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define UMI_OK 0
#define UMI_ERR_ARG (-1)   /* invalid argument */
#define UMI_ERR_HIP (-2)   /* HIP runtime failure (message has the hipError) */
#define UMI_ERR_ORDER (-3) /* entries of a bucket are not in rank order / freq < 1 */
#define UMI_ERR_NOMEM (-4)
#define UMI_ERR_NODEV (-5) /* no usable gfx950 device */
#define UMI_ERR_CHAR (-6)  /* character outside ATCGN (reference: panic, utils/mod.rs:77-79) */

#define UMI_ALGO_DIRECTIONAL 0 /* src/algo/directional.rs */
#define UMI_ALGO_ADJACENCY 1   /* src/algo/adjacency.rs  */
#define UMI_ALGO_CLUSTER 2     /* connected components of "within k" (the reference's unimplemented `cc`) */

#define UMI_MAX_UMI_LEN 21 /* one 64-bit word per key (3 bits per base) */
#define UMI_MAX_WIDE_UMI_LEN 85 /* the _wide entry points: up to 4 words per key */
#define UMI_MAX_SEQ_LEN 256     /* whole reads (umi_dedup_seqs): up to 12 words per key */

typedef struct umi_ctx umi_ctx;   /* one per process/GPU; not re-entrant (the reference calls
                                     apply strictly sequentially, deduplicate_sam.rs:207) */
typedef struct umi_data umi_data; /* device-backed DataStruct instance */

/* Counters of one batched call.  n_pairs is the algorithmic unit of work
 * W = sum_b n_b(n_b-1)/2; ms_* are HIP-event times on the call's
 * stream and are filled only when the "profile" option is on. */
typedef struct umi_stats {
    uint64_t n_umis;
    uint64_t n_buckets;
    uint64_t max_bucket;        /* max_umi_count of deduplicate_sam.rs:218 */
    uint64_t n_kept;            /* deduped_count of deduplicate_sam.rs:219 */
    uint64_t n_pairs;           /* W */
    uint64_t n_pairs_evaluated; /* pairs the filter kernels walked (tile padding included; key-sorted
                                 * buckets: only the column tiles their scan kept, see bs_tables) */
    uint64_t n_candidates;      /* filter hits sent to the exact check */
    uint64_t n_edges;           /* directed edges fed to the collapse */
    uint32_t n_rounds;          /* label-propagation rounds */
    uint32_t n_pair_launches;
    float ms_total;
    float ms_prep;
    float ms_pairs;
    float ms_collapse;
    float ms_finalize;
    /* (ABI version 2) with "profile": HIP-event time of the kernel that does the call's pair work, alone
     * -- what a roofline of the call is quoted on -- and which one it was */
    float ms_kernel;
    uint32_t kernel_id; /* UMI_KERNEL_* */
} umi_stats;
#define UMI_KERNEL_NONE 0
#define UMI_KERNEL_FUSED 1     /* small_bucket_kernel: one wave per position of <= 128 UMIs */
#define UMI_KERNEL_SEG_PAIRS 2 /* seg_pair_kernel: all pairs inside the n-gram sub-buckets of deep positions */
#define UMI_KERNEL_SEQ_PAIRS 3 /* seq_pair_kernel: the whole-read keys of umi_dedup_seqs */
#define UMI_KERNEL_EDIT_PAIRS 4 /* edit_pair_kernel: the Levenshtein distance of umi_dedup_batch_edit */

/* ---- context ----------------------------------------------------------- */
int umi_ctx_create(int device_id, umi_ctx **out);
/* One context over several GPUs of the node (n_devices in 1..64; an id may repeat: two workers on
 * one GPU).  umi_dedup_batch on it shards the call: independent buckets -- the iterations of
 * src/deduplicate_sam.rs:207-233 share nothing but additive counters -- go to the devices by
 * longest-processing-time on n_b^2, one host thread, stream and workspace per device, results
 * scattered back at the buckets' own offsets (no exchange between devices); a call whose work is
 * one giant bucket (>= "split_min" entries, more than half of the call's n_b^2) has that bucket's
 * pair work split over the devices instead, the edge lists gathered on the first one and collapsed
 * there.  Options set on it apply to every device.  The device-pointer entry points take a
 * single-device context (a device pointer belongs to one device); umi_data_new uses the first
 * device. */
int umi_ctx_create_multi(const int *device_ids, int n_devices, umi_ctx **out);
int umi_ctx_device_count(const umi_ctx *ctx); /* 1 for umi_ctx_create's, n_devices for the above */
void umi_ctx_destroy(umi_ctx *ctx);
/* The bucket -> rank assignment the multi-device context uses, for hosts that run one process per
 * GPU: owner[b] in [0, n_ranks) for every bucket, deterministic (every rank computes the same
 * table from bucket_off alone).  Host code, no GPU. */
int umi_partition_buckets(const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n_ranks,
                          uint32_t *owner);
/* Thread-local text of the last failure on this thread ("" if none). */
const char *umi_last_error(void);
/* Options (none of them changes a result; unknown name -> UMI_ERR_ARG):
 *   "profile"        0/1: record HIP events, fill the ms_* fields of umi_stats
 *   "edge_capacity"  initial capacity of the permitted-pair list, entries (it grows by itself)
 *   "fused_max"      0..128 (default 128): largest bucket the fused one-wave-per-bucket kernel takes
 *   "fused_blocks"   1..64 (default 20): 256-thread blocks per CU of that kernel's persistent grid
 *   "fused_sliced"   0/1 (default 1): that kernel's bit-sliced body for k <= 3 (0: columns one by one)
 *   "small_max"      (default 1024) largest bucket taken as 64-row popcount chunks; above, 2048-row tiles
 *   "seg_index"      0/1 (default 1): buckets of at least "seg_min" entries (default 512) are cut into
 *                    n-gram sub-buckets on the device -- two UMIs within k substitutions agree on one of
 *                    k + 1 base ranges -- and only the pairs inside a sub-bucket are evaluated; same
 *                    result as the all-pairs popcount kernels, which take those buckets when it is 0 or
 *                    when k + 1 parts would be shorter than 3 bases (the parity suite's cross-check);
 *                    n_pairs_evaluated counts the pairs inside the sub-buckets
 *   "seg_min"        2..2^31, see above
 *   "seg_blocks"     one-wave blocks of the segment index's pair kernel (0 = 16 per CU)
 *   "grid_cus"       0..the device's CUs (default 0 = the device's): the number of CUs every call sizes its grids
 *                    from.  A test handle: at 1 a few thousand items send every grid-stride kernel round its loop
 *                    several times, as half a million do on a whole device.  A value above the device's is
 *                    refused: the persistent grids must stay resident
 *   "seg_lds"        0/1 (default 1): its counting sort through per-block LDS histograms (0: one atomic
 *                    per entry)
 *   "seg_unite"      0/1 (default 1): symmetric pairs united where the pair kernel finds them (0: through
 *                    the list)
 *   "seg_local"      0/1 (default 1): on the batched directional path with "seg_unite" and 32-bit compare
 *                    keys, the part-0 sub-buckets of at most "seg_local_cap" entries are evaluated and
 *                    their symmetric pairs united in LDS by a kernel of their own, ahead of the pair kernel
 *                    (0: every sub-bucket through the pair kernel); same result and statistics
 *   "seg_local_cap"  2..2048 (default 512): largest part-0 sub-bucket that kernel takes (LDS: 16 bytes per entry)
 *   "seg_probe"      0/1 (default 1): k = 1 without N: in the sub-buckets that kernel takes, where at most six
 *                    bases lie outside the bins, the pairs are decided by lookups in a bitmap of the
 *                    sub-bucket instead of being compared one by one (0: the tile walk); same result and
 *                    statistics
 *   "seg_probe_min"  2..2048 (default 129): smallest sub-bucket decided by lookups
 *   "seg_super"      0/1 (default 1): k = 1 without N, on the calls "seg_local" applies to (whatever its value): a run
 *                    of 4^g adjacent part-0 sub-buckets -- they share all but g bases of their bin code and lie back
 *                    to back -- is decided as one unit out of LDS by a multi-wave block, so that the pairs that differ
 *                    in one of those g bases are united there instead of by the pair kernel's global unions (0: the
 *                    sub-buckets one by one); same result and statistics
 *   "seg_super_coarse" 0/1 (default 1): where "seg_super" and "seg_lds" apply, the counting sort files a part-0 entry
 *                    under the first sub-bucket of its run instead of its own -- nothing reads the order inside a
 *                    run, and a (block, run) costs one atomic and one stretch of stores where the 4^g sub-buckets
 *                    cost one each; a run above "seg_super_cap" goes through the pair kernel as one sub-bucket, a
 *                    hit kept only inside a sub-bucket (0: every entry under its own); same result and statistics
 *   "seg_cross"      0/1 (default 1): where "seg_super_coarse" applies, the pairs that differ in one of the bases a run
 *                    shares are read off the runs' bitmaps -- two such entries agree on every other base, so they are
 *                    the set bits of the AND of two runs' maps -- and the second partition of the segment is counted
 *                    but neither filed nor walked (0: through the pair kernel); same result and statistics.  A call
 *                    that holds a key twice or a run above "seg_super_cap" is done again without the path, and so are
 *                    the context's later calls until the option is set again
 *   "seg_cross_map_mb" 0..64 (default 8): the maps of one segment, 4^umi_len / 8 bytes, may take this much (12 and 13
 *                    bases by default; 64 MB per call)
 *   "seg_super_bases" 0..4 (default 0): g; 0 = the largest for which the other bases number at most 8 and the expected
 *                    run n / 4^(bin bases - g) lies between "seg_super_min" and 3/4 of "seg_super_cap", another
 *                    value = that g where those conditions hold (else none)
 *   "seg_super_cap"  2..8192 (default 5632): largest run that kernel takes (LDS: 16 bytes per entry + 16 KB + a hit queue of 512 bytes
 *                    per wave -- 155,648 bytes at 8192 with 1,024 threads, 51,200 at 2048 with 256); a larger
 *                    one goes through the pair kernel whole
 *   "seg_super_min"  2..8192 (default 1024): smallest expected run the path is planned for
 *   "collapse_kept_only" 0/1 (default 1): a batched directional call without d_root leaves the union-find
 *                    forest unflattened: only the endpoints of the one-way pairs are followed to their
 *                    roots, and the mask is read off parent[] and lab[] (0: flatten as a call with d_root does)
 *   "seg_ckey"       0/1 (default 1): the pair kernel compares 3-bit-per-base compare keys where the bases
 *                    outside a bin fit 32 bits (0: the 2-bit filter keys)
 *   "seg_sliced"     0/1 (default 1): ... 64 columns of a tile at a time, from wave ballots of the columns'
 *                    code bits (k <= 3); 0: one broadcast column at a time
 *   "spin_wait"      0/1 (default 1): the end of a batched call is seen by watching a word in pinned host
 *                    memory that the stream's last kernel writes (0: hipStreamSynchronize)
 *   "table_pieces"   1..64 (default 1): a bucket table of more than 4096 positions is walked, uploaded
 *                    and handed to the fused kernel in this many pieces
 *   "split_min"      multi-device contexts, see umi_ctx_create_multi
 *   "cons_split"     2..2^30 (default 512): umi_consensus_seqs / umi_consensus_bam sum a cluster of at least this many reads in
 *                    pieces over the whole grid instead of by one wave (raised by itself where the deep
 *                    clusters' accumulators, 12 KB each, would pass 512 MB)
 *   "stats_split"    64..2^30 (default 4096): umi_dedup_stats counts a bucket of at least this many entries in pieces
 *                    over the whole grid instead of by one wave (raised by itself where the deep buckets' tables,
 *                    80 bytes per base each, would pass 512 MB)
 *   "cr_small_max"   0..1024 (default 128): umi_dedup_batch_cr decides a bucket of at most this many entries with one
 *                    lane per entry, a larger one from the list of neighbour pairs (0: every bucket from the list)
 *   "gene_top"       0/1 (default 1): umi_assign_genes searches a sampled top of its index in LDS before the
 *                    index itself (0: the index alone); umi_assign_genes_introns likewise, for both its tiers,
 *                    and umi_assign_genes_transcripts for its distinct exons
 *   "gene_body_top"  0/1 (default 1): with gene_top 1, umi_assign_genes_introns holds the gene bodies' tops in LDS
 *                    beside the exons' (0: the exons' alone); umi_assign_genes_classes takes both options alike
 *   "velocity_skip"  0/1 (default 0): 1: umi_velocity_matrix's reads load their molecule's evidence first and leave the
 *                    atomic out where their bit is set (0: an atomic per read with evidence).  The result is the same;
 *                    measured, the load costs more than it saves unless a molecule has very many reads
 *   "saturation_skip" 0/1 (default 0): 1: umi_saturation_curve's reads load their molecule's word of levels first and
 *                    leave the atomic out where their bit is set (0: an atomic per counted read).  The curve is the same
 * The round-1 tile kernels (bit-sliced masks, key-sorted scan + item walk, range pruning, hook/jump
 * collapse) and their options ("bitslice", "bs_*", "prune", "two_phase", "ovf_capacity") exist in the
 * development build only (make dev: libumihip_dev.so, -DUMIHIP_DEV), as cross-checks. */
int umi_ctx_set_option(umi_ctx *ctx, const char *name, int64_t value);
/* What a context has done since it was created, by name (for tests and tuning; the results of a call never depend on it):
 *   "seg_cross_launches"  attempts of its batched calls in which the kernel of "seg_cross" was launched
 *   "seg_cross_abandoned" calls that did their pair work again without that path (a key twice, a run above the cap) */
int umi_ctx_get_counter(const umi_ctx *ctx, const char *name, uint64_t *out);
/* Version of this header the library was built from (umi_stats grew in 2), for loaders */
#define UMI_ABI_VERSION 2
int umi_abi_version(void);

/* ---- staging helper: src/utils/mod.rs:63-83 (to_bitset) ---------------- */
/* n UMIs of umi_len ASCII bytes each, packed back to back -> keys / nmask
 * (nmask may be NULL).  Host code, no GPU.  UMI_ERR_CHAR where the reference
 * panics. */
int umi_encode_umis(const uint8_t *ascii, uint64_t n, int umi_len, uint64_t *keys,
                    uint64_t *nmask);

/* ---- keys of more than one word (umi_len 22..UMI_MAX_WIDE_UMI_LEN): BitSet.bits as
 *      n_words = ceil(3 * umi_len / 64) words per key, entry-major (keys[i * n_words + w] =
 *      bits[w] of entry i; nmask likewise or NULL), everything else as in umi_dedup_batch.  The
 *      distance is the reference's per-word arithmetic (src/utils/bitset.rs:77-91), a base that
 *      straddles two words included.  Positions of up to 128 UMIs go through the fused kernel (all
 *      words' bases sliced), deep positions through the n-gram partition of the first word's 21 bases
 *      (two UMIs within k overall are within k there) with every candidate pair decided on all words,
 *      the ones in between through an exact all-pairs kernel; a multi-device context shards the
 *      positions as for one-word keys.  Dual 12 + 12 UMIs are the 24-base, two-word case.
 *      algo = UMI_ALGO_CLUSTER: the connected components of that distance <= k (no fused kernel for these
 *      keys in that mode: the positions of up to 128 UMIs go through the all-pairs kernel as well).
 *      umi_encode_umis_wide is to_bitset (src/utils/mod.rs:63-83) for these lengths, host code. */
int umi_encode_umis_wide(const uint8_t *ascii, uint64_t n, int umi_len, int n_words, uint64_t *keys,
                         uint64_t *nmask);
int umi_dedup_batch_wide(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words,
                         const int32_t *freq, const uint64_t *bucket_off, uint64_t n_buckets,
                         int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                         uint8_t *kept, uint32_t *root, umi_stats *stats);
int umi_dedup_batch_wide_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                                int n_words, const int32_t *d_freq, const uint64_t *bucket_off,
                                uint64_t n_buckets, int umi_len, int k, float percentage, int algo,
                                int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root,
                                void *hip_stream, umi_stats *stats);

/* ---- whole reads as keys (FASTQ mode: the reference's src/main.rs:49-50 is a TODO; this build defines
 *      it, see host/umicollapse_main.cpp).  One bucket per read length, several lengths in one call.
 *      keys / nmask: n_words words per entry, entry-major (nmask may be NULL); 1 <= n_words <= 12 and
 *      n_words >= ceil(3 * bucket_len[b] / 64) for every bucket.  Bucket b uses the first
 *      ceil(3 * bucket_len[b] / 64) words of its keys (bucket_len[b] in 0..UMI_MAX_SEQ_LEN), the words
 *      behind them are zero.  Everything else -- rank order inside a bucket, kept / root, stats, any
 *      k >= 0, algo (UMI_ALGO_CLUSTER included), UMI_ERR_* -- as in umi_dedup_batch_wide; the distance is the reference's per-word
 *      arithmetic (src/utils/bitset.rs:77-91), straddling bases included.  Deep buckets are cut into
 *      k + 1 parts of the whole read and only pairs that agree exactly on one part are evaluated
 *      (n_pairs_evaluated counts them; kernel_id UMI_KERNEL_SEQ_PAIRS).  A multi-device context is
 *      UMI_ERR_ARG.  umi_encode_seqs is to_bitset (src/utils/mod.rs:63-83) per read, read i being the
 *      bytes [seq_off[i], seq_off[i + 1]) of ascii; host code, no GPU; UMI_ERR_CHAR outside ATCGN. */
int umi_encode_seqs(const uint8_t *ascii, const uint64_t *seq_off, uint64_t n, int n_words, uint64_t *keys,
                    uint64_t *nmask);
int umi_dedup_seqs(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                   const uint64_t *bucket_off, const int32_t *bucket_len, uint64_t n_buckets, int k,
                   float percentage, int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root,
                   umi_stats *stats);
int umi_dedup_seqs_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, int n_words,
                          const int32_t *d_freq, const uint64_t *bucket_off, const int32_t *bucket_len,
                          uint64_t n_buckets, int k, float percentage, int algo, int32_t adj_max_freq,
                          uint8_t *d_kept, uint32_t *d_root, void *hip_stream, umi_stats *stats);

/* ---- read staging on the device: the per-read part of
 *      DeduplicateSAM::deduplicate_and_merge, src/deduplicate_sam.rs:148-176
 *      (to_bitset per read, the per-position map UMI -> ReadFreq with freq += 1 and the kept read
 *      chosen by Merge, src/merge/mod.rs:18-51), and the rank order of a position's UMIs
 *      (src/algo/directional.rs:67-72), in the canonical determinisation: positions by first
 *      appearance in the file, UMIs of a position by freq descending, ties by first appearance.
 * in : per read, in file order: align_key (the caller's injective packing of the reference's
 *      Alignment -- strand, unclipped position, reference id, deduplicate_sam.rs:141-145,507-514 --
 *      into 64 bits, or any dense id; only its low align_key_bits bits are looked at),
 *      umi_len ASCII bytes of UMI, score (avg qual or mapq, may be NULL).
 *      merge: 0 = keep the first read of a UMI (merge "any"), 1 = the highest score, the first
 *      on ties (merge/mod.rs:35,49).
 * out: the batched path's input -- keys / nmask (may be NULL) / freq per unique (position, UMI)
 *      in canonical order, rep = file index of the read that represents it, bucket_off
 *      [*n_buckets + 1]; capacity n_reads (bucket_off: n_reads + 1), caller-owned.
 * UMI_ERR_CHAR for a character outside ATCGN (the reference panics, utils/mod.rs:77-79).
 * n_reads < 2^30 per call (UMI_ERR_ARG beyond).  The smaller align_key_bits, the fewer passes the
 * sort of the reads takes: where align_key_bits + 7 bits per 3 bases of UMI fit 64 bits (12-bp UMIs:
 * up to 36 bits of alignment key) the reads are sorted once, on one composed key.
 * The _device form takes and leaves everything in device memory (one synchronisation inside for
 * the two counts); the plain form copies host arrays in and out around it. */
int umi_stage_reads_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                           const uint8_t *d_umi_ascii, const int32_t *d_score, uint64_t n_reads,
                           int umi_len, int merge, uint64_t *d_keys, uint64_t *d_nmask,
                           int32_t *d_freq, uint64_t *d_rep, uint64_t *d_bucket_off,
                           uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream);
int umi_stage_reads(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits,
                    const uint8_t *umi_ascii, const int32_t *score, uint64_t n_reads, int umi_len,
                    int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq, uint64_t *rep,
                    uint64_t *bucket_off, uint64_t *n_entries, uint64_t *n_buckets);
/* The same for UMIs of up to UMI_MAX_WIDE_UMI_LEN bases: keys / nmask hold n_words =
 * ceil(3 * umi_len / 64) words per entry, entry-major (the input of umi_dedup_batch_wide). */
int umi_stage_reads_wide_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                                const uint8_t *d_umi_ascii, const int32_t *d_score, uint64_t n_reads, int umi_len,
                                int n_words, int merge, uint64_t *d_keys, uint64_t *d_nmask, int32_t *d_freq,
                                uint64_t *d_rep, uint64_t *d_bucket_off, uint64_t *n_entries, uint64_t *n_buckets,
                                void *hip_stream);
int umi_stage_reads_wide(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint8_t *umi_ascii,
                         const int32_t *score, uint64_t n_reads, int umi_len, int n_words, int merge, uint64_t *keys,
                         uint64_t *nmask, int32_t *freq, uint64_t *rep, uint64_t *bucket_off, uint64_t *n_entries,
                         uint64_t *n_buckets);
/* Grouped staging: the four calls above with a second per-read key, group_key (the low group_key_bits
 * bits looked at; 0 = none, group_key may then be NULL, and the call is the plain one).  A position is
 * then the pair (align_key, group_key): reads of different groups never share a bucket -- a cell barcode's
 * dense id puts every cell of a single-cell file in buckets of its own.  Buckets are ranked by first
 * appearance of the pair; merge, rank order, rep, outputs and errors as above.  The device sort takes the
 * group bits as more key bits: where align_key_bits + group_key_bits fit 64 bits the two are one word
 * (and with the UMI's 7 bits per 3 bases still one composed sort key where that fits 64 bits), else the
 * group word is sorted in passes of its own behind the alignment key's, and bucket boundaries look at
 * both words.  group_key_bits in 0..64, else UMI_ERR_ARG.  The plain calls are these with 0. */
int umi_stage_reads_grouped_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                                   const uint64_t *d_group_key, int group_key_bits, const uint8_t *d_umi_ascii,
                                   const int32_t *d_score, uint64_t n_reads, int umi_len, int merge, uint64_t *d_keys,
                                   uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep, uint64_t *d_bucket_off,
                                   uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream);
int umi_stage_reads_grouped(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint64_t *group_key,
                            int group_key_bits, const uint8_t *umi_ascii, const int32_t *score, uint64_t n_reads, int umi_len,
                            int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq, uint64_t *rep, uint64_t *bucket_off,
                            uint64_t *n_entries, uint64_t *n_buckets);
int umi_stage_reads_grouped_wide_device(umi_ctx *ctx, const uint64_t *d_align_key, int align_key_bits,
                                        const uint64_t *d_group_key, int group_key_bits, const uint8_t *d_umi_ascii,
                                        const int32_t *d_score, uint64_t n_reads, int umi_len, int n_words, int merge,
                                        uint64_t *d_keys, uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep,
                                        uint64_t *d_bucket_off, uint64_t *n_entries, uint64_t *n_buckets, void *hip_stream);
int umi_stage_reads_grouped_wide(umi_ctx *ctx, const uint64_t *align_key, int align_key_bits, const uint64_t *group_key,
                                 int group_key_bits, const uint8_t *umi_ascii, const int32_t *score, uint64_t n_reads,
                                 int umi_len, int n_words, int merge, uint64_t *keys, uint64_t *nmask, int32_t *freq,
                                 uint64_t *rep, uint64_t *bucket_off, uint64_t *n_entries, uint64_t *n_buckets);

/* ---- read staging of whole reads (FASTQ mode): the staging of run_fastq on the device.
 * in : read i is len[i] bases at text + seq_pos[i]; its quality, as long, at text + qual_pos[i]
 *      (qual_pos may be NULL with merge 0), so one buffer may hold the whole FASTQ file.
 *      merge: 0 = the first read represents a sequence (any), 1 = the read of the highest average
 *      quality, (int)(sum(q - 33) as f32 / len as f32), the first on ties.
 * out: the input of umi_dedup_seqs: buckets are read lengths in order of first appearance, entries
 *      of a bucket by freq descending, first appearance on ties; keys / nmask (may be NULL) n_words
 *      words per entry, zero behind the read's own ceil(3L/64); freq; rep = file index of the
 *      representative read; entry_of_read[i] (may be NULL) = read i's entry.  Capacity n_reads.
 *      bucket_off [*n_buckets + 1] and bucket_len [*n_buckets] are HOST arrays in both forms (at most
 *      UMI_MAX_SEQ_LEN + 1 lengths); *any_n = whether any N occurred (else nmask is all zero and
 *      umi_dedup_seqs may take NULL for it).
 * UMI_ERR_ARG: n_reads >= 2^30, a read over UMI_MAX_SEQ_LEN bases, n_words outside 1..12 or below
 * what the longest read needs, merge 1 without qualities.  UMI_ERR_CHAR: a byte outside ATCGN;
 * umi_last_error() names the smallest such read and its first bad byte:
 * "Unknown character in sequence: <byte> (read <index>)".
 * The _device form takes and leaves the per-read and per-entry arrays in device memory (it
 * synchronises the stream); the plain form copies host arrays in and out around it. */
int umi_stage_seqs_device(umi_ctx *ctx, const uint8_t *d_text, const uint64_t *d_seq_pos,
                          const uint64_t *d_qual_pos, const uint32_t *d_len, uint64_t n_reads, int n_words,
                          int merge, uint64_t *d_keys, uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep,
                          uint32_t *d_entry_of_read, uint64_t *bucket_off, int32_t *bucket_len,
                          uint64_t *n_entries, uint64_t *n_buckets, int *any_n, void *hip_stream);
int umi_stage_seqs(umi_ctx *ctx, const uint8_t *text, const uint64_t *seq_pos, const uint64_t *qual_pos,
                   const uint32_t *len, uint64_t n_reads, int n_words, int merge, uint64_t *keys,
                   uint64_t *nmask, int32_t *freq, uint64_t *rep, uint32_t *entry_of_read,
                   uint64_t *bucket_off, int32_t *bucket_len, uint64_t *n_entries, uint64_t *n_buckets,
                   int *any_n);

/* ---- consensus of the clusters of whole reads (FASTQ mode's --consensus): one read per cluster, voted
 *      column by column from all its members.  No counterpart in the reference (its fastq mode is a TODO,
 *      src/main.rs:49-50); the vote is the quality-weighted majority that consensus callers of UMI families
 *      start from, in integers.
 * in : what umi_stage_seqs[_device] and umi_dedup_seqs[_device] leave behind -- the text with every read's
 *      seq_pos / qual_pos / len, entry_of_read, freq, kept, root, the bucket table (HOST arrays in both
 *      forms, bucket_off[n_buckets] = n_entries).
 *      A cluster is a kept entry r (kept[r] != 0) with every entry e whose root[e] == r; its members are
 *      the reads i with root[entry_of_read[i]] == r, all of the bucket's length L.
 *      Column c, base b of A, C, G, T: S_b = sum of max(0, quality byte - 33) over the members with b at c,
 *      n_b = their number (an N votes for nothing).  Called: the b with the greatest (S_b, n_b), S first;
 *      the first of A, C, G, T on a tie.  n_b == 0 (every member has N): 'N' with quality '!'.  Else the
 *      quality byte is 33 + min(93, max(0, S_win - (sum of the other three S))).  The sums are 64-bit.
 * out: cons_seq / cons_qual (capacity: the sum of len over all reads): the consensus of the kept entries
 *      back to back in ascending entry order, *cons_bytes of them; cons_off[r] (defined where kept): where
 *      entry r's begins, its length being its bucket's; cluster_reads[r] (defined where kept; may be
 *      NULL): its members.
 * UMI_ERR_ARG: a multi-device context, n_reads >= 2^30, a NULL among the required pointers, no qual_pos,
 * a bucket table that does not end at n_entries.  UMI_ERR_ORDER, found on the device before anything is
 * written (nothing is read out of bounds): an entry_of_read or a root outside [0, n_entries), a root that
 * is not kept, a read that is not as long as its entry's bucket, a kept entry without a member, freq not
 * summing to n_reads.  A deferred call (umi_dedup_batch_device_begin) that is out on the context ends
 * first; its result keeps waiting for umi_dedup_batch_end.
 * The _device form takes and leaves the per-read and per-entry arrays in device memory and synchronises
 * the stream (twice: after the checks, at the end); the plain form copies host arrays in and out around it. */
int umi_consensus_seqs_device(umi_ctx *ctx, const uint8_t *d_text, const uint64_t *d_seq_pos,
                              const uint64_t *d_qual_pos, const uint32_t *d_len, uint64_t n_reads,
                              const uint32_t *d_entry_of_read, const int32_t *d_freq, const uint8_t *d_kept,
                              const uint32_t *d_root, uint64_t n_entries, const uint64_t *bucket_off,
                              const int32_t *bucket_len, uint64_t n_buckets, uint8_t *d_cons_seq,
                              uint8_t *d_cons_qual, uint64_t *d_cons_off, uint32_t *d_cluster_reads,
                              uint64_t *cons_bytes, void *hip_stream);
int umi_consensus_seqs(umi_ctx *ctx, const uint8_t *text, const uint64_t *seq_pos, const uint64_t *qual_pos,
                       const uint32_t *len, uint64_t n_reads, const uint32_t *entry_of_read, const int32_t *freq,
                       const uint8_t *kept, const uint32_t *root, uint64_t n_entries, const uint64_t *bucket_off,
                       const int32_t *bucket_len, uint64_t n_buckets, uint8_t *cons_seq, uint8_t *cons_qual,
                       uint64_t *cons_off, uint32_t *cluster_reads, uint64_t *cons_bytes);

/* ---- consensus of the clusters of aligned reads (BAM mode's --call-consensus): one sequence and quality
 *      string per cluster, voted column by column over BAM's own encodings.  No counterpart in the reference;
 *      the caller says which reads vote where (the program: the reads of a cluster whose length and CIGAR
 *      are the representative's, host/umicollapse_main.cpp).
 * in : read i is len[i] bases, packed two per byte, high nibble first, at data + seq_pos[i]; its qualities,
 *      raw Phred bytes, at data + qual_pos[i].  No offset needs any alignment: one buffer may be the whole
 *      inflated BAM.  cluster[i] in [0, n_clusters) makes read i a voter of that cluster, UMI_NO_CLUSTER
 *      leaves it out (nothing of such a read is looked at).  cluster_len[c] <= UMI_MAX_CONS_LEN: the length
 *      of cluster c, and of every voter of it.
 *      Column c: nibble 1, 2, 4, 8 votes for A, C, G, T, every other nibble (=, N, the ambiguity codes) for
 *      nothing, with weight w = min(quality byte, 93).  S_b = sum of w over the voters that show b, n_b =
 *      their number.  Called: the b with the greatest (S_b, n_b), S first; the first of A, C, G, T on a tie;
 *      quality min(93, max(0, S_win - (sum of the other three S))).  A column nobody voted on is nibble 15
 *      with quality 0.  The unused low nibble of the last byte of an odd length is 0.  The sums are 64-bit.
 * out: cons_seq (capacity: the sum of ceil(cluster_len / 2)) / cons_qual (the sum of cluster_len): the
 *      clusters' consensus back to back in ascending order, *seq_bytes / *qual_bytes of them, nothing
 *      written behind; seq_off[c] / qual_off[c]: where cluster c's begins; depth[c]: its voters;
 *      disagree[c] (may be NULL): the sum over its columns of (sum of n_b) - n_win, the base votes that
 *      lost.  A cluster without a voter is all nibble 15 with quality 0 and depth 0.
 * UMI_ERR_ARG: a multi-device context, n_reads or n_clusters >= 2^30, a NULL among the required pointers.
 * UMI_ERR_ORDER, found on the device before anything is written (nothing is read out of bounds): a
 * cluster_len above UMI_MAX_CONS_LEN, a cluster id that is neither in range nor UMI_NO_CLUSTER, a voter
 * whose len differs from its cluster's.  A deferred call (umi_dedup_batch_device_begin) that is out on the
 * context ends first; its result keeps waiting for umi_dedup_batch_end.  "cons_split" applies as to
 * umi_consensus_seqs (an accumulator slot is 48 KB here; a cluster of 2^24 voters or more always takes
 * that path).
 * The _device form takes and leaves every array in device memory and synchronises the stream (twice:
 * after the checks, at the end); the plain form copies host arrays in and out around it. */
#define UMI_MAX_CONS_LEN 1024
#define UMI_NO_CLUSTER 0xFFFFFFFFu
int umi_consensus_bam_device(umi_ctx *ctx, const uint8_t *d_data, const uint64_t *d_seq_pos,
                             const uint64_t *d_qual_pos, const uint32_t *d_len, const uint32_t *d_cluster,
                             uint64_t n_reads, const uint32_t *d_cluster_len, uint64_t n_clusters,
                             uint8_t *d_cons_seq, uint8_t *d_cons_qual, uint64_t *d_seq_off, uint64_t *d_qual_off,
                             uint32_t *d_depth, uint32_t *d_disagree, uint64_t *seq_bytes, uint64_t *qual_bytes,
                             void *hip_stream);
int umi_consensus_bam(umi_ctx *ctx, const uint8_t *data, const uint64_t *seq_pos, const uint64_t *qual_pos,
                      const uint32_t *len, const uint32_t *cluster, uint64_t n_reads, const uint32_t *cluster_len,
                      uint64_t n_clusters, uint8_t *cons_seq, uint8_t *cons_qual, uint64_t *seq_off,
                      uint64_t *qual_off, uint32_t *depth, uint32_t *disagree, uint64_t *seq_bytes,
                      uint64_t *qual_bytes);

/* ---- correction of UMIs to a fixed list (the program's --umi-whitelist): every read's UMI against every
 *      listed one, on the GPU.  No counterpart in the reference; the two conditions are those of fgbio
 *      CorrectUmis, and the distance is the reference's umi_dist (src/utils/bitset.rs:77-91) on the encoded keys.
 * in : n_reads UMIs of umi_len bytes each, back to back, every byte one of ATCGN (the pointer needs no
 *      alignment); whitelist_ascii: n_wl UMIs of the same length, every byte one of ACGT, a HOST array in
 *      both forms.  d(u, w) = the positions whose bytes differ: an N of a read differs from every listed base.
 *      Per read: best = the smallest d over the list, idx = the smallest index that reaches it, second =
 *      the smallest d over every entry other than idx (umi_len + 1 with n_wl == 1; a listed UMI that
 *      occurs twice makes second == best).  The read is matched iff best <= max_mismatches and
 *      second - best >= min_distance; a max_mismatches of umi_len or more lets every distance pass.
 * out: match[i] = idx where read i is matched, else -1; best[i] / second[i] (each may be NULL) for every
 *      read, matched or not; out_ascii (may be NULL, may be the input itself): the listed UMI's bytes for
 *      a matched read, the input bytes for any other; counts (host): reads matched at distance 0, matched
 *      at a distance above 0, not matched.
 * n_reads == 0: UMI_OK, counts all zero, nothing else touched.  A multi-device context uses its first
 * device, as umi_data_new does.  A deferred call (umi_dedup_batch_device_begin) that is out on the context
 * ends first; its result keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG: n_wl == 0 or above 2^24, a NULL among ctx, the UMIs, the list, match and counts, a negative
 * max_mismatches or min_distance, umi_len outside 1..UMI_MAX_WIDE_UMI_LEN, n_reads >= 2^30.  UMI_ERR_CHAR:
 * a listed byte outside ACGT ("Unknown character in whitelist: <byte> (entry <index>)", found on the host
 * before anything is launched), or a read byte outside ATCGN -- a pass of its own over the reads finds
 * the smallest such read before anything is written, the outputs stay as they were, and umi_last_error()
 * names it and its first bad byte: "Unknown character in UMI sequence: <byte> (read <index>)".
 * The _device form takes and leaves the per-read arrays in device memory and synchronises the stream
 * (twice: after the check, at the end); the plain form copies host arrays in and out around it. */
int umi_correct_umis_device(umi_ctx *ctx, const uint8_t *d_umi_ascii, uint64_t n_reads, int umi_len,
                            const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int min_distance,
                            uint8_t *d_out_ascii, int32_t *d_match, uint8_t *d_best, uint8_t *d_second,
                            uint64_t counts[3], void *hip_stream);
int umi_correct_umis(umi_ctx *ctx, const uint8_t *umi_ascii, uint64_t n_reads, int umi_len,
                     const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int min_distance,
                     uint8_t *out_ascii, int32_t *match, uint8_t *best, uint8_t *second, uint64_t counts[3]);

/* ---- correction of cell barcodes to a kit's list (the program's --cell-whitelist): every read's barcode and
 *      its single substitutions looked up in an index of the list, on the GPU.  No counterpart in the
 *      reference; the rule is STARsolo's 1MM.  Where umi_correct_umis compares every read with every entry
 *      (right for 10^2 to 10^5 UMIs), this call costs a read one probe when its barcode is listed and
 *      3 bc_len otherwise, whatever the list's size (10x lists: 737,280 and 6,794,880 barcodes).
 * in : n_reads barcodes of bc_len bytes each, back to back, every byte one of ACGTN (the pointer needs no
 *      alignment); whitelist_ascii: n_wl different barcodes of the same length, every byte one of ACGT, a
 *      HOST array in both forms.  max_mismatches is 0 or 1.  An N of a read differs from every listed base.
 * out: per read status[i] (may be NULL) and match[i]:
 *        UMI_BARCODE_EXACT      the barcode is listed; match = its index
 *        UMI_BARCODE_CORRECTED  not exact, max_mismatches 1, exactly one listed barcode differs in exactly
 *                               one position; match = its index
 *        UMI_BARCODE_NONE       no listed barcode within max_mismatches; match = -1
 *        UMI_BARCODE_AMBIGUOUS  not exact, max_mismatches 1, two or more listed barcodes differ in exactly
 *                               one position; match = -1
 *      counts (host): the reads of each status, counts[status].  match is what umi_correct_umis gives with
 *      the same max_mismatches and min_distance 1.
 * n_reads == 0: UMI_OK, counts all zero, nothing else touched.  A multi-device context uses its first
 * device.  A deferred call (umi_dedup_batch_device_begin) that is out on the context ends first; its result
 * keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG: n_wl == 0 or above 2^24, a NULL among ctx, the barcodes, the list, match and counts,
 * max_mismatches outside 0..1, bc_len outside 1..32, n_reads >= 2^30, a listed barcode that occurs twice
 * ("duplicate entry in the barcode whitelist: entry <index> equals an earlier one", the smallest such index,
 * found on the device while the index is built).  UMI_ERR_CHAR: a listed byte outside ACGT ("Unknown
 * character in whitelist: <byte> (entry <index>)", found on the host before anything is launched), or a
 * read byte outside ACGTN -- a pass of its own over the reads finds the smallest such read before anything
 * is written: "Unknown character in cell barcode: <byte> (read <index>)".  After any refusal the outputs
 * are as they were.  The _device form takes and leaves the per-read arrays in device memory and
 * synchronises the stream (twice: after the index and the check, at the end); the plain form copies host
 * arrays in and out around it. */
#define UMI_BARCODE_EXACT 0
#define UMI_BARCODE_CORRECTED 1
#define UMI_BARCODE_NONE 2
#define UMI_BARCODE_AMBIGUOUS 3
int umi_correct_barcodes_device(umi_ctx *ctx, const uint8_t *d_bc_ascii, uint64_t n_reads, int bc_len,
                                const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int32_t *d_match,
                                uint8_t *d_status, uint64_t counts[4], void *hip_stream);
int umi_correct_barcodes(umi_ctx *ctx, const uint8_t *bc_ascii, uint64_t n_reads, int bc_len,
                         const uint8_t *whitelist_ascii, uint32_t n_wl, int max_mismatches, int32_t *match,
                         uint8_t *status, uint64_t counts[4]);

/* ---- ambiguous cell barcodes decided by posterior (the program's --cell-whitelist-multi): the call above with
 *      max_mismatches 1, and the reads it leaves ambiguous weighed as STARsolo's 1MM_multi[_pseudocounts] and
 *      Cell Ranger weigh them.  No counterpart in the reference; tests/barcode_multi_model.py defines the rule.
 * in : as umi_correct_barcodes, and bc_qual: the barcodes' qualities, bc_len bytes per read beside bc_ascii's,
 *      Phred + 33, every byte in 33..126; min_posterior_permille in 0..1000; pseudocount in 0..1000.
 * out: exact, corrected and none are what umi_correct_barcodes gives (a single candidate is accepted whatever
 *      its count).  exact_reads[e] (uint32 [n_wl], may be NULL): the reads of this call that are exact with
 *      match e.  For a read with two or more listed barcodes one substitution away (one N: that agree
 *      everywhere else), candidate e with its mismatch at position p has the weight
 *        w_e = (exact_reads[e] + pseudocount) * T[min(qual[p] - 33, 40)],  T[q] = round(2^26 * 10^(-q / 10)),
 *      W is the sum of the weights and e* the candidate of greatest weight, the smallest index on ties.  Where
 *      W > 0 and 1000 * w_e* >= min_posterior_permille * W the read is UMI_BARCODE_RESOLVED with match = e*;
 *      otherwise it stays UMI_BARCODE_AMBIGUOUS, match = -1.  All in integers (the comparison in 128 bits):
 *      the result is exact and the same in every run.  counts (host): the reads of each of the five statuses;
 *      counts[3] + counts[4] is umi_correct_barcodes' counts[3].
 * n_reads == 0, a multi-device context and a deferred call that is out: as umi_correct_barcodes.
 * Refusals as umi_correct_barcodes, and UMI_ERR_ARG: bc_qual NULL with n_reads > 0, min_posterior_permille or
 * pseudocount outside 0..1000.  UMI_ERR_CHAR: a quality byte outside 33..126, "Unknown character in cell
 * barcode quality: <byte> (read <index>)", the smallest such read, found beside the barcodes' check before
 * anything is written; a bad barcode byte of that read or an earlier one is reported in its place.  After any
 * refusal the outputs are as they were. */
#define UMI_BARCODE_RESOLVED 4
int umi_correct_barcodes_multi_device(umi_ctx *ctx, const uint8_t *d_bc_ascii, const uint8_t *d_bc_qual, uint64_t n_reads,
                                      int bc_len, const uint8_t *whitelist_ascii, uint32_t n_wl,
                                      int min_posterior_permille, int pseudocount, int32_t *d_match, uint8_t *d_status,
                                      uint32_t *d_exact_reads, uint64_t counts[5], void *hip_stream);
int umi_correct_barcodes_multi(umi_ctx *ctx, const uint8_t *bc_ascii, const uint8_t *bc_qual, uint64_t n_reads, int bc_len,
                               const uint8_t *whitelist_ascii, uint32_t n_wl, int min_posterior_permille,
                               int pseudocount, int32_t *match, uint8_t *status, uint32_t *exact_reads,
                               uint64_t counts[5]);

/* ---- reads assigned to genes from an annotation (the program's --gene-annotation), on the GPU.  No counterpart
 *      in the reference; the rule is featureCounts' default (-t exon -g gene_id -s 0|1|2, minimum overlap 1, no
 *      -O, single-end) and tests/annotation_model.py defines it:
 *        Blocks of a read: start at read_pos (0-based) and walk the CIGAR (BAM's words, len << 4 | op).  M, =, X
 *          and D (0, 7, 8, 2) extend the current block on the reference; N (3) closes the block and skips its
 *          length; I, S, H and P (1, 4, 5, 6) consume nothing.  Blocks are half-open [s, e); a read without a
 *          reference-consuming operation has no block.  Op codes 9 to 15 are an error.
 *        Exons: (ref, start, end, strand, gene), half-open, 0-based, strand '+', '-' or '.'.
 *        Hits: gene g hits a read when one of its exons is on the read's reference, on an admissible strand, and
 *          shares at least one base with one of the read's blocks.
 *        Admissible strand: the read's strand is '-' where read_reverse is not 0 (flag 0x10), else '+'.
 *          UMI_STRAND_FORWARD: the exon's strand equals the read's; UMI_STRAND_REVERSE: it is the opposite;
 *          UMI_STRAND_UNSTRANDED: any.  A '.' exon is admissible under all three.
 *        Result: exactly one gene hits: UMI_GENE_ASSIGNED, gene = its index; none: UMI_GENE_NONE, gene = -1; two
 *          or more: UMI_GENE_SEVERAL, gene = -1.  Overlapping exons of one gene count as one gene.
 *      Transcript-level containment (STARsolo's Gene) is umi_assign_genes_transcripts, below.  Not built: paired
 *      reads, fractional assignment, a minimum overlap above 1.
 * in : the n_exons exons in five HOST arrays in both forms (exon_strand: the ASCII bytes), exon_gene in
 *      0..n_genes - 1; per read read_ref, read_pos, read_reverse, and its CIGAR words cigar[cigar_off[i] ..
 *      cigar_off[i + 1]), the reads' words back to back, cigar_off of n_reads + 1 entries (cigar may be NULL
 *      where there is no word).  The index is built on the host inside the call; the walk and the lookups run on
 *      the device.  n_exons == 0 is legal: every read is UMI_GENE_NONE.
 * out: gene int32 [n_reads], status uint8 [n_reads], counts (host): the reads of each status, counts[status].
 * n_reads == 0: UMI_OK, counts all zero, nothing else touched.  A multi-device context uses its first device.
 * A deferred call (umi_dedup_batch_device_begin) that is out on the context ends first; its result keeps
 * waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG, found on the host before anything is launched: an exon with end <= start, start < 0 or ref < 0,
 * exon_gene outside 0..n_genes - 1, an unknown exon_strand or strand_mode, a NULL among ctx, counts and the arrays
 * a positive count asks for, n_reads or n_exons >= 2^30.  Found on the device, told after the call's one
 * synchronisation, the outputs then not defined: UMI_ERR_ARG for a read_ref < 0 or a CIGAR op code above 8,
 * UMI_ERR_ORDER for a cigar_off that falls (nothing is read outside cigar[0 .. cigar_off[n_reads])); the message
 * names the smallest such read.  Option "gene_top" (0/1, default 1): the sampled top of the index in LDS.  The
 * _device form takes and leaves the per-read arrays in device memory; the plain form copies host arrays in and
 * out around it. */
#define UMI_GENE_ASSIGNED 0
#define UMI_GENE_NONE 1
#define UMI_GENE_SEVERAL 2
#define UMI_STRAND_FORWARD 0
#define UMI_STRAND_REVERSE 1
#define UMI_STRAND_UNSTRANDED 2
int umi_assign_genes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                            const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                            int strand_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                            const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                            uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint64_t counts[3], void *hip_stream);
int umi_assign_genes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                     const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                     int strand_mode, const int32_t *read_ref, const int32_t *read_pos, const uint8_t *read_reverse,
                     const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads, int32_t *gene, uint8_t *status,
                     uint64_t counts[3]);

/* ---- ... by transcript model (the program's --gene-rule transcript), on the GPU.  No counterpart in the reference;
 *      the rule is STARsolo's default feature (Gene) and Cell Ranger's transcriptome-compatible reads, and
 *      tests/transcript_model.py defines it.  Blocks of a read and admissible strands are umi_assign_genes', unchanged
 *      (a zero-length N closes a block too: two abutting blocks; empty blocks are left out).  New:
 *        Exons: (ref, start, end, strand, gene, transcript), transcript in 0..n_transcripts - 1.  All exons of one
 *          transcript share ref, strand and gene.  A transcript's exons are taken in ascending order, whatever order
 *          they were passed in; those that overlap or abut are united: x_1 < x_2 < ... < x_n, disjoint, at least one
 *          base between neighbours.
 *        Fit: a read with blocks b_1 .. b_m fits transcript t when t is on the read's reference and on an admissible
 *          strand (a '.' transcript always), m >= 1, and there is a j such that b_i lies inside x_{j+i-1} for every i,
 *          and for every i < m: end(b_i) == end(x_{j+i-1}) and start(b_{i+1}) == start(x_{j+i}).  A D never splits a
 *          block: a deletion across an intron makes a block that no exon contains.  A read with more blocks than t
 *          has exons from j on does not fit t.  Coordinates are compared in 64 bits: a block that starts before 0 or
 *          ends beyond 2^31 - 1 lies in nothing, and nothing wraps.
 *        Result: G = the genes with a transcript the read fits.  One gene: UMI_GENE_ASSIGNED, gene = its index; none:
 *          UMI_GENE_NONE, gene = -1; two or more: UMI_GENE_SEVERAL, gene = -1.  Two fitting transcripts of one gene
 *          are one gene.  G is a subset of the genes that hit the read under umi_assign_genes.
 *      A body tier and read classes by transcript model: umi_assign_genes_transcripts_classes, below.  Not built:
 *      paired reads, STARsolo's multi-gene modes.
 * in : umi_assign_genes' arguments, and exon_transcript (HOST, n_exons entries) and n_transcripts (it may lie above the
 *      transcripts used).  The index is built on the host inside the call; the walks and the lookups run on the device.
 * out: gene, status and counts[3] as umi_assign_genes writes them.
 * Everything else is umi_assign_genes' contract: n_reads == 0 (UMI_OK, counts all zero, nothing else touched),
 * n_exons == 0 (legal: every read is none), the first device of a multi-device context, a deferred call that is out
 * ends first, the errors and when they are found, the limit of 2^30, options "gene_top" and "grid_cus".  UMI_ERR_ARG
 * before anything is launched, beside umi_assign_genes' own: exon_transcript NULL with exons, an entry outside
 * 0..n_transcripts - 1, a transcript whose exons lie on two references, on two strands or in two genes,
 * n_transcripts >= 2^31. */
int umi_assign_genes_transcripts_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start,
                                        const int32_t *exon_end, const uint8_t *exon_strand, const int32_t *exon_gene,
                                        const int32_t *exon_transcript, uint64_t n_exons, uint32_t n_genes,
                                        uint32_t n_transcripts, int strand_mode, const int32_t *d_read_ref,
                                        const int32_t *d_read_pos, const uint8_t *d_read_reverse, const uint32_t *d_cigar,
                                        const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene, uint8_t *d_status,
                                        uint64_t counts[3], void *hip_stream);
int umi_assign_genes_transcripts(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                 const uint8_t *exon_strand, const int32_t *exon_gene, const int32_t *exon_transcript,
                                 uint64_t n_exons, uint32_t n_genes, uint32_t n_transcripts, int strand_mode,
                                 const int32_t *read_ref, const int32_t *read_pos, const uint8_t *read_reverse,
                                 const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads, int32_t *gene,
                                 uint8_t *status, uint64_t counts[3]);

/* ---- ... with their introns (the program's --gene-introns), on the GPU.  No counterpart in the reference; the
 *      rules are STARsolo's GeneFull_ExonOverIntron and GeneFull, stated with this project's overlap of one base, and
 *      tests/intron_model.py defines them.  Blocks of a read, exons, admissible strands and the set E of genes
 *      that hit a read are umi_assign_genes', unchanged.  New:
 *        Gene body: the exons of a gene are grouped by (reference, strand as written: '+', '-' or '.').  Each group
 *          gives one body, [min start, max end) over the group's exons; the minimum and the maximum may come from
 *          different exons.  A gene with exons on two references, or on '+' and '.', has one body per group.  No
 *          `gene` or `transcript` line is needed: bodies come from whatever the caller passes as exons.
 *        B: the genes with a body on the read's reference, on an admissible strand (the exons' rule; a '.' body is
 *          always admissible), that shares at least one base with one of the read's blocks.  E is a subset of B.
 *        UMI_INTRONS_EXON_FIRST: |E| = 1: assigned to that gene, tier exon.  |E| >= 2: several.  |E| = 0 and
 *          |B| = 1: assigned, tier intron.  |E| = 0 and |B| = 0: none.  |E| = 0 and |B| >= 2: several.
 *        UMI_INTRONS_ALL (plain GeneFull on derived bodies): |B| = 1: assigned, tier exon if E is not empty, else
 *          intron.  |B| = 0: none.  |B| >= 2: several.
 *        UMI_INTRONS_OFF: umi_assign_genes' result, every assigned read tier exon.
 *      The minimum overlap is 1 throughout: a block that starts in an exon and runs into the intron is tier exon.
 *      Not built: STARsolo's Ex50pAS half-of-the-read rule, antisense counting, paired reads.  (Spliced / unspliced
 *      matrices: umi_assign_genes_classes and umi_velocity_matrix, below.)
 * in : umi_assign_genes' arguments, and intron_mode, one of UMI_INTRONS_*.  The bodies are derived and both tiers
 *      of the index built on the host inside the call; a read is walked against the exons, and again against the
 *      bodies only where its verdict still depends on them.
 * out: gene int32 [n_reads] and status uint8 [n_reads] as umi_assign_genes writes them; tier uint8 [n_reads],
 *      UMI_GENE_TIER_EXON or UMI_GENE_TIER_INTRON, 0 where the read is not assigned; counts (host): the reads
 *      assigned by an exon, assigned by an intron, none, several.
 * Everything else is umi_assign_genes' contract: n_reads == 0 (UMI_OK, counts all zero, nothing else touched),
 * n_exons == 0 (legal: every read is none), the first device of a multi-device context, a deferred call that is out
 * ends first, and the errors and when they are found, tier among the required pointers; an unknown intron_mode is
 * UMI_ERR_ARG before anything is launched.  Options "gene_top" and "gene_body_top". */
#define UMI_INTRONS_OFF 0
#define UMI_INTRONS_EXON_FIRST 1
#define UMI_INTRONS_ALL 2
#define UMI_GENE_TIER_EXON 0
#define UMI_GENE_TIER_INTRON 1
int umi_assign_genes_introns_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                    const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                                    int strand_mode, int intron_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                                    const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                                    uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint64_t counts[4],
                                    void *hip_stream);
int umi_assign_genes_introns(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                             const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                             int strand_mode, int intron_mode, const int32_t *read_ref, const int32_t *read_pos,
                             const uint8_t *read_reverse, const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads,
                             int32_t *gene, uint8_t *status, uint8_t *tier, uint64_t counts[4]);

/* ---- ... and the class of every assigned read (the program's --velocity), on the GPU.  A gene-level rule in exact
 *      integers, NOT velocyto's or STARsolo's transcript-model rule: this project keeps no transcript models.
 *      tests/velocity_model.py defines it.  A read's blocks, exons, admissible strands, E, B, status, gene and tier
 *      are umi_assign_genes_introns', unchanged.  New, for an assigned read with gene g:
 *        Blocks are cut to [0, 2^31), and the empty ones left out: b1 .. bm.  A gap is the stretch between one
 *          block's end and the next one's start (what N operations skipped).
 *        cover of an interval [s, e): the number of its positions that lie in an exon of g on the read's reference
 *          and on an admissible strand.
 *        UMI_READ_CLASS_INTRONIC: tier intron.  Tier exon: UMI_READ_CLASS_SPANNING where the blocks' summed cover
 *          is less than their summed length (the read leaves the exons into an intron or past the gene's end);
 *          otherwise UMI_READ_CLASS_JUNCTION where m >= 2 and some gap has cover < its length (the read skips an
 *          intron); otherwise UMI_READ_CLASS_EXONIC.  UMI_READ_CLASS_NONE where the read is not assigned.
 *      The classes are relative to the exons passed: where the caller passes whole genes as exons, every assigned
 *      read is EXONIC.  Classes by transcript model: umi_assign_genes_transcripts_classes, below.  Not built:
 *      velocyto's or STARsolo's own rules, paired reads.
 * in : umi_assign_genes_introns' arguments.
 * out: gene, status, tier and counts[4], bit for bit what umi_assign_genes_introns writes on the same input; cls
 *      uint8 [n_reads], one of UMI_READ_CLASS_*; class_counts (host) [5]: the reads by class, indexed by
 *      UMI_READ_CLASS_*.
 * Everything else is umi_assign_genes_introns' contract (n_reads == 0, n_exons == 0, the first device of a
 * multi-device context, a deferred call that is out ends first, the errors and when they are found, cls and
 * class_counts among the required pointers, options "gene_top" and "gene_body_top"). */
#define UMI_READ_CLASS_NONE 0
#define UMI_READ_CLASS_EXONIC 1
#define UMI_READ_CLASS_JUNCTION 2
#define UMI_READ_CLASS_SPANNING 3
#define UMI_READ_CLASS_INTRONIC 4
int umi_assign_genes_classes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                                    const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                                    int strand_mode, int intron_mode, const int32_t *d_read_ref, const int32_t *d_read_pos,
                                    const uint8_t *d_read_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                                    uint64_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls,
                                    uint64_t counts[4], uint64_t class_counts[5], void *hip_stream);
int umi_assign_genes_classes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start, const int32_t *exon_end,
                             const uint8_t *exon_strand, const int32_t *exon_gene, uint64_t n_exons, uint32_t n_genes,
                             int strand_mode, int intron_mode, const int32_t *read_ref, const int32_t *read_pos,
                             const uint8_t *read_reverse, const uint32_t *cigar, const uint64_t *cigar_off, uint64_t n_reads,
                             int32_t *gene, uint8_t *status, uint8_t *tier, uint8_t *cls, uint64_t counts[4],
                             uint64_t class_counts[5]);

/* ---- ... by transcript model, with the gene bodies behind it and the class of every assigned read (the program's
 *      --transcript-introns), on the GPU.  No counterpart in the reference.  Stated after Cell Ranger 7's counting with
 *      introns (a read is tried against the transcript models first and falls back to the gene body) and velocyto's /
 *      STARsolo Velocyto's classes, not claimed equal to them: no intron validation, no per-model logic across a
 *      molecule's reads.  Exact integers; tests/transcript_intron_model.py defines it.
 *        Blocks, admissible strands, fit and G (the genes with a transcript the read fits) are
 *          umi_assign_genes_transcripts', unchanged; m is the number of non-empty blocks.  Bodies and B (the genes whose
 *          admissible body on the read's reference shares a base with a block) are umi_assign_genes_introns', derived
 *          from the same lines, grouped per gene by reference and strand as written; E is umi_assign_genes'.
 *          G is a subset of E, E of B.
 *        UMI_INTRONS_EXON_FIRST: |G| = 1: assigned to it, tier transcript (UMI_GENE_TIER_EXON).  |G| >= 2: several.
 *          |G| = 0 and |B| = 1: assigned, tier body (UMI_GENE_TIER_INTRON).  |G| = 0 and |B| = 0: none.  |G| = 0 and
 *          |B| >= 2: several.
 *        UMI_INTRONS_ALL: |B| = 1: assigned to it, tier transcript where G is not empty, else body.  |B| = 0: none.
 *          |B| >= 2: several.
 *        UMI_INTRONS_OFF: umi_assign_genes_transcripts' gene and status, every assigned read tier transcript.
 *        Class of an assigned read with gene g.  Tier transcript: UMI_READ_CLASS_JUNCTION where m >= 2, else
 *          UMI_READ_CLASS_EXONIC (every gap of a fitting read is an intron of a transcript it fits).  Tier body: the
 *          blocks are cut to [0, 2^31), the empty ones left out; c is the summed cover of the blocks by g's
 *          admissible exon lines on the reference (umi_assign_genes_classes' cover).  c == 0:
 *          UMI_READ_CLASS_INTRONIC.  0 < c < the summed length: UMI_READ_CLASS_SPANNING.  c == the summed length:
 *          UMI_READ_CLASS_JUNCTION where a gap is not covered whole by g's own exons (a spliced read of an isoform
 *          the annotation does not have is spliced evidence), else UMI_READ_CLASS_EXONIC (two abutting blocks after a
 *          zero-length N, an N inside an exon).  Not assigned: UMI_READ_CLASS_NONE.
 *      Where it differs from umi_assign_genes_classes: a read spliced over an intron that another isoform of the gene
 *      retains is EXONIC there (the long exon line covers the gap) and JUNCTION here (it fits the spliced isoform).
 *      Not built: paired reads, Ex50pAS, antisense counting.
 * in : umi_assign_genes_transcripts' arguments, and intron_mode, one of UMI_INTRONS_*.  The three indices (transcripts,
 *      bodies and, for the classes, the exons' overlap table with its covers) are built on the host inside the call.
 * out: gene, status and tier as umi_assign_genes_introns writes them; counts (host) [4]: the reads assigned by a
 *      transcript, by a body, none, several; cls uint8 [n_reads] and class_counts (host) [5] as umi_assign_genes_classes
 *      writes them.  cls and class_counts may both be NULL: no class is computed, and the overlap table and its covers
 *      are neither built nor uploaded; gene, status, tier and counts are the same.  One of the two NULL alone is
 *      UMI_ERR_ARG.
 * Everything else is umi_assign_genes_transcripts' contract (n_reads == 0, n_exons == 0, the first device of a
 * multi-device context, a deferred call that is out ends first, the limit of 2^30, the transcript errors, the errors
 * and when they are found, tier among the required pointers); an unknown intron_mode is UMI_ERR_ARG before anything is
 * launched.  Options "gene_top", "gene_body_top" and "grid_cus". */
int umi_assign_genes_transcripts_classes_device(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start,
                                                const int32_t *exon_end, const uint8_t *exon_strand, const int32_t *exon_gene,
                                                const int32_t *exon_transcript, uint64_t n_exons, uint32_t n_genes,
                                                uint32_t n_transcripts, int strand_mode, int intron_mode,
                                                const int32_t *d_read_ref, const int32_t *d_read_pos,
                                                const uint8_t *d_read_reverse, const uint32_t *d_cigar,
                                                const uint64_t *d_cigar_off, uint64_t n_reads, int32_t *d_gene,
                                                uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls, uint64_t counts[4],
                                                uint64_t class_counts[5], void *hip_stream);
int umi_assign_genes_transcripts_classes(umi_ctx *ctx, const int32_t *exon_ref, const int32_t *exon_start,
                                         const int32_t *exon_end, const uint8_t *exon_strand, const int32_t *exon_gene,
                                         const int32_t *exon_transcript, uint64_t n_exons, uint32_t n_genes,
                                         uint32_t n_transcripts, int strand_mode, int intron_mode, const int32_t *read_ref,
                                         const int32_t *read_pos, const uint8_t *read_reverse, const uint32_t *cigar,
                                         const uint64_t *cigar_off, uint64_t n_reads, int32_t *gene, uint8_t *status,
                                         uint8_t *tier, uint8_t *cls, uint64_t counts[4], uint64_t class_counts[5]);

/* ---- molecules and reads per (column, row) pair (the program's --count-matrix): what a batched call kept,
 *      summed over its buckets into the triplets of a sparse matrix, on the GPU.  No counterpart in the
 *      reference; the counting is umi_tools count --per-gene --per-cell's, tests/gene_model.py (count_model)
 *      defines it.
 * in : kept / freq: the N = bucket_off[n_buckets] entries of a batched call (kept as that call wrote it: any
 *      byte other than 0 counts as kept); bucket_off: a HOST array in both forms, [n_buckets + 1], starting
 *      at 0 and never falling; row[b] / col[b]: the row id (gene) and column id (cell) of bucket b.  A bucket
 *      is non-empty when bucket_off[b] < bucket_off[b + 1]; several buckets may carry the same pair.
 * out: one triplet for every distinct (col, row) among the non-empty buckets, sorted by col, then by row:
 *      out_row / out_col the pair, out_molecules the entries with kept != 0 and out_reads the sum of freq
 *      (64 bits) over all buckets that carry it; *nnz their number.  Empty buckets contribute nothing, and
 *      their ids are not looked at; a triplet may have 0 molecules.  The four arrays have room for
 *      n_buckets triplets; what lies behind the first *nnz is not defined.
 * n_buckets == 0 or every bucket empty: UMI_OK, *nnz = 0, nothing launched, nothing else touched.  A
 * multi-device context uses its first device.  A deferred call (umi_dedup_batch_device_begin) that is out on
 * the context ends first; its result keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG: a NULL among ctx, nnz and the arrays the call would touch, n_buckets >= 2^30, a bucket_off
 * that does not start at 0 or that falls (found on the host before anything is launched), n_rows == 0 or
 * n_cols == 0 with a non-empty bucket, a non-empty bucket whose row >= n_rows or col >= n_cols (counted on the
 * device, told after the call's synchronisation: *nnz is 0 and the outputs are not defined).
 * The _device form takes and leaves everything but bucket_off and nnz in device memory and synchronises the
 * stream once, at the end; the plain form copies host arrays in and out around it. */
int umi_count_matrix_device(umi_ctx *ctx, const uint8_t *d_kept, const int32_t *d_freq, const uint64_t *bucket_off,
                            uint64_t n_buckets, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows,
                            uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules,
                            uint64_t *d_out_reads, uint64_t *nnz, void *hip_stream);
int umi_count_matrix(umi_ctx *ctx, const uint8_t *kept, const int32_t *freq, const uint64_t *bucket_off,
                     uint64_t n_buckets, const uint32_t *row, const uint32_t *col, uint32_t n_rows, uint32_t n_cols,
                     uint32_t *out_row, uint32_t *out_col, uint32_t *out_molecules, uint64_t *out_reads, uint64_t *nnz);

/* ---- spliced, unspliced and ambiguous molecules per (column, row) pair (the program's --velocity): the classes of
 *      the reads carried to their molecules, and the molecules counted in three layers, on the GPU.
 *      tests/velocity_model.py defines it.  A molecule is a kept entry r (kept[r] != 0); its reads are the reads i
 *      with read_entry[i] != UMI_READ_UNSTAGED and root[read_entry[i]] == r.  s: one of them is
 *      UMI_READ_CLASS_JUNCTION; u: one of them is UMI_READ_CLASS_SPANNING or UMI_READ_CLASS_INTRONIC.  s and not u:
 *      spliced.  u and not s: unspliced.  Otherwise (both, or neither -- EXONIC reads alone, or no read at all):
 *      ambiguous.  An entry with kept == 0 counts nowhere.
 * in : read_entry uint32 [n_reads]: the entry a read was staged into, UMI_READ_UNSTAGED: none, the read is skipped;
 *      read_class uint8 [n_reads]: umi_assign_genes_classes' cls; kept uint8 [N] and root uint32 [N] of a batched
 *      call (N = bucket_off[n_buckets]); bucket_off (a HOST array in both forms), row, col, n_rows, n_cols as
 *      umi_count_matrix takes them.
 * out: the triplets of umi_count_matrix for the same kept, bucket_off, row and col, in the same order: out_row,
 *      out_col, and out_spliced, out_unspliced, out_ambiguous (uint32), whose sum is that call's molecules for every
 *      triplet; *nnz their number.  The five arrays have room for n_buckets triplets.
 * n_buckets == 0 or every bucket empty: UMI_OK, *nnz = 0, nothing launched.  n_reads == 0 is legal: every molecule is
 * ambiguous.  A multi-device context uses its first device; a deferred call that is out ends first.
 * UMI_ERR_ARG: umi_count_matrix's own (NULL pointers, n_buckets >= 2^30, bucket_off, n_rows, n_cols, a row or col
 * out of range), n_reads >= 2^32, and, found on the device and told after the call's one synchronisation with *nnz
 * 0 and the outputs not defined, the smallest read named: a read_entry >= N other than UMI_READ_UNSTAGED, a
 * read_class above 4, a root[read_entry[i]] >= N. */
#define UMI_READ_UNSTAGED 0xFFFFFFFFu
int umi_velocity_matrix_device(umi_ctx *ctx, const uint32_t *d_read_entry, const uint8_t *d_read_class, uint64_t n_reads,
                               const uint8_t *d_kept, const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets,
                               const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols,
                               uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_spliced, uint32_t *d_out_unspliced,
                               uint32_t *d_out_ambiguous, uint64_t *nnz, void *hip_stream);
int umi_velocity_matrix(umi_ctx *ctx, const uint32_t *read_entry, const uint8_t *read_class, uint64_t n_reads,
                        const uint8_t *kept, const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets,
                        const uint32_t *row, const uint32_t *col, uint32_t n_rows, uint32_t n_cols, uint32_t *out_row,
                        uint32_t *out_col, uint32_t *out_spliced, uint32_t *out_unspliced, uint32_t *out_ambiguous,
                        uint64_t *nnz);

/* ---- sequencing saturation and median genes / molecules per cell as a function of depth (the program's
 *      --saturation-curve): nested read subsampling on the GPU.  tests/saturation_model.py defines it.  Everything is
 *      exact integer arithmetic, the same in every run.  The collapse is the full-depth one: the curve takes kept[] and
 *      root[] as they are and does NOT collapse again at each depth (what Cell Ranger does from its molecule table).
 *      Hash of read i (its index in read_entry), mod 2^64:  z = seed + (i + 1) * 0x9E3779B97F4A7C15;
 *        z = (z ^ z >> 30) * 0xBF58476D1CE4E5B9;  z = (z ^ z >> 27) * 0x94D049BB133111EB;  z ^= z >> 31;  h = z >> 32.
 *      Level of a read: lev = (h * L) >> 32, in 0..L-1.  A read is in depth j -- the sample of (j + 1) / L of the reads
 *        -- when lev <= j; the samples are nested and depth L-1 holds every read.
 *      A molecule is an entry r with kept[r] != 0; its reads are the reads i with read_entry[i] != UMI_READ_UNSTAGED and
 *        root[read_entry[i]] == r; its level is the smallest level of its reads, and it is absent at every depth if it
 *        has none.  A counted read is a read whose root is kept; reads under a root with kept == 0 count nowhere.  A
 *        molecule belongs to the bucket that holds r.  A pair is a distinct (col, row) among the non-empty buckets
 *        (several buckets may share one); its level is the smallest level of the molecules of its buckets.
 *      Selected columns: with cell_mask, those with cell_mask[c] != 0, whether they hold a molecule or not; with
 *        cell_mask NULL, the columns with a molecule at full depth.  n_sel is their number.
 * in : read_entry, n_reads, kept, root, bucket_off (a HOST array in both forms), row, col, n_rows, n_cols as
 *      umi_velocity_matrix takes them; seed; n_levels = L in 1..32; cell_mask uint8 [n_cols] or NULL.
 * out: curve uint64 [L][8], HOST memory in both forms, row j = depth j, everything cumulative (lev <= j):
 *      0 reads (counted reads), 1 molecules, 2 pairs, 3 cells (selected columns with a molecule at this depth),
 *      4 molecules_in_cells and 5 pairs_in_cells (those in selected columns), 6 median_molecules: over all n_sel
 *      selected columns -- those with none count as 0 -- the lower median (element floor((n_sel - 1) / 2) in
 *      ascending order) of a column's molecules at this depth, 0 for n_sel = 0; 7 median_genes: the same for a
 *      column's pairs.  The device form writes nothing else the caller can see.
 * n_buckets == 0 or every bucket empty: UMI_OK, the curve all zeros, nothing launched, the reads not looked at.  A
 * multi-device context uses its first device; a deferred call that is out ends first.  Grids come from the context's
 * CU count (option "grid_cus").  Workspace, bytes: 4 N + 52 m + 56 L n_cols + the temporaries of the library's sort
 * of max(m, 2 L n_cols) keys and of its scan of m + 4 KB, m the non-empty buckets; the column tables and the median
 * sort are sized by n_cols, not n_sel (the selected columns are not compacted), and 2 L n_cols < 2^30.
 * UMI_ERR_ARG, nothing written to curve: n_levels outside 1..32 and n_reads >= 2^32 (both before any HIP call), NULL
 * pointers, umi_count_matrix's own (n_buckets >= 2^30, bucket_off, n_rows, n_cols, a row or col of a non-empty bucket
 * out of range), 2 L n_cols >= 2^30, and, found on the device and told after the call's one synchronisation, the
 * smallest read named: a read_entry >= N other than UMI_READ_UNSTAGED, a root[read_entry[i]] >= N.
 * Option "saturation_skip" 0/1: see umi_ctx_set_option. */
int umi_saturation_curve_device(umi_ctx *ctx, const uint32_t *d_read_entry, uint64_t n_reads, const uint8_t *d_kept,
                                const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *d_row,
                                const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint64_t seed, int n_levels,
                                const uint8_t *d_cell_mask, uint64_t *curve, void *hip_stream);
int umi_saturation_curve(umi_ctx *ctx, const uint32_t *read_entry, uint64_t n_reads, const uint8_t *kept, const uint32_t *root,
                         const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *row, const uint32_t *col, uint32_t n_rows,
                         uint32_t n_cols, uint64_t seed, int n_levels, const uint8_t *cell_mask, uint64_t *curve);

/* ---- molecules and reads per (column, splice junction) pair (the program's --junction-matrix): a count matrix whose
 *      rows are the splice junctions of the reads' CIGARs, on the GPU.  The matrix is what STARsolo's --soloFeatures SJ
 *      writes, with two differences stated below; tests/junction_model.py defines it.  Exact integer arithmetic.
 *        Blocks of a read are umi_assign_genes_transcripts' blocks, unchanged: start at read_pos, M, =, X and D extend
 *          the current block, an N of any length, 0 included, closes it and skips its length, I, S, H and P consume
 *          nothing, empty blocks are left out, op codes 9 to 15 are an error.
 *        A junction of a read is the stretch [e, s) between two consecutive non-empty blocks: the end of one, the start
 *          of the next.  It counts where 0 <= e < s <= 2^31 - 1.  So several N with only I, S, H or P between them are
 *          one junction; a leading, a trailing or a zero-length N gives none; a D never makes one.  Positions are
 *          computed in 64 bits, and a gap that reaches beyond 2^31 - 1 is left out.  Positions only grow along a read:
 *          a read has a given junction at most once.  The junction's identity is (ref, e, s) = (ref, start, end).
 *          It has NO strand: there is no genome here to read a motif from (STARsolo tells the strand by the motif).
 *        A molecule is an entry r with kept[r] != 0; its reads are the reads i with read_entry[i] !=
 *          UMI_READ_UNSTAGED and root[read_entry[i]] == r (umi_velocity_matrix' statement).  A molecule supports a
 *          junction when one of its reads has it.  Reads under a root with kept == 0 -- what umi_filter_multigene
 *          removed -- count nowhere, and unstaged reads contribute no junction.  The collapse is the call's own:
 *          NOTHING is collapsed again per junction (STARsolo's SJ dedups UMIs per cell and junction).
 *        The column of a molecule is col[b] of the bucket b that holds r.
 * in : read_ref, read_pos int32 [n_reads], cigar, cigar_off as umi_assign_genes takes them; read_entry uint32
 *      [n_reads]; kept uint8 [N] and root uint32 [N] of a batched call (N = bucket_off[n_buckets]); bucket_off (a HOST
 *      array in both forms); col uint32 [n_buckets], n_cols; capacity: the elements every output array has room for.
 *      The read_ref and the CIGAR words of a read that is unstaged or under a root that is not kept are not looked at.
 * out: the junction table jn_ref, jn_start, jn_end (int32): the distinct junctions of counted reads, sorted by (ref,
 *      start, end) ascending and numbered in that order, counts[2] of them.  The triplets out_jn, out_col (uint32),
 *      out_molecules (uint32), out_reads (uint64): one per distinct (col, junction), sorted by col, then junction,
 *      counts[3] of them; molecules = the distinct molecules of that column that support the junction, reads = the
 *      reads under kept roots of that column that have it.  counts (HOST, 4 words): 0 the counted reads with a
 *      junction, 1 the junction occurrences (the sum of reads over the triplets), 2 the junctions, 3 the triplets.
 * n_buckets == 0, every bucket empty or n_reads == 0: UMI_OK, counts all zero, nothing launched.  A multi-device
 * context uses its first device; a deferred call that is out ends first.  Grids come from the context's CU count
 * (option "grid_cus").  The stream is synchronised twice: once when the occurrences have been counted -- their number
 * T sizes the sorts and the workspace, and an error ends the call there with nothing written to the outputs -- and once
 * at the end.  Workspace, bytes: 16 n_reads + 12 m (m the non-empty buckets) and 48 T, and the temporaries of the
 * library's sort and scan.
 * UMI_ERR_ARG before any HIP call: NULL pointers the call would touch (counts always; every array where there are reads
 * and entries), n_reads >= 2^32, n_buckets >= 2^30, N >= 2^32, a bucket_off that does not start at 0 or that falls,
 * n_cols == 0 with a non-empty bucket.  Found on the device and told after the first synchronisation, the smallest
 * such read named and the outputs not defined: UMI_ERR_ARG for a read_ref < 0, a CIGAR op code above 8, a read_entry >=
 * N other than UMI_READ_UNSTAGED, a root[read_entry[i]] >= N; UMI_ERR_ORDER for a cigar_off that falls (nothing is
 * read outside cigar[0 .. cigar_off[n_reads])); UMI_ERR_ARG for a col >= n_cols of a non-empty bucket.
 * UMI_ERR_ARG where T exceeds capacity or reaches 2^30: counts[1] then holds T, the other counts 0, so the caller can
 * size the arrays and call again; nothing is written to the outputs.  The number of N words among the CIGARs is an upper
 * bound of T. */
int umi_junction_matrix_device(umi_ctx *ctx, const int32_t *d_read_ref, const int32_t *d_read_pos, const uint32_t *d_cigar,
                               const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint64_t n_reads,
                               const uint8_t *d_kept, const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets,
                               const uint32_t *d_col, uint32_t n_cols, uint64_t capacity, int32_t *d_jn_ref,
                               int32_t *d_jn_start, int32_t *d_jn_end, uint32_t *d_out_jn, uint32_t *d_out_col,
                               uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t counts[4], void *hip_stream);
int umi_junction_matrix(umi_ctx *ctx, const int32_t *read_ref, const int32_t *read_pos, const uint32_t *cigar,
                        const uint64_t *cigar_off, const uint32_t *read_entry, uint64_t n_reads, const uint8_t *kept,
                        const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets, const uint32_t *col,
                        uint32_t n_cols, uint64_t capacity, int32_t *jn_ref, int32_t *jn_start, int32_t *jn_end,
                        uint32_t *out_jn, uint32_t *out_col, uint32_t *out_molecules, uint64_t *out_reads,
                        uint64_t counts[4]);

/* ---- UMIs a group shows in several buckets (the program's --umi-filtering multi-gene): the molecules of a batched
 *      call joined across its buckets, on the GPU.  A UMI that one cell shows under two or more genes is a chimera
 *      or a mis-assignment: only the gene with the most reads keeps it, none where the top count is shared.  The
 *      rule is Cell Ranger's and STARsolo's --soloUMIfiltering MultiGeneUMI_CR; no counterpart in the reference,
 *      tests/multigene_model.py (filter_model) defines it.  Everything is exact integer arithmetic.
 * in : keys: n_words words per entry, entry-major, umi_len in 1..UMI_MAX_WIDE_UMI_LEN, n_words = ceil(3 * umi_len /
 *      64); no nmask: code 100 (N) is a letter of its own.  freq / kept / root: the N = bucket_off[n_buckets] entries
 *      as a batched call took and wrote them (any byte of kept other than 0 counts as kept).  bucket_off: a HOST
 *      array in both forms, [n_buckets + 1], starting at 0 and never falling.  group[b] < n_groups: the group (cell)
 *      of bucket b; the groups of empty buckets are not looked at.
 * A molecule is an entry with kept != 0; its UMI is its key's bits below 3 * umi_len (what lies above is not looked
 * at), its reads are total[r] = the sum of freq[i] over root[i] == r (64 bits).  The molecules of non-empty
 * buckets with the same (group, UMI) form a run, whatever their buckets are: the library never sees a gene, and two
 * buckets are two candidates even where a caller gave them the same (cell, gene).  A run of one molecule survives.
 * In a longer run the molecule whose total is strictly greater than every other's survives and the rest are
 * removed; where two or more hold the greatest total, all molecules of the run are removed.
 * out: kept_out[i] = 1 for the surviving molecules, 0 for every other entry.  freq_out (may be NULL): freq[i], or 0
 *      where root[i] was removed: umi_count_matrix on (kept_out, freq_out) counts the molecules and reads of
 *      survivors only.  counts[0] the runs of two or more molecules, counts[1] the molecules removed, counts[2]
 *      the sum of their total.  Only kept_out[0..N) and freq_out[0..N) are written, and they must not be the
 *      inputs.
 * n_buckets == 0 or every bucket empty: UMI_OK, counts zeroed, nothing launched, nothing else touched.  A
 * multi-device context uses its first device.  A deferred call (umi_dedup_batch_device_begin) that is out on the
 * context ends first; its result keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG: a NULL among ctx, counts and the arrays the call would touch, umi_len or n_words out of range, a
 * bucket_off that does not start at 0 or that falls, 2^30 entries or buckets or more, kept_out == kept or freq_out
 * == freq, n_groups == 0 with a non-empty bucket -- all found on the host before anything is launched.  Counted on
 * the device and told after the call's synchronisation, the outputs then not defined and counts zeroed: a
 * non-empty bucket whose group >= n_groups, a root[i] outside i's bucket or at an entry with kept == 0, a kept
 * entry with root[i] != i.
 * The _device form takes and leaves everything but bucket_off and counts in device memory, works on hip_stream
 * and synchronises it once, at the end; the plain form copies host arrays in and out around it. */
int umi_filter_multigene_device(umi_ctx *ctx, const uint64_t *d_keys, int n_words, int umi_len, const int32_t *d_freq,
                                const uint8_t *d_kept, const uint32_t *d_root, const uint64_t *bucket_off,
                                uint64_t n_buckets, const uint32_t *d_group, uint32_t n_groups, uint8_t *d_kept_out,
                                int32_t *d_freq_out, uint64_t counts[3], void *hip_stream);
int umi_filter_multigene(umi_ctx *ctx, const uint64_t *keys, int n_words, int umi_len, const int32_t *freq,
                         const uint8_t *kept, const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets,
                         const uint32_t *group, uint32_t n_groups, uint8_t *kept_out, int32_t *freq_out,
                         uint64_t counts[3]);

/* ---- cell calling (the program's --cell-filter): which columns of a count matrix are cells, their table, the
 *      run's summary numbers and the filtered matrix, on the GPU.  The rules are STARsolo's --soloCellFilter
 *      CellRanger2.2 (Cell Ranger 2.2's knee) and TopCells, and a plain threshold; no counterpart in the reference,
 *      tests/cells_model.py (call_model) defines them.  Everything is exact integer arithmetic.
 * in : the nnz triplets (row, col, molecules, reads) as umi_count_matrix leaves them: sorted by col, then row, every
 *      (col, row) pair once; a triplet may have 0 molecules.
 * For column c: T[c] the sum of molecules and R[c] the sum of reads (64 bits), G[c] its triplets with molecules > 0.
 * The candidates are the n columns with T[c] >= 1, S[0..n) their totals in descending order.  A rule yields one
 * threshold t, and column c is called iff T[c] >= 1 && T[c] >= t: a tie at the threshold is called whole.
 *   UMI_CELLS_CR22: i = min(n - 1, floor(expect_cells * (1000 - percentile_permille) / 1000)), m = S[i],
 *                   t = max(1, floor((2 m + max_min_ratio) / (2 max_min_ratio))) -- m / max_min_ratio rounded half up.
 *                   STARsolo's defaults are 3000, 990 and 10.
 *   UMI_CELLS_TOP : t = S[min(n - 1, expect_cells - 1)].
 *   UMI_CELLS_MIN : t = max(1, min_molecules).
 *   n == 0        : t = 0, nothing is called.
 * A rule reads only the parameters named in its line; the others are not looked at.
 * out: per column, n_cols elements each: cell_molecules = T, cell_reads = R, cell_genes = G, called (0 or 1) and
 *      new_col, the called columns' dense number in ascending col, 0xFFFFFFFF where the column is not called.  The
 *      filtered triplets (room for nnz each): the triplets of called columns with molecules > 0, in their input
 *      order, col replaced by new_col; *nnz_out their number; what lies behind is not defined.  counts[0] candidates,
 *      [1] called, [2] t, [3] m (0 under the other rules), [4] molecules and [5] reads in called columns, [6] all
 *      molecules, [7] all reads, [8] the median of T and [9] of G over the called columns: the lower median, element
 *      floor((k - 1) / 2) of the k values in ascending order, 0 for k = 0.
 * nnz == 0: UMI_OK, the per-column arrays zeroed (new_col all ones), counts zeroed, *nnz_out = 0, nothing launched.
 * A multi-device context uses its first device.  A deferred call (umi_dedup_batch_device_begin) that is out on the
 * context ends first; its result keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG, found on the host before anything is launched: a NULL among ctx, nnz_out, counts and the arrays the
 * call would touch, nnz or n_cols >= 2^30, n_cols == 0 or n_rows == 0 with nnz > 0, an unknown rule, expect_cells
 * < 1, percentile_permille outside 0..1000 or max_min_ratio < 1 where the rule reads them.  Counted on the device and
 * told after the call's one synchronisation, *nnz_out then 0 and the outputs not defined: UMI_ERR_ARG for a triplet
 * with row >= n_rows or col >= n_cols, UMI_ERR_ORDER for triplets that are not strictly increasing in (col, row).
 * The _device form takes and leaves everything but nnz_out and counts in device memory, works on hip_stream and
 * synchronises it once, at the end; the plain form copies host arrays in and out around it. */
#define UMI_CELLS_CR22 0
#define UMI_CELLS_TOP 1
#define UMI_CELLS_MIN 2
int umi_call_cells_device(umi_ctx *ctx, const uint32_t *d_row, const uint32_t *d_col, const uint32_t *d_molecules,
                          const uint64_t *d_reads, uint64_t nnz, uint32_t n_rows, uint32_t n_cols, int rule,
                          int64_t expect_cells, int percentile_permille, int64_t max_min_ratio, int64_t min_molecules,
                          uint64_t *d_cell_molecules, uint64_t *d_cell_reads, uint32_t *d_cell_genes, uint8_t *d_called,
                          uint32_t *d_new_col, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules,
                          uint64_t *d_out_reads, uint64_t *nnz_out, uint64_t counts[10], void *hip_stream);
int umi_call_cells(umi_ctx *ctx, const uint32_t *row, const uint32_t *col, const uint32_t *molecules,
                   const uint64_t *reads, uint64_t nnz, uint32_t n_rows, uint32_t n_cols, int rule, int64_t expect_cells,
                   int percentile_permille, int64_t max_min_ratio, int64_t min_molecules, uint64_t *cell_molecules,
                   uint64_t *cell_reads, uint32_t *cell_genes, uint8_t *called, uint32_t *new_col, uint32_t *out_row,
                   uint32_t *out_col, uint32_t *out_molecules, uint64_t *out_reads, uint64_t *nnz_out,
                   uint64_t counts[10]);

/* ---- what a batched call did, as tables (the program's --output-stats): family sizes before and after, the mean
 *      UMI distance of every bucket before and after against a null, and how every UMI sequence is used, on the
 *      GPU.  No counterpart in the reference; the tables are umi_tools dedup --output-stats's, tests/stats_model.py
 *      defines them.  Everything is exact integer arithmetic.
 * in : keys: n_words words per entry, entry-major, umi_len in 1..UMI_MAX_WIDE_UMI_LEN, n_words = ceil(3 * umi_len /
 *      64); no nmask: code 100 is N.  freq / kept / root: the N = bucket_off[n_buckets] entries as a batched call
 *      took and wrote them (any byte of kept other than 0 counts as kept).  bucket_off: a HOST array in both forms,
 *      [n_buckets + 1], starting at 0 and never falling.  hist_bins in 2..2^24.
 * out: count_pre / count_post [hist_bins]: count_pre[min(freq[i], hist_bins - 1)] counts every entry;
 *      total[r] = the sum of freq[i] over root[i] == r (64 bits), and count_post[min(total[i], hist_bins - 1)]
 *      counts every kept entry; the last bin collects everything at or above it.
 *      dist [4][umi_len + 2], rows 0 pre, 1 pre-null, 2 post, 3 post-null; column j <= umi_len is bin j, column
 *      umi_len + 1 is "single".  A UMI's letter at base b is the 3-bit code at bits [3b, 3b + 3) of its key read
 *      as one little-endian integer (000 A, 110 C, 011 G, 101 T, 100 N); two letters differ iff their codes
 *      differ, so N is a letter of its own (the rule of umi_dedup_batch_edit; for UMIs without N: umi_dist).  A
 *      set of m UMIs (a multiset for the nulls; equal UMIs are at distance 0) contributes nothing if m = 0, one
 *      to "single" if m = 1, else one to bin (S + P - 1) / P, S the sum of its pair distances and P = m (m - 1) /
 *      2: the mean rounded up, where umi_tools' digitize(..., right=True) puts it.  Per non-empty bucket [s, e)
 *      with m kept entries: pre the UMIs of all its entries, post those of the kept ones, pre-null those of the
 *      entries pick(i) for i in [s, e), post-null those of pick(i) for i in [s, s + m).  pick(i) draws an entry
 *      with probability proportional to its reads: x = seed + 0x9E3779B97F4A7C15 * (i + 1) mod 2^64; x ^= x >>
 *      30; x *= 0xBF58476D1CE4E5B9; x ^= x >> 27; x *= 0x94D049BB133111EB; x ^= x >> 31; t = the high 64 bits of
 *      x * R, R the sum of all freq; pick(i) = the smallest e with cum[e] > t, cum the inclusive scan of freq.
 *      The per-UMI table (its five arrays NULL together: left out, n_umis may then be NULL too; else room for N
 *      rows each): one row per distinct key among the N entries, in ascending order of the key as a little-endian
 *      integer (word n_words - 1 the most significant; bits from 3 * umi_len up are not looked at).  umi_entry the
 *      smallest entry that holds the key, times_pre the entries that hold it, reads_pre the sum of their freq,
 *      times_post the kept entries among them, reads_post the sum of their total[]; *n_umis the rows.  What lies
 *      behind them is not defined.
 * n_buckets == 0 or every bucket empty: UMI_OK, the three tables zeroed, *n_umis = 0, nothing else launched.  A
 * multi-device context uses its first device.  A deferred call (umi_dedup_batch_device_begin) that is out on the
 * context ends first; its result keeps waiting for umi_dedup_batch_end.
 * UMI_ERR_ARG: a NULL among ctx and the arrays the call would touch, some but not all of the table's five,
 * umi_len, n_words or hist_bins out of range, a bucket_off that does not start at 0 or that falls, 2^31 entries or
 * more (2^30 with the per-UMI table: its sort's index space), a bucket of 2^28 entries or more (S would pass 64
 * bits at 85 bases) -- all found on the host before anything is launched.  Counted on the device and told after the
 * call's synchronisation, the outputs then not defined: a code other than the five at a base below umi_len, a
 * root[i] outside i's bucket or at an entry with kept == 0, a kept entry with root[i] != i.
 * Option "stats_split" (64..2^30, default 4096): a bucket of at least this many entries is counted in pieces by
 * the whole grid instead of by one wave; same result.
 * The _device form takes and leaves everything but bucket_off and n_umis in device memory, works on hip_stream
 * and synchronises it once, at the end; the plain form copies host arrays in and out around it. */
int umi_dedup_stats_device(umi_ctx *ctx, const uint64_t *d_keys, int n_words, const int32_t *d_freq, const uint8_t *d_kept,
                           const uint32_t *d_root, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t seed,
                           uint32_t hist_bins, uint64_t *d_count_pre, uint64_t *d_count_post, uint64_t *d_dist,
                           uint32_t *d_umi_entry, uint32_t *d_times_pre, uint64_t *d_reads_pre, uint32_t *d_times_post,
                           uint64_t *d_reads_post, uint64_t *n_umis, void *hip_stream);
int umi_dedup_stats(umi_ctx *ctx, const uint64_t *keys, int n_words, const int32_t *freq, const uint8_t *kept,
                    const uint32_t *root, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint64_t seed,
                    uint32_t hist_bins, uint64_t *count_pre, uint64_t *count_post, uint64_t *dist, uint32_t *umi_entry,
                    uint32_t *times_pre, uint64_t *reads_pre, uint32_t *times_post, uint64_t *reads_post, uint64_t *n_umis);

/* ---- batched path: replaces the whole bucket loop
 *      src/deduplicate_sam.rs:207-233 (apply::<UcSAMRead,Naive> per bucket,
 *      counters :217-219) = Directional/Adjacency::apply
 *      (src/algo/directional.rs:57-91, src/algo/adjacency.rs:29-63) over the
 *      Naive store (src/data/naive.rs:26-44). -------------------------------
 * keys/nmask/freq: N = bucket_off[n_buckets] entries; bucket b owns
 * [bucket_off[b], bucket_off[b+1]).  Inside a bucket entries MUST already be in
 * rank order: freq descending (directional.rs:72), ties in first-appearance
 * order (canonical determinisation); freq >= 1.
 * percentage = Cli.percentage (src/cli.rs:25-26), k = Cli.k (src/cli.rs:18-19):
 * any k >= 0 up to INT_MAX; a k no distance can reach (128 and more: umi_dist is at most 32 per
 * key word) means every pair of a bucket, in every entry point that takes a k.
 * adj_max_freq: third argument of remove_near in adjacency.rs:56 (reference: 0).
 * kept[i] = 1 iff entry i survives; survivors in ascending index order are the
 * reference's output order (deduplicate_sam.rs:227-231).  root (may be NULL):
 * global index of the root that removed entry i (ClusterTracker::add_all,
 * directional.rs:42-44).  stats may be NULL.
 * algo = UMI_ALGO_CLUSTER: connected components.  Per bucket, the graph on its entries with an edge
 * i ~ j iff dist(i, j) <= k (the distance of the entry point: umi_dist here, the per-word arithmetic in
 * the _wide and _seqs forms, d_E in umi_dedup_batch_edit; N semantics and any k as for the other two).
 * kept[i] = 1 iff i is the smallest index of its connected component, root[i] = that smallest index --
 * in rank order the entry the root loop reaches first.  Frequencies take no part in the result:
 * percentage is accepted with any bit pattern (NaN, negative, inf) and ignored, and so is adj_max_freq.
 * The bucket contract holds and is checked all the same (freq >= 1 and non-increasing inside a bucket,
 * nmask covering every N code: UMI_ERR_ORDER); freq = INT32_MAX is legal, there is no threshold to wrap.
 * It is the `cc` the reference's help names and its main() refuses (src/cli.rs:33-36,
 * src/main.rs:86-91), umi_tools' `--method cluster`, with k = 1 STARsolo's `--soloUMIdedup 1MM_All`, and
 * -- while freq < 2^31 - 1 -- the directional result at percentage = +inf.  umi_stats: n_edges = the pairs
 * within k found outside the fused buckets, each once; n_rounds <= 1 (the union pass; no round along
 * one-way pairs exists); the other counters as for a directional call on the same path.  Any other algo
 * value is UMI_ERR_ARG.
 * Buffers are caller-owned host memory; the library never frees them. */
int umi_dedup_batch(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask,
                    const int32_t *freq, const uint64_t *bucket_off, uint64_t n_buckets,
                    int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                    uint8_t *kept, uint32_t *root, umi_stats *stats);

/* Same contract with keys/nmask/freq/kept/root already resident in this GPU's
 * HBM (d_*), work enqueued on hip_stream (a hipStream_t, NULL = default
 * stream); bucket_off stays a host array.  Returns after the results are
 * complete on the device (the call synchronises the stream to read its
 * counters). */
int umi_dedup_batch_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                           const int32_t *d_freq, const uint64_t *bucket_off,
                           uint64_t n_buckets, int umi_len, int k, float percentage, int algo,
                           int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root,
                           void *hip_stream, umi_stats *stats);
/* The same with the bucket table resident on the device as well (d_bucket_off: a device copy of
 * bucket_off, or NULL for the call above): nothing of the table is staged or uploaded inside the
 * call -- for a batch of 10^5 small positions that copy is what the first kernel waits for.  The
 * host copy is still the one that is validated and planned from; a device table that differs from
 * it is the caller's error (entries it would lead outside the arrays are skipped and reported as
 * UMI_ERR_ORDER). */
int umi_dedup_batch_device_table(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                                 const int32_t *d_freq, const uint64_t *bucket_off,
                                 const uint64_t *d_bucket_off, uint64_t n_buckets, int umi_len, int k,
                                 float percentage, int algo, int32_t adj_max_freq, uint8_t *d_kept,
                                 uint32_t *d_root, void *hip_stream, umi_stats *stats);

/* ---- the batched call by Levenshtein (edit) distance: umi_dedup_batch's contract with d_E in place of
 *      umi_dist (src/utils/mod.rs:24-26).  No counterpart in the reference; the distance is the one
 *      starcode and the long-read UMI pipelines cluster by, because a base lost or gained in synthesis
 *      shifts the rest of a fixed-length UMI window: ACGTACGTACGT without its first base is read as
 *      CGTACGTACGTx, Hamming distance ~9, edit distance 2.
 *      d_E(a, b): substitution, insertion and deletion cost 1 each, over the umi_len letters of A T C G N;
 *      two letters match iff they are the same letter (N matches N and nothing else, as in umi_dist).
 *      For equal lengths d_E <= d_H, and d_E == d_H wherever either is at most 1 -- one indel alone changes
 *      the length, so an indel costs 2 and k <= 1 gives umi_dedup_batch's result bit for bit; the two differ
 *      from k = 2 on.  Rank order inside a bucket, the f32 threshold, algo (UMI_ALGO_CLUSTER: the connected
 *      components of d_E <= k), adj_max_freq, kept / root, stats,
 *      UMI_ERR_ORDER: as umi_dedup_batch.  Any k >= 0 up to INT_MAX; min(k, umi_len) is what is computed
 *      with (no distance is larger), k >= umi_len means every pair of a bucket.
 *      Keys are one word, umi_len 1..UMI_MAX_UMI_LEN; code 100 in a key is N, so nmask may be NULL whatever
 *      the keys hold.  Where it is given, a key with code 100 at a base it does not cover is UMI_ERR_ORDER.
 *      UMI_ERR_ARG: umi_len above 21, a multi-device context, 2^31 entries or more.
 *      Every bucket goes through edit_pair_kernel (kernel_id UMI_KERNEL_EDIT_PAIRS), all pairs behind a
 *      filter on the keys' letter counts: n_pairs_evaluated = n_pairs = W, n_candidates = the pairs that
 *      passed the filter and had their exact distance taken.  A deferred call
 *      (umi_dedup_batch_device_begin) that is out on the context ends first; its result keeps waiting for
 *      umi_dedup_batch_end. */
int umi_dedup_batch_edit(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                         const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k, float percentage,
                         int algo, int32_t adj_max_freq, uint8_t *kept, uint32_t *root, umi_stats *stats);
int umi_dedup_batch_edit_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                                const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets,
                                int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                                uint8_t *d_kept, uint32_t *d_root, void *hip_stream, umi_stats *stats);

/* ---- the batched call by Cell Ranger's one-mismatch correction (umihip_cr.hip).  No counterpart in the
 *      reference; the rule is stated after Cell Ranger's correct_umi loop and STARsolo's --soloUMIdedup 1MM_CR and
 *      is not claimed byte-equal to either program.  It is not transitive, so no k and percentage of the other
 *      algorithms reaches it; this is a call of its own, not a fourth `algo` (umi_dedup_batch*(algo = 3) stays
 *      UMI_ERR_ARG).  Exact integers and letters; tests/cr_model.py states it twice in plain Python.
 *      Inside one bucket of distinct UMIs of umi_len letters over A C G T N, with freq:
 *        candidates  t is a candidate for s when the two differ at exactly one base p and t[p] is one of A C G T
 *                    (the loop substitutes the four nucleotides at every position and looks the result up): an N
 *                    in s may be replaced, an N is never substituted in;
 *        target      target(s) = the maximum of {s} and its candidates under (freq, then the UMI as a byte string,
 *                    A < C < G < N < T): a higher count wins, among equal counts the lexicographically largest
 *                    string, s itself included (the sequential loop's `value > count or (value == count and
 *                    corrected < test)`);
 *        molecules   a UMI is a molecule iff it is some UMI's target, its own included: for a -> b, b -> c both b
 *                    and c are molecules.
 *      kept[i] = 1 iff entry i is a target.  root[i] (may be NULL) = i where kept[i], else target(i), which is kept
 *      by construction: kept[i] implies root[i] == i, and kept[root[i]] -- the contract umi_count_matrix,
 *      umi_filter_multigene, umi_dedup_stats, the velocity, saturation and junction calls check, so they take the
 *      result unchanged.  target[i] (may be NULL) = the raw target, which may be a kept entry whose own target lies
 *      elsewhere.  Difference from Cell Ranger: the reads of a kept UMI that Cell Ranger would itself correct stay
 *      with that UMI under root[]; molecule counts are the same, reads per molecule in such chains are not.
 *      The distance is fixed at one substitution: no k, no percentage, no adj_max_freq.
 *      Keys are one word, umi_len 1..UMI_MAX_UMI_LEN; code 100 in a key is N, so nmask may be NULL whatever the
 *      keys hold (where it is given, a key with code 100 at a base it does not cover is UMI_ERR_ORDER).  Entries of
 *      a bucket in rank order and freq >= 1 as for umi_dedup_batch (UMI_ERR_ORDER).  UMI_ERR_ARG: umi_len above
 *      21, a multi-device context, 2^31 entries or more, NULL keys / freq / kept with entries present.  No entries:
 *      UMI_OK.  A deferred call that is out on the context ends first.
 *      Option "cr_small_max" (0..1024, default 128): a bucket of at most this many entries is decided by a kernel
 *      with one lane per entry that walks the bucket and keeps its best (count, string, index) in registers; a
 *      larger one through the list of pairs within one substitution that the pipeline of umi_data_new leaves,
 *      resolved by three passes that do not depend on the list's order (best count, best string at that count,
 *      the one index that has it).  Same bytes on either path.
 *      umi_stats: n_umis, n_buckets, max_bucket, n_kept, n_pairs as for the other calls; n_edges = the unordered
 *      pairs of one bucket at exactly one mismatching base, admissible or not, on both paths; ms_* under "profile"
 *      (ms_pairs: the small buckets' kernel and the pipeline; ms_collapse: the list's resolution).
 *      The symbols are additive: UMI_ABI_VERSION stays 2. */
int umi_dedup_batch_cr(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                       const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint8_t *kept, uint32_t *root,
                       uint32_t *target, umi_stats *stats);
int umi_dedup_batch_cr_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                              const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, uint8_t *d_kept,
                              uint32_t *d_root, uint32_t *d_target, void *hip_stream, umi_stats *stats);

/* The kept mask as one bit per entry (bit i % 8 of byte i / 8; ceil(n / 8) bytes at d_bits), packed
 * on the device and enqueued on hip_stream: what a one-process-per-GPU host all-gathers over RCCL
 * to reassemble the mask of a bucket-sharded job (n / 8 bytes per rank instead of n). */
int umi_pack_mask_device(umi_ctx *ctx, const uint8_t *d_kept, uint64_t n, uint8_t *d_bits,
                         void *hip_stream);

/* The device-pointer call in two halves, for a host that has more to enqueue behind it (the packing
 * and gathering of the kept mask of a multi-GPU step: ~30 us of host time that would otherwise pass
 * with the GPU idle).  umi_dedup_batch_device_begin enqueues the call's work on hip_stream; where every
 * position is the fused kernel's (no host decision is left: BASELINE configs 3, 4, 5) it returns
 * without waiting -- d_kept / d_root are then final in stream order, and work enqueued on the same
 * stream behind the call may read them -- otherwise it runs to its end like umi_dedup_batch_device_table.
 * umi_dedup_batch_end waits for the call's end (if it is still out), reports a contract violation
 * (UMI_ERR_ORDER) and fills stats.  One call may be out per context; any other call on the context
 * that needs its workspace lets it end first (its result keeps waiting for umi_dedup_batch_end; a
 * second begin replaces it). */
int umi_dedup_batch_device_begin(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                                 const int32_t *d_freq, const uint64_t *bucket_off,
                                 const uint64_t *d_bucket_off /* may be NULL */, uint64_t n_buckets,
                                 int umi_len, int k, float percentage, int algo, int32_t adj_max_freq,
                                 uint8_t *d_kept, uint32_t *d_root, void *hip_stream);
int umi_dedup_batch_end(umi_ctx *ctx, umi_stats *stats);

/* ---- one process, several GPUs, resident shards: the batched call on every device of a multi-device
 *      context at once -- device r works on its own arrays d_*[r] (its share of the positions: the
 *      iterations of src/deduplicate_sam.rs:207-233 share nothing but additive counters, so there is no
 *      exchange on the data path), bucket_off[r] / n_buckets[r] are its host tables -- and then the
 *      all-gatherv that reassembles the kept mask on every device: each device's mask packed to bits
 *      (umi_pack_mask_device's layout), padded to slice_bytes, all-gathered over RCCL / xGMI into
 *      d_mask_bits_all[r] (device r's buffer of n_devices * slice_bytes bytes; slice q = device q's
 *      entries in its own order).  d_nmask, d_root, d_mask_bits_all may be NULL (no N anywhere / no roots
 *      wanted / no gather); slice_bytes >= ceil(n_r / 8) for every r.  librccl.so is opened at the
 *      first call that asks for the gather; the device ids of the context must then be distinct. */
int umi_dedup_batch_device_multi(umi_ctx *ctx, const uint64_t *const *d_keys, const uint64_t *const *d_nmask,
                                 const int32_t *const *d_freq, const uint64_t *const *bucket_off,
                                 const uint64_t *n_buckets, int umi_len, int k, float percentage, int algo,
                                 int32_t adj_max_freq, uint8_t *const *d_kept, uint32_t *const *d_root,
                                 uint8_t *const *d_mask_bits_all, uint64_t slice_bytes, umi_stats *stats);

/* ---- multi-GPU split of ONE call's all-pairs work (a single giant bucket
 *      does not shard by buckets).  Each of n_parts ranks holds the same inputs on its own
 *      GPU, evaluates every n_parts-th tile task and gets its share of the permitted-edge
 *      list; the ranks all-gather their lists (RCCL) and every rank -- or one -- collapses the
 *      union.  Entries of d_edges are (src | flag<<31, dst) pairs of uint32 packed in a uint64
 *      and are opaque to the caller.  No counterpart in the reference (it has no second
 *      device); the result equals umi_dedup_batch_device on the same inputs. ------------ */
/* part in [0, n_parts), n_parts >= 2.  d_edges: caller's device buffer of edge_capacity
 * entries; *n_edges_out = entries produced (if it exceeds edge_capacity: UMI_ERR_NOMEM,
 * nothing copied, call again with a larger buffer).  algo = UMI_ALGO_CLUSTER: every pair within k,
 * each once and every one flagged. */
int umi_pairs_partial_device(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                             const int32_t *d_freq, const uint64_t *bucket_off,
                             uint64_t n_buckets, int umi_len, int k, float percentage, int algo,
                             int32_t adj_max_freq, uint32_t part, uint32_t n_parts,
                             uint64_t *d_edges, uint64_t edge_capacity, uint64_t *n_edges_out,
                             void *hip_stream, umi_stats *stats);
/* Collapse of a gathered edge list over n entries (same index space as the calls that
 * produced it): kept / root as in umi_dedup_batch_device.  algo = UMI_ALGO_CLUSTER: the unions of the
 * flagged entries and one write-out (the lists of a cluster call hold no other; an entry without the flag
 * is the caller's error and is not looked at). */
int umi_collapse_edges_device(umi_ctx *ctx, uint64_t n, const uint64_t *d_edges, uint64_t n_edges,
                              int algo, uint8_t *d_kept, uint32_t *d_root, void *hip_stream,
                              umi_stats *stats);

/* ---- per-bucket path: 1:1 with trait DataStruct (src/data/mod.rs:11-17) as
 *      implemented by Naive (src/data/naive.rs).  UMIs are addressed by their
 *      index in the arrays handed to umi_data_new. -------------------------- */
/* DataStruct::new (naive.rs:22-24): takes the {umi -> freq} map of one bucket
 * (n entries, host memory, copied) and builds the all-pairs neighbour lists
 * dist <= max_edits on the GPU once. */
int umi_data_new(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                 uint32_t n, int umi_len, int max_edits, umi_data **out);
/* The same for keys of n_words = ceil(3 * umi_len / 64) words (umi_len up to UMI_MAX_WIDE_UMI_LEN,
 * entry-major as in umi_dedup_batch_wide); remove_near / contains / free as above. */
int umi_data_new_wide(umi_ctx *ctx, const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                      uint32_t n, int umi_len, int max_edits, umi_data **out);
/* DataStruct::remove_near (naive.rs:26-40): removes and returns every remaining
 * entry o with dist(query,o) <= k && (dist == 0 || freq[o] <= max_freq).
 * k must be <= max_edits.  out_idx has capacity n; ascending index order. */
int umi_data_remove_near(umi_data *d, uint32_t query, int k, int32_t max_freq, uint32_t *out_idx,
                         uint32_t *out_n);
/* DataStruct::contains (naive.rs:42-44): 1 / 0, negative on error. */
int umi_data_contains(const umi_data *d, uint32_t idx);
/* Drop of the store. */
void umi_data_free(umi_data *d);

#ifdef __cplusplus
}
#endif
#endif
