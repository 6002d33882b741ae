// Internal interface between the host side (umihip_pipeline.cpp) and the gfx950
// kernels (umihip_kernels.hip).  Not part of the C ABI.
#pragma once

#include <hip/hip_runtime_api.h>
#include <stdint.h>

namespace umihip {

// One unit of all-pairs work: rows [row0, min(row0 + tile_rows, row_end)) against
// columns [col0, col1), all global entry indices of one bucket.  Only pairs with
// row < col are reported, so a task whose column range starts at row0 covers
// the diagonal tile.
struct PairTask {
    uint32_t row0;
    uint32_t row_end;
    uint32_t col0;
    uint32_t col1;
};

enum PairMode : int {
    MODE_DIRECTIONAL = 0, // directed edges u->v with freq[v] <= thr[u]   (directional.rs:38-39)
    MODE_ADJACENCY = 1,   // forward edges u->v (u<v) with freq[v] <= max_freq (adjacency.rs:56)
    MODE_NEIGHBOURS = 2,  // undirected (i<j, dist) lists for the DataStruct path
    MODE_CLUSTER = 3,     // connected components: every pair within k is a symmetric pair, freq takes no part
};

enum Counter : int {
    CNT_EDGES = 0,      // directed edges appended (may exceed capacity: overflow)
    CNT_CANDIDATES = 1, // filter hits that reached the exact check
    CNT_ERROR = 2,      // prep validation failures
    CNT_KEPT = 3,       // survivors
    CNT_UNKNOWN = 4,    // adjacency collapse: undecided entries
    CNT_RISES = 5,      // entries whose freq is above their predecessor's
    CNT_START_RISES = 6, // ... of which sit at the start of a bucket (the only legal place)
    CNT_OVF = 7,        // filter hits that did not fit a block's LDS queue (global overflow list)
    CNT_ITEMS = 8,      // table kernel: (row tile, column tile) items its scan found to walk ...
    CNT_DIAG_ITEMS = 9, // ... and those on a bucket's diagonal (dense in hits; listed apart, worked off first)
    CNT_GRAB = 10,      // next item to hand out
    CNT_DIAG_GRAB = 11,
    CNT_SEG_TASKS = 12, // segment index: (sub-bucket, 64-row chunk) tasks its scan produced
    CNT_SEG_PAIRS = 13, // ... and the pairs inside its sub-buckets (what the pair kernel compares)
    CNT_KEPT_FUSED = 14, // survivors of the buckets the fused one-wave kernel finished by itself
    CNT_UF_DIRECT = 15, // symmetric pairs the segment index's pair kernel united on the spot (not in the list)
    CNT_EDGES_MOVED = 16, // edges the flatten launch moved from the pair kernel's private slots to the list, behind
                          // the CNT_EDGES it found there (the list's length is the sum of the two)
    CNT_SEG_CROSS_ABANDONED = 17, // a super-bin of a cross segment could not be served (a key twice, a run above the cap):
                                  // the call's cross pairs are to be found again through part 1 (a plain store of 1)
    CNT_COUNT = 18,
};
// The flags of the collapse rounds ("round r changed a label") sit behind the counters in the
// same device block, so that one memset clears and one copy reads everything the host looks at.
constexpr int MAX_ROUNDS_PER_SYNC = 16; // rounds enqueued between two host checks
constexpr size_t CTRL_FLAGS_OFF = CNT_COUNT * sizeof(unsigned long long);
constexpr size_t CTRL_BYTES = (CTRL_FLAGS_OFF + (MAX_ROUNDS_PER_SYNC + 1) * sizeof(uint32_t) + 255) & ~(size_t)255; // (one fill kernel: a whole number of 16-byte words)

// Bit-sliced kernel: one block works on rows [bucket_start + 32*group0, ...) of one
// bucket (256*G or 64*G groups of 32 rows, see BS_* below) against columns [col0, col1).
struct BsTask {
    uint32_t bucket_start; // global index of the bucket's first entry
    uint32_t bucket_end;
    uint32_t group0;       // first 32-row group of this tile, relative to the bucket
    uint32_t ngroups;      // groups in the bucket = ceil(n / 32)
    uint64_t plane_off;    // word offset of the bucket's planes: planes[plane_off + g*np + b] (group-major)
    uint32_t col0, col1;   // global column range
    uint32_t diag;         // 1 if some column index <= some row index (needs the row<col mask)
    uint32_t pad;
};

// A run of entries for the per-entry kernels (prep, finalize): one block each.
struct RangeTask {
    uint32_t start, end;
    uint32_t seg; // segment (SegDesc index) of the bucket the run lies in, SEG_NONE if it has none
};
constexpr uint32_t SEG_NONE = 0xFFFFFFFFu;

// ---- segment index: the n-gram partition of a large bucket ----------------------------------
// Two UMIs within k substitutions agree exactly on at least one of k+1 disjoint base ranges
// ("parts", pigeonhole).  A large bucket (a segment) is therefore cut k+1 times into
// sub-buckets of entries that share a part's bases, and the all-pairs evaluation runs inside
// the sub-buckets only: every pair within k is in one of them, every pair inside one is decided
// by the same distance arithmetic as before.  The reference family's own n-gram index
// (`--data ngram*` of the CLI, src/cli.rs:43-44, never implemented in the Rust port) prunes the
// same way; the result is Naive's (src/data/naive.rs:26-40), which is all the reference ever runs.
constexpr int SEG_MAX_PARTS = 8; // k + 1
#if defined(__HIPCC__)
#define UMIHIP_HD __host__ __device__
#else
#define UMIHIP_HD
#endif
struct SegDesc {
    uint32_t start, end;             // global entry range of the bucket
    uint32_t bin_off[SEG_MAX_PARTS]; // first bin of part j in the call's bin array
    uint8_t b0[SEG_MAX_PARTS];       // first base of part j
    uint8_t nb[SEG_MAX_PARTS];       // leading bases of part j that index its bins (4^nb bins)
    uint64_t mask[SEG_MAX_PARTS];    // filter-key bits those bases occupy: two entries share the bin of
                                     // part j iff (key_a ^ key_b) & mask[j] == 0
    uint8_t sup_g;                   // super-bin exponent of part 0 (seg_super_kernel): 4^sup_g adjacent part-0 bins --
                                     // they share the upper nb[0] - sup_g bases of the bin code and lie back to back in
                                     // the sub-bucket arrays -- are decided as one unit in LDS; 0: none
    uint8_t cross;                   // 1: the pairs that differ in a base the super-bins share are found by ANDing the
                                     // super-bins' rest-code maps (seg_cross_kernel) -- part 1 is counted, not filed
    uint8_t sup_pad[6];              // (zero: the plan's tables are compared byte by byte)
};
// One super-bin: the part-0 bins [bin0, bin0 + 4^g) of a segment whose part 0 is indexed by nb bases and leaves
// rest = umi_len - nb + g bases to tell its entries apart
struct SegSuper {
    uint32_t bin0;
    uint8_t g, nb, rest, cross; // cross: SegDesc::cross of its segment
    uint32_t seg;               // its segment
    uint32_t map0;              // cross: first word of its rest-code map in SegArgs::cross_map (4^rest / 32 words; the
                                // segment's maps lie back to back in super-bin order)
};
static_assert(sizeof(SegSuper) == 16, "no padding: the plan's tables are compared byte by byte");
// words of a super-bin's rest-code map (rest >= 4: a segment's part 0 takes half the bases at most)
UMIHIP_HD inline uint32_t seg_cross_words(uint32_t rest) { return rest >= 3u ? 1u << (2u * rest - 5u) : 1u; }
// An entry in sub-bucket order: everything the pair kernel needs of it, 16 bytes
struct SegRec32 {
    uint32_t key; // filter key
    uint32_t idx; // entry index
    int32_t freq;
    uint32_t ckey; // compare key of the part the record is filed under: the bases outside the bin's own
                   // (those agree inside a sub-bucket), 3 bits each in the reference's code (N folded
                   // onto A), so that bases differing = popcount(a ^ b) / 2; 0 where it does not fit
};
struct SegRec64 {
    uint64_t key;
    uint32_t idx;
    int32_t freq;
};
// One block of the bin scan: bins [bin0, bin0 + nbins) of part `part` of segment `seg`.
struct SegScanChunk {
    uint32_t bin0, nbins; // nbins <= SEG_SCAN_CHUNK
    uint32_t seg, part;
};
constexpr uint32_t SEG_SCAN_CHUNK = 256;
// One unit of sub-bucket work: rows [row0, min(row0 + 64, end)) against columns [col0,
// min(end, col0 + 64 * 2^e)) of the same sub-bucket (which ends at `end`), all positions in the
// sub-bucket arrays; only pairs with row < column count.  A 64-row chunk faces nt - t tiles of 64
// later entries (t = its number, nt = the sub-bucket's chunks).  Up to 16 chunks (1025 entries)
// every tile is a task of its own, e = 0: tasks of one size, which the pair kernel's persistent
// waves can be dealt statically (whole chunks of 1..nt tiles each left the slowest wave of config
// 2 with 1.7 times the average; drawing tasks from counters costs a returning atomic's round trip
// per task, more than a tile).  Beyond that e grows so that a chunk never gives more than 16 tasks.
struct SegTask {
    uint32_t row0, end;
    uint32_t col0;
    uint32_t where; // segment | part << 24 | e << 28
};
UMIHIP_HD inline uint32_t seg_chunks_of(uint32_t c) { return c >= 2 ? (c - 1 + 63) / 64 : 0u; } // nt
UMIHIP_HD inline uint32_t seg_span_log2(uint32_t nt)
{
    uint32_t e = 0;
    while (((nt + 15) / 16) > (1u << e)) e++;
    return e;
}
// tasks of a sub-bucket of c entries: sum over its chunks t of ceil((nt - t) / span)
UMIHIP_HD inline uint32_t seg_tasks_of_bin(uint32_t c)
{
    const uint32_t nt = seg_chunks_of(c);
    if (nt == 0) return 0;
    const uint32_t span = 1u << seg_span_log2(nt), q = nt / span, r = nt % span;
    return span * (q * (q + 1) / 2) + r * (q + 1);
}
// ... and an upper bound for a part of n entries over `bins` bins (seg_tasks_of_bin(c) <= 1 + c / 7)
inline uint64_t seg_task_bound(uint64_t n, uint64_t bins) { return n / 7 + (bins < n / 2 ? bins : n / 2) + 64; }
// One block of the counting sort's LDS path: entries [start, end) of segment `seg`
// (<= SEG_BLOCK_ENTRIES of them).  The block counts its entries per bin in LDS and touches a bin's
// global word once (count pass: one add; scatter pass: one returning add that reserves the
// block's run inside the bin), so a bin's word takes one atomic per block instead of one per entry
// -- device-scope atomics are served at the memory side of the fabric (~3e10 per second over the
// whole chip, ~90 per microsecond on one word), which is what bounded the per-entry version.
struct SegBlock {
    uint32_t start, end;
    uint32_t seg, pad;
};
constexpr uint32_t SEG_BLOCK_THREADS = 1024;
constexpr uint32_t SEG_BLOCK_ENTRIES = 8 * SEG_BLOCK_THREADS;
constexpr uint32_t SEG_LDS_BINS = 16384; // bins of one part the LDS path takes (64 KB of counters)
constexpr uint32_t RANGE_CHUNK = 2048; // entries per range task (one block of 256 threads)

constexpr int BS_TAB_G = 1;     // row groups of 32 per lane of the table variant (a wave: 64 * 32 * G rows)
constexpr int BS_TAB_TILE = 256;       // columns per work item of the table variant
constexpr int FUSED_MAX = 128; // largest bucket the fused one-wave kernel takes (2 rows per lane)

// One wave transposes 64 rows of one bucket into bit planes.
struct PlaneTask {
    uint32_t row0;       // global index of the first row
    uint32_t bucket_end;
    uint64_t plane_off;
    uint32_t ngroups;
    uint32_t group;      // group index of row0 inside the bucket (even)
};

struct PairArgs {
    const uint64_t *keys;
    const uint64_t *nmask; // may be null
    const int32_t *freq;
    const int32_t *thr;
    const void *fkey; // uint32_t[N] (2 bits/base, umi_len <= 16) or uint64_t[N] (see prep)
    const PairTask *tasks;
    const BsTask *bs_tasks;
    const uint32_t *planes;
    const uint32_t *perm; // prune mode: sorted position -> original entry index (else null)
    uint2 *edges;
    uint8_t *edge_dist; // MODE_NEIGHBOURS only
    unsigned long long *counters;
    uint2 *ovf;        // (row, column) of the filter hits beyond a block's LDS queue, tile indices
    uint32_t ovf_cap;
    uint32_t edge_cap;
    uint32_t n_entries; // entries of the call (keys, fkey, ... have this many)
    int k;
    int mode;
    int32_t adj_max_freq;
};

// tile geometry of the two pair kernels (rows per block)
constexpr int SMALL_THREADS = 64;
constexpr int SMALL_RPT = 1;
constexpr int BIG_THREADS = 256;
constexpr int BIG_RPT = 8;
constexpr int SMALL_ROWS = SMALL_THREADS * SMALL_RPT;
constexpr int BIG_ROWS = BIG_THREADS * BIG_RPT;
constexpr int COL_TILE = 1024; // column keys staged in LDS per step

// segs/bin_cnt (may be null): entries of ranges with a segment also count themselves into the
// bins of their n_seg_parts parts
// skip_seg: the ranges of segments are the count kernel's (SegArgs::prep_keys), which also tells a
// rise at its bucket's start from one inside (seg_from: the smallest segment); entries_too false:
// every range is a segment's, nothing to launch
hipError_t launch_prep(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                       const uint64_t *bucket_off, uint64_t n_buckets, const RangeTask *ranges,
                       uint32_t n_ranges, uint32_t n, uint32_t fused_max, int umi_len, float percentage,
                       bool key32, void *fkey, int32_t *thr, uint32_t *label, uint32_t *lab,
                       unsigned long long *counters, const SegDesc *segs, int n_seg_parts,
                       uint32_t *bin_cnt, hipStream_t s, bool skip_seg = false, bool entries_too = true,
                       uint32_t seg_from = 0xFFFFFFFFu, int key_words = 1, int full_umi_len = 0);

// ---- segment index (umihip_seg.hip) ----
struct SegArgs {
    const SegDesc *segs;
    const SegScanChunk *chunks;
    uint32_t n_chunks;
    int n_parts;            // k + 1
    uint32_t *bin_cnt;      // [n_bins] entries per bin (prep); reused as the scatter cursor
    uint32_t *bin_start;    // [n_bins] first position of the bin in the sub-bucket arrays
    unsigned long long *scan_state; // [1 + n_chunks + segments] the scan's ticket counter, its chunks' status words
                                    // and a word per segment (seg_scan_flag_word); zeroed with bin_cnt: they sit
                                    // behind it in one block
    SegTask *tasks;         // [task_cap]
    uint32_t task_cap;
    void *sub_rec;          // [n_parts * M] entries in sub-bucket order: SegRec32 / SegRec64, one
                            // 16-byte store per entry and part
    const RangeTask *ranges;
    uint32_t n_ranges;
    const SegBlock *blocks; // LDS path of the counting sort (null: per-entry atomics, histogram by prep)
    uint32_t n_blocks;
    uint32_t lds_bins;      // most bins any part of any segment has
    uint32_t parts_per_pass; // parts whose counters fit the LDS side by side (1..4)
    // the pair kernel's blocks leave what their edge stage still holds at the end in a slot of their
    // own; seg_edge_append moves the slots to the edge list (no storm of atomics on the list's
    // counter when all blocks finish together)
    uint2 *priv_edges;      // [n_blocks * SEG_PRIV_CAP]
    uint8_t *priv_dist;     // ... their distances (DataStruct mode), else null
    uint32_t *priv_cnt;     // [n_blocks] entries in each slot, then (after the scan) their offsets
    // (candidates, symmetric pairs united) of each block, which the collapse's flatten launch adds to the
    // counters when it gathers the slots (null: every block adds its own with two atomics at its end --
    // ~90 per microsecond on one word, a queue when thousands of blocks end together)
    uint2 *priv_stat;       // [n_blocks]
    // directional batched path: parent array of the union-find (= label[]).  A pair permitted in both
    // directions is united where it is found instead of going through the edge list (null: listed)
    uint32_t *uf_parent;
    // LDS path: the count kernel's blocks also do the entry kernel's work for their entries (filter
    // key, threshold, label, contract check: prep_kernel then skips the segments' ranges) -- one
    // launch and one pass over the keys less.  prep_keys null: prep_kernel has done it.
    const uint64_t *prep_keys, *prep_nmask;
    const int32_t *prep_freq;
    int32_t *prep_thr;
    uint32_t *prep_label;
    uint32_t *prep_lab;     // lab[i] = i beside label[i] = i (may be null: the collapse's flatten pass writes lab[])
    float prep_percentage;
    unsigned long long *prep_counters;
    int umi_len;            // (keys of several words: 21, the bases of the first word the filter keys hold)
    int key_words;          // words per key in prep_keys / prep_nmask and in the pair kernel's exact check
    int full_umi_len;       // ... and the whole length of such keys (the N-code check of the entry pass)
    uint32_t use_ckey; // 32-bit keys: the pair kernel compares the records' compare keys (every part of
                       // every segment leaves at most 10 bases outside its bins)
    uint32_t col_sliced; // ... 64 columns at a time, bit-sliced (columns64_sliced), where k <= 3; 0: a broadcast per column
    // part-0 sub-buckets of 2..local_cap entries are seg_local_kernel's (united in LDS, launched ahead of
    // the pair kernel): the scan gives them no tile tasks.  0: every sub-bucket is the pair kernel's.
    uint32_t local_cap;
    // k = 1, no N in the call: where part 0 leaves at most probe_rest bases outside its bins, the local
    // kernel decides its sub-buckets of at least probe_min entries by bitmap lookups instead of the tile walk
    // (SEG_PROBE_MAX_REST, or 0: every sub-bucket is walked)
    uint32_t probe_rest, probe_min;
    // k = 1, no N in the call: in a segment with SegDesc::sup_g > 0 a super-bin of 2..super_cap entries is "taken" --
    // seg_super_kernel decides every pair inside it, its part-0 bins get no tile tasks and the pair kernel drops the
    // hits of the other part that lie inside it; every other super-bin's bins all go to the tiles, and the one-wave
    // local kernel leaves such a segment alone.  Whether a super-bin is taken is not stored: its entry count is
    // bin_start[first bin of the next run] - bin_start[its first bin], which the scan and both kernels read.
    // 0: no super-bins in this call (sup_g is ignored)
    uint32_t super_cap;
    const SegSuper *supers;
    uint32_t n_supers;
    // Coarse filing (LDS counting sort only): in a segment with super-bins the count and scatter kernels file a part-0
    // entry under the first bin of its run -- nobody reads the order of a run's entries by fine bin: seg_super_kernel
    // places a taken super-bin's records by rest-code, and a run above the cap is one sub-bucket for the tiles, whose
    // drain keeps a hit only if the two keys agree on all of mask[0].  The run's other bins count 0, so bin_start of
    // a run's first bin and of the next run's are what they were.  0: every entry under its own bin.
    uint32_t super_coarse;
    // ... and the pairs inside the fine bins of such a segment's part 0 (CNT_SEG_PAIRS), which the scan can no longer
    // see, are counted by seg_super_kernel (0 in the launch of a second attempt: they are counted once)
    uint32_t super_count_pairs;
    // Cross segments (SegDesc::cross): seg_super_kernel stores every super-bin's rest-code map, the set bits before each
    // of its words and (entry index, freq) by rank -- the last in the part-1 half of sub_rec, which the scatter leaves
    // free in such a segment: super-bin at position `start` of part 0, rank r -> the uint2 at
    // (uint2 *)(sub_rec + bin_start[bin_off[1]]) + (start - bin_start[bin_off[0]]) + r.  seg_cross_kernel reads them.
    uint32_t *cross_map;
    uint16_t *cross_pre;
#ifdef UMIHIP_DEV
    // development build: where seg_super_kernel's blocks add up the time they spend in each of their phases
    // ([blocks][SEG_SUPER_PHASES] ticks of the 100 MHz clock, zeroed by the host; null: no stamps)
    unsigned long long *super_stamps;
#endif
};
// seg_super_kernel's phases (development build's stamps): records in, map built, ranks and placement, bit tests,
// the hit rounds (decide and the unions), pointer jumping, atomicMin, label stores, the pairs inside the fine bins
// counted (coarse filing)
constexpr int SEG_SUPER_PHASES = 9;
// the scan's word of a segment with super-bins, behind the chunks' status words: left 0 where every super-bin of the
// segment is taken (none lies above the cap), so that a part-1 hit inside a super-bin is seg_super_kernel's for sure
UMIHIP_HD inline uint32_t seg_scan_flag_word(uint32_t n_chunks, uint32_t seg) { return 1u + n_chunks + seg; }
// exclusive scan of the bin counts -> bin_start, task list, counters[CNT_SEG_TASKS / _PAIRS];
// then every entry of a segment is copied to its position in each part's sub-bucket order
hipError_t launch_seg_build(const SegArgs &g, void *fkey, const int32_t *freq, bool key32,
                            unsigned long long *counters, hipStream_t s);
constexpr uint32_t SEG_PRIV_CAP = 512; // = the LDS edge stage of a block
// all pairs inside the sub-buckets: filter + exact check + edge emission (percentage: thresholds
// are recomputed from the staged freq).  part/n_parts: a multi-GPU split takes every n_parts-th task.
int seg_pair_blocks_per_cu(bool key32, bool has_n, bool ckey);
hipError_t launch_seg_pairs(const PairArgs &a, const SegArgs &g, bool key32, float percentage,
                            uint32_t part, uint32_t n_parts, uint32_t n_blocks, hipStream_t s);
hipError_t launch_seg_edge_append(const PairArgs &a, const SegArgs &g, uint32_t n_blocks, hipStream_t s);
// The part-0 sub-buckets of at most g.local_cap entries (batched directional path, 32-bit compare keys):
// every pair inside them evaluated by one wave out of LDS, the symmetric ones united in an LDS forest
// that is written to g.uf_parent as root = smallest entry index of the set (depth <= 1), the one-way
// ones left in the blocks' private slots (g.priv_edges / priv_cnt, n_blocks of them).  Must finish
// before any kernel unites through g.uf_parent: a launch of its own, ahead of the pair kernel.
constexpr uint32_t SEG_LOCAL_MAX_CAP = 2048;
constexpr uint32_t SEG_LOCAL_CAP = 512; // default cap (LDS: 16 bytes per entry + the hit queue)
// Lookups instead of pairs (k = 1, no N): inside a sub-bucket whose part leaves rest <= SEG_PROBE_MAX_REST
// bases outside its bins an entry is the 2 * rest bits of those bases, the sub-bucket a bitmap of 4^rest
// bits in LDS, and an entry's partners within one substitution are 3 * rest single-bit tests.
constexpr int SEG_PROBE_MAX_REST = 6;                                       // 4,096 bits: 512 bytes
constexpr uint32_t SEG_PROBE_WORDS = (1u << (2 * SEG_PROBE_MAX_REST)) / 32; // words of the bitmap
constexpr uint32_t SEG_PROBE_MIN = 129; // smallest sub-bucket decided by lookups (up to three tiles: the tile walk)
// Super-bins (see SegArgs::super_cap): LDS is 16 bytes per entry, a 4^8-bit map and its prefix -- one block per CU
constexpr int SEG_SUPER_MAX_REST = 8;
constexpr uint32_t SEG_SUPER_WORDS = (1u << (2 * SEG_SUPER_MAX_REST)) / 32; // 2,048
constexpr int SEG_SUPER_MAX_BASES = 4;                                      // g: a super-bin stays inside a scan chunk
constexpr uint32_t SEG_SUPER_MAX_CAP = 8192; // (eight records per thread of a 1,024-thread block in registers)
constexpr uint32_t SEG_SUPER_CAP = 5632;     // default: config 2's largest super-bin (~4,050) with headroom
constexpr uint32_t SEG_SUPER_MIN = 1024;     // smallest expected super-bin the planner gives the path to
constexpr uint32_t SEG_SUPER_SMALL = 2048;   // caps up to here: 256-thread blocks
inline uint32_t seg_super_threads(uint32_t cap) { return cap <= SEG_SUPER_SMALL ? 256u : 1024u; }
size_t seg_super_lds_bytes(uint32_t cap);
// private slots (one per wave) the kernel's grid needs: its blocks times its waves per block
uint32_t seg_super_blocks(uint32_t n_supers, uint32_t n_cus);
// Every taken super-bin: all pairs inside it by bitmap lookups out of LDS, symmetric ones united in an LDS forest
// written to g.uf_parent as seg_local_kernel does, one-way ones to the waves' private slots (g.priv_* point at the
// first of n_blocks * (threads / 64) slots).  A launch of its own ahead of the pair kernel, as launch_seg_local.
hipError_t launch_seg_super(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s);
// The pairs of the cross segments that differ in one base their super-bins share: two such entries have the same
// rest-code and lie in super-bins whose codes differ in that base, so they are the set bits of the AND of two maps.
// Persistent one-wave blocks, a private slot and a priv_stat entry each (g.priv_* point at the first of n_blocks
// slots); symmetric pairs united through g.uf_parent.  Behind launch_seg_super in stream order.  Does nothing in a
// call whose CNT_SEG_CROSS_ABANDONED is set.
constexpr uint32_t SEG_CROSS_CHUNKS = SEG_SUPER_WORDS / 64u; // 64-word chunks of the largest map: work items per super-bin
constexpr int SEG_CROSS_MAX_SHARED = 8;                      // bases a segment's super-bins can share (nb <= 8, g >= 1)
constexpr uint64_t SEG_CROSS_CALL_BYTES = 64ull << 20;       // maps of one call
constexpr uint32_t SEG_CROSS_MAP_MB = 8;                     // default "seg_cross_map_mb": maps of one segment (12, 13 bp)
hipError_t launch_seg_cross(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s);
size_t seg_local_lds_bytes(uint32_t cap);
int seg_local_blocks_per_cu(bool has_n, uint32_t cap);
hipError_t launch_seg_local(const PairArgs &a, const SegArgs &g, float percentage, uint32_t n_blocks, hipStream_t s);

// ---- multi-word keys (umihip_wide.hip): umi_len 22..85, n_words = 2..4 words per key, entry-major
// a.tasks: rows [row0, row0 + 64) x columns [col0, col1) of one bucket; exact distance from all words
hipError_t launch_wide_pairs(const PairArgs &a, uint32_t n_tasks, int n_words, hipStream_t s);

// ---- edit distance between one-word keys (umihip_edit.hip): umi_len 1..21, k <= umi_len
// the entry pass of such a call (every entry: threshold, label, contract check as launch_prep) with the two
// forms of a key its pair kernel reads: planes[i] = bit b of base j's code at bit 21 b + j, counts[i] = the
// key's A, C, G, T in bytes 0..3
hipError_t launch_edit_prep(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq, const uint64_t *bucket_off,
                            uint64_t n_buckets, uint32_t n, int umi_len, float percentage, uint64_t *planes,
                            uint32_t *counts, int32_t *thr, uint32_t *label, unsigned long long *counters, hipStream_t s);
// a.tasks: rows [row0, row0 + 64) x columns [col0, col1) of one bucket; a.fkey: the planes.  Count filter,
// LDS queue of its hits, exact Levenshtein distance of each; permitted pairs to the edge list
hipError_t launch_edit_pairs(const PairArgs &a, const uint32_t *counts, uint32_t n_tasks, int umi_len, hipStream_t s);

// ---- one-mismatch correction after Cell Ranger (umihip_cr.hip: umi_dedup_batch_cr): one-word keys, umi_len 1..21
// The call's own counters, eight words of device memory zeroed by the host
enum CrCounter : int {
    CR_BAD = 0,         // freq < 1, an N code a given nmask does not cover, a bucket outside the arrays
    CR_RISES = 1,       // entries whose freq is above their predecessor's ...
    CR_START_RISES = 2, // ... of which sit at the start of a bucket
    CR_HAS_N = 3,       // entries with an N
    CR_PAIRS = 4,       // unordered pairs of one bucket at exactly one mismatching base
    CR_KEPT = 5,
    CR_COUNT = 8,
};
constexpr uint32_t CR_SMALL_MAX_CAP = 1024; // option "cr_small_max" at most: a lane's place in its bucket is 10 bits
constexpr uint32_t CR_SMALL_MAX = 128;      // its default
constexpr uint32_t CR_GATHER_CHUNK = 4096;  // entries of one gather task
struct CrGatherTask {
    uint32_t src, dst, len; // entries [src, src + len) of the call become [dst, dst + len) of the compact arrays
};
// every entry: freq >= 1, rises, N codes (nmask may be null: code 100 is N)
hipError_t launch_cr_check(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq, uint32_t n, int umi_len,
                           unsigned long long *counters, uint32_t n_cus, hipStream_t s);
// every bucket: the rise at its start, and for a bucket of 1..small_max entries span[i] = (i - start) | size << 10 for
// its entries (the other entries' words are not written: the host zeroes span[] where there are any)
hipError_t launch_cr_spans(const uint64_t *d_bucket_off, uint64_t n_buckets, uint32_t n, uint32_t small_max,
                           const int32_t *freq, uint32_t *span, unsigned long long *counters, uint32_t n_cus, hipStream_t s);
// the small buckets, a lane per entry: target[i], kept[target[i]] = 1 (kept[] zeroed before), CR_PAIRS
hipError_t launch_cr_small(const uint64_t *keys, const int32_t *freq, const uint32_t *span, uint32_t n, int umi_len,
                           uint32_t *target, uint8_t *kept, unsigned long long *counters, uint32_t n_cus, hipStream_t s);
// the larger buckets' entries into compact arrays (gidx: where each came from)
hipError_t launch_cr_gather(const CrGatherTask *tasks, uint32_t n_tasks, const uint64_t *keys, const int32_t *freq,
                            uint64_t *ckeys, int32_t *cfreq, uint32_t *gidx, hipStream_t s);
hipError_t launch_cr_nmask(const uint64_t *ckeys, uint32_t nl, int umi_len, uint64_t *nmask, uint32_t n_cus, hipStream_t s);
// ... resolved from the (i, j) list of the pipeline's MODE_NEIGHBOURS at k = 1 over the compact arrays: best count,
// best string among the candidates at that count, the one index that has it; then kept[target] = 1.  gidx null: the
// compact arrays are the call's.  best_f [nl], best_k [nl]: workspace
hipError_t launch_cr_resolve(const uint2 *edges, uint32_t n_edges, const uint64_t *ckeys, const int32_t *cfreq, uint32_t nl,
                             int umi_len, const uint32_t *gidx, int32_t *best_f, unsigned long long *best_k, uint32_t *target,
                             uint8_t *kept, unsigned long long *counters, uint32_t n_cus, hipStream_t s);
// root[i] = i where kept[i], else target[i] (root may be null); CR_KEPT
hipError_t launch_cr_finish(const uint8_t *kept, const uint32_t *target, uint32_t n, uint32_t *root,
                            unsigned long long *counters, uint32_t n_cus, hipStream_t s);

// ---- whole-read keys (umihip_seq.hip): reads of up to 256 bases, 1..12 words per key, stride words apart
constexpr int SEQ_MAX_WORDS = 12;
constexpr uint32_t SEQ_TILE = 64;           // rows / columns of a pair task
constexpr uint32_t SEQ_ALL_PAIRS = 0xFFFFFFFFu; // SeqGroup::part of a bucket evaluated without the partition
// one part of one bucket: its records are [rec_off, rec_off + n), entry bstart + (r - rec_off)
struct SeqGroup {
    uint32_t rec_off, bstart, n;
    uint32_t len, nw;     // read length (bases) and words of the bucket's keys
    uint32_t part, n_parts; // part j of k + 1 (bases [j len / P, (j + 1) len / P)), or SEQ_ALL_PAIRS
    uint32_t pad;
};
struct SeqPairArgs {
    const SeqGroup *groups;
    const uint64_t *rkey;   // sorted records: group << 32 | hash of the part
    const uint32_t *rval;   // ... their entries
    uint32_t n_rec;
    const uint64_t *run_id; // inclusive scan of the run starts (run_id[n_rec - 1] = runs)
    const uint32_t *run_start; // [runs + 1]
    const uint64_t *task_end;  // inclusive scan of the tiles per run
    const uint64_t *keys, *nmask; // nmask may be null
    int stride;
    const int32_t *freq, *thr;
    uint2 *edges;
    unsigned long long *counters;
    uint32_t edge_cap;
    int k, mode;
    int32_t adj_max_freq;
};
hipError_t launch_seq_records(const SeqGroup *groups, uint32_t n_groups, uint32_t n_rec, const uint64_t *keys,
                              const uint64_t *nmask, int stride, const int32_t *freq, float percentage, int32_t *thr,
                              uint64_t *rkey, uint32_t *rval, unsigned long long *counters, hipStream_t s);
// runs of equal sorted records -> run_start, task_end; flag is scratch of n_rec words;
// counters[CNT_SEG_PAIRS] += the pairs inside the runs
hipError_t launch_seq_runs(const uint64_t *rkey, uint32_t n_rec, uint64_t *flag, uint64_t *run_id,
                           uint32_t *run_start, uint64_t *task_end, void *scan_temp, size_t scan_temp_size,
                           unsigned long long *counters, hipStream_t s);
hipError_t launch_seq_pairs(const SeqPairArgs &a, uint32_t n_blocks, hipStream_t s);

// ---- read staging on the device (umihip_stage.hip) ----
size_t stage_workspace_bytes(uint32_t n_reads, int n_words, bool grouped = false);
// reads (alignment key, UMI text, score) -> entries in canonical order + bucket table, all device
// memory (keys / nmask: n_words words per entry); h_pinned4: four pinned 64-bit words for the counts
// the host needs on the way.  d_group / group_bits (null / 0: none): a second per-read key, positions
// are (alignment, group); the workspace must then be the grouped size.  0 ok; 1 a character outside
// ATCGN; negative: -(hipError_t)
int stage_reads_on_device(void *workspace, const uint64_t *d_align, int align_bits, const uint64_t *d_group,
                          int group_bits, const uint8_t *d_umi,
                          const int32_t *d_score, uint32_t n, int umi_len, int n_words, int merge, uint64_t *d_keys,
                          uint64_t *d_nmask, int32_t *d_freq, uint64_t *d_rep, uint64_t *d_bucket_off,
                          uint64_t *n_entries_out, uint64_t *n_buckets_out, unsigned long long *h_pinned4,
                          hipStream_t s);

// whole reads (umi_stage_seqs): read i is len[i] bases at text + seq_pos[i], its quality at text +
// qual_pos[i] (may be null with merge 0); keys / nmask (may be null): n_words words per entry.  The
// bucket table (bucket_off [n_buckets + 1], bucket_len [n_buckets]) comes back to the host; eor (may be
// null): every read's entry.  0 ok; 1 a character outside ATCGN (fault: read, byte); 2 a read longer
// than UMI_MAX_SEQ_LEN, 3 longer than n_words hold (fault: value = the longest); negative: -(hipError_t)
struct SeqFault {
    uint64_t read = 0, value = 0;
};
size_t stage_seqs_workspace_bytes(uint32_t n_reads, int n_words);
int stage_seqs_on_device(void *workspace, const uint8_t *d_text, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                         const uint32_t *d_len, uint32_t n, int n_words, int merge, uint64_t *d_keys, uint64_t *d_nmask,
                         int32_t *d_freq, uint64_t *d_rep, uint32_t *d_eor, uint64_t *h_bucket_off, int32_t *h_bucket_len,
                         uint64_t *n_entries_out, uint64_t *n_buckets_out, int *any_n, SeqFault *fault,
                         unsigned long long *h_pinned4, hipStream_t s);

// ---- consensus of the clusters of whole reads (umihip_consensus.hip: umi_consensus_seqs) ----
// The inputs are what stage_seqs_on_device and the whole-read collapse leave on the device (n_entries >= 1,
// the bucket table on the host); cons_seq / cons_qual take the kept entries' consensus back to back in
// entry order, cons_off [n_entries] where each starts, cluster_reads (may be null) its members.  split:
// clusters of at least this many reads are summed in pieces by the whole grid.  h_pinned: 16 pinned
// words.  0 ok; 1 the inputs break the contract (fault says how, nothing was written); negative:
// -(hipError_t)
struct ConsFault {
    unsigned long long bad_root = 0, bad_read = 0, bad_len = 0, empty = 0, freq_sum = 0;
};
uint32_t consensus_effective_split(uint32_t n_reads, uint32_t split);
size_t consensus_workspace_bytes(uint32_t n_reads, uint32_t n_entries, uint32_t n_buckets, uint32_t split);
int consensus_on_device(void *workspace, const uint8_t *d_text, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                        const uint32_t *d_len, uint32_t n_reads, const uint32_t *d_eor, const int32_t *d_freq,
                        const uint8_t *d_kept, const uint32_t *d_root, uint32_t n_entries, const uint64_t *h_bucket_off,
                        const int32_t *h_bucket_len, uint32_t n_buckets, uint32_t split, uint32_t n_cus, uint8_t *d_cons_seq,
                        uint8_t *d_cons_qual, uint64_t *d_cons_off, uint32_t *d_cluster_reads, uint64_t *cons_bytes,
                        ConsFault *fault, unsigned long long *h_pinned, hipStream_t s);

// ---- consensus of the clusters of aligned reads (umihip_consensus_bam.hip: umi_consensus_bam) ----
// Everything in device memory; the clusters are given (cluster [n_reads], cluster_len [n_clusters]).
// cons_seq / cons_qual take the clusters' consensus back to back, seq_off / qual_off where each starts,
// depth its voters, disagree (may be null) its base votes that lost.  split: as for consensus_on_device
// (never above 2^24 here: one wave sums in 32 bits).  h_pinned: 16 pinned words.  0 ok; 1 the inputs
// break the contract (fault says how, nothing was written); negative: -(hipError_t)
struct ConsBamFault {
    unsigned long long bad_cluster_len = 0, bad_id = 0, bad_len = 0;
};
size_t consensus_bam_workspace_bytes(uint32_t n_reads, uint32_t n_clusters, uint32_t split);
int consensus_bam_on_device(void *workspace, const uint8_t *d_data, const uint64_t *d_seq_pos, const uint64_t *d_qual_pos,
                            const uint32_t *d_len, const uint32_t *d_cluster, uint32_t n_reads, const uint32_t *d_cluster_len,
                            uint32_t n_clusters, uint32_t split, uint32_t n_cus, uint8_t *d_cons_seq, uint8_t *d_cons_qual,
                            uint64_t *d_seq_off, uint64_t *d_qual_off, uint32_t *d_depth, uint32_t *d_disagree,
                            uint64_t *seq_bytes, uint64_t *qual_bytes, ConsBamFault *fault, unsigned long long *h_pinned,
                            hipStream_t s);

// ---- correction of UMIs to a fixed list (umihip_correct.hip: umi_correct_umis) ----
// The list is packed on the host, 2 bits per base (A 0, C 1, G 2, T 3), correct_words(umi_len) 32-bit
// words per entry (correct_pack_list: 1 and *bad_entry at a byte outside ACGT), and walked on the
// device in tiles of CORR_TILE entries.  d_out, d_best, d_second may be null; d_out may be d_umi.
// h_pinned: 4 pinned words.  0 ok; 1 a read byte outside ATCGN (*bad_read: the smallest such read;
// nothing was written); negative: -(hipError_t)
constexpr uint32_t CORR_TILE = 1024;          // entries of the list in LDS at a time
constexpr uint32_t CORR_MAX_LIST = 1u << 24;  // entries of a list, at most (an index is 24 bits of a compare key)
int correct_words(int umi_len);
int correct_pack_list(const uint8_t *ascii, uint32_t n_wl, int umi_len, uint32_t *packed, uint64_t *bad_entry);
size_t correct_workspace_bytes(uint32_t n_wl, int umi_len);
int correct_on_device(void *workspace, const uint8_t *d_umi, uint32_t n_reads, int umi_len, const uint32_t *h_packed,
                      uint32_t n_wl, int max_mismatches, int min_distance, uint8_t *d_out, int32_t *d_match, uint8_t *d_best,
                      uint8_t *d_second, uint64_t counts[3], uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned,
                      hipStream_t s);

// ---- correction of cell barcodes to a kit's list (umihip_barcode.hip: umi_correct_barcodes) ----
// The list is packed on the host, 2 bits per base in one 64-bit word per entry (barcode_pack_list: 1 and
// *bad_entry at a byte outside ACGT), indexed on the device (a table of barcode_table_slots(n_wl) slots)
// and looked up by every read and its single substitutions.  d_status may be null.  h_pinned: 8 pinned
// words.  0 ok; 1 a read byte outside ACGTN (*bad: the smallest such read); 2 a listed barcode that occurs
// twice (*bad: the smallest entry that equals an earlier one) -- nothing was written in either case;
// negative: -(hipError_t)
constexpr int BARCODE_MAX_LEN = 32;
int barcode_pack_list(const uint8_t *ascii, uint32_t n_wl, int bc_len, uint64_t *packed, uint64_t *bad_entry);
uint32_t barcode_table_slots(uint32_t n_wl);
size_t barcode_workspace_bytes(uint32_t n_wl);
int barcode_on_device(void *workspace, const uint8_t *d_bc, uint32_t n_reads, int bc_len, const uint64_t *h_packed, uint32_t n_wl,
                      int max_mismatches, int32_t *d_match, uint8_t *d_status, uint64_t counts[4], uint64_t *bad, uint32_t n_cus,
                      unsigned long long *h_pinned, hipStream_t s);
// umi_correct_barcodes_multi: the same with the qualities beside the barcodes (d_qual given: max_mismatches is 1),
// the exact reads per listed barcode (d_exact_reads may be null) and the ambiguous reads weighed in a second
// pass; the workspace holds barcode_multi_workspace_bytes, counts has 5 words and h_pinned 10.  Also 3: a
// quality byte outside 33..126 (*bad: the smallest such read, and no read up to it has a bad barcode byte).
// Without d_qual it is barcode_on_device.
size_t barcode_multi_workspace_bytes(uint32_t n_wl, uint32_t n_reads);
int barcode_multi_on_device(void *workspace, const uint8_t *d_bc, const uint8_t *d_qual, uint32_t n_reads, int bc_len,
                            const uint64_t *h_packed, uint32_t n_wl, int max_mismatches, uint32_t permille, uint32_t pseudocount,
                            int32_t *d_match, uint8_t *d_status, uint32_t *d_exact_reads, uint64_t *counts, uint64_t *bad,
                            uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s);

// ---- reads assigned to genes from an annotation (umihip_genes.hip: umi_assign_genes) ----
// The tables (umihip_gene_index.hpp: one for unstranded, else the exons a read on + and a read on - may hit under
// "forward"; flip: "reverse", the two change places) are built and sampled on the host and uploaded into the
// workspace.  One synchronisation, at the end.  h_pinned: 5 pinned words.  0 ok; 1 a read with read_ref < 0 or
// a CIGAR op code above 8; 2 a cigar_off that falls (*bad: the smallest such read; the outputs are then
// worthless); negative: -(hipError_t)
struct GeneTable;
constexpr int GENE_THREADS = 1024;        // lanes of a block, a read each
constexpr int GENE_BLOCKS_PER_CU = 2;     // resident blocks per CU: the grid's cap, a stride beyond
constexpr uint32_t GENE_TOP_CAP = 4096;   // sampled ends of a table in LDS, at most (option "gene_top")
size_t genes_workspace_bytes(const GeneTable *tables, int n_tables);
int genes_on_device(void *workspace, const GeneTable *tables, int n_tables, bool flip, bool use_top, const int32_t *d_ref,
                    const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                    uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint64_t counts[3], uint64_t *bad, uint32_t n_cus,
                    unsigned long long *h_pinned, hipStream_t s);

// ---- ... with their introns (umihip_gene_introns.hip: umi_assign_genes_introns) ----
// Two tiers of such tables, the exons' and the gene bodies' (n_tables of each, sampled at GENE_TOP_CAP and at
// GENE_BODY_TOP_CAP), uploaded alike; mode: UMI_INTRONS_*.  use_body_top counts only with use_top.  h_pinned: 6
// pinned words.  Returns as genes_on_device; counts: assigned by an exon, by an intron, none, several.
constexpr uint32_t GENE_BODY_TOP_CAP = 512; // sampled ends of a body table in LDS, at most (option "gene_body_top")
size_t gene_introns_workspace_bytes(const GeneTable *exons, const GeneTable *bodies, int n_tables);
int gene_introns_on_device(void *workspace, const GeneTable *exons, const GeneTable *bodies, int n_tables, bool flip, int mode,
                           bool use_top, bool use_body_top, const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse,
                           const uint32_t *d_cigar, const uint64_t *d_cigar_off, uint32_t n_reads, int32_t *d_gene, uint8_t *d_status,
                           uint8_t *d_tier, uint64_t counts[4], uint64_t *bad, uint32_t n_cus, unsigned long long *h_pinned,
                           hipStream_t s);

// ---- ... and the class of every assigned read (umihip_gene_classes.hip: umi_assign_genes_classes) ----
// gene_introns_on_device's arguments; beside every exon table its GeneCover (umihip_gene_index.hpp: the prefix array
// of covered bases and the genes' own exons), uploaded alike.  h_pinned: 9 pinned words.  class_counts: by UMI_READ_CLASS_*.
struct GeneCover;
size_t gene_classes_workspace_bytes(const GeneTable *exons, const GeneTable *bodies, const GeneCover *cover, int n_tables);
int gene_classes_on_device(void *workspace, const GeneTable *exons, const GeneTable *bodies, const GeneCover *cover,
                           int n_tables, bool flip, int mode, bool use_top, bool use_body_top, const int32_t *d_ref,
                           const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                           uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier, uint8_t *d_cls, uint64_t counts[4],
                           uint64_t class_counts[5], uint64_t *bad, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s);

// ---- reads assigned to genes by transcript model (umihip_gene_transcripts.hip: umi_assign_genes_transcripts) ----
// The tables (umihip_transcript_index.hpp: one per strand class, as genes_on_device's, sampled at GENE_TOP_CAP) are built
// on the host and uploaded into the workspace.  One synchronisation, at the end.  h_pinned: 5 pinned words.  Returns
// as genes_on_device.
struct TranscriptTable;
size_t gene_transcripts_workspace_bytes(const TranscriptTable *tables, int n_tables);
int gene_transcripts_on_device(void *workspace, const TranscriptTable *tables, int n_tables, bool flip, bool use_top, const int32_t *d_ref,
                               const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar, const uint64_t *d_cigar_off,
                               uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint64_t counts[3], uint64_t *bad, uint32_t n_cus,
                               unsigned long long *h_pinned, hipStream_t s);

// ---- ... with the gene bodies behind the transcripts, and classes (umihip_gene_transcript_classes.hip:
// ---- umi_assign_genes_transcripts_classes) ----
// Per strand class a transcript table (sampled at GENE_TOP_CAP), a body table (at GENE_BODY_TOP_CAP) and, where classes
// are asked for (cover != null), the exons' overlap table (not sampled: searched from global memory) with its GeneCover.
// cover null: exons, d_cls and class_counts are not looked at.  mode: UMI_INTRONS_*.  Two kernels, the second over a queue
// of n_reads words in the workspace; one synchronisation, at the end.  h_pinned: 9 pinned words.  Returns
// as genes_on_device; counts: assigned by a transcript, by a body, none, several; class_counts: by UMI_READ_CLASS_*.
size_t gene_transcript_classes_workspace_bytes(const TranscriptTable *transcripts, const GeneTable *bodies, const GeneTable *exons,
                                               const GeneCover *cover, int n_tables, uint32_t n_reads);
int gene_transcript_classes_on_device(void *workspace, const TranscriptTable *transcripts, const GeneTable *bodies, const GeneTable *exons,
                                      const GeneCover *cover, int n_tables, bool flip, int mode, bool use_top, bool use_body_top,
                                      const int32_t *d_ref, const int32_t *d_pos, const uint8_t *d_reverse, const uint32_t *d_cigar,
                                      const uint64_t *d_cigar_off, uint32_t n_reads, int32_t *d_gene, uint8_t *d_status, uint8_t *d_tier,
                                      uint8_t *d_cls, uint64_t counts[4], uint64_t *class_counts, uint64_t *bad, uint32_t n_cus,
                                      unsigned long long *h_pinned, hipStream_t s);

// ---- molecules and reads per (column, row) pair (umihip_count.hip: umi_count_matrix) ----
// h_off (pinned): the m + 1 offsets of the m >= 1 non-empty buckets; h_idx (pinned, null: nothing was left out):
// their numbers in d_row / d_col.  The outputs take the triplets sorted by column, then row (capacity m);
// *bad_ids: non-empty buckets with a row or column out of range (the outputs are then worthless).  One
// synchronisation, at the end.  h_pinned: 2 pinned words.  0 ok; negative: -(hipError_t)
size_t count_workspace_bytes(uint32_t m, bool has_idx);
int count_matrix_on_device(void *workspace, const uint8_t *d_kept, const int32_t *d_freq, const uint64_t *h_off,
                           const uint32_t *h_idx, uint32_t m, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows,
                           uint32_t n_cols, uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_molecules,
                           uint64_t *d_out_reads, uint64_t *nnz, uint64_t *bad_ids, uint32_t n_cus, unsigned long long *h_pinned,
                           hipStream_t s);

// ---- spliced, unspliced and ambiguous molecules per pair (umihip_velocity.hip: umi_velocity_matrix) ----
// count_matrix_on_device's bucket arguments; n entries (the last offset).  *bad_ids as there; *bad_kind: 0 none, 1 a
// read_entry out of range, 2 a read_class above 4, 3 a root out of range, of read *bad_read (the smallest read with
// any of them).  skip_set: a lane loads the evidence word and leaves the atomic out where its bit is set.  One
// synchronisation, at the end.  h_pinned: 5 pinned words.  0 ok; negative: -(hipError_t)
size_t velocity_workspace_bytes(uint64_t n, uint32_t m, bool has_idx);
int velocity_matrix_on_device(void *workspace, const uint32_t *d_read_entry, const uint8_t *d_read_class, uint32_t n_reads,
                              const uint8_t *d_kept, const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx,
                              uint32_t m, const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols,
                              uint32_t *d_out_row, uint32_t *d_out_col, uint32_t *d_out_spliced, uint32_t *d_out_unspliced,
                              uint32_t *d_out_ambiguous, bool skip_set, uint64_t *nnz, uint64_t *bad_ids, int *bad_kind,
                              uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s);

// ---- saturation and medians per depth (umihip_saturation.hip: umi_saturation_curve) ----
// velocity_matrix_on_device's read and bucket arguments without the classes; 1 <= n_levels <= 32, 2 n_levels n_cols < 2^30;
// d_cell_mask may be null.  *bad_ids as there; *bad_kind: 0 none, 1 a read_entry out of range, 2 a root out of range, of
// read *bad_read.  skip_set: a lane loads its molecule's word and leaves the atomic out where its bit is set.  One
// synchronisation, at the end.  h_pinned: 4 + 8 n_levels pinned words; the curve lies from word 4 on.  0 ok;
// negative: -(hipError_t)
size_t saturation_workspace_bytes(uint64_t n, uint32_t m, bool has_idx, uint32_t n_cols, int n_levels);
int saturation_curve_on_device(void *workspace, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                               const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx, uint32_t m,
                               const uint32_t *d_row, const uint32_t *d_col, uint32_t n_rows, uint32_t n_cols, uint64_t seed,
                               int n_levels, const uint8_t *d_cell_mask, bool skip_set, uint64_t *bad_ids, int *bad_kind,
                               uint64_t *bad_read, uint32_t n_cus, unsigned long long *h_pinned, hipStream_t s);

// ---- molecules and reads per (column, splice junction) pair (umihip_junctions.hip: umi_junction_matrix) ----
// Two halves, each with one synchronisation at its end: the sorts of the second take the occurrences T as a host
// argument.  junction_count_on_device: count_matrix_on_device's bucket arguments without the rows, the reads'
// ref, pos, CIGAR words and entries; *got: what the host decides on.  bad_kind: 0 none, 1 a falling cigar_off, 2 a
// read_entry out of range, 3 a root out of range, 4 a read_ref < 0, 5 an op code above 8, of read bad_read (the
// smallest read with any of them).  h_pinned: 10 pinned words.  junction_fill_on_device: runs only where got has no
// error and 1 <= got.occurrences < 2^30; workspace1 is the first half's, untouched since; workspace2 holds
// junction_fill_workspace_bytes(T); the outputs have room for T.  0 ok; -(hipError_t).
struct JunctionCounted {
    uint64_t bad_cols, bad_read, spliced, occurrences, max_ref, max_pos;
    int bad_kind;
};
size_t junction_count_workspace_bytes(uint32_t n_reads, uint32_t m, bool has_idx);
size_t junction_fill_workspace_bytes(uint32_t t);
int junction_count_on_device(void *workspace, const int32_t *d_ref, const int32_t *d_pos, const uint32_t *d_cigar,
                             const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                             const uint32_t *d_root, uint64_t n, const uint64_t *h_off, const uint32_t *h_idx, uint32_t m,
                             const uint32_t *d_col, uint32_t n_cols, JunctionCounted *got, uint32_t n_cus, unsigned long long *h_pinned,
                             hipStream_t s);
int junction_fill_on_device(void *workspace1, void *workspace2, const int32_t *d_ref, const int32_t *d_pos, const uint32_t *d_cigar,
                            const uint64_t *d_cigar_off, const uint32_t *d_read_entry, uint32_t n_reads, const uint8_t *d_kept,
                            const uint32_t *d_root, uint64_t n, uint32_t m, bool has_idx, uint32_t n_cols, const JunctionCounted &got,
                            int32_t *d_jn_ref, int32_t *d_jn_start, int32_t *d_jn_end, uint32_t *d_out_jn, uint32_t *d_out_col,
                            uint32_t *d_out_molecules, uint64_t *d_out_reads, uint64_t *junctions, uint64_t *nnz, uint32_t n_cus,
                            unsigned long long *h_pinned, hipStream_t s);

// ---- family sizes, UMI distances and UMI usage of a batched call (umihip_stats.hip: umi_dedup_stats) ----
constexpr uint32_t STATS_LANE_MAX = 8;    // a bucket of more entries is a wave's
constexpr uint32_t STATS_HIST_LDS = 2048; // family-size bins a block counts in LDS; the others by global atomics
constexpr uint32_t STATS_PIECE = 1024;    // entries of a deep bucket a wave takes at a time
constexpr uint32_t STATS_SPLIT = 4096;    // option "stats_split": buckets of at least this many entries go to the whole grid
struct StatsTask {                        // a piece [lo, hi) of deep bucket `deep`
    uint64_t lo, hi;
    uint32_t deep, pad;
};
// the split that is used (raised by itself where the deep buckets' tables would pass 512 MB), the buckets at or
// above it and their pieces; h_off: the m + 1 offsets of the m >= 1 non-empty buckets
void stats_plan(const uint64_t *h_off, uint32_t m, uint32_t split, int umi_len, uint32_t *split_used, uint32_t *n_deep,
                uint32_t *n_tasks);
size_t stats_workspace_bytes(uint32_t n, uint32_t m, uint32_t n_deep, uint32_t n_tasks, int umi_len, bool per_umi);
struct StatsCall {
    const uint64_t *d_keys;
    const int32_t *d_freq;
    const uint8_t *d_kept;
    const uint32_t *d_root;
    const uint64_t *h_off; // pinned
    uint32_t n, m, split, n_deep, n_tasks, hist_bins, n_cus;
    int umi_len, n_words;
    uint64_t seed;
    uint64_t *d_count_pre, *d_count_post, *d_dist;
    uint32_t *d_umi_entry, *d_times_pre, *d_times_post; // the per-UMI table: all five or none
    uint64_t *d_reads_pre, *d_reads_post;
    uint32_t *h_deep_j;          // pinned, [n_deep]
    StatsTask *h_tasks;          // pinned, [n_tasks]
    unsigned long long *h_pinned; // 3 pinned words: keys with a bad code, entries with a bad root, rows of the table
};
// One synchronisation, at the end.  0 ok; negative: -(hipError_t)
int stats_on_device(void *workspace, const StatsCall &c, hipStream_t s);

// ---- UMIs a group shows in several buckets (umihip_multigene.hip: umi_filter_multigene) ----
size_t multigene_workspace_bytes(uint32_t n, uint32_t m, bool has_idx);
struct MultigeneCall {
    const uint64_t *d_keys;
    const int32_t *d_freq;
    const uint8_t *d_kept;
    const uint32_t *d_root;
    const uint32_t *d_group; // per bucket of the caller's table
    const uint64_t *h_off;   // pinned: the m + 1 offsets of the m >= 1 non-empty buckets
    const uint32_t *h_idx;   // pinned: their numbers in d_group (null: nothing was left out)
    uint32_t n, m, n_groups, n_cus; // n = h_off[m] entries, 1 <= n < 2^30; n_groups >= 1
    int umi_len, n_words;
    uint8_t *d_kept_out;
    int32_t *d_freq_out; // may be null
    // 5 pinned words: non-empty buckets with a group out of range, entries with a bad root (either: the outputs are
    // worthless), runs of two or more molecules, molecules removed, their reads
    unsigned long long *h_pinned;
};
// One synchronisation, at the end.  0 ok; negative: -(hipError_t)
int multigene_on_device(void *workspace, const MultigeneCall &c, hipStream_t s);

// ---- cell calling over the triplets of a count matrix (umihip_cells.hip: umi_call_cells) ----
constexpr int CELLS_CTL_WORDS = 12; // the control block's words, in h_pinned's order
enum CellsRule : int { CELLS_CR22 = 0, CELLS_TOP = 1, CELLS_MIN = 2 }; // the values of UMI_CELLS_* (umihip.h)
size_t cells_workspace_bytes(uint32_t nnz, uint32_t n_cols);
struct CellsCall {
    const uint32_t *d_row, *d_col, *d_molecules; // the nnz triplets, sorted by column, then row
    const uint64_t *d_reads;
    uint32_t nnz, n_rows, n_cols, n_cus; // 1 <= nnz < 2^30, 1 <= n_cols < 2^30, n_rows >= 1
    int rule;                            // CELLS_* (= UMI_CELLS_*), known
    // what the rule's index is the smaller of, beside n - 1: floor(N (1000 - P) / 1000) or N - 1; its ratio (>= 1
    // where it is read); min_molecules, negative ones as 0
    unsigned long long pick, ratio, min_molecules;
    uint64_t *d_cell_molecules, *d_cell_reads; // per column
    uint32_t *d_cell_genes, *d_new_col;
    uint8_t *d_called;
    uint32_t *d_out_row, *d_out_col, *d_out_molecules; // the filtered triplets (capacity nnz)
    uint64_t *d_out_reads;
    // CELLS_CTL_WORDS + 1 pinned words: triplets with an id out of range, triplets not above their predecessor
    // (either: the outputs are worthless), candidates, all molecules, all reads, t, m, molecules and reads in called
    // columns, called columns, their median molecules and genes; then the filtered triplets
    unsigned long long *h_pinned;
};
// One synchronisation, at the end.  0 ok; negative: -(hipError_t)
int call_cells_on_device(void *workspace, const CellsCall &c, hipStream_t s);

// ---- sort and scan primitives of the staging (umihip_radix.hip) ----
constexpr int RADIX_BINS = 256, RADIX_MAX_PASSES = 8; // 8-bit digits; a 64-bit key has at most eight
constexpr int RADIX_HIST_PARTS = 2048;                // blocks of a kernel that counts digits, at most
size_t radix_sort_temp_bytes(uint32_t n);
// stable sort of (key, value) pairs by bits [begin_bit, end_bit) of the key (n < 2^30); the buffers
// are used in turn, *result_in_b says where the result lies.  temp holds radix_sort_temp_bytes(n)
// bytes or more, whatever the bit range: less is hipErrorInvalidValue.  hist_parts > 0: the digit counts were
// taken by the kernel that wrote the keys -- block b of its hist_parts blocks put its counts of pass
// p (bits [begin_bit + 8p, +8)) and digit d at parts[(b * passes + p) * 256 + d], zeros included,
// parts being what radix_sort_prepare returned; that call zeroes the sort's temporaries and
// therefore comes before that kernel
hipError_t radix_sort_prepare(void *temp, size_t temp_bytes, uint32_t n, int begin_bit, int end_bit, uint32_t **hist_parts,
                              hipStream_t s);
hipError_t radix_sort_pairs_u64(uint64_t *keys_a, uint64_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, uint32_t n,
                                int begin_bit, int end_bit, void *temp, size_t temp_bytes, bool *result_in_b, hipStream_t s,
                                uint32_t hist_parts = 0);
hipError_t radix_sort_pairs_u32(uint32_t *keys_a, uint32_t *keys_b, uint32_t *vals_a, uint32_t *vals_b, uint32_t n,
                                int begin_bit, int end_bit, void *temp, size_t temp_bytes, bool *result_in_b, hipStream_t s,
                                uint32_t hist_parts = 0);
size_t scan_temp_bytes(uint32_t n);
hipError_t scan_inclusive_u64(const uint64_t *in, uint64_t *out, uint32_t n, void *temp, size_t temp_bytes, hipStream_t s);
// exclusive scan of a short array in place, by one block (the tile sums of a two-level scan)
hipError_t scan_spine_u64(unsigned long long *sums, uint32_t n, hipStream_t s);

// ---- directional collapse by union-find (umihip_collapse.hip) ----
// comp[] (= label[], identity on entry) becomes the smallest index of each entry's set under the
// symmetric pairs; lab[] is initialised to the identity
hipError_t launch_uf_components(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                                uint32_t *comp, uint32_t *lab, uint32_t n, uint32_t n_edges_hint,
                                hipStream_t s);
// The batched directional path: the sets of the listed symmetric pairs are joined (the segment
// index's pair kernel has united its own), the forest is flattened (launch_uf_flatten), then
// rounds along the listed one-way pairs without pointer jumps.
hipError_t launch_uf_union_list(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                                uint32_t *parent, uint32_t n_edges_hint, hipStream_t s);
// The collapse behind the pair kernels of the batched directional path: what it works on ...
struct CollapseDesc {
    uint32_t *parent, *lab;  // label[] (the union-find forest of the symmetric pairs) and lab[]
    const uint2 *edges;      // the list
    uint32_t edge_cap;
    const RangeTask *ranges; // entries the fused small-bucket kernel left (null: all n)
    uint32_t n_ranges, n;
    uint8_t *kept;
    uint32_t *root;
    bool kept_only = false;  // root is null and only kept[] is wanted: no flatten; round 0 (the flatten launch) resolves
                             // the one-way pairs' endpoints to roots, finalize reads parent[i] and lab[i] only.  lab[] must
                             // be the identity over the entries when the collapse starts (launch_prep, SegArgs::prep_lab)
    unsigned long long *counters;
    uint32_t *changed;       // the rounds' flags in the control block
    // what the segment index's pair kernel left in its blocks' private slots (one-way pairs only: the
    // symmetric ones were united where they were found); the flatten launch appends them to the list (kept_only: as
    // (root, root), hooked on the way)
    const uint2 *priv_edges = nullptr; // [priv_blocks * SEG_PRIV_CAP]
    const uint32_t *priv_cnt = nullptr;
    const uint2 *priv_stat = nullptr; // (candidates, united pairs) of each such block (null: counted already)
    uint32_t priv_blocks = 0;
};
// bytes (a multiple of 8) of the control block to its pinned, device-visible host mirror
// h_seq (pinned, may be null): set to seq once the block has arrived
hipError_t launch_control_to_host(const void *d_ctrl, void *h_ctrl, size_t bytes, hipStream_t s,
                                  unsigned long long *h_seq = nullptr, unsigned long long seq = 0);
// ... phase by phase: comp[v] = root of v in place and lab[v] = v; round `round` along the one-way pairs (a no-op
// once round - 1 was quiet); label = lab[comp[v]], kept, root, survivors.
// kept_only: the flatten launch is round 0 -- every one-way pair, in a private slot or in the list, resolved to
// (root, root) at its place in the list and hooked, changed[0] set if a label moved -- and the rounds behind it
// start at 1.
hipError_t launch_collapse_flatten(const CollapseDesc &d, hipStream_t s);
hipError_t launch_collapse_round(const CollapseDesc &d, int round, hipStream_t s);
// check_round >= 0: blocks of their own look, without a store, whether round check_round would still
// move a label (changed[check_round])
hipError_t launch_collapse_finalize(const CollapseDesc &d, hipStream_t s, int check_round = -1);
// bits[i / 8] bit (i % 8) = kept[i] != 0, for i < n (ceil(n / 8) bytes written)
// Connected components (MODE_CLUSTER): kept / root / CNT_KEPT straight from the union-find forest in d.parent
// -- with d.root the entries are flattened on the way, with d.kept_only and no root kept[i] = parent[i] == i and the
// forest stays as it is; d.lab, d.edges and d.changed are not looked at.  d.priv_stat (may be null): the counts of
// d.priv_blocks blocks of the segment index's kernels, added to the counters here.
hipError_t launch_cluster_write(const CollapseDesc &d, hipStream_t s);
hipError_t launch_pack_mask(const uint8_t *kept, uint64_t n, uint8_t *bits, hipStream_t s);

hipError_t launch_pairs(const PairArgs &a, uint32_t n_tasks, bool big, bool key32, hipStream_t s);

// bit-sliced path (buckets larger than small_max, k <= BS_MAX_K)
constexpr int BS_MAX_K = 3;
constexpr int BS_COL_TILE = 128;   // columns whose masks are staged in LDS per step
constexpr int BS_COL_CHUNK = 1024; // default columns per task (ctx option bs_col_chunk)
constexpr int BS_WIDE_MIN = 32768; // buckets at least this large use 256-thread blocks
// planes per key for a umi length: 2 bits per base, base count rounded up to 8/12/16/22
inline int bs_padded_len(int umi_len) { return umi_len <= 8 ? 8 : umi_len <= 12 ? 12 : umi_len <= 16 ? 16 : 22; }
inline int bs_groups_per_lane(int umi_len) { return umi_len <= 16 ? 2 : 1; }
hipError_t launch_build_planes(const void *fkey2, bool key32, const PlaneTask *tasks,
                               uint32_t n_tasks, uint32_t *planes, int umi_len, hipStream_t s);
// wide: the 4 waves of a block hold different row groups (256*G groups per tile); else they
// hold the same 64*G groups and split the columns
// unit: bases per counted unit of the filter (1 = exact base count, 2 = default)
hipError_t launch_bs_pairs(const PairArgs &a, uint32_t n_tasks, bool wide, bool key32,
                           int umi_len, int unit, int prefix_units, hipStream_t s);
// table variant (key-sorted buckets, 32-bit keys): row tiles of 64 * BS_TAB_G groups, the
// scan's list of (row tile, column tile) items to walk
struct TabRowTile {
    uint32_t bucket_start, bucket_end; // global entry indices
    uint32_t group0, ngroups;          // first group of the tile, groups in the bucket
    uint64_t plane_off;
};
struct TabItem {
    uint32_t row_tile; // index into the row tile list
    uint32_t col0;     // global index of the first column
    uint32_t ncols;    // <= BS_TAB_TILE
    uint32_t diag;     // some column index <= some row index (needs the row < column mask)
};
hipError_t launch_bs_tab(const PairArgs &a, const TabRowTile *rts, uint32_t n_row_tiles, TabItem *items,
                         uint32_t item_cap, int umi_len, uint32_t part, uint32_t n_parts, uint32_t n_waves,
                         bool transposed, hipStream_t s);
// exact check of the n_entries filter hits in a.ovf (the bit-sliced kernels' overflow list)
hipError_t launch_verify_list(const PairArgs &a, bool key32, uint32_t n_entries, hipStream_t s);

// ---- optional prune mode (umihip_sort.hip): sort a large bucket's entries by filter key
size_t sort_temp_bytes(bool key32, uint32_t n, int key_bits);
// true if a bucket of n entries goes through the library's onesweep passes (a restricted bit
// range is only handed to those; its merge path for smaller inputs gets the full key)
bool sort_is_onesweep(uint32_t n);
// fkey_sorted[start..start+n) = sorted keys, perm[start + i] = original global index of the
// i-th smallest; iota_tmp is scratch of the same extent
// (by the bits [begin_bit, key_bits) of the key only)
hipError_t sort_bucket(const void *fkey, bool key32, int begin_bit, int key_bits, uint32_t start, uint32_t n, void *fkey_sorted,
                       uint32_t *perm, uint32_t *iota_tmp, void *tmp, size_t tmp_bytes,
                       hipStream_t s);
// out[i] = keys[pos[i]] widened to 64 bits
hipError_t gather_keys(const void *keys, bool key32, const uint32_t *pos, uint32_t n, uint64_t *out,
                       hipStream_t s);

// Everything for the buckets of 1..fused_max entries, one wave per bucket: contract check,
// thresholds, all pairs, collapse, label[], kept[], root[] (may be NULL), survivors and
// violations into counters[].  Walks bucket_off (device copy) itself.
// sliced: use the bit-sliced body when k <= 3
hipError_t launch_small_buckets(const uint64_t *keys, const uint64_t *nmask, const int32_t *freq,
                                float percentage, const uint64_t *bucket_off, uint32_t n_buckets,
                                uint32_t fused_max, uint32_t n_entries, uint32_t *label, uint8_t *kept, uint32_t *root,
                                int k, int umi_len, bool sliced, int mode, int32_t adj_max_freq,
                                unsigned long long *counters, uint32_t max_blocks, hipStream_t s);

hipError_t launch_small_buckets_wide(const uint64_t *keys, const uint64_t *nmask, int n_words, const int32_t *freq,
                                     float percentage, const uint64_t *bucket_off, uint32_t n_buckets,
                                     uint32_t fused_max, uint32_t n_entries, uint8_t *kept, uint32_t *root, int k,
                                     int umi_len, unsigned long long *counters, uint32_t max_blocks, hipStream_t s);

// one label-propagation round (hook over edges + pointer jump); round r is a
// no-op on the device when round r-1 changed nothing.
hipError_t launch_prop_round(const uint2 *edges, const unsigned long long *counters,
                             uint32_t edge_cap, uint32_t *label, uint32_t n, uint32_t *changed,
                             int round, uint32_t n_edges_hint, hipStream_t s);

// label[i] = i (collapse of an external edge list)
hipError_t launch_iota(uint32_t *label, uint32_t n, hipStream_t s);
// two-phase directional collapse: components over the symmetric pairs, then the DAG of one-way pairs
hipError_t launch_cc_round(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                           uint32_t *comp, uint32_t n, uint32_t *changed, int round,
                           uint32_t n_edges_hint, hipStream_t s);
hipError_t launch_dag_round(const uint2 *edges, const unsigned long long *counters, uint32_t edge_cap,
                            const uint32_t *comp, uint32_t *lab, uint32_t n, uint32_t *changed,
                            int round, uint32_t n_edges_hint, hipStream_t s);
hipError_t launch_map_labels(uint32_t *comp, const uint32_t *lab, uint32_t n, hipStream_t s);

hipError_t launch_finalize(const uint32_t *label, const RangeTask *ranges, uint32_t n_ranges, uint32_t n,
                           uint8_t *kept, uint32_t *root, unsigned long long *counters, hipStream_t s);

// adjacency collapse with max_freq > 0 (greedy in rank order): one iteration
hipError_t launch_adj_iter(const uint2 *edges, const unsigned long long *counters,
                           uint32_t edge_cap, uint8_t *status, uint8_t *blocked, uint32_t *label,
                           uint32_t n, unsigned long long *counters_rw, uint32_t n_edges_hint,
                           hipStream_t s);
hipError_t launch_adj_finalize(const uint8_t *status, const uint32_t *label, const RangeTask *ranges,
                               uint32_t n_ranges, uint32_t n, uint8_t *kept, uint32_t *root,
                               unsigned long long *counters, hipStream_t s);

} // namespace umihip
