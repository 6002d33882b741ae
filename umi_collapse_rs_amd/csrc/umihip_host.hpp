// What the host .cpp files of libumihip.so share: error reporting, the two buffer classes, the
// RCCL loader, the context, the few functions one file offers the others, and the staging of a
// host-buffer call (HostIo).  Host code only: no .hip file includes this.
#pragma once
#include "../../include/umihip.h"

#include <cstring>
#include <dlfcn.h>
#include <string>
#include <type_traits>
#include <vector>

#include "umihip_internal.h"
#include "umihip_io_layout.hpp"
#include "umihip_plan.hpp"

#include <rccl/rccl.h> // (types only: the library itself is opened when the first collective is asked for)

namespace umihip {

// the calling thread's error text (umi_last_error): one string for the whole library, set by fail()
int fail(int code, const char *fmt, ...);
const std::string &last_error();

#define HIP_TRY(expr)                                                                        \
    do {                                                                                     \
        hipError_t e__ = (expr);                                                             \
        if (e__ != hipSuccess)                                                               \
            return fail(UMI_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(e__), \
                        __FILE__, __LINE__);                                                 \
    } while (0)

// grow-only device buffer; frees itself (with the device current that it was reserved on: umi_ctx_destroy)
struct DevBuf {
    void *p = nullptr;
    size_t cap = 0;
    DevBuf() = default;
    DevBuf(const DevBuf &) = delete;
    DevBuf &operator=(const DevBuf &) = delete;
    ~DevBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return UMI_OK;
        if (p) {
            hipError_t e = hipFree(p);
            p = nullptr;
            cap = 0;
            if (e != hipSuccess) return fail(UMI_ERR_HIP, "hipFree: %s", hipGetErrorString(e));
        }
        size_t want = bytes + bytes / 4 + 256;
        hipError_t e = hipMalloc(&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(e == hipErrorOutOfMemory ? UMI_ERR_NOMEM : UMI_ERR_HIP,
                        "hipMalloc(%zu): %s", want, hipGetErrorString(e));
        }
        cap = want;
        return UMI_OK;
    }
    void release()
    {
        if (p) (void)hipFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible_v<DevBuf>, "a DevBuf owns its allocation");

constexpr int MAX_ROUNDS = 1 << 20;
constexpr int DAG_ROUNDS = 3; // one-way rounds enqueued before the host first looks (freq at least
                              // halves along a one-way pair at p <= 0.5: depth 2 at config 2)

// grow-only pinned host buffer, frees itself; every write of bytes goes through put(), which checks the extent
struct PinnedBuf {
    char *p = nullptr;
    size_t cap = 0;
    PinnedBuf() = default;
    PinnedBuf(const PinnedBuf &) = delete;
    PinnedBuf &operator=(const PinnedBuf &) = delete;
    ~PinnedBuf() { release(); }
    int reserve(size_t bytes)
    {
        if (bytes <= cap) return UMI_OK;
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
        const size_t want = bytes + bytes / 4 + 4096;
        hipError_t e = hipHostMalloc((void **)&p, want);
        if (e != hipSuccess) {
            p = nullptr;
            return fail(UMI_ERR_NOMEM, "hipHostMalloc(%zu): %s", want, hipGetErrorString(e));
        }
        cap = want;
        return UMI_OK;
    }
    int put(size_t off, const void *src, size_t bytes)
    {
        if (off > cap || bytes > cap - off)
            return fail(UMI_ERR_HIP, "internal: staging write of %zu bytes at %zu beyond %zu", bytes, off, cap);
        if (bytes) memcpy(p + off, src, bytes);
        return UMI_OK;
    }
    void release()
    {
        if (p) (void)hipHostFree(p);
        p = nullptr;
        cap = 0;
    }
    template <typename T> T *as() const { return (T *)p; }
};
static_assert(!std::is_copy_constructible_v<PinnedBuf>, "a PinnedBuf owns its allocation");

// RCCL, opened on first use (dlopen: a process that never asks for a collective -- the umicollapse
// program, a single-GPU host -- does not map it; one that already holds a copy, PyTorch's, gets that
// copy instead of a second one beside it)
struct RcclApi {
    void *handle = nullptr;
    ncclResult_t (*CommInitAll)(ncclComm_t *, int, const int *) = nullptr;
    ncclResult_t (*CommDestroy)(ncclComm_t) = nullptr;
    ncclResult_t (*GroupStart)() = nullptr;
    ncclResult_t (*GroupEnd)() = nullptr;
    ncclResult_t (*AllGather)(const void *, void *, size_t, ncclDataType_t, ncclComm_t, hipStream_t) = nullptr;
    const char *(*GetErrorString)(ncclResult_t) = nullptr;
    std::string error;
    bool load()
    {
        if (handle) return true;
        for (const char *name : {"librccl.so.1", "librccl.so", "/opt/rocm/lib/librccl.so.1"}) {
            handle = dlopen(name, RTLD_NOW | RTLD_GLOBAL);
            if (handle) break;
        }
        if (!handle) {
            error = std::string("cannot open librccl.so: ") + dlerror();
            return false;
        }
        auto sym = [&](const char *name) {
            void *p = dlsym(handle, name);
            if (!p && error.empty()) error = std::string("librccl.so lacks ") + name;
            return p;
        };
        CommInitAll = (decltype(CommInitAll))sym("ncclCommInitAll");
        CommDestroy = (decltype(CommDestroy))sym("ncclCommDestroy");
        GroupStart = (decltype(GroupStart))sym("ncclGroupStart");
        GroupEnd = (decltype(GroupEnd))sym("ncclGroupEnd");
        AllGather = (decltype(AllGather))sym("ncclAllGather");
        GetErrorString = (decltype(GetErrorString))sym("ncclGetErrorString");
        if (!error.empty()) {
            handle = nullptr;
            return false;
        }
        return true;
    }
};

// No distance exceeds this: bit_count_xor is at most 64 per word, umi_dist halves it, and a batched key has at
// most 4 words (85 bases).  Every k from here up means "all pairs", and the clamped value is what the planner and
// the kernels see, so that their 2 k and 2 k + 1 stay far inside an int.
constexpr int BATCH_MAX_K = 32 * 4;

// the one place an `algo` of the interface becomes a mode of the pipeline
inline bool known_algo(int algo) { return algo == UMI_ALGO_DIRECTIONAL || algo == UMI_ALGO_ADJACENCY || algo == UMI_ALGO_CLUSTER; }
inline int mode_of(int algo)
{
    return algo == UMI_ALGO_DIRECTIONAL ? MODE_DIRECTIONAL : algo == UMI_ALGO_CLUSTER ? MODE_CLUSTER : MODE_ADJACENCY;
}

inline int wide_words(int umi_len) { return (3 * umi_len + 63) / 64; } // bitset.rs:17-18

} // namespace umihip

struct umi_ctx {
    // the communicators of a multi-device context's devices (umi_dedup_batch_device_multi), made on first use
    umihip::RcclApi rccl;
    std::vector<ncclComm_t> comms;
    // a multi-device context (umi_ctx_create_multi) owns one ordinary context per device and has
    // no device state of its own; an ordinary one has no subs
    std::vector<umi_ctx *> subs;
    // per-device staging of the sharded host-buffer call (pinned): this rank's entries gathered
    // from the caller's arrays, its share of the bucket table, its results
    umihip::PinnedBuf sh_in, sh_out;
    std::vector<uint64_t> sh_boff;
    int device = 0;
    hipStream_t own_stream = nullptr;
    bool profile = false;
    uint64_t edge_capacity = 1u << 20;
    uint64_t ovf_capacity = 1u << 18; // filter hits beyond the blocks' LDS queues (grows like the edge list)
    uint32_t small_max = 1024;
#ifdef UMIHIP_DEV
    static constexpr bool LEGACY_DEFAULT = true;
#else
    static constexpr bool LEGACY_DEFAULT = false; // the round-1 tile kernels are not in this build
#endif
    bool use_bitslice = LEGACY_DEFAULT;
    uint32_t bs_col_chunk = umihip::BS_COL_CHUNK;
    uint32_t bs_tab_min_run = 4; // table variant only where a run of equal high bases is about this long
    bool bs_transposed = true; // table variant: walk items with the columns of a run across the lanes
    uint32_t bs_tab_waves = 0; // one-wave blocks of the item walk (0: 128 per CU; items are dealt
                               // statically over them, the dispatcher evens out the rest)
    uint32_t fused_max = umihip::FUSED_MAX;
    uint32_t fused_blocks = 20; // 256-thread blocks per CU of the fused kernel's persistent grid
    bool fused_sliced = true;
    int bs_unit = 2;
    bool bs_sorted = LEGACY_DEFAULT; // sort large buckets by key and reuse prefix state along column runs
    bool bs_tables = LEGACY_DEFAULT; // ... and look the low units up in per-lane register tables (32-bit keys)
    int two_phase = 2; // directional collapse: 0 plain label propagation; 1 components of the symmetric
                       // pairs by hook/jump rounds, then the DAG; 2 the components by union-find
    bool seg_index = true;   // large buckets through the n-gram partition (umihip_seg.hip)
    uint32_t seg_min = 512;  // ... from this many entries up
    uint64_t split_min = 200000; // multi-device: a bucket at least this large that dominates the call
                                 // has its pairs split over the devices instead of the buckets
    uint32_t table_pieces = 1; // many buckets: the table is walked, uploaded and handed to the fused kernel in
                               // this many pieces (measured on 10^5 positions: one launch 0.13 ms, four 0.24)
    bool seg_ckey = true;    // its pair kernel compares 3-bit-per-base compare keys where they fit 32 bits
    bool seg_sliced = true;  // ... 64 columns at a time from ballots of the columns' code bits (k <= 3)
    bool seg_unite = true;   // its pair kernel unites symmetric pairs on the spot (batched directional path)
    bool seg_lds = true;     // counting sort of the partition through per-block LDS histograms (where
                             // every part has at most SEG_LDS_BINS bins), else one atomic per entry
    int seg_occ[2][2][2] = {{{0, 0}, {0, 0}}, {{0, 0}, {0, 0}}};
    bool seg_local = true;   // part-0 sub-buckets of at most seg_local_cap entries united in LDS by a kernel
    uint32_t seg_local_cap = umihip::SEG_LOCAL_CAP; // of their own, ahead of the pair kernel (batched directional path)
    bool seg_probe = true;   // ... k = 1 without N: their pairs decided by bitmap lookups where at most
                             // SEG_PROBE_MAX_REST bases lie outside the bins (0: the tile walk)
    uint32_t seg_probe_min = umihip::SEG_PROBE_MIN; // smallest sub-bucket decided by lookups
    bool seg_super = true;   // k = 1 without N: runs of 4^g adjacent part-0 bins decided as one unit in LDS (seg_super_kernel)
    bool seg_super_coarse = true; // ... and the counting sort files a part-0 entry of such a segment under its run's first
                                  // bin, not its own (SegArgs::super_coarse; 0 for A/B runs and as the tests' reference)
    bool seg_cross = true;   // ... and the pairs between its super-bins are found by ANDing their rest-code maps: part 1 is
                             // counted, not filed (SegDesc::cross, seg_cross_kernel)
    bool seg_cross_failed = false; // a call of this context fell back (a key twice, a run above the cap): its later calls
                                   // are planned without the path until "seg_cross" is set again
    uint64_t seg_cross_launches = 0;        // attempts of this context's calls that launched seg_cross_kernel ...
    uint64_t seg_cross_abandoned_calls = 0; // ... and calls that fell back (umi_ctx_get_counter)
    uint32_t seg_cross_map_mb = umihip::SEG_CROSS_MAP_MB; // the maps of one segment, 4^umi_len / 8 bytes, at most
    int seg_super_bases = 0; // ... g (0: the planner's choice, choose_super_bases)
    uint32_t seg_super_cap = umihip::SEG_SUPER_CAP; // largest super-bin that kernel takes (LDS: 16 bytes per entry + 16 KB)
    uint32_t seg_super_min = umihip::SEG_SUPER_MIN; // smallest expected super-bin the path is planned for
    int seg_local_occ[2] = {0, 0}; // its resident blocks per CU (without / with N) at seg_local_occ_cap
    uint32_t seg_local_occ_cap = 0;
    bool collapse_kept_only = true; // a batched directional call without root[] skips the forest flatten (umihip_collapse.hip)
    uint32_t seg_blocks = 0; // one-wave blocks of its pair kernel (0: all resident at once -- 24 per CU by
                             // registers, 28 by LDS with the compare keys' leaner loop)
    // workspace
    umihip::DevBuf fkey, thr, label, lab, edges, edge_dist, ovf, counters, boff, status, blocked;
    umihip::DevBuf plan_tables; // ranges, segment descriptors, scan chunks, popcount tile tasks: one upload
    umihip::DevBuf bs_tasks, plane_tasks, planes, tab_rows, tab_items;
    umihip::DevBuf seg_bin_cnt, seg_bin_start, seg_tasks, seg_sub_rec, seg_priv_edges, seg_priv_dist, seg_priv_cnt, seg_priv_stat;
    umihip::DevBuf seg_cross_maps; // cross segments: the super-bins' rest-code maps, then the u16 prefixes of their words
    umihip::PinnedBuf h_plan_alt[2]; // staging of the plan's tables, in turn; [plan_flip ^ 1] = what plan_tables holds
    int plan_flip = 0;
    size_t plan_uploaded = 0;
    const void *plan_uploaded_to = nullptr;
    int n_cus = 256;     // the CUs every call sizes its grids from: the device's, or option "grid_cus"
    int device_cus = 256; // the device's own count ("grid_cus" 0 puts it back)
    umihip::DevBuf fkey_sorted, perm, iota, sort_tmp, sample_pos, sample_out; // prune mode
    bool prune = false;
    umihip::Plan plan;
    umihip::TablePass table_pass;
    // the device copies of a host-buffer call's arrays: one block, laid out afresh by every call (HostIo below)
    umihip::DevBuf io;
    // the workspace of the single-shot device forms (staging, consensus, correction, count matrix, stats): each
    // call carves it anew and keeps nothing in it -- settle() leaves one call at a time in the context
    umihip::DevBuf call_ws;
    // umi_junction_matrix*: the workspace of its second half, sized by the occurrences its first half counted in call_ws
    umihip::DevBuf jn_ws;
    // whole-read keys (umi_dedup_seqs*): group table, records and their sort, runs, tile tasks
    umihip::DevBuf seq_groups, seq_ka, seq_kb, seq_va, seq_vb, seq_flag, seq_runid, seq_rs, seq_tend, seq_tmp;
    // pinned staging of umi_count_matrix* (the non-empty buckets' offsets and numbers) and of umi_dedup_stats*
    // (the non-empty buckets' offsets, the deep buckets and their pieces)
    umihip::PinnedBuf cm_h, ds_h;
    uint32_t stats_split = umihip::STATS_SPLIT; // buckets of at least this many entries are counted by the whole grid
    bool gene_top = true; // umi_assign_genes: the sampled top of each table in LDS (option "gene_top")
    bool velocity_skip = false; // umi_velocity_matrix: a read loads its molecule's evidence and skips the atomic where its bit is set (option "velocity_skip")
    bool saturation_skip = false; // umi_saturation_curve: likewise for its molecule's word of levels (option "saturation_skip")
    bool gene_body_top = true; //umi_assign_genes_introns: the body tables' tops too (option "gene_body_top"; counts with gene_top)
    // umi_dedup_batch_cr*: buckets of at most cr_small_max entries are decided a lane per entry, the others from the
    // neighbour list (option "cr_small_max"); its device table, and its workspace (counters, span, target, the larger
    // buckets' compact arrays and best words), carved anew by every call
    uint32_t cr_small_max = umihip::CR_SMALL_MAX;
    umihip::DevBuf cr_boff, cr_ws;
    uint32_t cons_split = 512; // clusters of at least this many reads are summed in pieces by the whole grid
    umihip::PinnedBuf h_boff;                 // pinned staging of the bucket table
    umihip::PinnedBuf h_tasks;                // pinned staging of the bit-sliced tile-task lists
    unsigned long long *h_counters = nullptr; // pinned mirror of the control block (CTRL_BYTES), then, in a line of
                                              // its own, the sequence number of the last copy that has arrived
    unsigned long long ctrl_seq = 0;          // ... and of the last copy asked for
    int dag_rounds_ahead = umihip::DAG_ROUNDS; // one-way rounds enqueued before the host first looks: as many as the
                                              // call before needed (a quiet round returns at once)
    // umi_dedup_batch_device_begin / umi_dedup_batch_end: a call whose work is all on the stream and whose
    // control block has not been looked at yet (deferred), or whose result waits to be handed out
    struct PendingCall {
        bool deferred = false, have_result = false;
        unsigned long long seq = 0;
        hipStream_t stream = nullptr;
        int rc = UMI_OK;
        std::string err; // the text of a non-OK rc, told again when the result is handed out
        umi_stats st;
    } pending;
    bool spin_wait = true;                    // watch that number instead of hipStreamSynchronize (option "spin_wait")
    unsigned long long *h_seq() const { return h_counters + umihip::CTRL_BYTES / sizeof(unsigned long long); }
    uint32_t *h_changed() const { return (uint32_t *)(h_counters + umihip::CNT_COUNT); }
    uint32_t *d_changed() const { return (uint32_t *)(counters.as<unsigned long long>() + umihip::CNT_COUNT); }
    static constexpr int N_EVENTS = 10;
    hipEvent_t ev[N_EVENTS] = {};
};

namespace umihip {

// umihip_api.cpp: the checks every batched call starts with; *n_out = the call's entries
int check_common(umi_ctx *ctx, const uint64_t *bucket_off, uint64_t n_buckets, int umi_len, int k,
                 int algo, uint64_t *n_out, int max_len = UMI_MAX_UMI_LEN);

// umihip_pipeline.cpp: a whole batched call on stream s (lets a deferred call end first)
int run_pipeline(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                 const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n,
                 int umi_len, int k, float percentage, int mode, int32_t adj_max_freq,
                 uint8_t *d_kept, uint32_t *d_root, hipStream_t s, umi_stats *stats,
                 const uint64_t *d_bucket_off = nullptr, int n_words = 1, bool may_defer = false, bool edit = false);
// ... share `part` of `n_parts` of its tile tasks, up to the pair kernels: the pairs found stay in
// ctx->edges, *n_edges of them (the caller has settled the context)
int run_pipeline_part(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                      const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n, int umi_len, int k,
                      float percentage, int mode, int32_t adj_max_freq, hipStream_t s, uint32_t part,
                      uint32_t n_parts, umi_stats *stats, uint64_t *n_edges);
// ... the collapse of an edge list that is already on the device (EdgeCollapse)
int collapse_edges(umi_ctx *ctx, uint32_t n, const uint2 *d_edges, uint32_t n_edges, int mode, uint8_t *d_kept,
                   uint32_t *d_root, hipStream_t s, umi_stats *stats);
// ... the end of a deferred call (umi_dedup_batch_end), and what every other entry point that touches
// the context's workspace does first
int finish_pending(umi_ctx *ctx, umi_stats *stats);
void settle(umi_ctx *ctx);

// a device pointer into the staging block, good once the call's HostIo is open; null for an absent array
template <typename T> struct IoPtr {
    const DevBuf *block = nullptr;
    size_t off = IO_ABSENT;
    operator T *() const { return (T *)io_at(block->p, off); }
};

// One host-buffer call on a single-device context: its arrays' device copies are slots of ctx->io.  Declare
// them, open(), run the device form on stream(), fetch() what came out, close().  However the call ends, the
// stream has run dry before the caller has its arrays back: what close() did not see to, the destructor does.
class HostIo {
    struct Upload {
        const void *host;
        size_t off, bytes;
    };
    umi_ctx *ctx;
    IoLayout layout;
    std::vector<Upload> uploads;
    bool busy = false; // a copy from or to the caller's memory may be in flight

public:
    explicit HostIo(umi_ctx *c) : ctx(c) {}
    HostIo(const HostIo &) = delete;
    HostIo &operator=(const HostIo &) = delete;
    ~HostIo()
    {
        if (busy) (void)hipStreamSynchronize(ctx->own_stream);
    }
    hipStream_t stream() const { return ctx->own_stream; }
    // an input: `bytes` of `host` are uploaded into a slot of bytes + pad (absent where host is null)
    template <typename T> IoPtr<T> in(const T *host, size_t bytes, size_t pad = 0)
    {
        const IoPtr<T> p{&ctx->io, layout.add(host != nullptr, bytes + pad)};
        also(p, 0, host, bytes);
        return p;
    }
    // ... one more array into the pad of a slot that is present, `at` bytes from its start
    template <typename T> void also(IoPtr<T> slot, size_t at, const T *host, size_t bytes)
    {
        if (host && bytes) uploads.push_back({host, slot.off + at, bytes});
    }
    // an output of this many bytes; the second form is absent where the caller did not ask for the array
    template <typename T> IoPtr<T> out(size_t bytes) { return {&ctx->io, layout.add(true, bytes)}; }
    template <typename T> IoPtr<T> out(const T *host, size_t bytes) { return {&ctx->io, layout.add(host != nullptr, bytes)}; }
    // the device made current, a deferred call let end, the block reserved, the inputs put on the stream
    int open()
    {
        HIP_TRY(hipSetDevice(ctx->device));
        settle(ctx);
        if (int rc = ctx->io.reserve(layout.total + 1)) return rc; // (+ 1: a block, and an address, even for no bytes)
        busy = true;
        for (const Upload &u : uploads)
            HIP_TRY(hipMemcpyAsync(ctx->io.as<char>() + u.off, u.host, u.bytes, hipMemcpyHostToDevice, ctx->own_stream));
        return UMI_OK;
    }
    // the first `count` elements of an output to the caller (nothing where host is null)
    template <typename T> int fetch(T *host, IoPtr<T> from, size_t count)
    {
        if (host && count) HIP_TRY(hipMemcpyAsync(host, (T *)from, count * sizeof(T), hipMemcpyDeviceToHost, ctx->own_stream));
        return UMI_OK;
    }
    int close()
    {
        busy = false;
        HIP_TRY(hipStreamSynchronize(ctx->own_stream));
        return UMI_OK;
    }
};

} // namespace umihip
