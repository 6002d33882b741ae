// The pipeline of a batched call, host side: the stages of one call over one stream (Pipeline), the collapse
// of an edge list that is on the device already (EdgeCollapse), and the end of a deferred call.  The entry
// points reach it through umihip_host.hpp (run_pipeline, run_pipeline_part, collapse_edges, finish_pending,
// settle); the context and the error text are umihip_api.cpp's.
#include "umihip_host.hpp"

#include <algorithm>
#include <chrono>

using namespace umihip;

namespace {

// rounds of one propagation phase until a whole round changes nothing; the per-round flags
// are checked on the device (a round after a quiet one returns at once), the host looks
// every `batch` rounds
template <class LaunchRound>
int run_rounds(umi_ctx *ctx, hipStream_t s, LaunchRound launch_round, int &rounds, int batch = 4)
{
    uint32_t *d_changed = ctx->d_changed();
    for (;;) {
        HIP_TRY(hipMemsetAsync(d_changed, 0, sizeof(uint32_t) * MAX_ROUNDS_PER_SYNC, s));
        for (int r = 0; r < batch; r++) HIP_TRY(launch_round(d_changed, r));
        HIP_TRY(hipMemcpyAsync(ctx->h_changed(), d_changed, sizeof(uint32_t) * batch, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        bool done = false;
        for (int r = 0; r < batch && !done; r++) {
            rounds++;
            done = ctx->h_changed()[r] == 0;
        }
        if (done) return UMI_OK;
        if (rounds > MAX_ROUNDS) return fail(UMI_ERR_HIP, "label propagation diverged");
        batch = std::min(2 * batch, MAX_ROUNDS_PER_SYNC);
    }
}

// label[v] = smallest rank that reaches v over the permitted-edge list (directional.rs:30-54,
// 78-88); ctx->label holds the start labels (v itself, or what the fused kernel left)
int directional_labels(umi_ctx *ctx, const uint2 *d_edges, unsigned long long *d_cnt, uint32_t edge_cap,
                       uint64_t n_edges, uint32_t n, hipStream_t s, int &rounds)
{
    int rc;
    uint32_t *d_label = ctx->label.as<uint32_t>();
    if ((rc = ctx->lab.reserve((size_t)n * 4))) return rc;
    uint32_t *d_lab = ctx->lab.as<uint32_t>();
#ifdef UMIHIP_DEV
    if (!ctx->two_phase) // (one phase: lab[] stays unused)
        return run_rounds(ctx, s, [&](uint32_t *d_changed, int r) {
            return launch_prop_round(d_edges, d_cnt, edge_cap, d_label, n, d_changed, r, (uint32_t)n_edges, s);
        }, rounds);
    if (ctx->two_phase != 2) {
        HIP_TRY(launch_iota(d_lab, n, s));
        if ((rc = run_rounds(ctx, s, [&](uint32_t *d_changed, int r) {
                 return launch_cc_round(d_edges, d_cnt, edge_cap, d_label, n, d_changed, r, (uint32_t)n_edges, s);
             }, rounds, 6))) // a giant component of 10^6 entries settles in 5
            return rc;
    } else
#endif
    {
        HIP_TRY(launch_uf_components(d_edges, d_cnt, edge_cap, d_label, d_lab, n, (uint32_t)n_edges, s));
        rounds++;
    }
    if ((rc = run_rounds(ctx, s, [&](uint32_t *d_changed, int r) {
             return launch_dag_round(d_edges, d_cnt, edge_cap, d_label, d_lab, n, d_changed, r,
                                     (uint32_t)n_edges, s);
         }, rounds, 3))) // (the common depth: freq at least halves along a one-way pair at p <= 0.5; a deeper
                         // chain -- 255 pairs in tests/test_gpu_deep_chains.py -- goes on in batches of 6, 12, 16)
        return rc;
    HIP_TRY(launch_map_labels(d_label, d_lab, n, s));
    return UMI_OK;
}

// adjacency with max_freq >= 1: the greedy root loop over the edge list, one decision level per iteration
// (ctx->status and ctx->blocked: cleared by the caller; ctx->label holds the start labels)
int adjacency_status(umi_ctx *ctx, const uint2 *d_edges, unsigned long long *d_cnt, uint32_t edge_cap,
                     uint64_t n_edges, uint32_t n, hipStream_t s, int &iters)
{
    for (;;) {
        HIP_TRY(hipMemsetAsync(&d_cnt[CNT_UNKNOWN], 0, sizeof(unsigned long long), s));
        HIP_TRY(launch_adj_iter(d_edges, d_cnt, edge_cap, ctx->status.as<uint8_t>(), ctx->blocked.as<uint8_t>(),
                                ctx->label.as<uint32_t>(), n, d_cnt, (uint32_t)n_edges, s));
        HIP_TRY(hipMemcpyAsync(&ctx->h_counters[CNT_UNKNOWN], &d_cnt[CNT_UNKNOWN],
                               sizeof(unsigned long long), hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        iters++;
        if (ctx->h_counters[CNT_UNKNOWN] == 0) return UMI_OK;
        if (iters > MAX_ROUNDS) return fail(UMI_ERR_HIP, "adjacency collapse diverged");
    }
}

// The control block's arrival is the end of the stream's work: copy number `seq` is watched for (numbers only
// grow), bounded -- a stream in error never delivers, and the runtime's wait reports why
hipError_t await_control(umi_ctx *ctx, unsigned long long seq, hipStream_t s)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (unsigned spins = 0;; spins++) {
        if (__atomic_load_n(ctx->h_seq(), __ATOMIC_ACQUIRE) >= seq) return hipSuccess;
        if ((spins & 1023u) == 1023u && std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    return hipStreamSynchronize(s);
}

// what the control block that has arrived says about the call's input
int contract_verdict(umi_ctx *ctx)
{
    const unsigned long long bad =
        ctx->h_counters[CNT_ERROR] + (ctx->h_counters[CNT_RISES] - ctx->h_counters[CNT_START_RISES]);
    if (bad)
        return fail(UMI_ERR_ORDER,
                    "%llu entries break the input contract (freq < 1, not in freq-descending rank "
                    "order inside a bucket, or an N base without nmask)",
                    bad);
    return UMI_OK;
}

// The device pipeline shared by both batched entry points and by umi_data_new, as a
// sequence of stages over one stream.  mode MODE_NEIGHBOURS stops after the pair kernels
// (the edge list then holds the neighbour pairs).
class Pipeline {
  public:
    Pipeline(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
             const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n, int umi_len, int k,
             float percentage, int mode, int32_t adj_max_freq, uint8_t *d_kept, uint32_t *d_root,
             hipStream_t s, uint32_t part = 0, uint32_t n_parts = 1)
        : ctx(ctx), d_keys(d_keys), d_nmask(d_nmask), d_freq(d_freq), bucket_off(bucket_off),
          n_buckets(n_buckets), n(n), umi_len(umi_len), k(std::min(k, BATCH_MAX_K)), percentage(percentage), mode(mode),
          adj_max_freq(adj_max_freq), d_kept(d_kept), d_root(d_root), s(s), pl(ctx->plan),
          key32(umi_len <= 16),
          need_pairs(!(mode == MODE_ADJACENCY && adj_max_freq < 1)), // reference adj: only the query goes
          // the fused kernel collapses whole buckets itself: not when only an edge list is wanted
          fused_max((mode == MODE_NEIGHBOURS || !need_pairs || n_parts > 1)
                        ? 0u
                        : std::min<uint32_t>(ctx->fused_max, FUSED_MAX)),
          prof(ctx->profile), part(part), n_parts(n_parts)
    {
        memset(&st, 0, sizeof(st));
        st.n_umis = n;
        st.n_buckets = n_buckets;
    }

    int run(umi_stats *stats)
    {
        HIP_TRY(hipSetDevice(ctx->device));
        int rc = run_stages();
        // Leave with the stream drained on every path: enqueued work reads caller memory
        // (bucket_off) and workspace buffers that the next call may reallocate.
        if (!drained) (void)hipStreamSynchronize(s);
        if (rc == UMI_OK && stats) *stats = st;
        return rc;
    }

    uint64_t edge_count() const { return n_edges; }
    // the caller keeps a copy of bucket_off in device memory (resident like keys and freq): no
    // staging copy, no upload
    void use_device_table(const uint64_t *d_table) { d_boff_caller = d_table; }
    // keys of n_words > 1 words per entry (umi_len > 21).  Filter keys and the segment index work on
    // the first word's 21 bases (two UMIs within k overall are within k there), every hit is decided
    // on all words; the fused kernel slices all words' bases; buckets in between go to the exact
    // all-pairs kernel of umihip_wide.hip.
    void use_wide_keys(int words) { n_words = words; }
    void allow_deferred_end() { may_defer = true; }
    // Levenshtein distance between one-word keys (umi_dedup_batch_edit): every bucket as 64-row chunks
    // against its later entries through the kernel of umihip_edit.hip -- no fused kernel, no segment
    // index (two UMIs within k edits need not agree on any fixed base range).  No distance exceeds
    // umi_len, and the clamped k is what the kernel sees.
    void use_edit_distance()
    {
        edit = true;
        k = std::min(k, umi_len);
        fused_max = 0;
    }

  private:
    umi_ctx *ctx;
    const uint64_t *d_keys, *d_nmask;
    const int32_t *d_freq;
    const uint64_t *bucket_off;
    const uint64_t *d_boff_caller = nullptr;
    int n_words = 1;
    bool edit = false;
    bool wide() const { return n_words > 1; }
    int plan_umi_len() const { return wide() ? 21 : umi_len; } // bases the filter keys hold
    const uint64_t *d_boff() const { return d_boff_caller ? d_boff_caller : ctx->boff.as<uint64_t>(); }
    uint64_t n_buckets;
    uint32_t n;
    int umi_len, k;
    float percentage;
    int mode;
    int32_t adj_max_freq;
    uint8_t *d_kept;
    uint32_t *d_root;
    hipStream_t s;
    Plan &pl; // lives in the context: its vectors keep their capacity between calls
    const bool key32, need_pairs;
    uint32_t fused_max; // (0 for multi-word keys)
    const bool prof;
    const uint32_t part, n_parts; // n_parts > 1: evaluate only every n_parts-th tile task, stop
                                  // after the pair kernels (multi-GPU split of one call's pairs)
    uint64_t task_counter = 0;    // running index over all tile tasks, for that split
    bool prune = false, drained = false, fused_ran = false, seg_timed = false, edit_timed = false;
    bool may_defer = false; // umi_dedup_batch_device_begin: the end of the call may be left on the stream
    size_t zero_behind_control = 0; // bytes of the segment index's counters that sit behind the control block
    uint32_t priv_blocks_for_collapse = 0; // blocks of the segment index's local and pair kernels whose private edge
                                           // slots the collapse's flatten launch appends to the list (0: appended already)
    uint64_t seg_local_bins = 0; // part-0 bins of the call's segments (the local kernel's grid at most)
    bool super_pairs_counted = false; // seg_super_kernel has run with SegArgs::super_count_pairs in this call
    uint32_t launches_before_attempt = 0; // st.n_pair_launches when run_one_sync's attempt in hand began
    umi_stats st;
    unsigned long long *d_cnt = nullptr;
    size_t n_tasks = 0;              // tile tasks of the pair kernels (fused buckets excluded)
    uint64_t n_edges = 0;  // entries the pair kernels appended to the edge list
    uint64_t n_direct = 0; // symmetric pairs united where they were found
    uint64_t seg_tasks_made = 0;
    uint32_t cap_used = 0;
    const void *bs_fkey = nullptr;   // filter keys the bit-sliced tiles are cut from
    [[maybe_unused]] const uint32_t *bs_perm = nullptr;
    // device tables of the plan (inside ctx->plan_tables)
    const RangeTask *d_ranges = nullptr;
    const SegDesc *d_segs = nullptr;
    const SegScanChunk *d_chunks = nullptr;
    const PairTask *d_small = nullptr, *d_big = nullptr;
    const SegBlock *d_seg_blocks = nullptr;
    const SegSuper *d_supers = nullptr;
    SegArgs seg;

    // Everything of a call enqueued back to back, one synchronisation at the end: the batched
    // directional path (and the reference's adjacency, which needs no pairs) without the development build's tiles.
    bool one_sync() const
    {
        return (mode == MODE_DIRECTIONAL || mode == MODE_CLUSTER || !need_pairs) && n_parts == 1 && ctx->two_phase == 2 &&
               !legacy_tiles();
    }
    // the forest of the unions is the result (MODE_CLUSTER) or the first phase of it (MODE_DIRECTIONAL)
    bool unions_collapse() const { return mode == MODE_DIRECTIONAL || mode == MODE_CLUSTER; }
    // the call's collapse is the mask-only directional one (CollapseDesc::kept_only): its round 0 has no entry pass,
    // so lab[] = identity is the entry kernels' to store
    bool mask_only_collapse() const { return d_root == nullptr && ctx->collapse_kept_only; }
    // (asked before the development build's tiles are cut: every call that may still turn out one_sync())
    uint32_t *prep_lab() const
    {
        return mode == MODE_DIRECTIONAL && n_parts == 1 && ctx->two_phase == 2 && mask_only_collapse() ? ctx->lab.as<uint32_t>() : nullptr;
    }

    int run_stages()
    {
        int rc;
        if (wide() && (mode != MODE_DIRECTIONAL || k > 3)) fused_max = 0; // (the wide fused kernel: directional, sliced)
        // The fused kernel needs nothing from the plan (it walks the bucket table itself and does
        // everything for its buckets): with many buckets it is enqueued first, and the host walks
        // the table -- tile tasks, pair counts, the entry ranges left for prep and finalize --
        // while it runs.  With few buckets the plan is there at once and says whether any bucket
        // is the fused kernel's at all.
        const bool plan_first = n_buckets <= 4096;
        if (plan_first) {
            // (a table that steps backwards must not reach the planner)
            for (uint64_t b = 0; b < n_buckets; b++)
                if (bucket_off[b + 1] < bucket_off[b])
                    return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
            plan_host();
            // the segment index's bin counters and scan words go behind the control block: one fill
            // clears both
            if (pl.seg_parts && need_pairs) zero_behind_control = seg_zero_bytes();
        }
        if ((rc = reserve_core())) return rc;
        if ((rc = upload_table(!plan_first))) return rc;
        if (plan_first && pl.n_fused && (rc = fused_stage(0, n_buckets))) return rc;
        if (!plan_first) plan_host();
        if (ctx->table_pass.bad_at != ~0ull)
            return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)ctx->table_pass.bad_at);
        if ((rc = upload_plan())) return rc;
        if ((rc = configure_seg())) return rc;
        if ((rc = prep_stage())) return rc;
        if ((rc = cut_legacy_tiles())) return rc;
        if (need_pairs && pl.seg_parts)
            HIP_TRY(launch_seg_build(seg, ctx->fkey.p, d_freq, key32, d_cnt, s));
        if ((rc = upload_legacy_tiles())) return rc;
        if ((rc = count_tasks())) return rc;
        if (one_sync()) return run_one_sync();
        // (connected components have the one collapse path: what keeps a call off it are development options)
        if (mode == MODE_CLUSTER && n_parts == 1)
            return fail(UMI_ERR_ARG, "algo cluster does not run with the development option two_phase below 2");
        if ((rc = pair_stage())) return rc;
        if (mode == MODE_NEIGHBOURS || n_parts > 1) return finish_neighbours();
        if (mode == MODE_DIRECTIONAL || !need_pairs)
            rc = collapse_directional();
        else
            rc = collapse_adjacency();
        if (rc) return rc;
        return finish();
    }

    // significant bits of a filter key: 2 per base in 32-bit keys, 3 in 64-bit ones
    int key_bits() const { return key32 ? 2 * umi_len : std::min(64, 3 * umi_len); }

    // keep this rank's share of a task list (round-robin over one running index: the tasks
    // of a list are similar in size and adjacent ones touch the same tiles)
    template <class T> void keep_my_share(std::vector<T> &v)
    {
        if (n_parts <= 1) return;
        size_t w = 0;
        for (size_t i = 0; i < v.size(); i++)
            if ((task_counter++ % n_parts) == part) v[w++] = v[i];
        v.resize(w);
    }

    // the tail of a call that may be left on the stream: the control copy with its sequence number, no wait
    // (umi_dedup_batch_device_begin; the caller's umi_dedup_batch_end looks)
    int defer_control()
    {
        ctx->pending.seq = ++ctx->ctrl_seq;
        ctx->pending.stream = s;
        HIP_TRY(launch_control_to_host(d_cnt, ctx->h_counters, CTRL_BYTES, s, ctx->h_seq(), ctx->pending.seq));
        ctx->pending.st = st;
        ctx->pending.deferred = true;
        drained = true; // (run() does not wait either)
        return UMI_OK;
    }
    int read_control()
    {
        if (ctx->spin_wait && !prof) { // (the phase profile reads events afterwards: they want the runtime's wait)
            const unsigned long long seq = ++ctx->ctrl_seq;
            HIP_TRY(launch_control_to_host(d_cnt, ctx->h_counters, CTRL_BYTES, s, ctx->h_seq(), seq));
            HIP_TRY(await_control(ctx, seq, s));
        } else {
            HIP_TRY(launch_control_to_host(d_cnt, ctx->h_counters, CTRL_BYTES, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
        return contract_verdict(ctx);
    }

    // workspace whose size follows from n and n_buckets alone
    int reserve_core()
    {
        int rc;
        if ((rc = ctx->fkey.reserve((size_t)n * 8)) || (rc = ctx->thr.reserve((size_t)n * 4)) ||
            (rc = ctx->label.reserve((size_t)n * 4)) || (rc = ctx->lab.reserve((size_t)n * 4)) ||
            (rc = ctx->counters.reserve(CTRL_BYTES + zero_behind_control)) || (rc = ctx->boff.reserve((n_buckets + 1) * 8)))
            return rc;
        if (mode == MODE_ADJACENCY && need_pairs)
            if ((rc = ctx->status.reserve(n)) || (rc = ctx->blocked.reserve(n))) return rc;
        if (edit && (rc = ctx->planes.reserve((size_t)n * 4))) return rc; // (the keys' letter counts; fkey: their bit planes)
        d_cnt = ctx->counters.as<unsigned long long>();
        bs_fkey = ctx->fkey.p;
        return UMI_OK;
    }

    // host planning: which kernel takes which bucket
    void plan_host()
    {
        // (the table is monotone: upload_table has looked)
        scan_table_range(bucket_off, 0, n_buckets, fused_max, nullptr, ctx->table_pass);
        // (connected components: the popcount tiles and the segment index only -- the development build's
        // bit-sliced tiles keep an overflow list of their own, which that mode's one collapse path does not read)
        const bool dev_tiles = mode != MODE_CLUSTER;
        const bool seg_on = ctx->seg_index && need_pairs && !(ctx->prune && dev_tiles) && !edit;
        // super-bins of part 0: a call whose part-0 sub-buckets may be united in LDS (as the one-wave local kernel's:
        // unions on the spot, one device's whole call, 32-bit compare keys), k = 1 (the planner looks), no N mask.
        // Nothing of "seg_local", "seg_probe" or their sizes in here: no count may move with those
        SegSuperOpt sup;
        sup.on = ctx->seg_super && ctx->seg_unite && ctx->seg_ckey && unions_collapse() && n_parts == 1 && ctx->two_phase == 2 &&
                 key32 && !wide() && !edit && !d_nmask;
        sup.bases = ctx->seg_super_bases;
        sup.cap = ctx->seg_super_cap;
        sup.min = ctx->seg_super_min;
        // ... and the cross path where part 0 is filed by super-bin (configure_seg takes the bits back if the call turns
        // out to be none seg_super_kernel runs in)
        sup.cross = sup.on && ctx->seg_cross && !ctx->seg_cross_failed && ctx->seg_super_coarse && ctx->seg_lds && k == 1;
        sup.cross_map_mb = ctx->seg_cross_map_mb;
        build_plan(bucket_off, n_buckets, wide() || edit ? 0x7FFFFFFFu : ctx->small_max,
                   ctx->use_bitslice && k <= BS_MAX_K && !wide() && !edit && dev_tiles,
                   plan_umi_len(), fused_max, ctx->prune && dev_tiles, ctx->bs_sorted && ctx->bs_unit == 2 && need_pairs && dev_tiles,
                   ctx->bs_tables && key32 && dev_tiles, ctx->bs_tab_min_run, seg_on ? std::max(ctx->seg_min, 1u) : 0u, k, key32, pl,
                   &ctx->table_pass, sup);
        prune = ctx->prune && dev_tiles && need_pairs && !pl.bs_buckets.empty() && !wide() && !edit;
        keep_my_share(pl.small_tasks);
        keep_my_share(pl.big_tasks);
        st.max_bucket = pl.max_bucket;
        st.n_pairs = pl.n_pairs;
    }

    size_t seg_bins_bytes() const { return (pl.seg_bins * 4 + 15) & ~(size_t)15; }
    size_t seg_zero_bytes() const
    {
        // (... and one word per segment: seg_scan_flag_word)
        return (seg_bins_bytes() + (1 + pl.seg_chunks.size() + pl.segs.size()) * sizeof(unsigned long long) + 15) & ~(size_t)15;
    }

    // the plan's tables -- entry ranges, segment descriptors and scan chunks, popcount tile tasks --
    // through one pinned block and one copy; workspace whose size the plan gives
    int upload_plan()
    {
        int rc;
        size_t off = 0;
        auto place = [&](size_t bytes) {
            const size_t at = off;
            off = (off + bytes + 63) & ~(size_t)63;
            return at;
        };
        const size_t o_ranges = place(pl.ranges.size() * sizeof(RangeTask));
        const size_t o_segs = place(pl.segs.size() * sizeof(SegDesc));
        const size_t o_chunks = place(pl.seg_chunks.size() * sizeof(SegScanChunk));
        const size_t o_blocks = place(pl.seg_blocks.size() * sizeof(SegBlock));
        const size_t o_supers = place(pl.seg_supers.size() * sizeof(SegSuper));
        const size_t o_small = place(pl.small_tasks.size() * sizeof(PairTask));
        const size_t o_big = place(pl.big_tasks.size() * sizeof(PairTask));
        const size_t total = std::max<size_t>(off, 64);
        // (two staging blocks in turn: what the previous call uploaded stays comparable -- a host that
        // calls again with the same bucket table, a resident job's next step, uploads nothing)
        PinnedBuf &hp = ctx->h_plan_alt[ctx->plan_flip];
        if ((rc = hp.reserve(total)) || (rc = ctx->plan_tables.reserve(total))) return rc;
        if (off) memset(hp.p, 0, off); // (padding between the tables: compared too)
        if ((rc = hp.put(o_ranges, pl.ranges.data(), pl.ranges.size() * sizeof(RangeTask))) ||
            (rc = hp.put(o_segs, pl.segs.data(), pl.segs.size() * sizeof(SegDesc))) ||
            (rc = hp.put(o_chunks, pl.seg_chunks.data(), pl.seg_chunks.size() * sizeof(SegScanChunk))) ||
            (rc = hp.put(o_blocks, pl.seg_blocks.data(), pl.seg_blocks.size() * sizeof(SegBlock))) ||
            (rc = hp.put(o_supers, pl.seg_supers.data(), pl.seg_supers.size() * sizeof(SegSuper))) ||
            (rc = hp.put(o_small, pl.small_tasks.data(), pl.small_tasks.size() * sizeof(PairTask))) ||
            (rc = hp.put(o_big, pl.big_tasks.data(), pl.big_tasks.size() * sizeof(PairTask))))
            return rc;
        const PinnedBuf &prev = ctx->h_plan_alt[ctx->plan_flip ^ 1];
        const bool same = off && ctx->plan_uploaded == off && ctx->plan_uploaded_to == ctx->plan_tables.p &&
                          prev.p && prev.cap >= off && memcmp(prev.p, hp.p, off) == 0;
        if (off && !same) {
            HIP_TRY(hipMemcpyAsync(ctx->plan_tables.p, hp.p, off, hipMemcpyHostToDevice, s));
            ctx->plan_uploaded = off;
            ctx->plan_uploaded_to = ctx->plan_tables.p;
            ctx->plan_flip ^= 1; // (this block now holds what the device holds)
        }
        const char *d = (const char *)ctx->plan_tables.p;
        d_ranges = (const RangeTask *)(d + o_ranges);
        d_segs = (const SegDesc *)(d + o_segs);
        d_chunks = (const SegScanChunk *)(d + o_chunks);
        d_seg_blocks = (const SegBlock *)(d + o_blocks);
        d_supers = (const SegSuper *)(d + o_supers);
        d_small = (const PairTask *)(d + o_small);
        d_big = (const PairTask *)(d + o_big);

        if ((rc = ctx->plane_tasks.reserve(std::max<size_t>(1, pl.plane_tasks.size()) * sizeof(PlaneTask))) ||
            (rc = ctx->planes.reserve(std::max<uint64_t>(1, pl.plane_words) * sizeof(uint32_t))))
            return rc;
        return UMI_OK;
    }

    // the plan without the cross path: every segment's part 1 is filed and walked again
    void strip_cross()
    {
        for (SegDesc &sd : pl.segs) sd.cross = 0;
        for (SegSuper &su : pl.seg_supers) {
            su.cross = 0;
            su.map0 = 0;
        }
        pl.seg_cross = pl.seg_cross_words = 0;
    }
    // ... uploaded in place of the one the device holds (same sizes: the tables stay where they are)
    int upload_stripped_plan()
    {
        int rc;
        strip_cross();
        if ((rc = upload_plan())) return rc;
        seg.segs = d_segs;
        seg.chunks = d_chunks;
        seg.ranges = d_ranges;
        if (seg.blocks) seg.blocks = d_seg_blocks;
        if (seg.supers) seg.supers = d_supers;
        seg.cross_map = nullptr;
        seg.cross_pre = nullptr;
        return UMI_OK;
    }

    // what the segment index's kernels of this call work with (SegArgs over the uploaded tables): its workspace,
    // compare keys, super-bins, the local kernel and its probe, the LDS counting sort; the bin counters cleared
    int configure_seg()
    {
        int rc;
        memset(&seg, 0, sizeof(seg));
        if (pl.seg_parts && need_pairs) {
            if (pl.seg_task_cap > 0x7FFFFFF0ull / sizeof(SegTask) || pl.seg_bins > 0x7FFFFFF0ull ||
                pl.seg_entries * (uint64_t)pl.seg_parts > 0x7FFFFFF0ull)
                return fail(UMI_ERR_NOMEM, "segment index of this call too large (set seg_index=0)");
            const size_t m = (size_t)pl.seg_entries * (size_t)pl.seg_parts;
            if (pl.segs.size() >= (1u << 24)) return fail(UMI_ERR_NOMEM, "too many segments in one call (set seg_index=0)");
            // (the bin counters and, behind them, the scan's ticket and status words: one block, one memset)
            const size_t bins_bytes = seg_bins_bytes(), zero_bytes = seg_zero_bytes();
            if ((!zero_behind_control && (rc = ctx->seg_bin_cnt.reserve(zero_bytes))) ||
                (rc = ctx->seg_bin_start.reserve(pl.seg_bins * 4)) ||
                (rc = ctx->seg_tasks.reserve(pl.seg_task_cap * sizeof(SegTask))) ||
                (rc = ctx->seg_sub_rec.reserve(m * sizeof(SegRec32))))
                return rc;
            static_assert(sizeof(SegRec32) == 16 && sizeof(SegRec64) == 16, "one 16-byte store per record");
            seg.segs = d_segs;
            seg.chunks = d_chunks;
            seg.n_chunks = (uint32_t)pl.seg_chunks.size();
            seg.n_parts = pl.seg_parts;
            seg.bin_cnt = zero_behind_control ? (uint32_t *)((char *)ctx->counters.p + CTRL_BYTES) : ctx->seg_bin_cnt.as<uint32_t>();
            seg.bin_start = ctx->seg_bin_start.as<uint32_t>();
            seg.scan_state = (unsigned long long *)((char *)seg.bin_cnt + bins_bytes);
            seg.tasks = ctx->seg_tasks.as<SegTask>();
            seg.task_cap = (uint32_t)pl.seg_task_cap;
            seg.sub_rec = ctx->seg_sub_rec.p;
            seg.ranges = d_ranges;
            seg.n_ranges = (uint32_t)pl.ranges.size();
            seg.umi_len = plan_umi_len();
            seg.key_words = n_words;
            seg.full_umi_len = umi_len;
            seg.use_ckey = key32 && ctx->seg_ckey && pl.seg_max_rest <= 10 ? 1u : 0u;
            seg.col_sliced = ctx->seg_sliced ? 1u : 0u;
            // super-bins (the planner has set SegDesc::sup_g where the call's shape allows): the same kind of call as
            // the local kernel's below, whatever "seg_local" says
            const bool super_on = !pl.seg_supers.empty() && ctx->seg_unite && unions_collapse() && one_sync() && seg.use_ckey &&
                                  k == 1 && !d_nmask;
            if (super_on) {
                seg.super_cap = ctx->seg_super_cap;
                seg.supers = d_supers;
                seg.n_supers = (uint32_t)pl.seg_supers.size();
            }
            // part 0 in LDS: where the pair kernel would unite symmetric pairs on the spot (the batched
            // directional path, one device's whole call) and compares 32-bit compare keys
            if (ctx->seg_local && ctx->seg_unite && unions_collapse() && one_sync() && seg.use_ckey) {
                seg.local_cap = ctx->seg_local_cap;
                seg_local_bins = 0;
                for (const SegDesc &sd : pl.segs) seg_local_bins += 1ull << (2 * sd.nb[0]);
                if (super_on && pl.seg_plain == 0) seg_local_bins = 0; // (every segment has super-bins: nothing for it)
                // k = 1 without N: inside a bin every pair within k differs in one base outside the bin's own,
                // and no two entries agree there (with N folded onto A they could)
                if (ctx->seg_probe && k == 1 && !d_nmask) {
                    seg.probe_rest = SEG_PROBE_MAX_REST;
                    seg.probe_min = ctx->seg_probe_min;
                }
            }
            if (ctx->seg_lds && pl.seg_max_bins <= SEG_LDS_BINS && !pl.seg_blocks.empty()) {
                seg.blocks = d_seg_blocks;
                seg.n_blocks = (uint32_t)pl.seg_blocks.size();
                seg.lds_bins = pl.seg_max_bins;
                seg.parts_per_pass = std::max(1u, std::min({4u, (uint32_t)pl.seg_parts, SEG_LDS_BINS / std::max(1u, pl.seg_max_bins)}));
                // (the per-entry path of the counting sort files by fine bin, prep_kernel's histogram with it)
                seg.super_coarse = super_on && ctx->seg_super_coarse ? 1u : 0u;
            }
            if (pl.seg_cross) {
                // the cross path: a call seg_super_kernel runs in, part 0 filed by super-bin
                if (!(super_on && seg.super_coarse)) {
                    if ((rc = upload_stripped_plan())) return rc;
                } else {
                    if ((rc = ctx->seg_cross_maps.reserve(pl.seg_cross_words * (sizeof(uint32_t) + sizeof(uint16_t))))) return rc;
                    seg.cross_map = ctx->seg_cross_maps.as<uint32_t>();
                    seg.cross_pre = (uint16_t *)(seg.cross_map + pl.seg_cross_words);
                }
            }
            if (!zero_behind_control) HIP_TRY(hipMemsetAsync(seg.bin_cnt, 0, zero_bytes, s));
        } else if (pl.seg_cross) {
            strip_cross(); // (no kernel of the index runs: nothing on the device reads the bits)
        }
        return UMI_OK;
    }

    // control block, bucket table
    // fuse: the table is walked in a few pieces, each uploaded and handed to the fused kernel while
    // the host walks the next (a batch of 10^5 small positions: the walk and the 0.8 MB copy are
    // what the kernel would otherwise wait for)
    int upload_table(bool fuse)
    {
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[0], s));
        HIP_TRY(hipMemsetAsync(d_cnt, 0, CTRL_BYTES + zero_behind_control, s));
        // the bucket table goes through a pinned buffer: a true async DMA instead of the
        // runtime's staged copy of pageable memory (it is on the critical path of prep)
        int rc;
        if ((rc = ctx->h_boff.reserve((n_buckets + 1) * 8))) return rc;
        uint64_t *h_boff = ctx->h_boff.as<uint64_t>();
        if (mode == MODE_ADJACENCY && need_pairs) {
            HIP_TRY(hipMemsetAsync(ctx->status.p, 0, n, s));
            HIP_TRY(hipMemsetAsync(ctx->blocked.p, 0, n, s));
        }
        // What stands between the call and the first kernel is kept short: copy and monotonicity
        // (a table that steps backwards must not reach the device).  The counters and the list of
        // buckets beyond the fused kernel's reach are gathered by plan_host, behind the launch.
        TablePass &tp = ctx->table_pass;
        scan_table_reset(tp);
        const uint64_t pieces = fuse && fused_max >= 1 ? ctx->table_pieces : 1;
        h_boff[0] = bucket_off[0];
        for (uint64_t c = 0; c < pieces; c++) {
            const uint64_t b0 = n_buckets * c / pieces, b1 = n_buckets * (c + 1) / pieces;
            uint64_t prev = bucket_off[b0], back = 0;
            if (d_boff_caller) {
                // The table is on the device already: nothing to copy, and nothing to look at before
                // the launch either -- the fused kernel refuses entries that step backwards or lead
                // outside the arrays by itself, and the host's walk behind the launch (plan_host)
                // notes the first such bucket: run_stages fails the call on it.
            } else {
                for (uint64_t b = b0; b < b1; b++) {
                    const uint64_t v = bucket_off[b + 1];
                    back |= v < prev;
                    h_boff[b + 1] = prev = v;
                }
            }
            if (back) {
                for (uint64_t b = b0; b < b1; b++)
                    if (bucket_off[b + 1] < bucket_off[b])
                        return fail(UMI_ERR_ARG, "bucket_off not monotone at bucket %llu", (unsigned long long)b);
            }
            if (!d_boff_caller)
                HIP_TRY(hipMemcpyAsync(ctx->boff.as<uint64_t>() + b0, h_boff + b0, (b1 - b0 + 1) * 8,
                                       hipMemcpyHostToDevice, s));
            if (fuse && b1 > b0 && (rc = fused_stage(b0, b1))) return rc;
        }
        return UMI_OK;
    }

    // buckets [b0, b1) of the table
    int fused_stage(uint64_t b0, uint64_t b1)
    {
        if (fused_max < 1 || b1 <= b0) return UMI_OK;
        if (prof && !fused_ran) HIP_TRY(hipEventRecord(ctx->ev[5], s));
        // (label[] of a bucket the fused kernel finishes is read by nobody on the one-synchronisation
        // path -- its collapse covers the other buckets' ranges only: the store is left out there)
        const bool need_label = collapse_walks_all_labels() || !((unions_collapse() || !need_pairs) && n_parts == 1);
        if (wide())
            HIP_TRY(launch_small_buckets_wide(d_keys, d_nmask, n_words, d_freq, percentage, d_boff() + b0, (uint32_t)(b1 - b0),
                                              fused_max, n, d_kept, d_root, k, umi_len, d_cnt,
                                              (uint32_t)ctx->n_cus * ctx->fused_blocks, s));
        else
        HIP_TRY(launch_small_buckets(d_keys, d_nmask, d_freq, percentage, d_boff() + b0,
                                     (uint32_t)(b1 - b0), fused_max, n, need_label ? ctx->label.as<uint32_t>() : nullptr, d_kept,
                                     d_root, k, umi_len, ctx->fused_sliced, mode, adj_max_freq, d_cnt,
                                     (uint32_t)ctx->n_cus * ctx->fused_blocks, s));
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[6], s));
        if (!fused_ran) st.n_pair_launches += 1;
        fused_ran = true;
        return UMI_OK;
    }

    // filter keys / thresholds / labels / contract check of the entries the fused kernel left;
    // the entries of a segment also count themselves into the bins of its parts
    int prep_stage()
    {
        if (edit) {
            HIP_TRY(launch_edit_prep(d_keys, d_nmask, d_freq, d_boff(), n_buckets, n, umi_len, percentage,
                                     ctx->fkey.as<uint64_t>(), ctx->planes.as<uint32_t>(), ctx->thr.as<int32_t>(),
                                     ctx->label.as<uint32_t>(), d_cnt, s));
            if (prep_lab()) HIP_TRY(launch_iota(prep_lab(), n, s)); // (that entry kernel knows no lab[])
            return UMI_OK;
        }
        // With the LDS counting sort the segments' entries are prepared by its count kernel; the
        // entry kernel keeps the other buckets' ranges (none at all for a call of deep positions:
        // only the rises at bucket starts are left to count)
        const bool fold = seg.blocks != nullptr;
        if (fold) {
            seg.prep_keys = d_keys;
            seg.prep_nmask = d_nmask;
            seg.prep_freq = d_freq;
            seg.prep_thr = ctx->thr.as<int32_t>();
            seg.prep_label = ctx->label.as<uint32_t>();
            seg.prep_lab = prep_lab();
            seg.prep_percentage = percentage;
            seg.prep_counters = d_cnt;
        }
        bool other_ranges = false;
        for (const RangeTask &r : pl.ranges) other_ranges = other_ranges || r.seg == SEG_NONE;
        HIP_TRY(launch_prep(d_keys, d_nmask, d_freq, d_boff(), n_buckets, d_ranges,
                            (uint32_t)pl.ranges.size(), n, fused_max, plan_umi_len(), percentage, key32, ctx->fkey.p,
                            ctx->thr.as<int32_t>(), ctx->label.as<uint32_t>(), prep_lab(), d_cnt,
                            seg.n_chunks && !seg.blocks ? d_segs : nullptr, pl.seg_parts, seg.bin_cnt, s, fold,
                            !fold || other_ranges, std::max({ctx->seg_min, fused_max + 1, 1u}), n_words, umi_len));
        return UMI_OK;
    }

    // ---- the development build's stages, and what the shipped build has in their place -----------------
    // The bit-sliced tile kernels of the earlier versions (options bs_sorted / bs_tables / prune,
    // k > the segment index's reach, seg_index = 0) keep their own overflow list, which the host
    // has to look at between the pair stage and the collapse.
#ifdef UMIHIP_DEV
    bool legacy_tiles() const { return pl.n_bs() || !pl.tab_rows.empty(); }
    // (the tile kernels' collapse variants walk label[] of every entry, the fused buckets' too)
    static constexpr bool collapse_walks_all_labels() { return true; }

    // the large buckets' keys sorted (or pruned), their tile tasks cut
    int cut_legacy_tiles()
    {
        int rc;
        if (prune) return prune_stage();
        // the sorts are enqueued first: the host cuts the tile tasks (tens of thousands for a
        // deep position) while they run
        if (need_pairs && pl.any_sorted() && (rc = sort_stage())) return rc;
        gen_bs_tasks(pl, umi_len, ctx->bs_col_chunk, k, nullptr, key32);
        for (auto &v : pl.bs_tasks) keep_my_share(v);
        return UMI_OK;
    }

    // optional: sort every large bucket by filter key, read back the keys at the tile
    // boundaries, keep only the tile tasks whose key ranges can still hold a pair within k
    int prune_stage()
    {
        const size_t ksz = key32 ? 4 : 8;
        size_t tmp_bytes = 0, n_pos = 0;
        for (auto &bb : pl.bs_buckets) {
            tmp_bytes = std::max(tmp_bytes, sort_temp_bytes(key32, (uint32_t)(bb.e - bb.s), key_bits()));
            n_pos += (bb.e - bb.s + BS_COL_TILE - 1) / BS_COL_TILE + 1;
        }
        int rc;
        if ((rc = ctx->fkey_sorted.reserve((size_t)n * ksz)) || (rc = ctx->perm.reserve((size_t)n * 4)) ||
            (rc = ctx->iota.reserve((size_t)n * 4)) || (rc = ctx->sort_tmp.reserve(tmp_bytes)) ||
            (rc = ctx->sample_pos.reserve(n_pos * 4)) || (rc = ctx->sample_out.reserve(n_pos * 8)))
            return rc;
        std::vector<uint32_t> pos;
        pos.reserve(n_pos);
        for (auto &bb : pl.bs_buckets) {
            HIP_TRY(sort_bucket(ctx->fkey.p, key32, 0, key_bits(), (uint32_t)bb.s, (uint32_t)(bb.e - bb.s),
                                ctx->fkey_sorted.p, ctx->perm.as<uint32_t>(),
                                ctx->iota.as<uint32_t>(), ctx->sort_tmp.p, tmp_bytes, s));
            for (uint64_t q = bb.s; q < bb.e; q += BS_COL_TILE) pos.push_back((uint32_t)q);
            pos.push_back((uint32_t)(bb.e - 1));
        }
        std::vector<uint64_t> flat(pos.size());
        HIP_TRY(hipMemcpyAsync(ctx->sample_pos.p, pos.data(), pos.size() * 4, hipMemcpyHostToDevice, s));
        HIP_TRY(gather_keys(ctx->fkey_sorted.p, key32, ctx->sample_pos.as<uint32_t>(),
                            (uint32_t)pos.size(), ctx->sample_out.as<uint64_t>(), s));
        HIP_TRY(hipMemcpyAsync(flat.data(), ctx->sample_out.p, pos.size() * 8, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        std::vector<std::vector<uint64_t>> samples(pl.bs_buckets.size());
        size_t o = 0;
        for (size_t bi = 0; bi < pl.bs_buckets.size(); bi++) {
            const size_t cnt =
                (pl.bs_buckets[bi].e - pl.bs_buckets[bi].s + BS_COL_TILE - 1) / BS_COL_TILE + 1;
            samples[bi].assign(flat.begin() + o, flat.begin() + o + cnt);
            o += cnt;
        }
        gen_bs_tasks(pl, umi_len, ctx->bs_col_chunk, k, &samples, key32);
        for (auto &v : pl.bs_tasks) keep_my_share(v);
        bs_fkey = ctx->fkey_sorted.p;
        bs_perm = ctx->perm.as<uint32_t>();
        return UMI_OK;
    }

    // Buckets whose tiles reuse the counter state of the high units along runs of columns are
    // sorted by filter key (the runs come from the order); the other large buckets keep their
    // order behind an identity permutation, so that one pair of arrays serves every tile.
    int sort_stage()
    {
        const size_t ksz = key32 ? 4 : 8;
        size_t tmp_bytes = 0;
        bool all = true;
        for (auto &bb : pl.bs_buckets) {
            if (bb.pu || bb.live) tmp_bytes = std::max(tmp_bytes, sort_temp_bytes(key32, (uint32_t)(bb.e - bb.s), key_bits()));
            else all = false;
        }
        int rc;
        // + 64 B: the table kernel reads column keys a group ahead of the chunk it works on
        if ((rc = ctx->fkey_sorted.reserve((size_t)n * ksz + 64)) || (rc = ctx->perm.reserve((size_t)n * 4)) ||
            (rc = ctx->iota.reserve((size_t)n * 4)) || (rc = ctx->sort_tmp.reserve(tmp_bytes)))
            return rc;
        if (!all) {
            HIP_TRY(hipMemcpyAsync(ctx->fkey_sorted.p, ctx->fkey.p, (size_t)n * ksz, hipMemcpyDeviceToDevice, s));
            HIP_TRY(launch_iota(ctx->perm.as<uint32_t>(), n, s));
        }
        for (auto &bb : pl.bs_buckets)
            if (bb.pu || bb.live) {
                // The scan + item walk never look at the order inside a column run: the two live
                // units (8 bits) can stay unsorted, one radix pass less.  Only on the onesweep
                // path (the library's merge path for smaller inputs gets the full key).
                const int begin_bit = bb.live && sort_is_onesweep((uint32_t)(bb.e - bb.s)) ? 4 * bb.live : 0;
                HIP_TRY(sort_bucket(ctx->fkey.p, key32, begin_bit, key_bits(), (uint32_t)bb.s, (uint32_t)(bb.e - bb.s),
                                    ctx->fkey_sorted.p, ctx->perm.as<uint32_t>(),
                                    ctx->iota.as<uint32_t>(), ctx->sort_tmp.p, tmp_bytes, s));
            }
        bs_fkey = ctx->fkey_sorted.p;
        bs_perm = ctx->perm.as<uint32_t>();
        return UMI_OK;
    }

    // bit-sliced tile tasks + bit planes of the large buckets the segment index does not take
    int upload_legacy_tiles()
    {
        if (!(need_pairs && legacy_tiles())) return UMI_OK;
        int rc;
        if (pl.tab_items_max > 0x7FFFFFF0ull / sizeof(TabItem))
            return fail(UMI_ERR_NOMEM, "item list of the table kernel too large (set bs_tables=0)");
        if ((rc = ctx->bs_tasks.reserve(pl.n_bs() * sizeof(BsTask))) ||
            (rc = ctx->tab_rows.reserve(pl.tab_rows.size() * sizeof(TabRowTile))) ||
            (rc = ctx->tab_items.reserve(pl.tab_items_max * sizeof(TabItem))))
            return rc;
        // through a pinned buffer (the runtime's staged copy of pageable memory runs at a
        // fifth of the DMA rate and holds the stream meanwhile)
        const size_t bs_bytes = pl.n_bs() * sizeof(BsTask);
        const size_t plane_bytes = pl.plane_tasks.size() * sizeof(PlaneTask);
        const size_t row_bytes = pl.tab_rows.size() * sizeof(TabRowTile);
        if ((rc = ctx->h_tasks.reserve(bs_bytes + plane_bytes + row_bytes))) return rc;
        const char *h = ctx->h_tasks.p;
        size_t off = 0;
        for (auto &v : pl.bs_tasks) {
            if ((rc = ctx->h_tasks.put(off, v.data(), v.size() * sizeof(BsTask)))) return rc;
            off += v.size() * sizeof(BsTask);
        }
        if (row_bytes) {
            if ((rc = ctx->h_tasks.put(bs_bytes + plane_bytes, pl.tab_rows.data(), row_bytes))) return rc;
            HIP_TRY(hipMemcpyAsync(ctx->tab_rows.p, h + bs_bytes + plane_bytes, row_bytes, hipMemcpyHostToDevice, s));
        }
        if ((rc = ctx->h_tasks.put(bs_bytes, pl.plane_tasks.data(), plane_bytes))) return rc;
        if (bs_bytes) HIP_TRY(hipMemcpyAsync(ctx->bs_tasks.p, h, bs_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(ctx->plane_tasks.p, h + bs_bytes, plane_bytes, hipMemcpyHostToDevice, s));
        HIP_TRY(launch_build_planes(bs_fkey, key32, ctx->plane_tasks.as<PlaneTask>(),
                                    (uint32_t)pl.plane_tasks.size(), ctx->planes.as<uint32_t>(),
                                    umi_len, s));
        return UMI_OK;
    }

    // the call's arguments as the bit-sliced tiles and their overflow list take them: cut from the key-sorted arrays
    PairArgs legacy_args(const PairArgs &a) const
    {
        PairArgs b = a;
        b.fkey = bs_fkey;
        b.perm = bs_perm;
        return b;
    }
    int enqueue_legacy_tiles(const PairArgs &a)
    {
        const PairArgs b = legacy_args(a);
        if (!pl.tab_rows.empty()) // the table variant first (the largest buckets)
            HIP_TRY(launch_bs_tab(b, ctx->tab_rows.as<TabRowTile>(), (uint32_t)pl.tab_rows.size(),
                                  ctx->tab_items.as<TabItem>(), (uint32_t)pl.tab_items_max, umi_len, part,
                                  n_parts,
                                  ctx->bs_tab_waves ? ctx->bs_tab_waves
                                                    : (ctx->bs_transposed ? 128u : 16u) * (uint32_t)ctx->n_cus,
                                  ctx->bs_transposed, s));
        size_t first = pl.n_bs();
        for (int li = 3; li >= 0; li--) { // lists sit in the device array in index order
            first -= pl.bs_tasks[li].size();
            PairArgs w = b;
            w.bs_tasks = b.bs_tasks + first;
            HIP_TRY(launch_bs_pairs(w, (uint32_t)pl.bs_tasks[li].size(), li != 0, key32, umi_len,
                                    ctx->bs_unit, li == 2 ? 3 : (li == 3 ? 4 : 0), s));
        }
        return UMI_OK;
    }
    // the n_ovf filter hits on the tiles' overflow list, checked one by one (of the arguments the kernel reads
    // the keys, the lists and their counters only: no task list, no planes)
    int verify_overflow(uint64_t n_ovf, uint64_t ovf_cap)
    {
        HIP_TRY(launch_verify_list(legacy_args(pair_args(ovf_cap)), key32, (uint32_t)n_ovf, s));
        st.n_pair_launches += 1;
        return read_control();
    }
#else
    bool legacy_tiles() const { return false; }
    static constexpr bool collapse_walks_all_labels() { return false; }
    static int cut_legacy_tiles() { return UMI_OK; }
    static int upload_legacy_tiles() { return UMI_OK; }
    static int enqueue_legacy_tiles(const PairArgs &) { return UMI_OK; }
    static int verify_overflow(uint64_t, uint64_t) { return UMI_OK; }
#endif

    // tile tasks of the call's pair kernels; what the plan says they evaluate
    int count_tasks()
    {
        n_tasks = pl.small_tasks.size() + pl.big_tasks.size() + pl.n_bs() + pl.tab_rows.size() +
                  (pl.seg_parts ? 1 : 0);
        if (need_pairs) st.n_pairs_evaluated = edit ? pl.n_pairs : pl.n_pairs_eval; // (edit: no tile padding counted)
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[1], s));
        return UMI_OK;
    }

    // lists the pair kernels append to
    int reserve_lists(uint64_t cap, uint64_t &ovf_cap)
    {
        int rc;
        if (cap > 0x7FFFFFF0ull) return fail(UMI_ERR_NOMEM, "edge list too large");
        if ((rc = ctx->edges.reserve(cap * sizeof(uint2)))) return rc;
        if (mode == MODE_NEIGHBOURS && (rc = ctx->edge_dist.reserve(cap))) return rc;
        cap_used = (uint32_t)cap;
        ovf_cap = std::min<uint64_t>(std::max<uint64_t>(ctx->ovf_capacity, 1024), 0x7FFFFFF0ull);
        if (legacy_tiles() && (rc = ctx->ovf.reserve(ovf_cap * sizeof(uint2)))) return rc;
        return UMI_OK;
    }

    // resident one-wave blocks per CU of the segment index's pair kernel variant in use (asked of the
    // runtime once per variant and context; capped at 16, four waves per SIMD: the kernel is bound by
    // VALU issue and by the unions' trips to memory, and config 2 takes the same time with 16, 22 or
    // 24 blocks per CU.  The runtime's answer is an upper bound only: it says 28 for the 39-register
    // variant, but of 26 blocks per CU the last start only when the first have left -- s_memrealtime
    // stamps; 24 per CU are all running 1.5 us after the first -- and a late block of a persistent
    // grid does its whole share alone)
    uint32_t seg_occupancy()
    {
        const bool has_n = d_nmask != nullptr, ck = seg.use_ckey != 0;
        int &slot = ctx->seg_occ[key32 ? 1 : 0][has_n ? 1 : 0][ck ? 1 : 0];
        if (!slot) slot = seg_pair_blocks_per_cu(key32, has_n, ck);
        return (uint32_t)slot;
    }
    uint32_t seg_local_occupancy()
    {
        if (ctx->seg_local_occ_cap != seg.local_cap) {
            ctx->seg_local_occ[0] = ctx->seg_local_occ[1] = 0;
            ctx->seg_local_occ_cap = seg.local_cap;
        }
        int &slot = ctx->seg_local_occ[d_nmask != nullptr ? 1 : 0];
        if (!slot) slot = seg_local_blocks_per_cu(d_nmask != nullptr, seg.local_cap);
        return (uint32_t)slot;
    }

    // what every pair kernel of the call is handed
    PairArgs pair_args(uint64_t ovf_cap) const
    {
        PairArgs a;
        a.keys = d_keys;
        a.nmask = d_nmask;
        a.freq = d_freq;
        a.thr = ctx->thr.as<int32_t>();
        a.fkey = ctx->fkey.p;
        a.tasks = d_small;
        a.bs_tasks = ctx->bs_tasks.as<BsTask>();
        a.planes = ctx->planes.as<uint32_t>();
        a.perm = nullptr;
        a.edges = ctx->edges.as<uint2>();
        a.edge_dist = ctx->edge_dist.as<uint8_t>();
        a.counters = d_cnt;
        a.ovf = ctx->ovf.as<uint2>();
        a.ovf_cap = (uint32_t)ovf_cap;
        a.edge_cap = cap_used;
        a.k = k;
        a.mode = mode;
        a.adj_max_freq = adj_max_freq;
        a.n_entries = n;
        return a;
    }

    // all pair kernels of the call, largest work first (nothing waits on the host in here)
    int enqueue_pairs(uint64_t ovf_cap)
    {
        int rc;
        const PairArgs a = pair_args(ovf_cap);
        if (pl.seg_parts) { // the large buckets' sub-buckets: persistent one-wave blocks
            const uint32_t blocks = std::max(1u, (uint32_t)std::min<uint64_t>(
                pl.seg_task_cap, ctx->seg_blocks ? ctx->seg_blocks : (uint64_t)ctx->n_cus * std::min(16u, seg_occupancy())));
            // the local kernel's blocks (resident all at once, no more than there are part-0 bins) take
            // the first private slots, the pair kernel's the ones behind them
            const uint32_t local_blocks = seg.local_cap && seg_local_bins ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>(
                                                              seg_local_bins, (uint64_t)ctx->n_cus * seg_local_occupancy()))
                                                        : 0u;
            // ... and the super-bin kernel's waves the ones in between
            const uint32_t super_blocks = seg.super_cap ? seg_super_blocks(seg.n_supers, (uint32_t)ctx->n_cus) : 0u;
            const uint32_t super_slots = super_blocks * (seg_super_threads(seg.super_cap) / 64u);
            // ... then the pair kernel's, where a segment is left to it, and the cross kernel's (work items: 64-word
            // chunks of the super-bins' maps)
            const uint32_t pair_blocks = pl.seg_cross < pl.segs.size() ? blocks : 0u;
            const uint32_t cross_blocks = pl.seg_cross && super_blocks
                                              ? (uint32_t)std::max<uint64_t>(1, std::min<uint64_t>((uint64_t)seg.n_supers * SEG_CROSS_CHUNKS,
                                                    ctx->seg_blocks ? ctx->seg_blocks : (uint64_t)ctx->n_cus * 16u))
                                              : 0u;
            if (pl.seg_cross && !cross_blocks) return fail(UMI_ERR_HIP, "internal: cross segments planned without super-bins");
            const size_t slots = (size_t)local_blocks + super_slots + pair_blocks + cross_blocks;
            if ((rc = ctx->seg_priv_edges.reserve(slots * SEG_PRIV_CAP * sizeof(uint2))) ||
                (rc = ctx->seg_priv_cnt.reserve(slots * 4)) || (rc = ctx->seg_priv_stat.reserve(slots * sizeof(uint2))) ||
                (mode == MODE_NEIGHBOURS && (rc = ctx->seg_priv_dist.reserve((size_t)blocks * SEG_PRIV_CAP))))
                return rc;
            seg.priv_edges = ctx->seg_priv_edges.as<uint2>();
            seg.priv_dist = ctx->seg_priv_dist.as<uint8_t>();
            seg.priv_cnt = ctx->seg_priv_cnt.as<uint32_t>();
            seg.uf_parent = one_sync() && ctx->seg_unite ? ctx->label.as<uint32_t>() : nullptr;
            // the slots go to the collapse's flatten launch, which adds up the blocks' counts as well
            const bool slots_to_collapse = seg.uf_parent && unions_collapse();
            seg.priv_stat = slots_to_collapse ? ctx->seg_priv_stat.as<uint2>() : nullptr;
            if ((seg.local_cap || seg.super_cap) && !seg.uf_parent) // (the scan has left the local bins without tasks)
                return fail(UMI_ERR_HIP, "internal: part-0 sub-buckets planned for the local kernel without unions");
            SegArgs super_seg = seg;
            // (the scan ran once: a second attempt's launch must not count the fine bins' pairs again)
            super_seg.super_count_pairs = seg.super_coarse && !super_pairs_counted ? 1u : 0u;
            super_pairs_counted = super_pairs_counted || super_blocks != 0;
            super_seg.priv_edges += (size_t)local_blocks * SEG_PRIV_CAP;
            super_seg.priv_cnt += local_blocks;
            if (super_seg.priv_stat) super_seg.priv_stat += local_blocks;
            SegArgs pair_seg = super_seg;
            pair_seg.priv_edges += (size_t)super_slots * SEG_PRIV_CAP;
            pair_seg.priv_cnt += super_slots;
            if (pair_seg.priv_stat) pair_seg.priv_stat += super_slots;

            if (prof) HIP_TRY(hipEventRecord(ctx->ev[7], s));
            // (part 0's plain label stores all land before the pair kernel's first union: stream order)
            if (local_blocks) HIP_TRY(launch_seg_local(a, seg, percentage, local_blocks, s));
#ifdef UMIHIP_DEV
            // UMIHIP_SUPER_PHASES=<file>: the super-bin kernel's blocks stamp their phases, the call waits for them here
            // and appends the phases' mean and maximum over the blocks to the file (a measuring run, never a timed one)
            const char *phase_file = super_blocks ? getenv("UMIHIP_SUPER_PHASES") : nullptr;
            if (phase_file && *phase_file) {
                const size_t n_stamps = (size_t)super_blocks * SEG_SUPER_PHASES;
                HIP_TRY(hipMalloc((void **)&super_seg.super_stamps, n_stamps * sizeof(unsigned long long)));
                HIP_TRY(hipMemsetAsync(super_seg.super_stamps, 0, n_stamps * sizeof(unsigned long long), s));
            }
#endif
            if (super_blocks) HIP_TRY(launch_seg_super(a, super_seg, percentage, super_blocks, s));
#ifdef UMIHIP_DEV
            if (super_seg.super_stamps) {
                std::vector<unsigned long long> ticks((size_t)super_blocks * SEG_SUPER_PHASES);
                const hipError_t e = hipMemcpyAsync(ticks.data(), super_seg.super_stamps, ticks.size() * sizeof(unsigned long long),
                                                    hipMemcpyDeviceToHost, s);
                const hipError_t e2 = e == hipSuccess ? hipStreamSynchronize(s) : e;
                (void)hipFree(super_seg.super_stamps);
                HIP_TRY(e2);
                if (FILE *f = fopen(phase_file, "a")) {
                    static const char *const names[SEG_SUPER_PHASES] = {"records in", "map built", "ranks and placement",
                        "bit tests, pushes (w0)", "drains", "pointer jumping", "atomicMin", "label stores",
                        "fine-bin pairs counted"};
                    fprintf(f, "seg_super_kernel: %u blocks, us per block (100 MHz clock): phase, mean, max\n", super_blocks);
                    double sum_mean = 0;
                    for (int i = 0; i < SEG_SUPER_PHASES; i++) {
                        unsigned long long tot = 0, mx = 0;
                        for (uint32_t b = 0; b < super_blocks; b++) {
                            const unsigned long long t = ticks[(size_t)b * SEG_SUPER_PHASES + i];
                            tot += t;
                            mx = std::max(mx, t);
                        }
                        sum_mean += (double)tot / super_blocks / 100.0;
                        fprintf(f, "  %-22s %8.2f %8.2f\n", names[i], (double)tot / super_blocks / 100.0, (double)mx / 100.0);
                    }
                    fprintf(f, "  %-22s %8.2f\n", "all phases", sum_mean);
                    fclose(f);
                }
            }
#endif
            if (pair_blocks) HIP_TRY(launch_seg_pairs(a, pair_seg, key32, percentage, part, n_parts, pair_blocks, s));
            if (cross_blocks) {
                SegArgs cross_seg = pair_seg;
                cross_seg.priv_edges += (size_t)pair_blocks * SEG_PRIV_CAP;
                cross_seg.priv_cnt += pair_blocks;
                cross_seg.priv_stat += pair_blocks; // (cross segments: the slots go to the collapse)
                HIP_TRY(launch_seg_cross(a, cross_seg, percentage, cross_blocks, s));
                ctx->seg_cross_launches++;
            }
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[8], s));
            seg_timed = true;
            // what the blocks still hold in their private slots: one-way pairs only when the symmetric
            // ones were united where they were found, and then the collapse's flatten launch moves them
            // to the list (collapse_desc); else two small launches here, ahead of the list's unions
            priv_blocks_for_collapse = slots_to_collapse ? (uint32_t)slots : 0u;
            if (!priv_blocks_for_collapse) HIP_TRY(launch_seg_edge_append(a, seg, pair_blocks, s));
            st.n_pair_launches += 1;
        }
        if ((rc = enqueue_legacy_tiles(a))) return rc;
        if (edit) { // every bucket as 64-row chunks against its later entries, by edit distance
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[7], s));
            HIP_TRY(launch_edit_pairs(a, ctx->planes.as<uint32_t>(), (uint32_t)pl.small_tasks.size(), umi_len, s));
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[8], s));
            edit_timed = true;
            st.n_pair_launches += pl.small_tasks.empty() ? 0 : 1;
            return UMI_OK;
        }
        if (wide()) { // every bucket as 64-row chunks against its later entries
            HIP_TRY(launch_wide_pairs(a, (uint32_t)pl.small_tasks.size(), n_words, s));
            st.n_pair_launches += pl.small_tasks.empty() ? 0 : 1;
            return UMI_OK;
        }
        PairArgs big = a;
        big.tasks = d_big;
        HIP_TRY(launch_pairs(big, (uint32_t)pl.big_tasks.size(), true, key32, s));
        HIP_TRY(launch_pairs(a, (uint32_t)pl.small_tasks.size(), false, key32, s));
        for (auto &v : pl.bs_tasks) st.n_pair_launches += v.empty() ? 0 : 1;
        st.n_pair_launches += pl.tab_rows.empty() ? 0 : 2;
        st.n_pair_launches += (pl.small_tasks.empty() ? 0 : 1) + (pl.big_tasks.empty() ? 0 : 1);
        return UMI_OK;
    }

    // what the control block that has just been read says about the pair kernels' work
    int note_pair_counters()
    {
        n_edges = ctx->h_counters[CNT_EDGES] + ctx->h_counters[CNT_EDGES_MOVED];
        n_direct = ctx->h_counters[CNT_UF_DIRECT];
        seg_tasks_made = ctx->h_counters[CNT_SEG_TASKS];
        st.n_candidates = ctx->h_counters[CNT_CANDIDATES];
        st.n_pairs_evaluated = edit ? pl.n_pairs : pl.n_pairs_eval + ctx->h_counters[CNT_SEG_PAIRS];
        if (!pl.tab_rows.empty()) // the table kernel walks only the column tiles its scan kept
            st.n_pairs_evaluated = st.n_pairs_evaluated - pl.n_pairs_eval_tab +
                                   (ctx->h_counters[CNT_ITEMS] + ctx->h_counters[CNT_DIAG_ITEMS]) *
                                       (64ull * BS_TAB_G * 32) * BS_TAB_TILE;
        if (pl.seg_parts && seg_tasks_made > seg.task_cap)
            return fail(UMI_ERR_HIP, "internal: %llu segment tasks for a list of %u", (unsigned long long)seg_tasks_made, seg.task_cap);
        return UMI_OK;
    }

    // an attempt's lists were too short and its pair work is to be done again: the edge list as long as the count
    // that is known now (the context keeps it for its next call), the list's counters cleared.  What else the
    // attempt has counted or written is the caller's to reset, behind this
    int grow_edge_list(uint64_t &cap, int attempt)
    {
        if (attempt >= 3) return fail(UMI_ERR_HIP, "edge list overflow persists");
        if (n_edges > cap) {
            cap = n_edges + n_edges / 16 + 1024;
            ctx->edge_capacity = cap;
        }
        HIP_TRY(hipMemsetAsync(&d_cnt[CNT_EDGES], 0, 2 * sizeof(unsigned long long), s));
        return UMI_OK;
    }

    // all-pairs: fused small buckets straight to label[]/status[]; tile kernels to the edge list
    // (redone once with a larger list if it overflowed: the exact count is known by then)
    int pair_stage()
    {
        if (!(need_pairs && n_tasks)) {
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[2], s));
            return UMI_OK;
        }
        int rc;
        uint64_t cap = std::max<uint64_t>(ctx->edge_capacity, 1024);
        for (int attempt = 0;; attempt++) {
            uint64_t ovf_cap = 0;
            if ((rc = reserve_lists(cap, ovf_cap))) return rc;
            if ((rc = enqueue_pairs(ovf_cap))) return rc;
            if ((rc = read_control())) return rc;
            // filter hits that did not fit the blocks' LDS queues (very dense tiles): checked now,
            // or -- if their list ran over as well -- everything again with a longer list
            const uint64_t n_ovf = ctx->h_counters[CNT_OVF];
            const bool redo = n_ovf > ovf_cap;
            if (redo)
                ctx->ovf_capacity = n_ovf + n_ovf / 8 + 1024;
            else if (n_ovf && (rc = verify_overflow(n_ovf, ovf_cap)))
                return rc;
            if (prof && !redo) HIP_TRY(hipEventRecord(ctx->ev[2], s));
            if ((rc = note_pair_counters())) return rc;
            if (!redo && n_edges <= cap) break;
            if ((rc = grow_edge_list(cap, attempt))) return rc;
            HIP_TRY(hipMemsetAsync(&d_cnt[CNT_OVF], 0, 5 * sizeof(unsigned long long), s)); // and the item counters
        }
        st.n_edges = n_edges;
        return UMI_OK;
    }

    CollapseDesc collapse_desc() const
    {
        CollapseDesc d;
        d.parent = ctx->label.as<uint32_t>();
        d.lab = ctx->lab.as<uint32_t>();
        d.edges = ctx->edges.as<uint2>();
        d.edge_cap = cap_used;
        d.ranges = d_ranges;
        d.n_ranges = (uint32_t)pl.ranges.size();
        d.n = n;
        d.kept = d_kept;
        d.root = d_root;
        // (label[] then holds the unflattened forest when the call ends: nobody reads it across calls, every
        // call's prep / launch_iota writes its entries afresh)
        d.kept_only = mask_only_collapse();
        d.counters = d_cnt;
        d.changed = ctx->d_changed();
        if (priv_blocks_for_collapse) {
            d.priv_edges = seg.priv_edges;
            d.priv_cnt = seg.priv_cnt;
            d.priv_stat = seg.priv_stat;
            d.priv_blocks = priv_blocks_for_collapse;
        }
        return d;
    }

    // The batched paths with one synchronisation, everything enqueued behind one another and the control block
    // read once (the kernels read the edge count on the device).
    // Directional: pair kernels, union-find over the symmetric pairs, forest flattened, `ahead` rounds along the
    // one-way pairs, kept mask (a round is a no-op once the one before it was quiet).  What the host may find then:
    // the edge list ran over (longer list, pairs and collapse again), or the last round still moved a label (more
    // rounds, finalize again: directional_rounds_end).
    // Connected components (MODE_CLUSTER): pair kernels, the unions of whatever reached the list, one write-out.
    // Every pair within k is a union -- united where it was found or listed flagged -- so there is no one-way pair,
    // no lab[], no round and no check beside the write-out, and dag_rounds_ahead stays what the directional calls
    // made it.  What the host may find: the edge list ran over (longer list, pairs and write-out again).
    int run_one_sync()
    {
        int rc;
        const bool cluster = mode == MODE_CLUSTER;
        uint32_t *d_label = ctx->label.as<uint32_t>();
        const bool have_pairs = need_pairs && n_tasks;
        uint64_t cap = std::max<uint64_t>(ctx->edge_capacity, 1024);
        // rounds along the one-way pairs enqueued ahead of the host's look (the last as the check beside the
        // finalize pass): what the call before on this context needed -- a position of clusters (chains of
        // one-way pairs down a freq ladder) takes five or six where a uniform one takes three, and each look
        // of the host in between costs a wait and a second finalize pass
        const int ahead = std::min(std::max(ctx->dag_rounds_ahead, DAG_ROUNDS), MAX_ROUNDS_PER_SYNC);
        for (int attempt = 0;;) { // (attempt: the edge list's retries)
            launches_before_attempt = st.n_pair_launches;
            if (have_pairs) {
                uint64_t ovf_cap = 0;
                if ((rc = reserve_lists(cap, ovf_cap))) return rc;
                if ((rc = enqueue_pairs(ovf_cap))) return rc;
            }
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[2], s));
            // (symmetric) pairs in the list: those of the tile kernels, and the segment index's when it does
            // not unite them itself
            if (have_pairs && (!seg.uf_parent || legacy_tiles() || !pl.small_tasks.empty() || !pl.big_tasks.empty()))
                HIP_TRY(launch_uf_union_list(ctx->edges.as<uint2>(), d_cnt, cap_used, d_label, cap_used, s));
            if (prof && cluster) HIP_TRY(hipEventRecord(ctx->ev[3], s)); // (the write-out is that mode's finalize phase)
            if (!have_pairs) // no pair of this call reaches the edge list: every entry outside the fused buckets survives
                HIP_TRY(launch_finalize(d_label, d_ranges, (uint32_t)pl.ranges.size(), n, d_kept, d_root, d_cnt, s));
            else if (cluster)
                HIP_TRY(launch_cluster_write(collapse_desc(), s));
            else if ((rc = enqueue_directional_collapse(ahead)))
                return rc;
            if (prof && !cluster) HIP_TRY(hipEventRecord(ctx->ev[3], s));
            if (prof) HIP_TRY(hipEventRecord(ctx->ev[4], s));
            // (a call without pair work -- every position the fused kernel's -- has nothing left to decide
            // on the host: its end may be left to the caller)
            if (may_defer && !have_pairs && !prof && ctx->spin_wait) {
                st.n_pairs_evaluated = pl.n_pairs_eval;
                return defer_control();
            }
            if ((rc = read_control())) return rc;
            if ((rc = note_pair_counters())) return rc;
            // a super-bin the cross path could not serve (a key twice, a run above the cap): the pair work again without
            // the path, everything the attempt has counted or united reset as for the edge list's retry
            const bool abandoned = have_pairs && pl.seg_cross && ctx->h_counters[CNT_SEG_CROSS_ABANDONED] != 0;
            // (an abandoned attempt's edge count is a part of the call's: the list grows by the next attempt's, as it
            // does in a call without the path)
            const bool over = have_pairs && !abandoned && n_edges > cap;
            if (!abandoned && !over) break;
            if (over) {
                if ((rc = grow_edge_list(cap, attempt++))) return rc;
            } else {
                HIP_TRY(hipMemsetAsync(&d_cnt[CNT_EDGES], 0, 2 * sizeof(unsigned long long), s));
            }
            if (abandoned && (rc = drop_cross())) return rc;
            HIP_TRY(hipMemsetAsync(&d_cnt[CNT_KEPT], 0, sizeof(unsigned long long), s));
            HIP_TRY(hipMemsetAsync(&d_cnt[CNT_UF_DIRECT], 0, 2 * sizeof(unsigned long long), s));
            if (!cluster) HIP_TRY(hipMemsetAsync(ctx->d_changed(), 0, CTRL_BYTES - CTRL_FLAGS_OFF, s)); // flags and sync words
            HIP_TRY(launch_iota(d_label, n, s)); // (the fused buckets' entries are finished: their labels are free)
            if (prep_lab()) HIP_TRY(launch_iota(prep_lab(), n, s)); // (the attempt's round 0 has lowered it)
        }
        st.n_edges = n_edges + n_direct;
        if (cluster)
            st.n_rounds = have_pairs && st.n_edges ? 1u : 0u; // (the union pass)
        else if ((rc = directional_rounds_end(have_pairs, ahead)))
            return rc;
        return finish_stats();
    }

    // The cross path's fallback: the context plans without it from now on ("seg_cross" arms it again), the plan's
    // cross bits are cleared, and the index is built again with part 1 -- the entries are prepared, so the count kernel
    // only counts.  The abandoned attempt's launch is not one of the call's.
    int drop_cross()
    {
        int rc;
        ctx->seg_cross_failed = true;
        if ((rc = upload_stripped_plan())) return rc;
        seg.prep_keys = nullptr;
        HIP_TRY(hipMemsetAsync(seg.bin_cnt, 0, seg_zero_bytes(), s));
        static_assert(CNT_SEG_PAIRS == CNT_SEG_TASKS + 1, "one fill");
        HIP_TRY(hipMemsetAsync(&d_cnt[CNT_SEG_TASKS], 0, 2 * sizeof(unsigned long long), s));
        HIP_TRY(hipMemsetAsync(&d_cnt[CNT_SEG_CROSS_ABANDONED], 0, sizeof(unsigned long long), s));
        HIP_TRY(launch_seg_build(seg, ctx->fkey.p, d_freq, key32, d_cnt, s));
        super_pairs_counted = false;
        st.n_pair_launches = launches_before_attempt; // (every pair launch of the attempt: the tiles of mid-size buckets too)
        ctx->seg_cross_abandoned_calls++;
        return UMI_OK;
    }

    // the directional collapse behind the unions: forest flattened, ahead - 1 rounds, finalize with the check round
    int enqueue_directional_collapse(int ahead)
    {
        const CollapseDesc cd = collapse_desc();
        HIP_TRY(launch_collapse_flatten(cd, s));
        // (the last of them as a check beside the finalize pass: in the common case it would change
        // nothing, and the kept mask stands)
        // (kept_only: the flatten launch is round 0 -- it resolves the one-way pairs' endpoints for the rounds
        // and the check behind it)
        static_assert(DAG_ROUNDS >= 2, "the check beside finalize needs a resolving round ahead of it");
        for (int r = cd.kept_only ? 1 : 0; r < ahead - 1; r++) HIP_TRY(launch_collapse_round(cd, r, s));
        HIP_TRY(launch_collapse_finalize(cd, s, ahead - 1));
        return UMI_OK;
    }

    // ... and what the control block says of its rounds: how many ran, and more of them where the check still
    // moved a label
    int directional_rounds_end(bool have_pairs, int ahead)
    {
        int rc;
        int rounds = have_pairs && st.n_edges ? 1 : 0;
        for (int r = 0; have_pairs && r < ahead; r++) rounds += (r == 0 || ctx->h_changed()[r - 1]) ? 1 : 0;
        const int rounds_first = rounds;
        if (have_pairs && ctx->h_changed()[ahead - 1]) { // a deeper chain of one-way pairs than that
            // (comp[] is flat -- kept_only: the list holds roots -- and lab[] only ever falls: the rounds go on
            // where the first ones stopped; their index restarts at 0 here, and none of them resolves again)
            const CollapseDesc cd = collapse_desc();
            if ((rc = run_rounds(ctx, s, [&](uint32_t *, int r) { return launch_collapse_round(cd, r, s); }, rounds, 4)))
                return rc;
            HIP_TRY(hipMemsetAsync(&d_cnt[CNT_KEPT], 0, sizeof(unsigned long long), s));
            HIP_TRY(launch_collapse_finalize(cd, s));
            if ((rc = read_control())) return rc;
        }
        // (rounds = 1 for the union-find pass + the rounds that ran, the last of them quiet)
        if (have_pairs) ctx->dag_rounds_ahead = std::max(DAG_ROUNDS, (rounds > rounds_first ? rounds : rounds_first) - 1);
        st.n_rounds = (uint32_t)rounds;
        return UMI_OK;
    }

    int finish_neighbours()
    {
        if (!(need_pairs && n_tasks)) { // pair_stage did not read the counters back
            int rc = read_control();
            if (rc) return rc;
        }
        drained = true;
        if (prof) {
            // (the pair stage records its end marker after its last synchronisation)
            HIP_TRY(hipEventSynchronize(ctx->ev[2]));
            HIP_TRY(hipEventElapsedTime(&st.ms_prep, ctx->ev[0], ctx->ev[1]));
            HIP_TRY(hipEventElapsedTime(&st.ms_pairs, ctx->ev[1], ctx->ev[2]));
            st.ms_total = st.ms_prep + st.ms_pairs;
        }
        return UMI_OK;
    }

    // min-rank label propagation to the fixed point: rounds are enqueued in growing batches,
    // each round skips itself on the device once the previous one changed nothing
    int collapse_directional()
    {
        if (n_edges) {
            int rounds = 0;
            const int rc = directional_labels(ctx, ctx->edges.as<uint2>(), d_cnt, cap_used, n_edges, n, s, rounds);
            if (rc) return rc;
            st.n_rounds = (uint32_t)rounds;
        }
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[3], s));
        HIP_TRY(launch_finalize(ctx->label.as<uint32_t>(), d_ranges, (uint32_t)pl.ranges.size(), n,
                                d_kept, d_root, d_cnt, s));
        return UMI_OK;
    }

    // adjacency with max_freq >= 1 (status[] and blocked[]: cleared in upload_table)
    int collapse_adjacency()
    {
        int iters = 0;
        const int rc = adjacency_status(ctx, ctx->edges.as<uint2>(), d_cnt, cap_used, n_edges, n, s, iters);
        if (rc) return rc;
        st.n_rounds = (uint32_t)iters;
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[3], s));
        HIP_TRY(launch_adj_finalize(ctx->status.as<uint8_t>(), ctx->label.as<uint32_t>(), d_ranges,
                                    (uint32_t)pl.ranges.size(), n, d_kept, d_root, d_cnt, s));
        return UMI_OK;
    }

    int finish()
    {
        if (prof) HIP_TRY(hipEventRecord(ctx->ev[4], s));
        int rc = read_control();
        if (rc) return rc;
        return finish_stats();
    }

    // (the control block has just been read and the stream is idle)
    int finish_stats()
    {
        drained = true;
        st.n_kept = ctx->h_counters[CNT_KEPT] + ctx->h_counters[CNT_KEPT_FUSED];
        if (prof) {
            hipEvent_t *ev = ctx->ev;
            HIP_TRY(hipEventElapsedTime(&st.ms_prep, ev[0], ev[1]));
            HIP_TRY(hipEventElapsedTime(&st.ms_pairs, ev[1], ev[2]));
            if (fused_ran) { // the fused kernel ran inside the prep window
                float ms_fused = 0.0f;
                HIP_TRY(hipEventElapsedTime(&ms_fused, ev[5], ev[6]));
                st.ms_prep -= ms_fused;
                st.ms_pairs += ms_fused;
            }
            HIP_TRY(hipEventElapsedTime(&st.ms_collapse, ev[2], ev[3]));
            HIP_TRY(hipEventElapsedTime(&st.ms_finalize, ev[3], ev[4]));
            HIP_TRY(hipEventElapsedTime(&st.ms_total, ev[0], ev[4]));
            // the kernel that does the call's pair work, by itself: the segment index's pair kernel
            // where a deep position is in the call, else the fused small-bucket kernel
            if (edit_timed) {
                HIP_TRY(hipEventElapsedTime(&st.ms_kernel, ev[7], ev[8]));
                st.kernel_id = UMI_KERNEL_EDIT_PAIRS;
            } else if (seg_timed) {
                HIP_TRY(hipEventElapsedTime(&st.ms_kernel, ev[7], ev[8]));
                st.kernel_id = UMI_KERNEL_SEG_PAIRS;
            } else if (fused_ran) {
                HIP_TRY(hipEventElapsedTime(&st.ms_kernel, ev[5], ev[6]));
                st.kernel_id = UMI_KERNEL_FUSED;
            }
        }
        return UMI_OK;
    }
};

// Collapse of an edge list that is already on the device (the multi-GPU split gathers the
// ranks' partial lists into one): labels start as the identity, then the same propagation /
// greedy passes as the single-call pipeline.
class EdgeCollapse {
  public:
    EdgeCollapse(umi_ctx *ctx, uint32_t n, const uint2 *d_edges, uint32_t n_edges, int mode,
                 uint8_t *d_kept, uint32_t *d_root, hipStream_t s)
        : ctx(ctx), n(n), d_edges(d_edges), n_edges(n_edges), mode(mode), d_kept(d_kept),
          d_root(d_root), s(s)
    {
    }
    int run(umi_stats *stats)
    {
        HIP_TRY(hipSetDevice(ctx->device));
        int rc = stages(stats);
        (void)hipStreamSynchronize(s);
        return rc;
    }

  private:
    umi_ctx *ctx;
    uint32_t n;
    const uint2 *d_edges;
    uint32_t n_edges;
    int mode;
    uint8_t *d_kept;
    uint32_t *d_root;
    hipStream_t s;

    int stages(umi_stats *stats)
    {
        int rc;
        if ((rc = ctx->label.reserve((size_t)n * 4)) || (rc = ctx->counters.reserve(CTRL_BYTES)))
            return rc;
        if (mode == MODE_ADJACENCY && ((rc = ctx->status.reserve(n)) || (rc = ctx->blocked.reserve(n))))
            return rc;
        unsigned long long *d_cnt = ctx->counters.as<unsigned long long>();
        memset(ctx->h_counters, 0, CNT_COUNT * sizeof(unsigned long long));
        ctx->h_counters[CNT_EDGES] = n_edges;
        HIP_TRY(hipMemcpyAsync(d_cnt, ctx->h_counters, CNT_COUNT * sizeof(unsigned long long),
                               hipMemcpyHostToDevice, s));
        HIP_TRY(launch_iota(ctx->label.as<uint32_t>(), n, s));
        umi_stats st;
        memset(&st, 0, sizeof(st));
        st.n_umis = n;
        st.n_edges = n_edges;
        if (mode == MODE_CLUSTER) { // every listed pair is a union (flagged: one without the flag is not looked at)
            if (n_edges) {
                HIP_TRY(launch_uf_union_list(d_edges, d_cnt, n_edges, ctx->label.as<uint32_t>(), n_edges, s));
                st.n_rounds = 1;
            }
            CollapseDesc cd{};
            cd.parent = ctx->label.as<uint32_t>();
            cd.n = n;
            cd.kept = d_kept;
            cd.root = d_root;
            cd.kept_only = d_root == nullptr && ctx->collapse_kept_only;
            cd.counters = d_cnt;
            HIP_TRY(launch_cluster_write(cd, s));
        } else if (mode == MODE_DIRECTIONAL) {
            if (n_edges) {
                int rounds = 0;
                if ((rc = directional_labels(ctx, d_edges, d_cnt, n_edges, n_edges, n, s, rounds))) return rc;
                st.n_rounds = (uint32_t)rounds;
            }
            HIP_TRY(launch_finalize(ctx->label.as<uint32_t>(), nullptr, 0, n, d_kept, d_root, d_cnt, s));
        } else {
            HIP_TRY(hipMemsetAsync(ctx->status.p, 0, n, s));
            HIP_TRY(hipMemsetAsync(ctx->blocked.p, 0, n, s));
            int iters = 0;
            if ((rc = adjacency_status(ctx, d_edges, d_cnt, n_edges, n_edges, n, s, iters))) return rc;
            st.n_rounds = (uint32_t)iters;
            HIP_TRY(launch_adj_finalize(ctx->status.as<uint8_t>(), ctx->label.as<uint32_t>(), nullptr, 0, n, d_kept, d_root,
                                        d_cnt, s));
        }
        HIP_TRY(hipMemcpyAsync(ctx->h_counters, d_cnt, CNT_COUNT * sizeof(unsigned long long),
                               hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        st.n_kept = ctx->h_counters[CNT_KEPT];
        if (stats) *stats = st;
        return UMI_OK;
    }
};

} // namespace

namespace umihip {

int run_pipeline(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask,
                 const int32_t *d_freq, const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n,
                 int umi_len, int k, float percentage, int mode, int32_t adj_max_freq,
                 uint8_t *d_kept, uint32_t *d_root, hipStream_t s, umi_stats *stats,
                 const uint64_t *d_bucket_off, int n_words, bool may_defer, bool edit)
{
    settle(ctx); // (a deferred call owns the workspace until its end has been seen)
    Pipeline p(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, n, umi_len, k, percentage, mode, adj_max_freq,
               d_kept, d_root, s);
    p.use_device_table(d_bucket_off);
    p.use_wide_keys(n_words);
    if (edit) p.use_edit_distance();
    if (may_defer) p.allow_deferred_end();
    return p.run(stats);
}

int run_pipeline_part(umi_ctx *ctx, const uint64_t *d_keys, const uint64_t *d_nmask, const int32_t *d_freq,
                      const uint64_t *bucket_off, uint64_t n_buckets, uint32_t n, int umi_len, int k,
                      float percentage, int mode, int32_t adj_max_freq, hipStream_t s, uint32_t part,
                      uint32_t n_parts, umi_stats *stats, uint64_t *n_edges)
{
    Pipeline p(ctx, d_keys, d_nmask, d_freq, bucket_off, n_buckets, n, umi_len, k, percentage, mode, adj_max_freq,
               nullptr, nullptr, s, part, n_parts);
    const int rc = p.run(stats);
    if (rc == UMI_OK) *n_edges = p.edge_count();
    return rc;
}

int collapse_edges(umi_ctx *ctx, uint32_t n, const uint2 *d_edges, uint32_t n_edges, int mode, uint8_t *d_kept,
                   uint32_t *d_root, hipStream_t s, umi_stats *stats)
{
    return EdgeCollapse(ctx, n, d_edges, n_edges, mode, d_kept, d_root, s).run(stats);
}

// the end of a deferred call: its control block has arrived, the contract verdict, the counts
int finish_pending(umi_ctx *ctx, umi_stats *stats)
{
    umi_ctx::PendingCall &pc = ctx->pending;
    if (pc.deferred) {
        pc.deferred = false;
        pc.have_result = true; // (a failure to see the end is the call's result as well)
        hipError_t e = hipSetDevice(ctx->device);
        if (e == hipSuccess) e = await_control(ctx, pc.seq, pc.stream);
        pc.rc = e != hipSuccess ? fail(UMI_ERR_HIP, "the end of the pending call: %s", hipGetErrorString(e))
                                : contract_verdict(ctx);
        pc.err = pc.rc ? last_error() : std::string(); // (told again at the hand-out: calls in between set texts of their own)
        pc.st.n_candidates = ctx->h_counters[CNT_CANDIDATES];
        pc.st.n_kept = ctx->h_counters[CNT_KEPT] + ctx->h_counters[CNT_KEPT_FUSED];
    }
    if (!pc.have_result) return fail(UMI_ERR_ARG, "umi_dedup_batch_end without umi_dedup_batch_device_begin");
    pc.have_result = false;
    if (pc.rc != UMI_OK) return fail(pc.rc, "%s", pc.err.c_str());
    if (stats) *stats = pc.st;
    return UMI_OK;
}
// every other entry point that touches the context's workspace first lets a deferred call end (its
// result keeps waiting for umi_dedup_batch_end)
void settle(umi_ctx *ctx)
{
    if (ctx && ctx->pending.deferred) {
        umi_stats st;
        (void)finish_pending(ctx, &st);
        ctx->pending.have_result = true;
    }
}

} // namespace umihip
