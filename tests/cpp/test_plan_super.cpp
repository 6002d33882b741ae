// The planner's super-bin rule (umihip_plan.hpp: choose_super_bases, plan_segment's SegSuper table) on the CPU:
// the exponent for the shapes the GPU tests and config 2 run at, the conditions one by one, and the table --
// every part-0 bin in exactly one super-bin, runs of 4^g bins that start at a multiple of 4^g.
#include <cinttypes>
#include <cstdio>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_plan.hpp"

using namespace umihip;

static int failures = 0;
#define CHECK(c, ...)                                                                                                  \
    do {                                                                                                               \
        if (!(c)) {                                                                                                    \
            failures++;                                                                                                \
            fprintf(stderr, "FAIL %s:%d: ", __FILE__, __LINE__);                                                       \
            fprintf(stderr, __VA_ARGS__);                                                                              \
            fprintf(stderr, "\n");                                                                                     \
        }                                                                                                              \
    } while (0)

static SegSuperOpt opt(bool on = true, int bases = 0, uint32_t cap = SEG_SUPER_CAP, uint32_t min = SEG_SUPER_MIN)
{
    SegSuperOpt o;
    o.on = on;
    o.bases = bases;
    o.cap = cap;
    o.min = min;
    return o;
}

int main()
{
    // config 2: 970,714 entries, 12 bases, 6 index the bins -> 16 bins, ~3,792 entries
    CHECK(choose_super_bases(970714, 12, 6, opt()) == 2, "config 2");
    CHECK(choose_super_bases(970714, 12, 6, opt(true, 1)) == 0, "config 2, g = 1 forced: 948 entries, below the minimum");
    CHECK(choose_super_bases(970714, 12, 6, opt(true, 1, SEG_SUPER_CAP, 64)) == 1, "config 2, g = 1 forced, low minimum");
    CHECK(choose_super_bases(970714, 12, 6, opt(true, 3)) == 0, "config 2, g = 3: 9 bases outside the shared ones");
    CHECK(choose_super_bases(970714, 12, 6, opt(false)) == 0, "switched off");
    CHECK(choose_super_bases(970714, 12, 6, opt(true, 0, 4096)) == 0, "3/4 of a cap of 4,096 is below 3,792; g = 1 below the minimum");
    // L = 10, ~39,000 entries, 5 bases per bin: g = 3 (16 super-bins of ~2,450); g = 4 would be ~9,800
    CHECK(choose_super_bases(39261, 10, 5, opt()) == 3, "L = 10");
    CHECK(choose_super_bases(39261, 10, 5, opt(true, 2, SEG_SUPER_CAP, 64)) == 2, "L = 10, g = 2 forced");
    CHECK(choose_super_bases(39261, 10, 5, opt(true, 0, 8192)) == 3, "L = 10, largest cap: g = 4 would leave 9 bases outside the shared ones");
    // L = 12, ~40,000: 7 bases outside the bins leave g = 1, ~156 entries
    CHECK(choose_super_bases(39990, 12, 5, opt()) == 0, "L = 12, default minimum");
    CHECK(choose_super_bases(39990, 12, 5, opt(true, 0, SEG_SUPER_CAP, 64)) == 1, "L = 12, low minimum");
    CHECK(choose_super_bases(39990, 13, 5, opt(true, 0, SEG_SUPER_CAP, 2)) == 0, "L = 13: 8 bases outside the bins already");
    // g never exceeds the bases that index the bins
    CHECK(choose_super_bases(3000, 6, 3, opt(true, 0, SEG_SUPER_CAP, 2)) == 3, "three bin bases: g = 3 at most");

    // the table of a planned segment
    for (uint64_t n : {39261ull, 970714ull}) {
        Plan pl;
        const int L = n > 100000 ? 12 : 10;
        plan_segment(pl, 0, n, L, 1, true, opt());
        const SegDesc &sd = pl.segs[0];
        const uint32_t g = sd.sup_g, bins = 1u << (2 * sd.nb[0]);
        CHECK(g > 0 && pl.seg_plain == 0, "planned");
        CHECK(pl.seg_supers.size() == (bins >> (2 * g)), "%zu super-bins", pl.seg_supers.size());
        std::vector<int> seen(bins, 0);
        for (const SegSuper &su : pl.seg_supers) {
            CHECK(su.g == g && su.nb == sd.nb[0] && su.rest == L - sd.nb[0] + g && su.rest <= SEG_SUPER_MAX_REST, "fields");
            CHECK(su.bin0 >= sd.bin_off[0] && (su.bin0 - sd.bin_off[0]) % (1u << (2 * g)) == 0, "alignment");
            // (the word behind the run's last bin exists: part 1's bins follow part 0's)
            CHECK(su.bin0 + (1u << (2 * g)) <= sd.bin_off[1], "the next run's first bin");
            for (uint32_t b = 0; b < (1u << (2 * g)); b++) seen[su.bin0 - sd.bin_off[0] + b]++;
        }
        for (uint32_t b = 0; b < bins; b++) CHECK(seen[b] == 1, "bin %u in %d super-bins", b, seen[b]);
        for (uint8_t b : sd.sup_pad) CHECK(b == 0, "padding");
    }
    { // not planned: k = 2, 64-bit keys, the path switched off
        Plan pl;
        plan_segment(pl, 0, 39261, 10, 2, true, opt());
        plan_segment(pl, 0, 39261, 10, 1, false, opt());
        plan_segment(pl, 0, 39261, 10, 1, true, opt(false));
        plan_segment(pl, 0, 39261, 10, 1, true);
        for (const SegDesc &sd : pl.segs) CHECK(sd.sup_g == 0, "not planned");
        CHECK(pl.seg_supers.empty() && pl.seg_plain == 4, "no table");
    }
    if (failures) return 1;
    printf("super plan ok\n");
    return 0;
}
