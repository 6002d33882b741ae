// The planner's cross rule (umihip_plan.hpp: choose_cross, plan_segment's SegDesc::cross and the map offsets of its
// SegSuper table) on the CPU: the length limit at 13 / 14 bases, the option, the conditions super-bins have already
// (k = 1, 32-bit keys, no N mask: sup_g > 0), a segment without super-bins, one super-bin for the whole segment, the
// per-call limit, and the maps of several segments back to back.
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

static SegSuperOpt opt(bool cross = true, uint32_t map_mb = SEG_CROSS_MAP_MB, bool on = true, uint32_t cap = SEG_SUPER_CAP,
                       uint32_t min = SEG_SUPER_MIN)
{
    SegSuperOpt o;
    o.on = on;
    o.cap = cap;
    o.min = min;
    o.cross = cross;
    o.cross_map_mb = map_mb;
    return o;
}

int main()
{
    // the rule by itself
    CHECK(choose_cross(12, 2, opt()), "config 2: 2 MB of maps");
    CHECK(choose_cross(13, 2, opt()), "13 bases: 8 MB, the default limit");
    CHECK(!choose_cross(14, 2, opt()), "14 bases: 32 MB");
    CHECK(choose_cross(14, 2, opt(true, 32)), "14 bases with seg_cross_map_mb = 32");
    CHECK(!choose_cross(15, 2, opt(true, 64)), "15 bases: 128 MB, beyond a call's 64");
    CHECK(!choose_cross(12, 2, opt(false)), "seg_cross = 0");
    CHECK(!choose_cross(12, 2, opt(true, SEG_CROSS_MAP_MB, false)), "a call super-bins are not planned in");
    CHECK(!choose_cross(12, 0, opt()), "a segment without super-bins");
    CHECK(choose_cross(8, 4, opt()), "g = nb0: one super-bin, no cross pair, still planned");
    CHECK(!choose_cross(12, 2, opt(true, 0)), "seg_cross_map_mb = 0");
    CHECK(choose_cross(13, 2, opt(), 56ull << 20) && !choose_cross(13, 2, opt(), (56ull << 20) + 1), "the call's 64 MB");
    static_assert(SEG_CROSS_MAP_MB == 8, "12 and 13 bases by default");

    { // config 2 planned: 256 super-bins, maps of 2,048 words back to back
        Plan pl;
        plan_segment(pl, 0, 970714, 12, 1, true, opt());
        const SegDesc &sd = pl.segs[0];
        CHECK(sd.sup_g == 2 && sd.cross == 1 && pl.seg_cross == 1, "planned");
        CHECK(pl.seg_cross_words == (1ull << 24) / 32, "4^12 bits");
        uint32_t at = 0;
        for (const SegSuper &su : pl.seg_supers) {
            CHECK(su.cross == 1 && su.seg == 0 && su.map0 == at, "map offset %u", su.map0);
            at += seg_cross_words(su.rest);
        }
        CHECK(at == pl.seg_cross_words, "the maps fill the array");
        for (uint8_t b : sd.sup_pad) CHECK(b == 0, "padding");
    }
    { // two segments in one plan: the second one's maps behind the first one's; then one that is not planned
        Plan pl;
        plan_segment(pl, 0, 39261, 10, 1, true, opt());
        plan_segment(pl, 39261, 39261 + 970714, 12, 1, true, opt());
        plan_segment(pl, 0, 39261, 10, 1, true, opt(false));
        CHECK(pl.segs[0].cross == 1 && pl.segs[1].cross == 1 && pl.segs[2].cross == 0 && pl.seg_cross == 2, "two of three");
        CHECK(pl.seg_cross_words == (1ull << 20) / 32 + (1ull << 24) / 32, "both segments' maps");
        const uint32_t n0 = 1u << (2 * (pl.segs[0].nb[0] - pl.segs[0].sup_g));
        CHECK(pl.seg_supers[n0].seg == 1 && pl.seg_supers[n0].map0 == (1u << 20) / 32, "the second segment's first map");
        for (const SegSuper &su : pl.seg_supers)
            if (su.seg == 2) CHECK(su.cross == 0 && su.map0 == 0, "no map");
    }
    { // not planned: k = 2, 64-bit keys (an N mask never reaches the planner with the path on: SegSuperOpt::on)
        Plan pl;
        plan_segment(pl, 0, 39261, 10, 2, true, opt());
        plan_segment(pl, 0, 39261, 10, 1, false, opt());
        plan_segment(pl, 0, 39261, 10, 1, true, opt(true, SEG_CROSS_MAP_MB, false));
        plan_segment(pl, 0, 39990, 12, 1, true, opt()); // (no super-bins at the default minimum)
        for (const SegDesc &sd : pl.segs) CHECK(sd.cross == 0 && sd.sup_g == 0, "not planned");
        CHECK(pl.seg_cross == 0 && pl.seg_cross_words == 0, "no maps");
    }
    { // g = nb0: one super-bin, its map the whole segment's
        Plan pl;
        plan_segment(pl, 0, 5000, 8, 1, true, opt(true, SEG_CROSS_MAP_MB, true, 8192));
        CHECK(pl.segs[0].sup_g == 4 && pl.segs[0].nb[0] == 4 && pl.segs[0].cross == 1 && pl.seg_supers.size() == 1, "one super-bin");
        CHECK(pl.seg_cross_words == (1ull << 16) / 32, "4^8 bits");
    }
    { // 14 bases: super-bins, no cross path at the default limit
        Plan pl;
        plan_segment(pl, 0, 970714, 14, 1, true, opt(true, SEG_CROSS_MAP_MB, true, SEG_SUPER_CAP, 2));
        CHECK(pl.segs[0].sup_g > 0 && pl.segs[0].cross == 0, "14 bases");
        Plan pl2;
        plan_segment(pl2, 0, 970714, 14, 1, true, opt(true, 32, true, SEG_SUPER_CAP, 2));
        CHECK(pl2.segs[0].cross == 1, "14 bases, 32 MB allowed");
    }
    if (failures) return 1;
    printf("cross plan ok\n");
    return 0;
}
