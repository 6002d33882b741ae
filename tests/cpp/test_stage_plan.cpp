// The host decisions of read staging (umihip_stage_plan.hpp: stage_sort_plan, stage_order_plan) on the CPU,
// against the table that the plain-Python statement of the same rules prints (tests/stage_edge_inputs.py,
// plan_table): every combination the GPU tests run at and the neighbours of every threshold.  argv[1]: the
// table.  Lines "S W L abits gbits -> combine align_bits group_bits second_word p5_bits one_key composed_bits"
// and "O n E B fmax pmax force -> local wide first_bits freq_bits rank_bits order_bits key64".
#include <cinttypes>
#include <cstdio>
#include <cstring>

#include "../../umi_collapse_rs_amd/csrc/umihip_stage_plan.hpp"

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

int main(int argc, char **argv)
{
    // the thresholds themselves, spelled out once
    CHECK(bits_for(0) == 1 && bits_for(1) == 1 && bits_for(2) == 2 && bits_for(32767) == 15 && bits_for(32768) == 16 &&
              bits_for(~0ull) == 64,
          "bits_for");
    CHECK(pack5_of(1).bits == 3 && pack5_of(2).bits == 5 && pack5_of(3).bits == 7 && pack5_of(12).bits == 28 &&
              pack5_of(21).bits == 49,
          "pack5_of");
    CHECK(stage_sort_plan(1, 12, 36, 0).one_key && !stage_sort_plan(1, 12, 37, 0).one_key, "36 + 28 bits compose, 37 + 28 do not");
    CHECK(stage_sort_plan(1, 12, 20, 44).combine && !stage_sort_plan(1, 12, 20, 45).combine, "alignment + group in one word");
    CHECK(!stage_order_plan(1u << 17, 99000, 97, 32767, 1024, false).wide && stage_order_plan(1u << 17, 99000, 97, 32768, 1024, false).wide,
          "2^17 reads: narrow up to fmax 32,767");
    CHECK(stage_order_plan(70000, 1025, 1, 3, 1024, false).local && !stage_order_plan(70000, 1025, 1, 3, 1025, false).local, "1,024 entries a wave");
    CHECK(stage_order_plan(700, 640, 40, 3, 16, false).local && !stage_order_plan(700, 639, 40, 3, 16, false).local, "E >= 16 B");
    CHECK(!stage_order_plan(200000, 1u << 17, 1u << 17, 32767, 1, false).key64 && stage_order_plan(200000, 1u << 17, 1u << 17, 32768, 1, false).key64,
          "15 + 17 bits sort as 32-bit keys, 16 + 17 do not");

    if (argc < 2) {
        fprintf(stderr, "usage: test_stage_plan <table>\n");
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        fprintf(stderr, "cannot open %s\n", argv[1]);
        return 2;
    }
    char line[256];
    int n_sort = 0, n_order = 0;
    while (fgets(line, sizeof line, f)) {
        if (line[0] == 'S') {
            int W, L, ab, gb, combine, a2, g2, second, p5, one, cb;
            if (sscanf(line, "S %d %d %d %d -> %d %d %d %d %d %d %d", &W, &L, &ab, &gb, &combine, &a2, &g2, &second, &p5, &one, &cb) != 11) {
                CHECK(false, "malformed: %s", line);
                continue;
            }
            const StageSortPlan p = stage_sort_plan(W, L, ab, gb);
            CHECK(p.combine == (combine != 0) && p.align_bits == a2 && p.group_bits == g2 && p.second_word == (second != 0) &&
                      p.p5.bits == p5 && p.p5.len == (W == 1 ? L : 1) && p.one_key == (one != 0) && p.composed_bits == cb,
                  "sort plan differs: %s", line);
            CHECK(!p.one_key || p.composed_bits <= 64, "a composed key of %d bits: %s", p.composed_bits, line);
            n_sort++;
        } else if (line[0] == 'O') {
            unsigned n, E, B, fmax, pmax;
            int force, local, wide, first, fb, rb, ob, k64;
            if (sscanf(line, "O %u %u %u %u %u %d -> %d %d %d %d %d %d %d", &n, &E, &B, &fmax, &pmax, &force, &local, &wide, &first, &fb, &rb, &ob,
                       &k64) != 13) {
                CHECK(false, "malformed: %s", line);
                continue;
            }
            const StageOrderPlan p = stage_order_plan(n, E, B, fmax, pmax, force != 0);
            CHECK(p.local == (local != 0) && p.wide == (wide != 0) && p.first_bits == first && p.freq_bits == fb && p.rank_bits == rb &&
                      p.order_bits == ob && p.key64 == (k64 != 0),
                  "order plan differs: %s", line);
            // what the kernels rely on: the narrow key holds (fmax - 1) << first_bits | (n - 1), the u32 sort key its rank and freq fields
            if (!p.wide && n && fmax)
                CHECK((((uint64_t)(fmax - 1) << p.first_bits) | (uint64_t)(n - 1)) <= 0xFFFFFFFFull, "narrow key overflows: %s", line);
            if (!p.key64 && B && fmax)
                CHECK((((uint64_t)(B - 1) << p.freq_bits) | (uint64_t)(fmax - 1)) <= 0xFFFFFFFFull, "u32 sort key overflows: %s", line);
            n_order++;
        } else {
            CHECK(line[0] == '\n' || line[0] == '#', "unknown line: %s", line);
        }
    }
    fclose(f);
    CHECK(n_sort > 100 && n_order > 100, "the table is short: %d sort and %d order lines", n_sort, n_order);
    if (failures) return 1;
    printf("stage plan ok: %d sort plans, %d order plans\n", n_sort, n_order);
    return 0;
}
