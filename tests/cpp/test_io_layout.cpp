// The layout of the staging block of a host-buffer call (umihip_io_layout.hpp: IoLayout, io_at) on the CPU.
// Slots start on multiples of 256 and do not overlap, pads included; an absent array takes no room and has
// no address; an array of no bytes takes no room and has one; the total is the end of the last slot.  An
// array of no bytes shares its offset with what follows it, so offsets rise strictly over the arrays that
// hold something and never fall.  The declarations of umi_count_matrix and umi_dedup_stats, in the order
// the library makes them, add up to the sums of 256-byte multiples those two calls used to write out by hand.
#include <cstdint>
#include <cstdio>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_io_layout.hpp"

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

static size_t up(size_t v) { return (v + 255) & ~(size_t)255; }

struct Decl {
    bool present;
    size_t bytes; // (an explicit pad included)
};

// every property of one list of declarations
static void check_list(const std::vector<Decl> &decls, const char *what)
{
    alignas(256) static char block[1]; // (an address to add to; nothing is read or written through it)
    IoLayout l;
    size_t end = 0, last_filled = IO_ABSENT;
    for (size_t i = 0; i < decls.size(); i++) {
        const size_t before = l.total, off = l.add(decls[i].present, decls[i].bytes);
        if (!decls[i].present) {
            CHECK(off == IO_ABSENT && l.total == before, "%s: absent array %zu takes room", what, i);
            CHECK(io_at(block, off) == nullptr, "%s: absent array %zu has an address", what, i);
            continue;
        }
        CHECK(off % IO_ALIGN == 0, "%s: slot %zu at %zu", what, i, off);
        CHECK(off >= end, "%s: slot %zu at %zu overlaps the one before, which ends at %zu", what, i, off, end);
        CHECK(io_at(block, off) == (void *)(block + off), "%s: slot %zu has the address of another offset", what, i);
        CHECK(io_at(block, off) != nullptr, "%s: slot %zu has no address", what, i);
        if (decls[i].bytes) {
            CHECK(last_filled == IO_ABSENT || off > last_filled, "%s: slot %zu at %zu does not lie behind %zu", what, i, off, last_filled);
            last_filled = off;
        } else {
            CHECK(l.total == before, "%s: the empty array %zu takes room", what, i);
        }
        end = off + decls[i].bytes;
        CHECK(l.total >= end && l.total - end < IO_ALIGN && l.total % IO_ALIGN == 0, "%s: total %zu after a slot that ends at %zu", what,
              l.total, end);
    }
    CHECK(l.total == up(end), "%s: total %zu, the last slot ends at %zu", what, l.total, end);
}

// umi_count_matrix: n entries in nb buckets, cap of them non-empty
static size_t count_matrix_total(size_t n, size_t nb, size_t cap)
{
    IoLayout l;
    l.add(true, n * 4);                                              // freq
    l.add(true, nb * 4), l.add(true, nb * 4);                        // row, col
    l.add(true, cap * 4), l.add(true, cap * 4), l.add(true, cap * 4); // out_row, out_col, out_molecules
    l.add(true, cap * 8);                                            // out_reads
    l.add(true, n);                                                  // kept
    return l.total;
}
static size_t count_matrix_by_hand(size_t n, size_t nb, size_t cap)
{
    const size_t o_freq = 0, o_row = o_freq + up(n * 4), o_col = o_row + up(nb * 4), o_orow = o_col + up(nb * 4),
                 o_ocol = o_orow + up(cap * 4), o_omol = o_ocol + up(cap * 4), o_oreads = o_omol + up(cap * 4),
                 o_kept = o_oreads + up(cap * 8);
    return o_kept + up(n);
}

// umi_dedup_stats: n entries of n_words words, the per-UMI table asked for or not
static size_t dedup_stats_total(size_t n, size_t n_words, size_t hist_bins, size_t umi_len, bool per_umi)
{
    const size_t dist_words = 4 * (umi_len + 2);
    IoLayout l;
    l.add(true, n * 8 * n_words);                           // keys
    l.add(true, n * 4), l.add(true, n * 4);                 // freq, root
    l.add(true, hist_bins * 8), l.add(true, hist_bins * 8); // count_pre, count_post
    l.add(true, dist_words * 8);                            // dist
    l.add(per_umi, n * 4), l.add(per_umi, n * 4);           // umi_entry, times_pre
    l.add(per_umi, n * 8);                                  // reads_pre
    l.add(per_umi, n * 4);                                  // times_post
    l.add(per_umi, n * 8);                                  // reads_post
    l.add(true, n);                                         // kept
    return l.total;
}
static size_t dedup_stats_by_hand(size_t n, size_t n_words, size_t hist_bins, size_t umi_len, bool per_umi)
{
    const size_t dist_words = 4 * (umi_len + 2), nu = per_umi ? n : 0;
    const size_t o_keys = 0, o_freq = o_keys + up(n * 8 * n_words), o_root = o_freq + up(n * 4), o_pre = o_root + up(n * 4),
                 o_post = o_pre + up(hist_bins * 8), o_dist = o_post + up(hist_bins * 8), o_entry = o_dist + up(dist_words * 8),
                 o_tpre = o_entry + up(nu * 4), o_rpre = o_tpre + up(nu * 4), o_tpost = o_rpre + up(nu * 8),
                 o_rpost = o_tpost + up(nu * 4), o_kept = o_rpost + up(nu * 8);
    return o_kept + up(n);
}

int main()
{
    check_list({}, "nothing");
    check_list({{false, 100}}, "one absent array");
    check_list({{true, 0}}, "one empty array");
    check_list({{true, 0}, {true, 0}, {false, 0}}, "empty arrays only");
    check_list({{true, 1}, {true, 255}, {true, 256}, {true, 257}, {true, 0}, {false, 4096}, {true, 512}}, "sizes around a slot");
    check_list({{true, 0}, {true, 8}, {false, 8}, {true, 0}, {true, 3}, {true, 0}}, "empty arrays between others");
    check_list({{true, 100 + 8}, {true, 100 + 8}, {true, 16 * 7}, {true, 1}}, "explicit pads (bytes + 8, two arrays in one slot, one byte)");
    check_list({{true, (size_t)5 << 32}, {true, 7}, {true, (size_t)3 << 31}}, "beyond 32 bits");
    for (size_t a : {0, 1, 23, 254, 255, 256, 257, 258, 511, 512, 513, 600})
        for (size_t b : {0, 1, 255, 256, 257, 1000})
            check_list({{true, a}, {b % 2 == 0, b}, {true, b}, {true, a + b}}, "pairs of sizes");

    const size_t sizes[] = {0, 1, 2, 31, 32, 33, 63, 64, 65, 255, 256, 257, 300, 70000};
    for (size_t n : sizes)
        for (size_t nb : sizes)
            for (size_t cap : {(size_t)0, (size_t)1, nb / 2, nb}) {
                const size_t got = count_matrix_total(n, nb, cap), want = count_matrix_by_hand(n, nb, cap);
                CHECK(got == want, "count matrix, n %zu in %zu buckets, %zu of them non-empty: %zu, by hand %zu", n, nb, cap, got, want);
            }
    // (255, 256 and 257 bytes: n = 255 .. 257 for kept, n = 64 for freq and root, n = 32 for one-word keys,
    // hist_bins = 32 and -- with 4 (umi_len + 2) words -- umi_len = 6)
    for (size_t n : sizes)
        for (size_t n_words : {1, 2, 4})
            for (size_t hist_bins : {2, 31, 32, 33, 1000})
                for (size_t umi_len : {1, 6, 12, 85})
                    for (int per_umi = 0; per_umi < 2; per_umi++) {
                        const size_t got = dedup_stats_total(n, n_words, hist_bins, umi_len, per_umi != 0),
                                     want = dedup_stats_by_hand(n, n_words, hist_bins, umi_len, per_umi != 0);
                        CHECK(got == want, "dedup stats, n %zu of %zu words, %zu bins, umi_len %zu, table %d: %zu, by hand %zu", n, n_words,
                              hist_bins, umi_len, per_umi, got, want);
                    }
    if (failures) {
        fprintf(stderr, "%d checks failed\n", failures);
        return 1;
    }
    printf("io layout ok\n");
    return 0;
}
