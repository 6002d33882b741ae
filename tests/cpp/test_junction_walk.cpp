// The junction walk of umi_junction_matrix on the CPU (csrc/umihip_junction_walk.hpp: the code the kernels run) against
// the junctions of tests/junction_model.py, read from the file that tests/test_junction_model_cpu.py writes, a read a
// line:
//   pos n_words words... n_junctions (start end)...      n_junctions -1: an op code above 8
// Stand-alone: built with -fsanitize=address,undefined by that test; `make` builds it plain.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../umi_collapse_rs_amd/csrc/umihip_junction_walk.hpp"

using namespace umihip;

int main(int argc, char **argv)
{
    if (argc < 2) {
        fprintf(stderr, "usage: %s VECTORS\n", argv[0]);
        return 2;
    }
    FILE *f = fopen(argv[1], "r");
    if (!f) {
        perror(argv[1]);
        return 2;
    }
    long reads = 0, junctions = 0, bad_ops = 0;
    int failures = 0;
    int64_t pos;
    unsigned long long n_words;
    while (fscanf(f, "%" SCNd64 " %llu", &pos, &n_words) == 2) {
        std::vector<uint32_t> cigar(n_words); // (exactly its words: a read beyond them is the sanitizer's to find)
        for (auto &w : cigar)
            if (fscanf(f, "%" SCNu32, &w) != 1) return 2;
        long long want_n;
        if (fscanf(f, "%lld", &want_n) != 1) return 2;
        std::vector<int64_t> want(want_n > 0 ? 2 * want_n : 0);
        for (auto &v : want)
            if (fscanf(f, "%" SCNd64, &v) != 1) return 2;
        reads++;
        // the count
        int64_t last = -1;
        const int64_t got_n = junction_count(cigar.data(), cigar.size(), pos, &last);
        if (got_n != want_n) {
            if (failures++ < 20) fprintf(stderr, "read %ld: %lld junctions, want %lld\n", reads - 1, (long long)got_n, want_n);
            continue;
        }
        if (want_n < 0) {
            bad_ops++;
            continue;
        }
        if (want_n > 0 && last != want.back() && failures++ < 20) fprintf(stderr, "read %ld: last position %lld\n", reads - 1, (long long)last);
        // the walk, junction by junction
        JnWalk w = junction_walk_begin(pos);
        int64_t e, s;
        long long k = 0;
        while (junction_next(cigar.data(), cigar.size(), w, &e, &s) == JN_FOUND) {
            if (k < want_n && (e != want[2 * k] || s != want[2 * k + 1]) && failures++ < 20)
                fprintf(stderr, "read %ld junction %lld: [%lld, %lld), want [%lld, %lld)\n", reads - 1, k, (long long)e, (long long)s,
                        (long long)want[2 * k], (long long)want[2 * k + 1]);
            k++;
        }
        if (k != want_n && failures++ < 20) fprintf(stderr, "read %ld: the walk gave %lld junctions, want %lld\n", reads - 1, k, want_n);
        junctions += k;
    }
    fclose(f);
    printf("%ld reads, %ld junctions, %ld bad op codes, %d failures\n", reads, junctions, bad_ops, failures);
    return failures ? 1 : 0;
}
