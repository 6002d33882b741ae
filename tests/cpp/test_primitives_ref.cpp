// CPU check of tests/cpp/primitives_ref.hpp (built with ASan + UBSan by tests/test_primitives_cpu.py):
// the reference sort equals an independent counting sort, every generator produces what its name
// says, and every checker rejects a host-made wrong answer and names the right index.  This is what
// shows that the checkers of tests/cpp/test_primitives.hip can fail.
#include <cstdio>
#include <cstdlib>

#include "primitives_ref.hpp"

using namespace primref;

static int failures = 0;
#define EXPECT(cond, ...)                                                                                                       \
    do {                                                                                                                        \
        if (!(cond)) {                                                                                                          \
            printf("FAIL %s:%d: %s: ", __FILE__, __LINE__, #cond);                                                              \
            printf(__VA_ARGS__);                                                                                                \
            printf("\n");                                                                                                       \
            failures++;                                                                                                         \
        }                                                                                                                       \
    } while (0)

struct Range {
    int b, e;
};
static const std::vector<Range> ranges64 = {{0, 64}, {0, 1},  {0, 7},  {0, 8},   {0, 9},   {0, 33},
                                            {0, 37}, {3, 20}, {8, 16}, {40, 64}, {56, 64}, {57, 64}};
static const std::vector<Range> ranges32 = {{0, 32}, {0, 1}, {0, 13}, {5, 32}, {24, 32}, {31, 32}};
static const std::vector<uint32_t> sizes = {1, 2, 63, 64, 65, 255, 256, 257, 4095, 4096, 4097, 8193, 20000};

// the distinct values of bits [b, e) of the keys, in order
template <typename K> static std::vector<uint64_t> distinct_fields(const std::vector<K> &k, int b, int e)
{
    std::vector<uint64_t> s;
    for (K x : k) s.push_back(field_of(x, b, e));
    std::sort(s.begin(), s.end());
    s.erase(std::unique(s.begin(), s.end()), s.end());
    return s;
}

// what every generator's name promises
template <typename K> static void check_generator(const std::string &gen, uint32_t n, Range r)
{
    const std::vector<K> k = make_keys<K>(gen, n, r.b, r.e, 1), again = make_keys<K>(gen, n, r.b, r.e, 1);
    const char *g = gen.c_str();
    EXPECT(k.size() == n && k == again, "%s n=%u (%d,%d): size or seed", g, n, r.b, r.e);
    const std::vector<uint64_t> distinct = distinct_fields(k, 0, (int)sizeof(K) * 8), fields = distinct_fields(k, r.b, r.e);
    const bool has_outside = r.e - r.b < (int)sizeof(K) * 8;
    const uint64_t field_values = field_mask(r.e - r.b); // (one less than their number)
    if (gen == "uniform") {
        // 1,000 draws from 2^bits values: all of a narrow field's values turn up, hardly any of a wide one's repeat
        if (n >= 4096 && field_values < 8) EXPECT(fields.size() == field_values + 1, "%s: %zu fields", g, fields.size());
        if (n >= 4096 && r.e - r.b >= 32) EXPECT(fields.size() > n - n / 100, "%s: %zu fields of %u", g, fields.size(), n);
    } else if (gen == "one_value") {
        EXPECT(distinct.size() == 1, "%s: %zu keys", g, distinct.size());
    } else if (gen == "all_ones") {
        EXPECT(distinct.size() == 1 && k[0] == (K) ~(K)0, "%s", g);
        EXPECT(fields == std::vector<uint64_t>{field_mask(r.e - r.b)}, "%s: field", g);
    } else if (gen == "two_values") {
        EXPECT(distinct.size() == (n > 1 ? 2u : 1u) && fields.size() == distinct.size(), "%s: %zu keys", g, distinct.size());
        for (uint32_t i = 2; i < n; i++) EXPECT(k[i] == k[i - 2] && k[i] != k[i - 1], "%s: not alternating at %u", g, i);
    } else if (gen == "three_values") {
        EXPECT(distinct.size() <= 3, "%s: %zu keys", g, distinct.size());
        if (n >= 64) {
            EXPECT(distinct.size() == 3, "%s: %zu keys", g, distinct.size());
            EXPECT(fields.size() == (r.e - r.b > 1 ? 3u : 2u), "%s: %zu fields", g, fields.size());
        }
    } else if (gen == "sorted" || gen == "reversed") {
        for (uint32_t i = 1; i < n; i++) {
            const uint64_t p = field_of(k[i - 1], r.b, r.e), q = field_of(k[i], r.b, r.e);
            EXPECT(gen == "sorted" ? p <= q : p >= q, "%s: out of order at %u", g, i);
        }
    } else if (gen == "outside_only") {
        EXPECT(fields.size() == 1, "%s: %zu fields", g, fields.size());
        if (n > 64 && has_outside) EXPECT(distinct.size() > 1, "%s: one key only", g);
    } else if (gen == "one_digit_per_tile") {
        for (uint32_t i = 0; i < n; i++) EXPECT(k[i] == (K)((uint64_t)(i / 4096u) << r.b), "%s: key %u", g, i);
    } else {
        EXPECT(false, "no check for generator %s", g);
    }
}

template <typename K> static void reference_against_counting_sort(const std::vector<Range> &ranges)
{
    for (const std::string &gen : generator_names())
        for (Range r : ranges)
            for (uint32_t n : sizes) {
                check_generator<K>(gen, n, r);
                const std::vector<K> k = make_keys<K>(gen, n, r.b, r.e, 2);
                const Sorted<K> a = reference_sort(k, r.b, r.e), c = counting_sort_lsd(k, r.b, r.e);
                EXPECT(a.keys == c.keys && a.vals == c.vals && a.result_in_b == c.result_in_b,
                       "%s n=%u (%d,%d) u%zu: stable_sort and counting sort differ", gen.c_str(), n, r.b, r.e, sizeof(K) * 8);
                // the reference is ordered by the field, stable, and made of the input's pairs
                for (uint32_t i = 0; i < n; i++) {
                    EXPECT(a.keys[i] == k[a.vals[i]], "pair %u torn", i);
                    if (!i) continue;
                    const uint64_t p = field_of(a.keys[i - 1], r.b, r.e), q = field_of(a.keys[i], r.b, r.e);
                    EXPECT(p < q || (p == q && a.vals[i - 1] < a.vals[i]), "%s n=%u (%d,%d): order at %u", gen.c_str(), n, r.b,
                           r.e, i);
                }
            }
}

// a device's buffers, made on the host: the reference in the result buffer, the guards filled
template <typename K> struct HostSort {
    std::vector<K> ka, kb;
    std::vector<uint32_t> va, vb;
    std::vector<unsigned char> tg;
    bool in_b;
    HostSort(const std::vector<K> &input, const Sorted<K> &ref) : tg(GUARD_BYTES, GUARD_BYTE), in_b(ref.result_in_b)
    {
        const size_t n = input.size();
        ka = input;
        kb.assign(n, (K)GUARD_KEY);
        va.resize(n);
        std::iota(va.begin(), va.end(), 0u);
        vb.assign(n, GUARD_VAL);
        keys() = ref.keys;
        vals() = ref.vals;
        for (auto *v : {&ka, &kb}) v->resize(n + GUARD_ELEMS, (K)GUARD_KEY);
        for (auto *v : {&va, &vb}) v->resize(n + GUARD_ELEMS, GUARD_VAL);
    }
    std::vector<K> &keys() { return in_b ? kb : ka; }
    std::vector<uint32_t> &vals() { return in_b ? vb : va; }
    SortOutput<K> out() const { return SortOutput<K>{ka.data(), kb.data(), va.data(), vb.data(), tg.data(), in_b}; }
};

static bool names(const std::string &msg, const char *what, size_t index)
{
    return msg.find(std::string(": ") + what + " index " + std::to_string(index) + ":") != std::string::npos;
}

template <typename K> static void sort_checker_rejects(Range r)
{
    const uint32_t n = 10000;
    const char *w = sizeof(K) == 8 ? "u64" : "u32";
    {
        const std::vector<K> k = make_keys<K>("three_values", n, r.b, r.e, 3);
        const Sorted<K> ref = reference_sort(k, r.b, r.e);
        HostSort<K> good(k, ref);
        EXPECT(check_sort<K>("good", ref, good.out()).empty(), "%s: %s", w, check_sort<K>("good", ref, good.out()).c_str());
        // sorted, but two neighbours of one field value have changed places
        uint32_t at = 5000;
        while (field_of(ref.keys[at], r.b, r.e) != field_of(ref.keys[at + 1], r.b, r.e)) at++;
        HostSort<K> unstable(k, ref);
        std::swap(unstable.keys()[at], unstable.keys()[at + 1]);
        std::swap(unstable.vals()[at], unstable.vals()[at + 1]);
        const std::string m = check_sort<K>("unstable", ref, unstable.out());
        EXPECT(m.rfind("unstable: ", 0) == 0 && (names(m, "key", at) || names(m, "value", at)), "%s at %u: '%s'", w, at, m.c_str());
        // the flag alone flipped; the flag flipped and the result moved with it
        HostSort<K> flipped(k, ref);
        flipped.in_b = !flipped.in_b;
        EXPECT(check_sort<K>("flag", ref, flipped.out()).find("result_in_b") != std::string::npos, "%s: flag alone", w);
        std::swap(flipped.ka, flipped.kb);
        std::swap(flipped.va, flipped.vb);
        EXPECT(check_sort<K>("flag", ref, flipped.out()).find("result_in_b") != std::string::npos, "%s: flag and buffers", w);
        // one guard word overwritten, behind each buffer in turn
        const size_t j = 17;
        HostSort<K> g1(k, ref), g2(k, ref), g3(k, ref), g4(k, ref), g5(k, ref);
        g1.ka[n + j] ^= 1;
        g2.kb[n + j] ^= 1;
        g3.va[n + j] ^= 1;
        g4.vb[n + GUARD_ELEMS - 1] = 0;
        g5.tg[GUARD_BYTES - 1] = 0;
        EXPECT(names(check_sort<K>("g", ref, g1.out()), "guard behind keys_a", j), "%s: keys_a guard", w);
        EXPECT(names(check_sort<K>("g", ref, g2.out()), "guard behind keys_b", j), "%s: keys_b guard", w);
        EXPECT(names(check_sort<K>("g", ref, g3.out()), "guard behind vals_a", j), "%s: vals_a guard", w);
        EXPECT(names(check_sort<K>("g", ref, g4.out()), "guard behind vals_b", GUARD_ELEMS - 1), "%s: vals_b guard", w);
        EXPECT(names(check_sort<K>("g", ref, g5.out()), "guard behind temp", GUARD_BYTES - 1), "%s: temp guard", w);
        // a value twice: the pairs still in field order, the values no permutation
        HostSort<K> twice(k, ref);
        twice.vals()[n - 1] = twice.vals()[n - 2];
        EXPECT(names(check_sort<K>("p", ref, twice.out()), "value", n - 1), "%s: value twice", w);
    }
    {
        const std::vector<K> k = make_keys<K>("uniform", n, r.b, r.e, 4);
        const Sorted<K> ref = reference_sort(k, r.b, r.e);
        // sorted by the whole key instead of the field
        std::vector<uint32_t> order(n);
        std::iota(order.begin(), order.end(), 0u);
        std::stable_sort(order.begin(), order.end(), [&](uint32_t a, uint32_t b) { return k[a] < k[b]; });
        HostSort<K> whole(k, ref);
        size_t first = n;
        for (uint32_t i = 0; i < n; i++) {
            whole.keys()[i] = k[order[i]];
            whole.vals()[i] = order[i];
            if (first == n && order[i] != ref.vals[i]) first = i;
        }
        const std::string m = check_sort<K>("whole", ref, whole.out());
        if (r.e == (int)sizeof(K) * 8) { // (the field is the key's top: the two orders differ in ties at the most)
            EXPECT(first < n || m.empty(), "%s whole key: '%s'", w, m.c_str());
        }
        if (first < n || r.e < (int)sizeof(K) * 8) {
            EXPECT(first < n, "%s: whole-key order equals field order", w);
            EXPECT(names(m, "key", first) || names(m, "value", first), "%s whole key at %zu: '%s'", w, first, m.c_str());
        }
        // shifted by one from index 4096 on
        HostSort<K> shifted(k, ref);
        for (uint32_t i = 4096; i < n; i++) {
            shifted.keys()[i] = ref.keys[i - 1];
            shifted.vals()[i] = ref.vals[i - 1];
        }
        const std::string s = check_sort<K>("shifted", ref, shifted.out());
        EXPECT(names(s, "key", 4096) || names(s, "value", 4096), "%s shifted: '%s'", w, s.c_str());
    }
}

static std::vector<uint64_t> guarded(const std::vector<uint64_t> &v)
{
    std::vector<uint64_t> g = v;
    g.resize(v.size() + GUARD_ELEMS, GUARD_KEY);
    return g;
}

static void scan_checkers_reject()
{
    const std::vector<unsigned char> tg(GUARD_BYTES, GUARD_BYTE);
    for (int random = 0; random < 2; random++) {
        // a scan that loses the carry into element 2,097,152: the sums start again there
        const size_t n = 2048 * 1024 + 1 + 2048, cut = 2097152;
        Rng rng(5);
        std::vector<uint64_t> in(n, 1);
        if (random)
            for (auto &x : in) x = rng.next();
        const std::vector<uint64_t> ref = reference_scan(in);
        if (!random) EXPECT(ref[n - 1] == n && ref[cut] == cut + 1, "scan reference");
        std::vector<uint64_t> out = guarded(ref);
        EXPECT(check_scan("good", in, in.data(), out.data(), tg.data()).empty(), "good scan refused");
        for (size_t i = cut; i < n; i++) out[i] = ref[i] - ref[cut - 1];
        EXPECT(names(check_scan("carry", in, in.data(), out.data(), tg.data()), "sum", cut), "scan carry lost");
        out = guarded(ref);
        out[n] = 0;
        EXPECT(names(check_scan("g", in, in.data(), out.data(), tg.data()), "guard behind out", 0), "scan out guard");
        out = guarded(ref);
        std::vector<unsigned char> bad = tg;
        bad[3] = 0;
        EXPECT(names(check_scan("g", in, in.data(), out.data(), bad.data()), "guard behind temp", 3), "scan temp guard");
        std::vector<uint64_t> touched = in;
        touched[2048] += 1;
        EXPECT(names(check_scan("in", in, touched.data(), out.data(), tg.data()), "input changed,", 2048), "scan input");
    }
    for (int random = 0; random < 2; random++) {
        // a spine that loses the carry into element 1024: its second round starts from zero
        const size_t n = 3000, cut = 1024;
        Rng rng(6);
        std::vector<uint64_t> in(n, 1);
        if (random)
            for (auto &x : in) x = rng.next();
        const std::vector<uint64_t> ref = reference_spine(in), incl = reference_scan(in);
        for (size_t i = 0; i < n; i++) EXPECT(ref[i] == incl[i] - in[i], "spine is not the exclusive form at %zu", i);
        std::vector<uint64_t> out = guarded(ref);
        EXPECT(check_spine("good", in, out.data()).empty(), "good spine refused");
        for (size_t i = cut; i < n; i++) out[i] = ref[i] - ref[cut];
        EXPECT(names(check_spine("carry", in, out.data()), "sum", cut), "spine carry lost");
        out = guarded(ref);
        out[n + 63] = 1;
        EXPECT(names(check_spine("g", in, out.data()), "guard behind sums", 63), "spine guard");
    }
    // the references on a sum that wraps
    const std::vector<uint64_t> wrap = {~0ull, 2, ~0ull - 5};
    EXPECT((reference_scan(wrap) == std::vector<uint64_t>{~0ull, 1, ~0ull - 4}), "scan wrap");
    EXPECT((reference_spine(wrap) == std::vector<uint64_t>{0, ~0ull, 1}), "spine wrap");
}

int main()
{
    reference_against_counting_sort<uint64_t>(ranges64);
    reference_against_counting_sort<uint32_t>(ranges32);
    for (Range r : {Range{0, 64}, Range{3, 20}, Range{0, 9}}) sort_checker_rejects<uint64_t>(r);
    for (Range r : {Range{0, 32}, Range{5, 32}, Range{0, 13}}) sort_checker_rejects<uint32_t>(r);
    scan_checkers_reject();
    bool threw = false;
    try {
        make_keys<uint64_t>("no_such", 4, 0, 8, 1);
    } catch (const std::invalid_argument &) {
        threw = true;
    }
    EXPECT(threw, "an unknown generator's name is accepted");
    if (failures) {
        printf("%d checks failed\n", failures);
        return 1;
    }
    printf("primitives reference ok\n");
    return 0;
}
