// Host-side reference for the sort and scan primitives of umihip_radix.hip: seeded input generators,
// the plain references (std::stable_sort on the sorted field, a running 64-bit sum) and the checkers
// that compare a device's output with them.  Plain C++17, no HIP header: tests/cpp/test_primitives.hip
// uses it on the GPU, tests/cpp/test_primitives_ref.cpp checks it on the CPU under ASan + UBSan.
#pragma once

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <numeric>
#include <stdexcept>
#include <string>
#include <vector>

namespace primref {

// what lies behind every buffer handed to a primitive: 64 elements behind keys and values, 256 bytes
// behind a temp, filled with these patterns
constexpr int GUARD_ELEMS = 64, GUARD_BYTES = 256;
constexpr uint64_t GUARD_KEY = 0xA5C3A5C3A5C3A5C3ull;
constexpr uint32_t GUARD_VAL = 0x5AC35AC3u;
constexpr unsigned char GUARD_BYTE = 0xC3;

inline uint64_t field_mask(int bits) { return bits >= 64 ? ~0ull : (1ull << bits) - 1ull; }
// bits [begin_bit, end_bit) of a key: what the sort orders by
template <typename K> inline uint64_t field_of(K k, int begin_bit, int end_bit)
{
    return ((uint64_t)k >> begin_bit) & field_mask(end_bit - begin_bit);
}
inline int passes_of(int begin_bit, int end_bit) { return end_bit > begin_bit ? (end_bit - begin_bit + 7) / 8 : 0; }

struct Rng { // splitmix64
    uint64_t s;
    explicit Rng(uint64_t seed) : s(seed) {}
    uint64_t next()
    {
        uint64_t z = (s += 0x9E3779B97F4A7C15ull);
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        return z ^ (z >> 31);
    }
    uint64_t below(uint64_t m) { return next() % m; }
};

// ---- generators.  The values that go with the keys are always the index 0..n-1.
inline const std::vector<std::string> &generator_names()
{
    static const std::vector<std::string> names = {"uniform", "one_value", "all_ones",     "two_values",        "three_values",
                                                   "sorted",  "reversed",  "outside_only", "one_digit_per_tile"};
    return names;
}

template <typename K> std::vector<K> make_keys(const std::string &gen, uint32_t n, int begin_bit, int end_bit, uint64_t seed)
{
    if (end_bit <= begin_bit || begin_bit < 0 || end_bit > (int)sizeof(K) * 8) throw std::invalid_argument("bit range");
    Rng rng(seed * 0x100000001B3ull + n * 131u + (uint64_t)begin_bit * 67u + (uint64_t)end_bit);
    const K in_field = (K)(field_mask(end_bit - begin_bit) << begin_bit);
    const K low = (K)((K)1 << begin_bit), high = (K)((K)1 << (end_bit - 1));
    std::vector<K> k(n);
    auto by_field = [&](K a, K b) { return field_of(a, begin_bit, end_bit) < field_of(b, begin_bit, end_bit); };
    if (gen == "uniform" || gen == "sorted" || gen == "reversed") {
        for (auto &x : k) x = (K)rng.next();
        if (gen == "sorted") std::stable_sort(k.begin(), k.end(), by_field);
        if (gen == "reversed") std::stable_sort(k.begin(), k.end(), [&](K a, K b) { return by_field(b, a); });
    } else if (gen == "one_value") {
        const K v = (K)rng.next();
        for (auto &x : k) x = v;
    } else if (gen == "all_ones") {
        for (auto &x : k) x = (K) ~(K)0;
    } else if (gen == "two_values") {
        const K v = (K)rng.next();
        for (uint32_t i = 0; i < n; i++) k[i] = (i & 1u) ? (K)(v ^ low) : v; // the two differ inside the field
    } else if (gen == "three_values") {
        const K v = (K)rng.next();
        // the second differs from the first in the field's lowest bit, the third in its highest and
        // outside the field (a 1-bit field has two values only: there the third ties with the second)
        const K three[3] = {v, (K)(v ^ low), (K)((v ^ high) ^ ((K)rng.next() & (K)~in_field))};
        for (auto &x : k) x = three[rng.below(3)];
    } else if (gen == "outside_only") {
        const K c = (K)((K)rng.next() & in_field);
        for (auto &x : k) x = (K)(c | ((K)rng.next() & (K)~in_field));
    } else if (gen == "one_digit_per_tile") {
        for (uint32_t i = 0; i < n; i++) k[i] = (K)((uint64_t)(i / 4096u) << begin_bit);
    } else {
        throw std::invalid_argument("unknown generator " + gen);
    }
    return k;
}

// ---- references
template <typename K> struct Sorted {
    std::vector<K> keys;
    std::vector<uint32_t> vals;
    bool result_in_b = false; // "odd number of 8-bit passes"
};

// std::stable_sort on the field; the values are the indices
template <typename K> Sorted<K> reference_sort(const std::vector<K> &keys, int begin_bit, int end_bit)
{
    Sorted<K> r;
    r.vals.resize(keys.size());
    std::iota(r.vals.begin(), r.vals.end(), 0u);
    std::stable_sort(r.vals.begin(), r.vals.end(), [&](uint32_t a, uint32_t b) {
        return field_of(keys[a], begin_bit, end_bit) < field_of(keys[b], begin_bit, end_bit);
    });
    r.keys.resize(keys.size());
    for (size_t i = 0; i < keys.size(); i++) r.keys[i] = keys[r.vals[i]];
    r.result_in_b = (passes_of(begin_bit, end_bit) & 1) != 0;
    return r;
}

// the same order by other means: a counting sort by 8-bit digits from begin_bit up, the last digit narrower
template <typename K> Sorted<K> counting_sort_lsd(const std::vector<K> &keys, int begin_bit, int end_bit)
{
    const size_t n = keys.size();
    Sorted<K> cur, nxt;
    cur.keys = keys;
    cur.vals.resize(n);
    std::iota(cur.vals.begin(), cur.vals.end(), 0u);
    nxt.keys.resize(n);
    nxt.vals.resize(n);
    int passes = 0;
    for (int sh = begin_bit; sh < end_bit; sh += 8, passes++) {
        const int bits = std::min(8, end_bit - sh);
        std::vector<size_t> start((size_t)1 << bits, 0);
        for (size_t i = 0; i < n; i++) start[field_of(cur.keys[i], sh, sh + bits)]++;
        size_t run = 0;
        for (auto &c : start) {
            const size_t here = c;
            c = run;
            run += here;
        }
        for (size_t i = 0; i < n; i++) {
            const size_t to = start[field_of(cur.keys[i], sh, sh + bits)]++;
            nxt.keys[to] = cur.keys[i];
            nxt.vals[to] = cur.vals[i];
        }
        std::swap(cur.keys, nxt.keys);
        std::swap(cur.vals, nxt.vals);
    }
    cur.result_in_b = (passes & 1) != 0;
    return cur;
}

// inclusive running sum, wrapping mod 2^64
inline std::vector<uint64_t> reference_scan(const std::vector<uint64_t> &in)
{
    std::vector<uint64_t> out(in.size());
    uint64_t run = 0;
    for (size_t i = 0; i < in.size(); i++) out[i] = (run += in[i]);
    return out;
}
// the exclusive form of the same sum
inline std::vector<uint64_t> reference_spine(const std::vector<uint64_t> &in)
{
    std::vector<uint64_t> out(in.size());
    uint64_t run = 0;
    for (size_t i = 0; i < in.size(); i++) {
        out[i] = run;
        run += in[i];
    }
    return out;
}

// ---- checkers: "" or the case's name with the first wrong index and both values
inline std::string wrong(const std::string &name, const char *what, size_t index, uint64_t got, uint64_t want)
{
    char buf[160];
    snprintf(buf, sizeof buf, ": %s index %zu: got 0x%llx, expected 0x%llx", what, index, (unsigned long long)got,
             (unsigned long long)want);
    return name + buf;
}

template <typename T> std::string check_guard(const std::string &name, const char *what, const T *guard, size_t count, T fill)
{
    for (size_t i = 0; i < count; i++)
        if (guard[i] != fill) return wrong(name, what, i, (uint64_t)guard[i], (uint64_t)fill);
    return "";
}

// a sort's four buffers as they came back, each n elements and GUARD_ELEMS behind them, the
// GUARD_BYTES behind its temp of exactly radix_sort_temp_bytes(n), and what it said of the result
template <typename K> struct SortOutput {
    const K *keys_a, *keys_b;
    const uint32_t *vals_a, *vals_b;
    const unsigned char *temp_guard;
    bool result_in_b;
};

template <typename K> std::string check_sort(const std::string &name, const Sorted<K> &ref, const SortOutput<K> &o)
{
    const size_t n = ref.keys.size();
    if (o.result_in_b != ref.result_in_b) return wrong(name, "result_in_b, no", 0, o.result_in_b, ref.result_in_b);
    std::string m;
    if (!(m = check_guard(name, "guard behind keys_a", o.keys_a + n, GUARD_ELEMS, (K)GUARD_KEY)).empty()) return m;
    if (!(m = check_guard(name, "guard behind keys_b", o.keys_b + n, GUARD_ELEMS, (K)GUARD_KEY)).empty()) return m;
    if (!(m = check_guard(name, "guard behind vals_a", o.vals_a + n, GUARD_ELEMS, GUARD_VAL)).empty()) return m;
    if (!(m = check_guard(name, "guard behind vals_b", o.vals_b + n, GUARD_ELEMS, GUARD_VAL)).empty()) return m;
    if (!(m = check_guard(name, "guard behind temp", o.temp_guard, GUARD_BYTES, GUARD_BYTE)).empty()) return m;
    const K *keys = o.result_in_b ? o.keys_b : o.keys_a;
    const uint32_t *vals = o.result_in_b ? o.vals_b : o.vals_a;
    for (size_t i = 0; i < n; i++) {
        if (keys[i] != ref.keys[i]) return wrong(name, "key", i, (uint64_t)keys[i], (uint64_t)ref.keys[i]);
        if (vals[i] != ref.vals[i]) return wrong(name, "value", i, vals[i], ref.vals[i]);
    }
    std::vector<bool> seen(n, false);
    for (size_t i = 0; i < n; i++) {
        if (vals[i] >= n || seen[vals[i]]) return wrong(name, "values no permutation,", i, vals[i], ref.vals[i]);
        seen[vals[i]] = true;
    }
    return "";
}

// out: n words and GUARD_ELEMS behind them; in_after: the input as it came back; temp_guard: the
// GUARD_BYTES behind a temp of exactly scan_temp_bytes(n)
inline std::string check_scan(const std::string &name, const std::vector<uint64_t> &in, const uint64_t *in_after,
                              const uint64_t *out, const unsigned char *temp_guard)
{
    const size_t n = in.size();
    std::string m;
    if (!(m = check_guard(name, "guard behind out", out + n, GUARD_ELEMS, GUARD_KEY)).empty()) return m;
    if (!(m = check_guard(name, "guard behind temp", temp_guard, GUARD_BYTES, GUARD_BYTE)).empty()) return m;
    for (size_t i = 0; i < n; i++)
        if (in_after[i] != in[i]) return wrong(name, "input changed,", i, in_after[i], in[i]);
    uint64_t run = 0;
    for (size_t i = 0; i < n; i++) {
        run += in[i];
        if (out[i] != run) return wrong(name, "sum", i, out[i], run);
    }
    return "";
}

// out: the n sums scanned in place and GUARD_ELEMS behind them
inline std::string check_spine(const std::string &name, const std::vector<uint64_t> &in, const uint64_t *out)
{
    const size_t n = in.size();
    const std::string m = check_guard(name, "guard behind sums", out + n, GUARD_ELEMS, GUARD_KEY);
    if (!m.empty()) return m;
    uint64_t run = 0;
    for (size_t i = 0; i < n; i++) {
        if (out[i] != run) return wrong(name, "sum", i, out[i], run);
        run += in[i];
    }
    return "";
}

} // namespace primref
