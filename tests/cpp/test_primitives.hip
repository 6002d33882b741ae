// The sort and scan primitives of umihip_radix.hip, called directly and compared with the plain
// references of primitives_ref.hpp at the sizes and bit ranges where tiles, rounds, look-back windows
// and spine rounds begin and end.  Links build/obj/umihip_radix.o and nothing else of the library
// (make primtest).  Run as `test_primitives <group>`, the groups being refusals, scan, spine, sort32,
// sort64, hist and reuse; tests/test_gpu_primitives.py runs them all.
//
// Exit 0 and "<group> ok: <cases> cases" if every case matches; exit 1 with the checker's message on
// a wrong result; exit 2, at once, on a HIP call that fails.  Every case's name is printed before it
// starts.  The group `refusals` makes no HIP call and runs without a GPU.
#include <hip/hip_runtime.h>
#include <unistd.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "primitives_ref.hpp"
#include "umihip_internal.h"

using namespace umihip;
using namespace primref;

#define HIP_OK(call)                                                                                                            \
    do {                                                                                                                        \
        const hipError_t e_ = (call);                                                                                           \
        if (e_ != hipSuccess) {                                                                                                 \
            printf("%s:%d: %s: %s\n", __FILE__, __LINE__, #call, hipGetErrorString(e_));                                        \
            fflush(stdout);                                                                                                     \
            _exit(2);                                                                                                           \
        }                                                                                                                       \
    } while (0)

static int n_cases = 0;

static void begin_case(const std::string &name)
{
    printf("%s\n", name.c_str());
    fflush(stdout);
    n_cases++;
}
// after a case: nothing pending on the stream, no error left behind; then the checker's verdict
static void end_case(hipStream_t s, const std::string &verdict)
{
    HIP_OK(hipStreamSynchronize(s));
    HIP_OK(hipGetLastError());
    if (!verdict.empty()) {
        printf("WRONG %s\n", verdict.c_str());
        fflush(stdout);
        exit(1);
    }
}

struct Range {
    int b, e;
};
static const std::vector<uint32_t> sort_sizes = {1,    2,    63,   64,   65,   255,   256,   257,   1023,  1024,  1025,
                                                 4095, 4096, 4097, 8191, 8192, 8193, 36864, 36865, 69637, 100003};
static const std::vector<Range> ranges64 = {{0, 64}, {0, 1},  {0, 7},  {0, 8},   {0, 9},   {0, 33},
                                            {0, 37}, {3, 20}, {8, 16}, {40, 64}, {56, 64}, {57, 64}};
static const std::vector<Range> ranges32 = {{0, 32}, {0, 1}, {0, 13}, {5, 32}, {24, 32}, {31, 32}};

static std::string case_name(const char *group, int key_bits, const std::string &gen, uint32_t n, Range r, uint32_t parts = 0)
{
    char buf[160];
    snprintf(buf, sizeof buf, "%s u%d %s n=%u bits=(%d,%d)", group, key_bits, gen.c_str(), n, r.b, r.e);
    std::string s = buf;
    if (parts) s += " parts=" + std::to_string(parts);
    return s;
}

static hipError_t sort_pairs(uint64_t *ka, uint64_t *kb, uint32_t *va, uint32_t *vb, uint32_t n, int b, int e, void *temp,
                             size_t temp_bytes, bool *in_b, hipStream_t s, uint32_t parts)
{
    return radix_sort_pairs_u64(ka, kb, va, vb, n, b, e, temp, temp_bytes, in_b, s, parts);
}
static hipError_t sort_pairs(uint32_t *ka, uint32_t *kb, uint32_t *va, uint32_t *vb, uint32_t n, int b, int e, void *temp,
                             size_t temp_bytes, bool *in_b, hipStream_t s, uint32_t parts)
{
    return radix_sort_pairs_u32(ka, kb, va, vb, n, b, e, temp, temp_bytes, in_b, s, parts);
}

// What a producer of the keys does when it supplies the digit counts: block b's counts of pass p and
// digit d go to parts[(b * passes + p) * 256 + d], zeros included.
template <typename K>
__global__ __launch_bounds__(256) void count_digits_kernel(const K *__restrict__ keys, uint32_t n, int begin_bit, int end_bit,
                                                           int passes, uint32_t *__restrict__ parts)
{
    __shared__ uint32_t h[RADIX_MAX_PASSES * RADIX_BINS];
    for (int i = threadIdx.x; i < passes * RADIX_BINS; i += 256) h[i] = 0;
    __syncthreads();
    for (uint32_t i = blockIdx.x * 256u + threadIdx.x; i < n; i += gridDim.x * 256u) {
        const uint64_t k = keys[i];
        for (int p = 0; p < passes; p++) {
            const int sh = begin_bit + 8 * p, bits = end_bit - sh < 8 ? end_bit - sh : 8;
            atomicAdd(&h[p * RADIX_BINS + (int)((k >> sh) & ((1u << bits) - 1u))], 1u);
        }
    }
    __syncthreads();
    uint32_t *mine = parts + (size_t)blockIdx.x * passes * RADIX_BINS;
    for (int i = threadIdx.x; i < passes * RADIX_BINS; i += 256) mine[i] = h[i];
}

// A temp on the device: room for `cap` bytes and the guard behind them.  A case uses the first
// `bytes` of it and puts the guard right behind those.  It starts out as all-ones, and later cases
// find what earlier ones left: a primitive that relied on a clean temp would show.
struct Temp {
    unsigned char *p = nullptr;
    size_t cap = 0, bytes = 0;
    void alloc(size_t cap_bytes)
    {
        cap = cap_bytes;
        HIP_OK(hipMalloc((void **)&p, cap + GUARD_BYTES));
        HIP_OK(hipMemset(p, 0xFF, cap + GUARD_BYTES));
    }
    void use(size_t n_bytes, hipStream_t s)
    {
        if (n_bytes > cap) {
            printf("temp of %zu bytes asked from %zu\n", n_bytes, cap);
            exit(1);
        }
        bytes = n_bytes;
        HIP_OK(hipMemsetAsync(p + bytes, GUARD_BYTE, GUARD_BYTES, s));
    }
    std::vector<unsigned char> guard() const
    {
        std::vector<unsigned char> g(GUARD_BYTES);
        HIP_OK(hipMemcpy(g.data(), p + bytes, GUARD_BYTES, hipMemcpyDeviceToHost));
        return g;
    }
    void release() { HIP_OK(hipFree(p)); }
};

// One sort's four buffers on the device, for up to `cap` pairs and the guards behind them.
template <typename K> struct SortRig {
    uint32_t cap = 0, n = 0;
    K *ka = nullptr, *kb = nullptr;
    uint32_t *va = nullptr, *vb = nullptr;
    bool in_b = false;
    std::vector<K> hk;
    std::vector<uint32_t> hv;

    void alloc(uint32_t cap_pairs)
    {
        cap = cap_pairs;
        HIP_OK(hipMalloc((void **)&ka, ((size_t)cap + GUARD_ELEMS) * sizeof(K)));
        HIP_OK(hipMalloc((void **)&kb, ((size_t)cap + GUARD_ELEMS) * sizeof(K)));
        HIP_OK(hipMalloc((void **)&va, ((size_t)cap + GUARD_ELEMS) * 4));
        HIP_OK(hipMalloc((void **)&vb, ((size_t)cap + GUARD_ELEMS) * 4));
    }
    // keys and indices into the a buffers, the fill pattern into the b buffers and all four guards
    void upload(const std::vector<K> &keys)
    {
        n = (uint32_t)keys.size();
        if (n > cap) {
            printf("%u pairs asked from a rig of %u\n", n, cap);
            exit(1);
        }
        const size_t m = (size_t)n + GUARD_ELEMS;
        hk = keys;
        hk.resize(m, (K)GUARD_KEY);
        hv.resize(m);
        for (size_t i = 0; i < m; i++) hv[i] = i < n ? (uint32_t)i : GUARD_VAL;
        HIP_OK(hipMemcpy(ka, hk.data(), m * sizeof(K), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(va, hv.data(), m * 4, hipMemcpyHostToDevice));
        std::fill(hk.begin(), hk.end(), (K)GUARD_KEY);
        std::fill(hv.begin(), hv.end(), GUARD_VAL);
        HIP_OK(hipMemcpy(kb, hk.data(), m * sizeof(K), hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(vb, hv.data(), m * 4, hipMemcpyHostToDevice));
    }
    // the sort, or with parts > 0: prepare, the counting kernel of `parts` blocks, the sort
    void launch(Range r, const Temp &t, hipStream_t s, uint32_t parts = 0)
    {
        if (parts) {
            uint32_t *where = nullptr;
            HIP_OK(radix_sort_prepare(t.p, t.bytes, n, r.b, r.e, &where, s));
            count_digits_kernel<K><<<parts, 256, 0, s>>>(ka, n, r.b, r.e, passes_of(r.b, r.e), where);
            HIP_OK(hipGetLastError());
        }
        HIP_OK(sort_pairs(ka, kb, va, vb, n, r.b, r.e, t.p, t.bytes, &in_b, s, parts));
    }
    // (after the stream has been synchronised)
    std::string check(const std::string &name, const Sorted<K> &ref, const Temp &t)
    {
        const size_t m = (size_t)n + GUARD_ELEMS;
        std::vector<K> oka(m), okb(m);
        std::vector<uint32_t> ova(m), ovb(m);
        HIP_OK(hipMemcpy(oka.data(), ka, m * sizeof(K), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(okb.data(), kb, m * sizeof(K), hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(ova.data(), va, m * 4, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(ovb.data(), vb, m * 4, hipMemcpyDeviceToHost));
        const std::vector<unsigned char> tg = t.guard();
        return check_sort<K>(name, ref, SortOutput<K>{oka.data(), okb.data(), ova.data(), ovb.data(), tg.data(), in_b});
    }
    void release()
    {
        HIP_OK(hipFree(ka));
        HIP_OK(hipFree(kb));
        HIP_OK(hipFree(va));
        HIP_OK(hipFree(vb));
    }
};

template <typename K>
static void sort_case(const char *group, SortRig<K> &rig, Temp &temp, hipStream_t s, const std::string &gen, uint32_t n, Range r)
{
    const std::string name = case_name(group, (int)sizeof(K) * 8, gen, n, r);
    begin_case(name);
    const std::vector<K> keys = make_keys<K>(gen, n, r.b, r.e, 11);
    const Sorted<K> ref = reference_sort(keys, r.b, r.e);
    rig.upload(keys);
    temp.use(radix_sort_temp_bytes(n), s);
    rig.launch(r, temp, s);
    HIP_OK(hipStreamSynchronize(s));
    end_case(s, rig.check(name, ref, temp));
}

template <typename K> static void group_sort(const char *group, const std::vector<Range> &ranges, bool big, hipStream_t s)
{
    const uint32_t cap = big ? 3000001u : sort_sizes.back();
    SortRig<K> rig;
    Temp temp;
    rig.alloc(cap);
    temp.alloc(radix_sort_temp_bytes(cap));
    for (uint32_t n : sort_sizes)
        for (Range r : ranges)
            for (const std::string &gen : generator_names()) sort_case<K>(group, rig, temp, s, gen, n, r);
    if (big) {
        // 245 tiles, and 733: more than the 512 that can be resident at once (256 CUs, two
        // workgroups of 1,024 threads and 65 KB of LDS each), so the last tiles draw their ticket
        // only after earlier ones have left
        for (Range r : {Range{0, 64}, Range{3, 20}})
            for (const char *gen : {"uniform", "one_value", "outside_only"}) sort_case<K>(group, rig, temp, s, gen, 1000003u, r);
        for (Range r : {Range{0, 64}, Range{0, 9}})
            for (const char *gen : {"uniform", "all_ones"}) sort_case<K>(group, rig, temp, s, gen, 3000001u, r);
    }
    rig.release();
    temp.release();
}

// the digit counts supplied by a kernel of P blocks: the same result as without
template <typename K> static void group_hist(const std::vector<Range> &ranges, hipStream_t s)
{
    const uint32_t cap = 100003;
    SortRig<K> rig;
    Temp temp;
    rig.alloc(cap);
    temp.alloc(radix_sort_temp_bytes(cap));
    for (uint32_t n : {1u, 4097u, 100003u})
        for (Range r : ranges)
            for (const char *gen : {"uniform", "one_value"}) {
                const std::vector<K> keys = make_keys<K>(gen, n, r.b, r.e, 12);
                const Sorted<K> ref = reference_sort(keys, r.b, r.e);
                for (uint32_t parts : {1u, 2u, 5u, 16u, 64u, 65u, 2048u}) {
                    const std::string name = case_name("hist", (int)sizeof(K) * 8, gen, n, r, parts);
                    begin_case(name);
                    rig.upload(keys);
                    temp.use(radix_sort_temp_bytes(n), s);
                    rig.launch(r, temp, s, parts);
                    HIP_OK(hipStreamSynchronize(s));
                    end_case(s, rig.check(name, ref, temp));
                }
            }
    rig.release();
    temp.release();
}

// ---- scan and spine
struct ScanRig {
    uint32_t cap = 0, n = 0;
    uint64_t *in = nullptr, *out = nullptr;
    void alloc(uint32_t cap_words)
    {
        cap = cap_words;
        HIP_OK(hipMalloc((void **)&in, (size_t)cap * 8));
        HIP_OK(hipMalloc((void **)&out, ((size_t)cap + GUARD_ELEMS) * 8));
    }
    void upload(const std::vector<uint64_t> &words)
    {
        n = (uint32_t)words.size();
        if (n > cap) {
            printf("%u words asked from a rig of %u\n", n, cap);
            exit(1);
        }
        const std::vector<uint64_t> fill((size_t)n + GUARD_ELEMS, GUARD_KEY);
        HIP_OK(hipMemcpy(in, words.data(), (size_t)n * 8, hipMemcpyHostToDevice));
        HIP_OK(hipMemcpy(out, fill.data(), fill.size() * 8, hipMemcpyHostToDevice));
    }
    void launch(const Temp &t, hipStream_t s) { HIP_OK(scan_inclusive_u64(in, out, n, t.p, t.bytes, s)); }
    std::string check(const std::string &name, const std::vector<uint64_t> &words, const Temp &t)
    {
        std::vector<uint64_t> after(n), got((size_t)n + GUARD_ELEMS);
        HIP_OK(hipMemcpy(after.data(), in, (size_t)n * 8, hipMemcpyDeviceToHost));
        HIP_OK(hipMemcpy(got.data(), out, got.size() * 8, hipMemcpyDeviceToHost));
        const std::vector<unsigned char> tg = t.guard();
        return check_scan(name, words, after.data(), got.data(), tg.data());
    }
    void release()
    {
        HIP_OK(hipFree(in));
        HIP_OK(hipFree(out));
    }
};

static std::vector<uint64_t> scan_input(int kind, uint32_t n)
{
    Rng rng(13 + n);
    std::vector<uint64_t> w(n, 0);
    switch (kind) {
    case 0: break;                                                        // all zero
    case 1: std::fill(w.begin(), w.end(), 1ull); break;                   // all one
    case 2: for (auto &x : w) x = rng.next(); break;                      // random 64-bit: the sum wraps
    case 3: for (auto &x : w) x = (1ull << 32) | rng.below(16); break;    // two counters in one word
    case 4: w[0] = 1; break;
    case 5: w[n - 1] = 1; break;
    case 6: w[2048] = 1; break;                                           // (n > 2048)
    }
    return w;
}
static const char *const scan_kinds[] = {"zeros", "ones", "random", "two_counters", "one_at_0", "one_at_last", "one_at_2048"};

static void group_scan(hipStream_t s)
{
    const std::vector<uint32_t> sizes = {1,    2,    7,    8,           9,           511,             512,            513, 2047,
                                         2048, 2049, 4096, 2048 * 1023 + 2047, 2048 * 1024, 2048 * 1024 + 1, 2048 * 1025 + 3};
    ScanRig rig;
    Temp temp;
    rig.alloc(sizes.back());
    temp.alloc(scan_temp_bytes(sizes.back()));
    for (uint32_t n : sizes)
        for (int kind = 0; kind < 7; kind++) {
            if (kind == 6 && n <= 2048) continue;
            const std::string name = std::string("scan ") + scan_kinds[kind] + " n=" + std::to_string(n);
            begin_case(name);
            const std::vector<uint64_t> words = scan_input(kind, n);
            rig.upload(words);
            temp.use(scan_temp_bytes(n), s);
            rig.launch(temp, s);
            HIP_OK(hipStreamSynchronize(s));
            end_case(s, rig.check(name, words, temp));
        }
    rig.release();
    temp.release();
}

static void group_spine(hipStream_t s)
{
    const std::vector<uint32_t> sizes = {1, 2, 63, 64, 65, 1023, 1024, 1025, 2047, 2048, 2049, 3000};
    unsigned long long *sums = nullptr;
    HIP_OK(hipMalloc((void **)&sums, ((size_t)sizes.back() + GUARD_ELEMS) * 8));
    for (uint32_t n : sizes)
        for (int kind = 1; kind <= 2; kind++) {
            const std::string name = std::string("spine ") + scan_kinds[kind] + " n=" + std::to_string(n);
            begin_case(name);
            const std::vector<uint64_t> words = scan_input(kind, n);
            std::vector<uint64_t> buf = words;
            buf.resize((size_t)n + GUARD_ELEMS, GUARD_KEY);
            HIP_OK(hipMemcpy(sums, buf.data(), buf.size() * 8, hipMemcpyHostToDevice));
            HIP_OK(scan_spine_u64(sums, n, s));
            HIP_OK(hipStreamSynchronize(s));
            HIP_OK(hipMemcpy(buf.data(), sums, buf.size() * 8, hipMemcpyDeviceToHost));
            end_case(s, check_spine(name, words, buf.data()));
        }
    HIP_OK(hipFree(sums));
}

// three sorts on one temp and a scan, back to back on one stream, checked after one synchronisation
static void reuse_on(hipStream_t s, const char *which)
{
    const uint32_t big = 100003;
    const Range r1{0, 64}, r2{0, 9}, r3{5, 32};
    const std::string name = std::string("reuse ") + which;
    begin_case(name);
    const std::vector<uint64_t> k1 = make_keys<uint64_t>("uniform", big, r1.b, r1.e, 21),
                                k2 = make_keys<uint64_t>("uniform", 4097, r2.b, r2.e, 22);
    const std::vector<uint32_t> k3 = make_keys<uint32_t>("uniform", big, r3.b, r3.e, 23);
    const std::vector<uint64_t> words = scan_input(3, big);
    SortRig<uint64_t> s1, s2;
    SortRig<uint32_t> s3;
    ScanRig sc;
    Temp temp, scan_temp;
    s1.alloc(big);
    s2.alloc(4097);
    s3.alloc(big);
    sc.alloc(big);
    temp.alloc(radix_sort_temp_bytes(big));
    scan_temp.alloc(scan_temp_bytes(big));
    s1.upload(k1);
    s2.upload(k2);
    s3.upload(k3);
    sc.upload(words);
    temp.use(radix_sort_temp_bytes(big), s);
    scan_temp.use(scan_temp_bytes(big), s);
    HIP_OK(hipStreamSynchronize(s));
    s1.launch(r1, temp, s);
    s2.launch(r2, temp, s);
    s3.launch(r3, temp, s);
    sc.launch(scan_temp, s);
    HIP_OK(hipStreamSynchronize(s));
    std::string verdict = s1.check(name + " 1: u64 n=100003 bits=(0,64)", reference_sort(k1, r1.b, r1.e), temp);
    if (verdict.empty()) verdict = s2.check(name + " 2: u64 n=4097 bits=(0,9)", reference_sort(k2, r2.b, r2.e), temp);
    if (verdict.empty()) verdict = s3.check(name + " 3: u32 n=100003 bits=(5,32)", reference_sort(k3, r3.b, r3.e), temp);
    if (verdict.empty()) verdict = sc.check(name + " 4: scan n=100003", words, scan_temp);
    end_case(s, verdict);
    s1.release();
    s2.release();
    s3.release();
    sc.release();
    temp.release();
    scan_temp.release();
}

// ---- what the host side refuses before any HIP call
static int refused = 0;
#define REFUSAL(cond)                                                                                                           \
    do {                                                                                                                        \
        n_cases++;                                                                                                              \
        if (!(cond)) {                                                                                                          \
            printf("WRONG refusals: %s (line %d)\n", #cond, __LINE__);                                                          \
            refused++;                                                                                                          \
        }                                                                                                                       \
    } while (0)

template <typename K> static void refusals_of_sort()
{
    const int width = (int)sizeof(K) * 8;
    const uint32_t n = 5000;
    const size_t bytes = radix_sort_temp_bytes(n);
    K *const k = nullptr;
    uint32_t *const v = nullptr;
    auto sort = [&](uint32_t n_pairs, int b, int e, size_t temp_bytes, uint32_t parts, bool *in_b) {
        *in_b = true;
        return sort_pairs(k, k, v, v, n_pairs, b, e, nullptr, temp_bytes, in_b, nullptr, parts);
    };
    bool in_b;
    REFUSAL(sort(0, 0, width, bytes, 0, &in_b) == hipSuccess && !in_b);
    REFUSAL(sort(0, 0, width, 0, 0, &in_b) == hipSuccess && !in_b);
    REFUSAL(sort(n, 8, 8, bytes, 0, &in_b) == hipSuccess && !in_b);
    REFUSAL(sort(n, 9, 8, bytes, 0, &in_b) == hipSuccess && !in_b);
    REFUSAL(sort(n, -1, 8, bytes, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, -8, width, bytes, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, 0, width + 1, bytes, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(1u << 30, 0, width, ~(size_t)0, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, 0, width, bytes - 1, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, 0, 8, bytes - 1, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, 0, width, 16, 0, &in_b) == hipErrorInvalidValue);
    REFUSAL(sort(n, 0, width, bytes, RADIX_HIST_PARTS + 1, &in_b) == hipErrorInvalidValue);
}

static void group_refusals()
{
    refusals_of_sort<uint64_t>();
    refusals_of_sort<uint32_t>();
    const uint32_t n = 5000;
    uint32_t sentinel = 0, *parts = &sentinel;
    REFUSAL(radix_sort_prepare(nullptr, radix_sort_temp_bytes(n), 0, 0, 64, &parts, nullptr) == hipSuccess && parts == nullptr);
    parts = &sentinel;
    REFUSAL(radix_sort_prepare(nullptr, radix_sort_temp_bytes(n) - 1, n, 0, 64, &parts, nullptr) == hipErrorInvalidValue &&
            parts == nullptr);
    parts = &sentinel;
    REFUSAL(radix_sort_prepare(nullptr, 16, n, 0, 9, &parts, nullptr) == hipErrorInvalidValue && parts == nullptr);
    REFUSAL(scan_inclusive_u64(nullptr, nullptr, 0, nullptr, 0, nullptr) == hipSuccess);
    REFUSAL(scan_inclusive_u64(nullptr, nullptr, n, nullptr, scan_temp_bytes(n) - 1, nullptr) == hipErrorInvalidValue);
    const uint32_t steps[] = {1, 4096, 4097, 3000001};
    for (int i = 0; i < 4; i++) {
        REFUSAL(radix_sort_temp_bytes(steps[i]) > 0 && scan_temp_bytes(steps[i]) > 0);
        if (i) REFUSAL(radix_sort_temp_bytes(steps[i]) >= radix_sort_temp_bytes(steps[i - 1]));
        if (i) REFUSAL(scan_temp_bytes(steps[i]) >= scan_temp_bytes(steps[i - 1]));
    }
    if (refused) exit(1);
}

int main(int argc, char **argv)
{
    const std::string group = argc > 1 ? argv[1] : "";
    if (group == "refusals") {
        group_refusals();
    } else if (group == "scan" || group == "spine" || group == "sort32" || group == "sort64" || group == "hist" ||
               group == "reuse") {
        hipStream_t s = nullptr;
        HIP_OK(hipStreamCreate(&s));
        if (group == "scan") group_scan(s);
        if (group == "spine") group_spine(s);
        if (group == "sort32") group_sort<uint32_t>("sort32", ranges32, false, s);
        if (group == "sort64") group_sort<uint64_t>("sort64", ranges64, true, s);
        if (group == "hist") {
            group_hist<uint64_t>({{0, 64}, {3, 20}, {0, 9}}, s);
            group_hist<uint32_t>({{0, 32}, {5, 32}, {0, 13}}, s);
        }
        if (group == "reuse") {
            reuse_on(s, "created stream");
            reuse_on(nullptr, "null stream");
        }
        HIP_OK(hipStreamSynchronize(s));
        HIP_OK(hipStreamDestroy(s));
        HIP_OK(hipDeviceSynchronize());
    } else {
        printf("usage: test_primitives refusals|scan|spine|sort32|sort64|hist|reuse\n");
        return 64;
    }
    printf("%s ok: %d cases\n", group.c_str(), n_cases);
    return 0;
}
