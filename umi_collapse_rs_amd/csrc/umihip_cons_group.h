// What the two consensus calls (umihip_consensus.hip: whole reads, umihip_consensus_bam.hip: BAM records)
// share on the device: the guarded unaligned word load, and the wave helpers of the group-by-cluster steps.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace umihip {

// The four bytes at [at, at + 4), bytes from `end` on replaced by those of `pad` (load4 of
// umihip_stage.hip): only aligned words that hold a byte of [at, end) are loaded.
__device__ __forceinline__ uint32_t text4(const uint8_t *p, uint64_t at, uint64_t end, uint32_t pad)
{
    const uintptr_t addr = (uintptr_t)(p + at), a = addr & ~(uintptr_t)3;
    const int sh = (int)(addr & 3);
    const uint32_t lo = *(const uint32_t *)a;
    uint32_t w = lo;
    if (sh) {
        const uint32_t hi = a + 4 < (uintptr_t)(p + end) ? *(const uint32_t *)(a + 4) : 0u;
        w = (uint32_t)((((uint64_t)hi << 32) | lo) >> (8 * sh));
    }
    const uint64_t have = end - at;
    if (have < 4) {
        const uint32_t keep = (1u << (8 * have)) - 1u;
        w = (w & keep) | (pad & ~keep);
    }
    return w;
}

__device__ __forceinline__ uint64_t shfl64(uint64_t v, int src)
{
    const uint32_t lo = (uint32_t)__shfl((int)(uint32_t)v, src), hi = (uint32_t)__shfl((int)(uint32_t)(v >> 32), src);
    return ((uint64_t)hi << 32) | lo;
}

// The lanes of a wave that hold the same cluster r: leader = the lowest of them, rank = this lane's
// place among them, cnt = how many.  Every lane of the wave calls it (invalid lanes stand alone).
__device__ __forceinline__ void wave_groups(uint32_t r, bool valid, int lane, int &leader, uint32_t &rank, uint32_t &cnt)
{
    leader = lane;
    rank = 0;
    cnt = 1;
    unsigned long long todo = __ballot(valid);
    while (todo) {
        const int l0 = __builtin_ctzll(todo);
        const uint32_t r0 = (uint32_t)__shfl((int)r, l0);
        const bool mine = valid && r == r0;
        const unsigned long long m = __ballot(mine);
        if (mine) {
            leader = l0;
            rank = (uint32_t)__builtin_popcountll(m & ((1ull << lane) - 1ull));
            cnt = (uint32_t)__builtin_popcountll(m);
        }
        todo &= ~m;
    }
}

// adds v over the wave to *dst (lane 0, if it is not zero)
__device__ __forceinline__ void wave_add_to(unsigned long long v, unsigned long long *dst, int lane)
{
    for (int o = 32; o > 0; o >>= 1) v += shfl64(v, lane ^ o);
    if (lane == 0 && v) atomicAdd(dst, v);
}

} // namespace umihip
