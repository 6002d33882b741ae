// Host-side decisions of read staging (umihip_stage.hip): how the reads are sorted -- one composed key
// or a sort per key word, the group key folded into the alignment word or a word of its own -- and how
// the entries are put in canonical order -- a wave per position or one more sort, with 32- or 64-bit
// order keys.  Pure functions of a handful of counts, no HIP calls: the file also builds with
// g++ -fsanitize=address,undefined for the CPU-only test tests/cpp/test_stage_plan.cpp, which checks
// it against the plain-Python statement of the same rules in tests/stage_edge_inputs.py.
#pragma once

#include <algorithm>
#include <cstdint>

namespace umihip {

// The UMI rides in the composed sort key at seven bits per three bases (5^3 = 125 letters' worth); a
// last group of one / two bases takes three / five bits (pack5 / unpack5 in umihip_stage.hip).
struct Pack5 {
    int len, bits;
};
inline Pack5 pack5_of(int umi_len)
{
    Pack5 p;
    p.len = umi_len;
    p.bits = 7 * (umi_len / 3) + (umi_len % 3 == 1 ? 3 : umi_len % 3 == 2 ? 5 : 0);
    return p;
}

// bits that hold v (1 for v = 0)
inline int bits_for(uint64_t v)
{
    int b = 1;
    while (b < 64 && (v >> b)) b++;
    return b;
}

// most entries of a position that a wave orders by itself in LDS
constexpr uint32_t STAGE_LOCAL_MAX = 1024;

// ---- the sort of the reads ----------------------------------------------------------------------------
// W key words per UMI, align_bits in 1..64, group_bits in 0..64 (0: no group key).
struct StageSortPlan {
    bool combine;      // alignment and group keys fit one word: combined first, group above alignment
    int align_bits;    // bits of the first position word from then on (align_bits + group_bits if combined)
    int group_bits;    // bits of the second position word (0: there is none)
    bool second_word;  // the group key is a word of its own: sorted last, compared at position heads
    Pack5 p5;          // the packing of the UMI in a composed key (one-word UMIs; of length 1 otherwise)
    bool one_key;      // position word and packed UMI fit 64 bits: one sort on the composed key
    int composed_bits; // first position word + packed UMI (the sort's end bit where one_key)
};
inline StageSortPlan stage_sort_plan(int W, int umi_len, int align_bits, int group_bits)
{
    StageSortPlan p;
    p.combine = group_bits > 0 && align_bits + group_bits <= 64;
    p.align_bits = p.combine ? align_bits + group_bits : align_bits;
    p.group_bits = p.combine || group_bits <= 0 ? 0 : group_bits;
    p.second_word = p.group_bits > 0;
    p.p5 = pack5_of(W == 1 ? umi_len : 1);
    p.composed_bits = p.align_bits + p.p5.bits;
    p.one_key = W == 1 && !p.second_word && p.composed_bits <= 64;
    return p;
}

// ---- the canonical order of the entries ---------------------------------------------------------------
// n reads, E entries in B positions, fmax the largest freq, pmax the most entries of a position.
struct StageOrderPlan {
    bool local;     // every position fits a wave's LDS and positions hold 16 entries on average: no sort
    // local: the order key of an entry is (fmax - freq, first read)
    bool wide;      // ... in 64 bits (the read index in the low word); else both in 32
    int first_bits; // ... bits of the read index in the narrow key (32 in the wide one)
    // sort: the order key is (position rank, fmax - freq)
    int freq_bits, rank_bits, order_bits;
    bool key64;     // ... sorted as 64-bit keys; else as 32-bit ones
};
inline StageOrderPlan stage_order_plan(uint32_t n, uint32_t E, uint32_t B, uint32_t fmax, uint32_t pmax, bool force_wide)
{
    StageOrderPlan p;
    p.freq_bits = bits_for(fmax);
    p.rank_bits = bits_for(B ? B - 1 : 0);
    p.order_bits = std::min(64, p.freq_bits + p.rank_bits);
    p.key64 = p.order_bits > 32;
    p.local = pmax <= STAGE_LOCAL_MAX && (uint64_t)E >= 16ull * B;
    p.first_bits = bits_for(n ? n - 1 : 0);
    // (the wide form is no rarity: 2^17 reads with one UMI read 32,768 times take 17 + 16 bits.
    // force_wide: UMIHIP_STAGE_WIDE_ORDER in the environment, the wide kernel on any input)
    p.wide = force_wide || p.first_bits + p.freq_bits > 32;
    if (p.wide) p.first_bits = 32;
    return p;
}

} // namespace umihip
