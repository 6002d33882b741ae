// The splice junctions of a read, one after another, its CIGAR read from memory (umi_junction_matrix, the program's
// --junction-matrix).  Host and device: the kernels of umihip_junctions.hip run this code, and
// tests/cpp/test_junction_walk.cpp runs it on the CPU against tests/junction_model.py.
//
// Blocks are umi_assign_genes_transcripts' (umihip_transcript_index.hpp: transcript_next_block): M, =, X and D extend
// the current block, an N of any length closes it and skips its length, I, S, H and P consume nothing, empty blocks are
// left out.  A junction is the stretch [e, s) between two consecutive non-empty blocks, told at the moment the second
// of them gets its first base; it counts where 0 <= e < s <= JN_POS_MAX.  Positions are 64-bit and only grow, so the
// junctions of a read come out in ascending order and none of them twice.
#pragma once
#include <cstdint>

#ifndef UMIHIP_HD
#if defined(__HIPCC__)
#define UMIHIP_HD __host__ __device__
#else
#define UMIHIP_HD
#endif
#endif

namespace umihip {

constexpr int64_t JN_POS_MAX = 2147483647; // 2^31 - 1: the largest position a junction may end at
enum JnStep : int { JN_END = 0, JN_FOUND = 1, JN_BAD_OP = -1 };

struct JnWalk {
    uint64_t c; // the next word
    int64_t bs; // the current block [bs, be)
    int64_t be;
    int64_t pe; // the end of the last non-empty block that an N closed
    bool open;  // ... and no block has begun behind it yet
};

UMIHIP_HD inline JnWalk junction_walk_begin(int64_t pos) { return {0, pos, pos, 0, false}; }

// The next junction [*e, *s) of the read: JN_FOUND; JN_END behind the last word; JN_BAD_OP at an op code above 8 (the
// walk is over then).  Every word is looked at exactly once over the calls of one walk.
UMIHIP_HD inline int junction_next(const uint32_t *cigar, uint64_t n_cigar, JnWalk &w, int64_t *e, int64_t *s)
{
    while (w.c < n_cigar) {
        const uint32_t word = cigar[w.c++], op = word & 15u;
        const int64_t len = (int64_t)(word >> 4);
        if (op > 8) {
            w.c = n_cigar;
            return JN_BAD_OP;
        }
        if (op == 0 || op == 2 || op == 7 || op == 8) {
            if (len == 0) continue;
            const bool begins = w.be == w.bs;
            w.be += len;
            if (begins && w.open) {
                w.open = false;
                if (w.pe >= 0 && w.bs > w.pe && w.bs <= JN_POS_MAX) {
                    *e = w.pe, *s = w.bs;
                    return JN_FOUND;
                }
            }
        } else if (op == 3) {
            if (w.be > w.bs) {
                w.pe = w.be;
                w.open = true;
            }
            w.bs = w.be = w.be + len;
        }
    }
    return JN_END;
}

// The number of junctions of a read, or JN_BAD_OP; *last_s: where the block behind its last junction starts (the
// largest coordinate any of its junctions has), untouched where there is none.
UMIHIP_HD inline int64_t junction_count(const uint32_t *cigar, uint64_t n_cigar, int64_t pos, int64_t *last_s)
{
    JnWalk w = junction_walk_begin(pos);
    int64_t k = 0, e, s;
    for (;;) {
        const int st = junction_next(cigar, n_cigar, w, &e, &s);
        if (st == JN_BAD_OP) return JN_BAD_OP;
        if (st == JN_END) return k;
        k++;
        *last_s = s;
    }
}

} // namespace umihip
