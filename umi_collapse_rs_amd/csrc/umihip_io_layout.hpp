// Where the arrays of one host-buffer call lie in the context's staging block (umi_ctx::io).  Arithmetic
// only -- no HIP include -- so that a CPU program can check it (tests/cpp/test_io_layout.cpp).
#pragma once
#include <cstddef>

namespace umihip {

constexpr size_t IO_ALIGN = 256;          // every slot starts on a multiple of this
constexpr size_t IO_ABSENT = ~(size_t)0;  // the offset of an array the caller did not give

// Slots are handed out in the order they are asked for.  An absent array takes no room; an array of no
// bytes takes none either, and still has an address (that of whatever follows it, or the block's end).
struct IoLayout {
    size_t total = 0; // the end of the last slot: what the block must hold
    size_t add(bool present, size_t bytes)
    {
        if (!present) return IO_ABSENT;
        const size_t off = total;
        total += (bytes + (IO_ALIGN - 1)) & ~(IO_ALIGN - 1);
        return off;
    }
};

// a slot's address in a block at `base` (non-null): null for an absent array
inline void *io_at(void *base, size_t off) { return off == IO_ABSENT ? nullptr : (char *)base + off; }

} // namespace umihip
