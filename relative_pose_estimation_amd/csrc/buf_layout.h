// buf_layout.h -- where the pieces of a buffer set (RpeBufSet, rpe_internal.h) sit inside its one device block.  Plain C++,
// nothing of HIP: sizes in, offsets and the total out, so tests/native/buf_layout_host.cpp runs it on the host.
#pragma once
#include <stddef.h>

constexpr size_t RPE_BUF_ALIGN = 256;             // every piece starts on a multiple of this (hipMalloc's own alignment)
constexpr size_t RPE_BUF_NONE = ~(size_t)0;       // the offset of a piece of 0 bytes: it gets no address

// Pieces in the order of place(): piece i sits at the running sum of the aligned sizes of the pieces before it; the total
// is that sum, and at least one unit (a block is never of 0 bytes).  All of it in size_t.
struct RpeBufLayout {
    size_t end = 0;
    size_t place(size_t bytes)
    {
        if (bytes == 0) return RPE_BUF_NONE;
        const size_t at = end;
        end += (bytes + RPE_BUF_ALIGN - 1) / RPE_BUF_ALIGN * RPE_BUF_ALIGN;
        return at;
    }
    size_t total() const { return end < RPE_BUF_ALIGN ? RPE_BUF_ALIGN : end; }
};
