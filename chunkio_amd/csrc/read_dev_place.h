// read_dev_place.h -- the arithmetic of the device read path's placement
// (read_dev_gpu.hip: read_headers, read_scan, read_place): which bytes of an
// image are its record, how large the record's slot in a packed output is, how
// two partial sums of slots combine, and when an entry fits.  No HIP type, so
// that the same text compiles for the device and, stand-alone on the host,
// under ASan + UBSan (tools/place_check.cpp, `make placecheck`).  Not installed.
#ifndef CIOA_READ_DEV_PLACE_H
#define CIOA_READ_DEV_PLACE_H

#include <stdint.h>

#include "image_dev.h"

namespace cioa {

constexpr uint32_t kReadBlock = 1024;       // images per workgroup of the header and place kernels
constexpr uint64_t kPlaceOver = ~0ull;      // a sum that left 64 bits (or reached 2^64 - 1)
constexpr int kReadMeta = 0, kReadContent = 1, kReadImage = 2;   // CIOA_READ_* (cio_read_dev.h)

// Record `what` of an image with meta bytes of metadata and content bytes of
// content: its first byte from the image's start, and its length.
CIOA_PLACE_FN void place_select(int what, uint32_t meta, uint64_t content, uint64_t &first, uint64_t &len)
{
    first = what == kReadMeta ? kReadHdr : what == kReadContent ? kReadHdr + meta : 0;
    len = what == kReadMeta ? (uint64_t) meta : what == kReadContent ? content : kReadHdr + meta + content;
}

// The slot of an accepted record of len bytes (nul: 0 or 1 terminator byte) in
// a packed output: len + nul rounded up to align, a power of two.  Saturates
// (the lengths of an image cannot reach that: the host check's can).
CIOA_PLACE_FN uint64_t place_slot(uint64_t len, uint64_t nul, uint64_t align)
{
    const uint64_t raw = len + nul;
    if (raw < len || raw + (align - 1) < raw) {
        return kPlaceOver;
    }
    return (raw + (align - 1)) & ~(align - 1);
}

// The scan's combine step: a + b, saturating at kPlaceOver.  Associative, so
// any grouping of the slots -- by workgroup, by pass of the scan workgroup --
// gives the sequential running sum, and a sum that has left 64 bits stays out.
CIOA_PLACE_FN uint64_t place_add(uint64_t a, uint64_t b)
{
    const uint64_t s = a + b;
    return s < a ? kPlaceOver : s;
}

// An entry whose slot starts at the exclusive prefix sum `before`: does it
// fit out_bytes?  Not from the point where the running sum overflowed.
CIOA_PLACE_FN bool place_fits(uint64_t before, uint64_t slot, uint64_t out_bytes)
{
    const uint64_t end = place_add(before, slot);
    return before != kPlaceOver && end != kPlaceOver && end <= out_bytes;
}

// Caller-placed: the slot [off, + cap) lies inside out_bytes and holds the
// record and its terminator.
CIOA_PLACE_FN bool placed_fits(uint64_t off, uint64_t cap, uint64_t out_bytes, uint64_t len, uint64_t nul)
{
    return off + cap >= off && off + cap <= out_bytes && len + nul >= len && len + nul <= cap;
}

}  // namespace cioa

#endif
