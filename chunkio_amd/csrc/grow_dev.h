// grow_dev.h -- the arithmetic of growing chunk images in HBM out of an arena
// (grow_dev_gpu.hip: grow_headers, grow_scan, grow_place, grow_zero,
// grow_commit): whether an image has room for what is about to be appended,
// the reference's growth rule for its new capacity, where its new slot lies in
// the arena, who writes the arena's new top, and which bytes one lane zeroes
// for a range of a tail region's units.  No HIP type, so that the same text
// compiles for the device and, stand-alone on the host, under ASan + UBSan
// (tools/grow_check.cpp, `make growcheck`).  Not installed.
#ifndef CIOA_GROW_DEV_H
#define CIOA_GROW_DEV_H

#include <stdint.h>

#include "read_dev_place.h"
#include "write_dev_copy.h"

namespace cioa {

constexpr uint32_t kGrowBlock = kReadBlock;            // images per workgroup of the header, place and commit kernels
constexpr uint64_t kGrowMaxContent = 0xffffffffull;    // the content length field is 32 bits
constexpr uint64_t kGrowLenClamp = 1ull << 32;         // a record length above it counts as this: never satisfiable
// What grow_place leaves per image for grow_commit (bits).
constexpr uint32_t kGrowMoved = 1;       // the image is grown: its offset and capacity are replaced
constexpr uint32_t kGrowTopAt = 2;       // the first cut image behind accepted ones: top = its offset
constexpr uint32_t kGrowTopEnd = 4;      // the last entry of a batch whose slots all fit: top = its slot's end
// grow_decide's verdicts.
constexpr int kGrowReject = 0, kGrowRoom = 1, kGrowGrow = 2;

// v rounded up to a, a power of two; kPlaceOver when that leaves 64 bits.
CIOA_PLACE_FN uint64_t grow_round_up(uint64_t v, uint64_t a)
{
    if (v == kPlaceOver || v + (a - 1) < v) {
        return kPlaceOver;
    }
    return (v + (a - 1)) & ~(a - 1);
}

// The reference's growth rule (cio_file_write): new = cap + realloc_size;
// while new < used + need, new += realloc_size; then rounded up to page.  In
// closed form, for used + need > cap: k = ceil((used + need - cap) /
// realloc_size) steps.  kPlaceOver when a value leaves 64 bits (or reaches
// 2^64 - 1).  used <= cap, need <= 2^32 - 1, realloc_size >= 1.
CIOA_PLACE_FN uint64_t grow_new_cap(uint64_t cap, uint64_t used, uint64_t need, uint64_t realloc_size,
                                    uint64_t page)
{
    const uint64_t lack = used + need - cap;           // > 0; used + need < 2^34
    const uint64_t k = (lack - 1) / realloc_size + 1;
    if (k > kPlaceOver / realloc_size) {
        return kPlaceOver;
    }
    return grow_round_up(place_add(cap, k * realloc_size), page);
}

// Does the image [off, off + cap) (inside dev_bytes: no wrap) share a byte
// with the arena's free part [top, end)?
CIOA_PLACE_FN bool grow_in_arena(uint64_t off, uint64_t cap, uint64_t top, uint64_t end)
{
    return top < end && cap != 0 && off < end && top < off + cap;
}

// Rules 2..4 for an image that passed the write path's image check (used = 24
// + meta + content <= cap) and has need != 0: rejected, room, or grown to
// new_cap.
CIOA_PLACE_FN int grow_decide(uint64_t off, uint64_t cap, uint64_t used, uint64_t content, uint64_t need,
                              uint64_t top, uint64_t end, uint64_t realloc_size, uint64_t page, uint64_t &new_cap)
{
    new_cap = 0;
    if (need > kGrowMaxContent || content + need > kGrowMaxContent || grow_in_arena(off, cap, top, end)) {
        return kGrowReject;
    }
    if (used + need <= cap) {
        return kGrowRoom;
    }
    const uint64_t c = grow_new_cap(cap, used, need, realloc_size, page);
    if (c == kPlaceOver) {
        return kGrowReject;
    }
    new_cap = c;
    return kGrowGrow;
}

// The slot of an image grown to new_cap (0: not grown, no slot).
CIOA_PLACE_FN uint64_t grow_slot(uint64_t new_cap, uint64_t align)
{
    return new_cap ? grow_round_up(new_cap, align) : 0;
}

// dev_total: the alignment gap in front of the first slot plus all slots; 0
// when there is no slot.  Does not depend on the arena's end.
CIOA_PLACE_FN uint64_t grow_total(uint64_t top, uint64_t align, uint64_t slots)
{
    const uint64_t base = grow_round_up(top, align);
    if (slots == 0) {
        return 0;
    }
    return base == kPlaceOver ? kPlaceOver : place_add(base - top, slots);
}

// One entry in grow_place: before = the exclusive sum of the slots in front of
// it, slot its own (0: not grown), last: it is entry n - 1.  off: its place,
// base + before.  Returns the kGrow* bits.  The arena must lie inside
// dev_bytes, or nothing is accepted.  Exactly one entry of a batch gets a
// kGrowTop* bit, and only when an image is accepted: the first cut image has
// every slot in front of it accepted and its own offset still <= end, every
// later one starts beyond end; without a cut image the last entry's slot end
// is the sum of all.
CIOA_PLACE_FN uint32_t grow_place_code(uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align,
                                       uint64_t before, uint64_t slot, bool last, uint64_t &off)
{
    const uint64_t base = grow_round_up(top, align);
    off = place_add(base, before);
    const bool arena_ok = end <= dev_bytes && base != kPlaceOver;
    uint32_t code = 0;
    if (slot != 0) {
        if (arena_ok && place_fits(off, slot, end)) {
            code |= kGrowMoved;
        } else if (arena_ok && before != 0 && off != kPlaceOver && off <= end) {
            code |= kGrowTopAt;
        }
    }
    if (last && arena_ok && place_add(before, slot) != 0 && place_fits(off, slot, end)) {
        code |= kGrowTopEnd;                  // off + slot = base + the sum of all slots
    }
    return code;
}

// ---------------------------------------------------------------- the zero fill
// The tail regions [new_off + used, new_off + new_cap) under the planner's
// partition, walked as the append copy walks its records (write_dev_copy.h).
// The planner counts a region's units from the region's own alignment, which
// here is the store's.

// Units [j0, j1) of one region of len bytes at d, by one lane of a wave: as
// copy_units, the stores without the loads.  Body stores are 16-byte stores
// aligned on the destination; the region's head (to the first 16-byte
// boundary) and tail go bytewise.  Nothing outside [d, d + len) is written.
CIOA_COPY_FN void fill_units(uint8_t *d, uint64_t len, uint64_t j0, uint64_t j1, uint32_t nunits, uint32_t lane)
{
    const uint64_t dh = (uint64_t) (uintptr_t) d & 15u;
    const uint64_t end = dh + len;            // positions are relative to A = d - dh
    uint64_t lo = j0 == 0 ? dh : j0 * (uint64_t) kStep;
    const uint64_t hi = j1 == nunits ? end : umin(j1 * (uint64_t) kStep, end);
    if (lo >= hi) {
        return;
    }
    uint8_t *A = d - dh;
    if (lo == dh && dh != 0) {                // the region's head
        const uint64_t he = umin((uint64_t) 16, hi);
        if (dh + lane < he) {
            A[dh + lane] = 0;
        }
        lo = he;
    }
    const uint64_t hi16 = hi & ~(uint64_t) 15;
    const u32x4 z = {0, 0, 0, 0};
    for (uint64_t x = lo + (uint64_t) lane * kGran; x < hi16; x += kRow) {
        *reinterpret_cast<u32x4 *>(A + x) = z;
    }
    const uint64_t tb = umax(lo, hi16);        // the region's tail (hi is a 4 KiB multiple otherwise)
    if (tb + lane < hi) {
        A[tb + lane] = 0;
    }
}

// Wave w of W, one lane of it: the wave's even share of the S steps (copy_wave).
CIOA_COPY_FN void fill_wave(uint8_t *base, const ChunkDesc *desc, const uint64_t *zoff, const uint64_t *zlen,
                            uint32_t n, uint64_t S, uint64_t W, uint64_t w, uint32_t lane)
{
    uint64_t t = (w * S) / W;
    const uint64_t t1 = ((w + 1) * S) / W;
    if (t >= t1) {
        return;
    }
    uint32_t c = record_of(desc, n, t);
    while (t < t1 && c < n) {
        const uint64_t g = desc[c].g;
        const uint32_t ns = desc[c].nsteps;
        if (ns != 0) {
            const uint64_t j1 = umin(t1, g + ns) - g;
            fill_units(base + zoff[c], zlen[c], t - g, j1, ns, lane);
            t = g + j1;
        }
        ++c;
    }
}

// Regions of 1..3 bytes have no step: bytewise, region first, first + stride, ...
CIOA_COPY_FN void fill_tiny(uint8_t *base, const uint64_t *zoff, const uint64_t *zlen, uint32_t n, uint64_t first,
                            uint64_t stride)
{
    for (uint64_t i = first; i < n; i += stride) {
        const uint64_t len = zlen[i];
        if (len != 0 && len < 4) {
            uint8_t *d = base + zoff[i];
            for (uint64_t k = 0; k < len; ++k) {
                d[k] = 0;
            }
        }
    }
}

}  // namespace cioa

#endif
