// write_dev_copy.h -- the arithmetic of the batched append copy
// (write_dev_gpu.hip: append_copy): which record a step belongs to and which
// bytes one lane moves for a range of a record's units.  No HIP type, so that
// the same text compiles for the device and, stand-alone on the host, under
// ASan + UBSan (tools/copy_check.cpp, `make copycheck`).  Not installed.
#ifndef CIOA_WRITE_DEV_COPY_H
#define CIOA_WRITE_DEV_COPY_H

#include <stdint.h>

#include "cio_plan.h"

#ifdef __HIPCC__
#define CIOA_COPY_FN __device__ __forceinline__
#else
#define CIOA_COPY_FN inline
#endif

namespace cioa {

typedef uint32_t u32x4 __attribute__((vector_size(16)));
// 16 bytes at any address: the backend emits one unaligned 16-byte vector load.
struct __attribute__((packed)) Unaligned16 {
    u32x4 v;
};

CIOA_COPY_FN uint64_t umin(uint64_t a, uint64_t b)
{
    return a < b ? a : b;
}

CIOA_COPY_FN uint64_t umax(uint64_t a, uint64_t b)
{
    return a > b ? a : b;
}

// First record whose end step is > t (t < S): never one without steps.
CIOA_COPY_FN uint32_t record_of(const ChunkDesc *desc, uint32_t n, uint64_t t)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (desc[mid].g + desc[mid].nsteps > t) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    return lo;
}

// Units [j0, j1) of one record of len bytes, by one wave.  The units tile the
// DESTINATION: with A = d rounded down to 16 bytes, unit j is [A + 4096 j,
// A + 4096 (j + 1)) cut to the record, and the record's last unit (j = nunits
// - 1) runs to the record's end -- the planner counts units from the source's
// alignment, which can differ from the destination's count by one either way.
// So every body store is a 16-byte store aligned on the destination, the
// source is read with unaligned 16-byte loads, and only the record's own head
// (to the first 16-byte boundary) and tail go bytewise.
CIOA_COPY_FN void copy_units(uint8_t *d, const uint8_t *s, uint64_t len, uint64_t j0, uint64_t j1,
                                           uint32_t nunits, uint32_t lane)
{
    const uint64_t dh = (uint64_t) (uintptr_t) d & 15u;
    const uint64_t end = dh + len;            // positions are relative to A = d - dh
    uint64_t lo = j0 == 0 ? dh : j0 * (uint64_t) kStep;
    const uint64_t hi = j1 == nunits ? end : umin(j1 * (uint64_t) kStep, end);
    if (lo >= hi) {
        return;
    }
    uint8_t *A = d - dh;
    const uint8_t *sA = s - dh;               // source of position x: sA + x (x >= dh)
    if (lo == dh && dh != 0) {                // the record's head
        const uint64_t he = umin((uint64_t) 16, hi);
        if (dh + lane < he) {
            A[dh + lane] = sA[dh + lane];
        }
        lo = he;
    }
    const uint64_t hi16 = hi & ~(uint64_t) 15;
    uint64_t x = lo + (uint64_t) lane * kGran;
    // four 1 KiB rows per iteration: the loads are issued before the stores
    for (; x + 3 * kRow < hi16; x += 4 * kRow) {
        const u32x4 v0 = reinterpret_cast<const Unaligned16 *>(sA + x)->v;
        const u32x4 v1 = reinterpret_cast<const Unaligned16 *>(sA + x + kRow)->v;
        const u32x4 v2 = reinterpret_cast<const Unaligned16 *>(sA + x + 2 * kRow)->v;
        const u32x4 v3 = reinterpret_cast<const Unaligned16 *>(sA + x + 3 * kRow)->v;
        *reinterpret_cast<u32x4 *>(A + x) = v0;
        *reinterpret_cast<u32x4 *>(A + x + kRow) = v1;
        *reinterpret_cast<u32x4 *>(A + x + 2 * kRow) = v2;
        *reinterpret_cast<u32x4 *>(A + x + 3 * kRow) = v3;
    }
    for (; x < hi16; x += kRow) {
        *reinterpret_cast<u32x4 *>(A + x) = reinterpret_cast<const Unaligned16 *>(sA + x)->v;
    }
    const uint64_t tb = umax(lo, hi16);        // the record's tail (hi is a 4 KiB multiple otherwise)
    if (tb + lane < hi) {
        A[tb + lane] = sA[tb + lane];
    }
}

// Wave w of W, one lane of it: the wave's even share of the S steps,
// [w S / W, (w + 1) S / W) (S < 2^40 by the planner's check, W < 2^16),
// whatever records they belong to.
CIOA_COPY_FN void copy_wave(uint8_t *dst_base, const uint8_t *src_base, const ChunkDesc *desc, const uint64_t *soff,
                            const uint64_t *slen, const uint64_t *dst, uint32_t n, uint64_t S, uint64_t W,
                            uint64_t w, uint32_t lane)
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
            copy_units(dst_base + dst[c], src_base + soff[c], slen[c], t - g, j1, ns, lane);
            t = g + j1;
        }
        ++c;
    }
}

// Records of 1..3 bytes have no step: bytewise, record first, first + stride, ...
CIOA_COPY_FN void copy_tiny(uint8_t *dst_base, const uint8_t *src_base, const uint64_t *soff, const uint64_t *slen,
                            const uint64_t *dst, uint32_t n, uint64_t first, uint64_t stride)
{
    for (uint64_t i = first; i < n; i += stride) {
        const uint64_t len = slen[i];
        if (len != 0 && len < 4) {
            uint8_t *d = dst_base + dst[i];
            const uint8_t *s = src_base + soff[i];
            for (uint64_t k = 0; k < len; ++k) {
                d[k] = s[k];
            }
        }
    }
}

}  // namespace cioa

#endif
