// route.h -- the arithmetic of routing records to chunk images in HBM by their
// metadata (route_gpu.hip: route_tag_regions, route_probe, route_count): when a
// tag is well-formed (R2), the lower bound of a key in the directory, the walk
// over the candidates of a key in a sorted array that may hold garbage (R3,
// R6), the choice among them given a verdict per candidate (R4), and the
// packed counts of the totals' scan (R5).  No HIP type, so that the same text
// compiles for the device and, stand-alone on the host, under ASan + UBSan
// (tools/route_check.cpp, `make routecheck`).  Not installed.
#ifndef CIOA_ROUTE_H
#define CIOA_ROUTE_H

#include <stdint.h>

#include "image_dev.h"

namespace cioa {

constexpr uint32_t kRouteBlock = 1024;          // entries per workgroup of the region, count and list kernels
constexpr uint64_t kRouteMaxTag = 65535;        // the metadata length field has 16 bits
constexpr uint32_t kRouteNone = 0xffffffffu;    // route_match: no candidate passed
constexpr uint32_t kRouteEmptyKey = 0xffffffffu;   // R0: the raw CRC-32 state before any byte
constexpr int32_t kRouteOk = 0, kRouteError = -1, kRouteRetry = -2;   // CIO_OK, CIO_ERROR, CIO_RETRY

// R2: a tag of length 0 has no source range; any other needs len <= 65535 and
// [off, off + len) inside tag_bytes without a wrap.
CIOA_PLACE_FN bool route_tag_ok(uint64_t off, uint64_t len, uint64_t tag_bytes)
{
    return len == 0 || (len <= kRouteMaxTag && range_ok(off, len, tag_bytes));
}

// The first position of keys[0 .. n) whose key is not below `key`, n when
// there is none.  Over an array that is not sorted it still ends after at most
// 32 steps with a position in 0 .. n, and reads keys[0 .. n) alone.
CIOA_PLACE_FN uint32_t route_lower_bound(const uint32_t *keys, uint32_t n, uint32_t key)
{
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] < key) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    return lo;
}

// R3 + R4: the candidates of `key` are the positions j from its lower bound on
// while keys[j] == key, at most n of them, with imgs[j] < n -- an entry >= n is
// skipped, so no load leaves the arrays whatever they hold.  pass(i) is the
// verdict on image i (the gate, the image check, the lengths, the bytes); the
// match is the image of the first candidate that passes, kRouteNone when none
// does.  With a sorted directory whose ties keep ascending i that is the lowest
// such i.
template <class Pass>
CIOA_PLACE_FN uint32_t route_match(const uint32_t *keys, const uint32_t *imgs, uint32_t n, uint32_t key, Pass pass)
{
    for (uint32_t j = route_lower_bound(keys, n, key); j < n && keys[j] == key; ++j) {
        const uint32_t i = imgs[j];
        if (i < n && pass(i)) {
            return i;
        }
    }
    return kRouteNone;
}

// R5, R7: a record's status from what was found.
CIOA_PLACE_FN int32_t route_status(bool dir_ok, bool tag_ok, bool matched)
{
    return !dir_ok || !tag_ok ? kRouteError : matched ? kRouteOk : kRouteRetry;
}

// The totals' scan carries two counts in one 64-bit word: the missed records
// in the low half (their exclusive sum is a record's place in the miss list),
// the matched in the high half.  Neither exceeds n_rec < 2^32, so no carry
// crosses the halves.
CIOA_PLACE_FN uint64_t route_count_pack(int32_t status)
{
    return status == kRouteRetry ? 1ull : status == kRouteOk ? 1ull << 32 : 0;
}

CIOA_PLACE_FN uint64_t route_count_missed(uint64_t packed)
{
    return packed & 0xffffffffull;
}

CIOA_PLACE_FN uint64_t route_count_matched(uint64_t packed)
{
    return packed >> 32;
}

}  // namespace cioa

#endif
