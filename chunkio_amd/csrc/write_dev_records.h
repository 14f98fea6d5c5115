// write_dev_records.h -- the arithmetic of the grouped append
// (write_records_gpu.hip: rec_images, rec_scan_local, rec_scan_groups,
// rec_place): where a run of records starts, what a record adds to its run's
// running sum, how two partial sums of a SEGMENTED scan combine, how much room
// an image has, and when a record is accepted.  No HIP type, so that the same
// text compiles for the device and, stand-alone on the host, under ASan + UBSan
// (tools/records_check.cpp, `make recordscheck`).  Not installed.
#ifndef CIOA_WRITE_DEV_RECORDS_H
#define CIOA_WRITE_DEV_RECORDS_H

#include <stdint.h>

#include "read_dev_place.h"

namespace cioa {

constexpr uint32_t kRecBlock = 1024;                // records per workgroup of the record and place kernels
constexpr uint64_t kRecMaxContent = 0xffffffffull;  // the length field is 32 bits
constexpr uint64_t kRecHdr = kReadHdr;

// A partial result of the segmented scan over records [a, b]: flag, whether a
// run starts in (a, b] or at a; sum, the lengths from the last such start (from
// a when there is none) to b, saturating.
struct RecSeg {
    uint32_t flag;
    uint64_t sum;
};

// The empty range: the operator's left and right identity.
CIOA_PLACE_FN RecSeg rec_none()
{
    const RecSeg r = {0, 0};
    return r;
}

// The scan's combine step, a = an earlier range, b = the one that follows it.
// Associative, so any grouping of the records -- by workgroup, by pass of the
// scan workgroup -- gives the sequential per-run running sum.
CIOA_PLACE_FN RecSeg rec_combine(RecSeg a, RecSeg b)
{
    const RecSeg r = {a.flag | b.flag, b.flag ? b.sum : place_add(a.sum, b.sum)};
    return r;
}

// Record r starts a run: the first record, or another image than its
// predecessor's.
CIOA_PLACE_FN bool rec_head(uint64_t r, uint32_t img, uint32_t prev)
{
    return r == 0 || img != prev;
}

// The grouping is malformed at record r: its image index is outside the batch,
// or lower than its predecessor's.
CIOA_PLACE_FN bool rec_malformed(uint64_t r, uint32_t img, uint32_t prev, uint64_t n_img)
{
    return img >= n_img || (r != 0 && img < prev);
}

// What record (off, len) adds to its run's sum: its length, or the saturated
// value when its source range overflows or leaves src_bytes, or when it is
// longer than a content can be.  A record of length 0 has no source range.
CIOA_PLACE_FN uint64_t rec_value(uint64_t off, uint64_t len, uint64_t src_bytes)
{
    if (len == 0) {
        return 0;
    }
    if (len > kRecMaxContent || off + len < off || off + len > src_bytes) {
        return kPlaceOver;
    }
    return len;
}

// The bytes an image of capacity cap (>= 24 + meta + content: the image check)
// can still take: up to its capacity, and up to a content of 2^32 - 1.
CIOA_PLACE_FN uint64_t rec_room(uint64_t cap, uint32_t meta, uint64_t content)
{
    const uint64_t by_cap = cap - kRecHdr - meta - content, by_field = kRecMaxContent - content;
    return by_cap < by_field ? by_cap : by_field;
}

// The exclusive running sum of record r's run: nothing for a run's first
// record; otherwise carry (everything before r's workgroup) combined with local
// (the records of r's workgroup before r).
CIOA_PLACE_FN uint64_t rec_before(bool head, RecSeg carry, RecSeg local)
{
    return head ? 0 : rec_combine(carry, local).sum;
}

// Record r, of value v (rec_value), whose run's sum before it is `before`, is
// accepted when its image passed the check and the run still fits up to and
// including r.  A rejected record stays in the sum, so the accepted records of
// a run are exactly those before the first rejected one.
CIOA_PLACE_FN bool rec_accept(bool img_ok, uint64_t before, uint64_t v, uint64_t room)
{
    return img_ok && before != kPlaceOver && place_add(before, v) <= room;
}

}  // namespace cioa

#endif
