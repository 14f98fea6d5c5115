// rotate_dev.h -- the arithmetic of rotating full chunk images in HBM
// (rotate_dev_gpu.hip: rotate_sums_wave, rotate_headers, rotate_scan,
// rotate_place, rotate_commit): whether an image is full, the slot of a fresh image and how
// many of them the arena and the list of finished chunks still take, who writes
// the arena's top and the list's count, the fresh image's 24 header bytes, the
// CRC state after its two length bytes, and the wave-level pre-reduction of the
// records variant's sums (rotate_sums_wave, measured and not shipped: DESIGN.md
// §19), lane by lane.  No HIP type, so that the same text
// compiles for the device and, stand-alone on the host, under ASan + UBSan
// (tools/rotate_check.cpp, `make rotatecheck`).  Not installed.
#ifndef CIOA_ROTATE_DEV_H
#define CIOA_ROTATE_DEV_H

#include <stdint.h>

#include "grow_dev.h"

namespace cioa {

constexpr uint32_t kRotBlock = kGrowBlock;             // images per workgroup of the header, place and commit kernels
constexpr uint32_t kRotSumBlock = 256;                 // records per workgroup of the sums kernel: 4 waves
constexpr uint32_t kRotLanes = 64;                     // a wave
constexpr uint32_t kRotNoImage = 0xffffffffu;          // the key of a lane without a record: never a valid index
constexpr uint32_t kRotPoly = 0xEDB88320u;             // CRC-32, reflected
// What rotate_place leaves per image for rotate_commit (bits).
constexpr uint32_t kRotAccepted = 1;     // the image is rotated
constexpr uint32_t kRotEndAt = 2;        // the first cut image behind accepted ones: it writes top and count
constexpr uint32_t kRotEndLast = 4;      // the last entry of a batch in which nothing is cut: it writes them
// rot_decide's verdicts.
constexpr int kRotReject = 0, kRotKeep = 1, kRotFull = 2;

// a + b > c in unbounded arithmetic.
CIOA_PLACE_FN bool rot_sum_exceeds(uint64_t a, uint64_t b, uint64_t c)
{
    return a + b < a || a + b > c;
}

// Rules 2..4 for an image that passed the write path's image check (used = 24
// + meta + content <= cap): rejected (it shares a byte with the arena's free
// part, or it is full and its metadata does not fit new_cap), kept (not full),
// or full and to be rotated.
CIOA_PLACE_FN int rot_decide(uint64_t off, uint64_t cap, uint32_t meta, uint64_t content, uint64_t need,
                             uint64_t limit, uint64_t new_cap, uint64_t top, uint64_t end)
{
    if (grow_in_arena(off, cap, top, end)) {
        return kRotReject;
    }
    const uint64_t used = kReadHdr + meta + content;
    const bool full = content > 0 && (rot_sum_exceeds(used, need, cap) ||
                                      (limit != 0 && rot_sum_exceeds(content, need, limit)));
    if (!full) {
        return kRotKeep;
    }
    return kReadHdr + meta <= new_cap ? kRotFull : kRotReject;
}

// The slots of count fresh images, each of `slot` bytes: every image that
// reaches the placement has the same slot, so the exclusive sum of the slots
// before one is its ordinal times the slot.  kPlaceOver when that leaves 64 bits.
CIOA_PLACE_FN uint64_t rot_slots(uint64_t count, uint64_t slot)
{
    if (slot == kPlaceOver || (count != 0 && slot > kPlaceOver / count)) {
        return kPlaceOver;
    }
    return count * slot;
}

// dev_total[0]: the alignment gap in front of the first slot plus all slots; 0
// when no image reaches the placement.  Does not depend on the arena's end.
CIOA_PLACE_FN uint64_t rot_total(uint64_t top, uint64_t align, uint64_t count, uint64_t slot)
{
    return grow_total(top, align, rot_slots(count, slot));
}

// Is the image with ordinal j among those that reach the placement accepted?
// Its slot [base + j slot, + slot) must end inside the arena, the arena inside
// dev_bytes, and its list index have0 + j lie below the list's capacity.  Both
// tests are monotone in j.
CIOA_PLACE_FN bool rot_accepts(uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align, uint64_t slot,
                               uint64_t have0, uint64_t list_cap, uint64_t j)
{
    const uint64_t base = grow_round_up(top, align);
    if (end > dev_bytes || base == kPlaceOver) {
        return false;
    }
    const uint64_t k = place_add(have0, j);
    return k != kPlaceOver && k < list_cap && place_fits(place_add(base, rot_slots(j, slot)), slot, end);
}

// One entry in rotate_place: before = the number of images in front of it that
// reach the placement, reach: it does itself, last: it is entry n - 1.  off:
// its fresh image's place, k: its list index (both meaningful with
// kRotAccepted only).  Returns the kRot* bits.  Exactly one entry of a batch
// gets a kRotEnd* bit, and only when an image is accepted: the first cut image
// has every image in front of it accepted, every later one has a cut image in
// front of it; without a cut image the last entry ends the batch.
CIOA_PLACE_FN uint32_t rot_place_code(uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align, uint64_t slot,
                                      uint64_t have0, uint64_t list_cap, uint64_t before, bool reach, bool last,
                                      uint64_t &off, uint64_t &k)
{
    off = place_add(grow_round_up(top, align), rot_slots(before, slot));
    k = place_add(have0, before);
    uint32_t code = 0;
    if (reach) {
        if (rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, before)) {
            code |= kRotAccepted;
        } else if (before != 0 && rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, before - 1)) {
            code |= kRotEndAt;
        }
    }
    const uint64_t all = before + (reach ? 1 : 0);
    if (last && all != 0 && rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, all - 1)) {
        code |= kRotEndLast;
    }
    return code;
}

// What the entry with a kRotEnd* bit writes, from its own (off, k) of
// rot_place_code -- rotate_commit must not read the words it replaces.  An
// entry that is not accepted stands where the next slot would begin; an
// accepted one (the batch's last entry) ends the batch with its own slot.  All
// accepted slots fit, so nothing wraps.
CIOA_PLACE_FN void rot_end_values(uint32_t code, uint64_t off, uint64_t k, uint64_t slot, uint64_t &top,
                                  uint64_t &count)
{
    const bool own = (code & kRotAccepted) != 0;
    top = own ? off + slot : off;
    count = own ? k + 1 : k;
}

// write_init_header's bytes 0..23 with the metadata length at 22..23.
CIOA_PLACE_FN void rot_fresh_header(uint8_t *h, uint32_t meta, bool checksum)
{
    h[0] = 0xc1;
    h[1] = 0x00;
    h[2] = checksum ? 0xff : 0;                // crc_finalize of the empty content, htonl, in an 8-byte crc_t
    h[3] = checksum ? 0x12 : 0;
    h[4] = checksum ? 0xd9 : 0;
    h[5] = checksum ? 0x41 : 0;
    for (uint32_t k = 6; k < 22; ++k) {
        h[k] = 0;
    }
    h[22] = (uint8_t) (meta >> 8);
    h[23] = (uint8_t) meta;
}

// crc_update over one byte, bit by bit (raw state).
CIOA_PLACE_FN uint32_t rot_crc_byte(uint32_t crc, uint32_t b)
{
    crc ^= b;
    for (int k = 0; k < 8; ++k) {
        crc = (crc >> 1) ^ (kRotPoly & (0u - (crc & 1u)));
    }
    return crc;
}

// crc_update(crc_init(), bytes 22..23): 0xBE26ED00 without metadata.
CIOA_PLACE_FN uint32_t rot_len_seed(uint32_t meta)
{
    return rot_crc_byte(rot_crc_byte(0xffffffffu, (meta >> 8) & 0xffu), meta & 0xffu);
}

// ---------------------------------------------------------------- the sums' pre-reduction
// Lane l of a wave holds record r's image index (its key; kRotNoImage without a
// record) and clamped length.  A run is a maximal range of lanes with one key;
// its last lane adds the run's sum to the image's need with ONE atomic.

// A lane is a run head where its key differs from the previous lane's.
CIOA_PLACE_FN bool rot_run_head(uint32_t lane, uint32_t key, uint32_t prev_key)
{
    return lane == 0 || key != prev_key;
}

// One step of the segmented inclusive scan, distance d: (v, f) are the lane's
// sum so far and whether the range it covers holds a run head; (v_up, f_up)
// those of lane - d.
CIOA_PLACE_FN void rot_seg_step(uint32_t lane, uint32_t d, uint64_t &v, bool &f, uint64_t v_up, bool f_up)
{
    if (lane >= d) {
        if (!f) {
            v += v_up;
        }
        f = f || f_up;
    }
}

#ifndef __HIPCC__
// The whole wave over explicit arrays, as the kernel does it with lane
// shuffles (host only: tools/rotate_check.cpp): sum[l] the inclusive sum of l's run up to l, issue[l] whether l is
// the last lane of a run with a valid key (it issues the atomic).
inline void rot_wave_sums(const uint32_t *key, const uint64_t *len, uint32_t n_img, uint64_t *sum, bool *issue)
{
    bool f[kRotLanes], head[kRotLanes];
    for (uint32_t l = 0; l < kRotLanes; ++l) {
        head[l] = rot_run_head(l, key[l], l ? key[l - 1] : 0);
        f[l] = head[l];
        sum[l] = len[l];
    }
    for (uint32_t d = 1; d < kRotLanes; d <<= 1) {
        uint64_t v_up[kRotLanes];
        bool f_up[kRotLanes];
        for (uint32_t l = 0; l < kRotLanes; ++l) {    // the shuffle: every lane reads before any lane writes
            v_up[l] = l >= d ? sum[l - d] : 0;
            f_up[l] = l >= d ? f[l - d] : false;
        }
        for (uint32_t l = 0; l < kRotLanes; ++l) {
            rot_seg_step(l, d, sum[l], f[l], v_up[l], f_up[l]);
        }
    }
    for (uint32_t l = 0; l < kRotLanes; ++l) {
        issue[l] = (l + 1 == kRotLanes || head[l + 1]) && key[l] < n_img;
    }
}
#endif

}  // namespace cioa

#endif
