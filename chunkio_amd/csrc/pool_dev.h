// pool_dev.h -- the arithmetic of recycling drained chunk slots in HBM
// (pool_dev_gpu.hip: release_headers, release_scan, release_place,
// release_commit, rotpool_place, rotpool_commit): when a pool's four words are
// sound, which entries of a release reach the placement and how many the pool
// still takes, who writes the pool's count, where a kept entry of a compacted
// list goes, how many pool entries a rotation may use, where the fresh image
// with ordinal j lies (a pool entry or an arena slot), and who writes the
// arena's top, the list's count and the pool's count.  No HIP type, so that
// the same text compiles for the device and, stand-alone on the host, under
// ASan + UBSan (tools/pool_check.cpp, `make poolcheck`).  Not installed.
#ifndef CIOA_POOL_DEV_H
#define CIOA_POOL_DEV_H

#include <stdint.h>

#include "rotate_dev.h"

namespace cioa {

constexpr uint32_t kPoolBlock = kRotBlock;             // entries per workgroup of the release kernels
// The pool's four words (dev_pool[]).
constexpr uint32_t kPoolCount = 0, kPoolCap = 1, kPoolCls = 2, kPoolAlign = 3;
// What release_headers and release_place leave per entry for release_commit (bits).
constexpr uint32_t kRelIn = 1;           // the entry is among the first m: it is looked at
constexpr uint32_t kRelReach = 2;        // it reaches the placement
constexpr uint32_t kRelAccepted = 4;     // it is pushed and its slot marked free
constexpr uint32_t kRelEndAt = 8;        // the first cut entry behind accepted ones: it writes the pool's count
constexpr uint32_t kRelEndLast = 16;     // entry m - 1 of a batch in which nothing is cut: it writes it
// What rotpool_place leaves for rotpool_commit beside rotate's kRot* bits.
constexpr uint32_t kRotPoolTop = 8;      // the ending entry writes the arena's top (an arena slot was taken)
constexpr uint32_t kRotPoolPop = 16;     // the ending entry writes the pool's count (a pool entry was taken)
constexpr uint32_t kPoolNoImage = 0xffffffffu;         // dev_img of a vacated list entry

CIOA_PLACE_FN bool pool_sound(uint64_t count, uint64_t cap, uint64_t cls, uint64_t pal)
{
    return count <= cap && cls >= kReadHdr && pal != 0 && (pal & (pal - 1)) == 0 && pal <= 4096;
}

// The entries a release looks at: n, or min(n, dev_count[0]).
CIOA_PLACE_FN uint64_t pool_m(uint64_t n, bool has_count, uint64_t count0)
{
    return has_count && count0 < n ? count0 : n;
}

// Rule 4: the slot belongs to the pool's size class and alignment (a sound pool).
CIOA_PLACE_FN bool pool_takes(uint64_t off, uint64_t cap, uint64_t cls, uint64_t pal)
{
    return cap >= cls && (off & (pal - 1)) == 0;
}

// The entries a sound pool still takes; 0 for an unsound one.
CIOA_PLACE_FN uint64_t pool_room(uint64_t count, uint64_t cap, uint64_t cls, uint64_t pal)
{
    return pool_sound(count, cap, cls, pal) ? cap - count : 0;
}

// One entry in release_place: before = the number of entries in front of it
// that reach the placement, reach: it does itself, last: it is entry m - 1.
// slot: its index in the pool's arrays, count + before.  Returns the kRel*
// bits of the placement.  Exactly one entry of a batch gets a kRelEnd* bit, and
// only when an entry is accepted (rot_place_code's pattern): the first cut
// entry has every entry in front of it accepted; without a cut entry the last
// one ends the batch.  No entry reaches the placement of an unsound pool.
CIOA_PLACE_FN uint32_t pool_release_code(uint64_t count, uint64_t room, uint64_t before, bool reach, bool last,
                                         uint64_t &slot)
{
    slot = place_add(count, before);
    uint32_t code = 0;
    if (reach) {
        if (before < room) {
            code |= kRelAccepted;
        } else if (before != 0 && before - 1 < room) {
            code |= kRelEndAt;
        }
    }
    const uint64_t all = before + (reach ? 1 : 0);
    if (last && all != 0 && all - 1 < room) {
        code |= kRelEndLast;
    }
    return code;
}

// What the entry with a kRelEnd* bit writes into the pool's count, from its own
// slot of pool_release_code: a cut entry stands where the next push would go;
// an accepted one (the batch's last entry) ends the batch with its own push.
CIOA_PLACE_FN uint64_t pool_release_end(uint32_t code, uint64_t slot)
{
    return (code & kRelAccepted) ? slot + 1 : slot;
}

// Where the kept entry i of a compacted list goes: the accepted entries are the
// first min(reach, room) that reach the placement, so min(before, room) of them
// lie in front of it.
CIOA_PLACE_FN uint64_t pool_kept_pos(uint64_t i, uint64_t before, uint64_t room)
{
    return i - (before < room ? before : room);
}

// dev_total[1]: the kept entries among the first m.
CIOA_PLACE_FN uint64_t pool_kept_total(uint64_t m, uint64_t reach, uint64_t room)
{
    return m - (reach < room ? reach : room);
}

// ---------------------------------------------------------------- rotating from the pool

// F: the pool entries a rotation to new_cap / align may use.
CIOA_PLACE_FN uint64_t pool_usable(uint64_t count, uint64_t cap, uint64_t cls, uint64_t pal, uint64_t new_cap,
                                   uint64_t align)
{
    return pool_sound(count, cap, cls, pal) && new_cap <= cls && (pal & (align - 1)) == 0 ? count : 0;
}

// Is the image with ordinal j among those that reach the placement accepted?
// Its list index have0 + j must lie below the list's capacity; from ordinal F
// on its arena slot [base + (j - F) slot, + slot) must end inside the arena and
// the arena inside dev_bytes.  Monotone in j: the list test is, and so is the
// arena test from F on.
CIOA_PLACE_FN bool pool_rot_accepts(uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align, uint64_t slot,
                                    uint64_t have0, uint64_t list_cap, uint64_t F, uint64_t j)
{
    const uint64_t k = place_add(have0, j);
    if (k == kPlaceOver || k >= list_cap) {
        return false;
    }
    if (j < F) {
        return true;
    }
    const uint64_t base = grow_round_up(top, align);
    if (end > dev_bytes || base == kPlaceOver) {
        return false;
    }
    return place_fits(place_add(base, rot_slots(j - F, slot)), slot, end);
}

// One entry in rotpool_place, as rot_place_code: off is the ARENA slot of an
// ordinal >= F (an ordinal below F takes pool entry count - 1 - before; the
// kernel reads it), k the list index.
CIOA_PLACE_FN uint32_t pool_rot_place_code(uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align,
                                           uint64_t slot, uint64_t have0, uint64_t list_cap, uint64_t F,
                                           uint64_t before, bool reach, bool last, uint64_t &off, uint64_t &k)
{
    off = place_add(grow_round_up(top, align), rot_slots(before < F ? 0 : before - F, slot));
    k = place_add(have0, before);
    uint32_t code = 0;
    if (reach) {
        if (pool_rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, F, before)) {
            code |= kRotAccepted;
        } else if (before != 0 && pool_rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, F, before - 1)) {
            code |= kRotEndAt;
        }
    }
    const uint64_t all = before + (reach ? 1 : 0);
    if (last && all != 0 && pool_rot_accepts(top, end, dev_bytes, align, slot, have0, list_cap, F, all - 1)) {
        code |= kRotEndLast;
    }
    return code;
}

// What the entry with a kRotEnd* bit writes, computed in rotpool_place from the
// words as they were -- rotpool_commit must not read the words it replaces.
// accepted = before + (the entry itself is accepted).  Returns kRotPoolTop /
// kRotPoolPop for the words that change beside the list's count, which always
// does.  All accepted slots fit, so nothing wraps.
CIOA_PLACE_FN uint32_t pool_rot_end_values(uint32_t code, uint64_t before, uint64_t F, uint64_t top, uint64_t align,
                                           uint64_t slot, uint64_t have0, uint64_t pool_count, uint64_t &new_top,
                                           uint64_t &count, uint64_t &new_pool)
{
    const uint64_t accepted = before + ((code & kRotAccepted) ? 1 : 0);
    const uint64_t from_pool = accepted < F ? accepted : F;
    count = have0 + accepted;
    new_pool = pool_count - from_pool;
    new_top = grow_round_up(top, align) + (accepted - from_pool) * slot;
    return (accepted > from_pool ? kRotPoolTop : 0) | (from_pool != 0 ? kRotPoolPop : 0);
}

// dev_total[0]: the alignment gap plus the arena slots of the reach - F images
// the pool does not serve; 0 when the pool serves them all.
CIOA_PLACE_FN uint64_t pool_rot_total(uint64_t top, uint64_t align, uint64_t reach, uint64_t F, uint64_t slot)
{
    return rot_total(top, align, reach > F ? reach - F : 0, slot);
}

}  // namespace cioa

#endif
