// pool_set.h -- the arithmetic of the size-classed pool set in HBM
// (pool_set_gpu.hip: relset_headers, relset_scan, relset_place, relset_kscan,
// relset_kmove, relset_commit, growset_class, growset_cscan, growset_serve,
// growset_ascan, growset_place, growset_commit): when the words of a set of K
// classes are sound, which class a released slot is filed into, which class a
// growing image asks, an entry's stable rank among the entries of its class
// (inside its wave from three ballots, across the waves of its workgroup a
// [wave][class] table, across the workgroups a class-major table), how many
// entries each class takes or serves, what every set word becomes, whether a
// pool entry may be handed to an image, and the capacity of an arena-bound
// slot.  No HIP type, so that the same text compiles for the device and,
// stand-alone on the host, under ASan + UBSan (tools/pool_set_check.cpp,
// `make poolsetcheck`).  Not installed.
#ifndef CIOA_POOL_SET_H
#define CIOA_POOL_SET_H

#include <stdint.h>

#include "pool_dev.h"
#include "sort_records.h"

namespace cioa {

constexpr uint32_t kPoolSetMax = 8;                    // CIOA_POOL_SET_MAX
constexpr uint32_t kSetNone = kPoolSetMax;             // the class index of an entry without a class
constexpr uint32_t kSetBits = 3;                       // ballots per rank: the bits of a class index
constexpr uint32_t kSetBlock = kGrowBlock;             // entries per workgroup of every kernel of both chains
constexpr uint32_t kSetWave = 64;
constexpr uint32_t kSetWaves = kSetBlock / kSetWave;
constexpr uint32_t kSetClsShift = 8;                   // an entry's class in bits 8..11 of its code word
// What growset_serve leaves per image for growset_place and growset_commit beside grow's kGrow* bits.
constexpr uint32_t kSetServed = 16;      // the image takes a pool entry (checked: it is moved there)
constexpr uint32_t kSetArena = 32;       // the image is arena-bound

// The per-call words behind the class table in the writer's scratch (64-bit
// words from set_words_at): the classes' totals, the end values of the set's
// count words, and the mask of the classes whose word changes.
constexpr uint32_t kSetWTotal = 0, kSetWEnd = kPoolSetMax, kSetWMask = 2 * kPoolSetMax, kSetWords = 2 * kPoolSetMax + 1;

// The class table is class-major, as the sort's histogram table is
// digit-major: entry (class k, workgroup wg) of nb workgroups.
CIOA_SORT_FN uint32_t set_tab_at(uint32_t k, uint32_t wg, uint32_t nb)
{
    return k * nb + wg;
}

// The first of the per-call words behind the table.
CIOA_SORT_FN uint32_t set_words_at(uint32_t nb)
{
    return kPoolSetMax * nb;
}

// The 64-bit scratch words a batch of nb workgroups needs; the sort's
// histogram table, kSortRadix 32-bit words per workgroup, holds them.
CIOA_SORT_FN uint32_t set_scratch_words(uint32_t nb)
{
    return kPoolSetMax * nb + kSetWords;
}
static_assert(kPoolSetMax + kSetWords <= kSortRadix / 2, "the sort's table of one workgroup holds a set batch's words");

// The set is sound: every class is (pool_sound), no capacity word exceeds the
// stride between two classes' entries, and cls rises strictly with k.
CIOA_PLACE_FN bool set_sound(const uint64_t *set, uint32_t n_cls, uint64_t stride)
{
    uint64_t below = 0;
    for (uint32_t k = 0; k < n_cls; ++k) {
        const uint64_t *p = set + 4 * k;
        if (!pool_sound(p[kPoolCount], p[kPoolCap], p[kPoolCls], p[kPoolAlign]) || p[kPoolCap] > stride ||
            (k != 0 && p[kPoolCls] <= below)) {
            return false;
        }
        below = p[kPoolCls];
    }
    return true;
}

// Rule 4': the class of a released slot in a sound set -- the largest k with
// cls_k <= cap and off a multiple of pal_k; kSetNone when there is none.
CIOA_PLACE_FN uint32_t set_release_class(const uint64_t *set, uint32_t n_cls, uint64_t off, uint64_t cap)
{
    uint32_t c = kSetNone;
    for (uint32_t k = 0; k < n_cls; ++k) {
        if (pool_takes(off, cap, set[4 * k + kPoolCls], set[4 * k + kPoolAlign])) {
            c = k;
        }
    }
    return c;
}

// The entries class k still takes: capacity - count of a sound set, else 0.
CIOA_PLACE_FN uint64_t set_room(const uint64_t *set, uint32_t k, bool sound)
{
    return sound ? set[4 * k + kPoolCap] - set[4 * k + kPoolCount] : 0;
}

// S1: the classes a grow with `align` may use, as a bit mask.
CIOA_PLACE_FN uint32_t set_usable(const uint64_t *set, uint32_t n_cls, uint64_t stride, uint64_t align)
{
    if (!set_sound(set, n_cls, stride)) {
        return 0;
    }
    uint32_t mask = 0;
    for (uint32_t k = 0; k < n_cls; ++k) {
        if ((set[4 * k + kPoolAlign] & (align - 1)) == 0) {
            mask |= 1u << k;
        }
    }
    return mask;
}

// S2: the smallest usable k with cls_k >= new_cap (new_cap != 0); kSetNone
// when there is none.
CIOA_PLACE_FN uint32_t set_grow_class(const uint64_t *set, uint32_t n_cls, uint32_t usable, uint64_t new_cap)
{
    for (uint32_t k = 0; k < n_cls; ++k) {
        if (((usable >> k) & 1u) && set[4 * k + kPoolCls] >= new_cap) {
            return k;
        }
    }
    return kSetNone;
}

// F_k: the entries of a usable class, else 0.
CIOA_PLACE_FN uint64_t set_serves(const uint64_t *set, uint32_t k, uint32_t usable)
{
    return ((usable >> k) & 1u) ? set[4 * k + kPoolCount] : 0;
}

// S3: may the pool entry [off, off + cap) be handed to an image of class cls
// under `align`?  Inside dev_bytes without a wrap, at least the class, aligned.
CIOA_PLACE_FN bool set_entry_ok(uint64_t off, uint64_t cap, uint64_t dev_bytes, uint64_t cls, uint64_t align)
{
    return off + cap >= off && off + cap <= dev_bytes && cap >= cls && (off & (align - 1)) == 0;
}

// S4: the capacity of an arena-bound image: its class's, so that the slot
// comes back to exactly that class, or new_cap without a class.
CIOA_PLACE_FN uint64_t set_arena_cap(const uint64_t *set, uint32_t c, uint64_t new_cap)
{
    return c != kSetNone ? set[4 * c + kPoolCls] : new_cap;
}

// A lane's match mask: the lanes of its wave that hold an entry with its own
// class, from the ballot of the lanes that hold a class at all and the three
// ballots of the class index's bits (sort_match_step, sort_records.h).
CIOA_PLACE_FN uint64_t set_match(uint64_t holds, const uint64_t *ballot, uint32_t c)
{
    uint64_t match = holds;
    for (uint32_t bit = 0; bit < kSetBits; ++bit) {
        match = sort_match_step(match, ballot[bit], c, bit);
    }
    return match;
}

// wcount[wave * kPoolSetMax + k] holds the entries of `wave` with class k; the
// "thread" of k turns its column into the exclusive sum along the wave index
// and returns the workgroup's count of the class (sort_wave_scan's shape).
CIOA_PLACE_FN uint32_t set_wave_scan(uint32_t *wcount, uint32_t k)
{
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kSetWaves; ++w) {
        const uint32_t c = wcount[w * kPoolSetMax + k];
        wcount[w * kPoolSetMax + k] = sum;
        sum += c;
    }
    return sum;
}

// After ONE linear exclusive scan of the class-major table: a class's total is
// the next class's first word (the grand total behind the last class) less its
// own first, and the count of the class before a workgroup is the workgroup's
// word less the class's first.
CIOA_PLACE_FN uint64_t set_class_total(uint64_t first, uint64_t next_first)
{
    return next_first - first;
}

CIOA_PLACE_FN uint64_t set_class_excl(uint64_t word, uint64_t first)
{
    return word - first;
}

// What set[4k] becomes after a release in which `reach` entries of class k
// reach the placement: count + min(reach, room).  changed: the word is written.
CIOA_PLACE_FN uint64_t set_release_end(uint64_t count, uint64_t room, uint64_t reach, bool &changed)
{
    const uint64_t acc = reach < room ? reach : room;
    changed = acc != 0;
    return count + acc;
}

// What set[4k] becomes after a grow in which `images` images have class k and
// the class serves F entries: count - min(images, F).
CIOA_PLACE_FN uint64_t set_grow_end(uint64_t count, uint64_t F, uint64_t images, bool &changed)
{
    const uint64_t take = images < F ? images : F;
    changed = take != 0;
    return count - take;
}

}  // namespace cioa

#endif
