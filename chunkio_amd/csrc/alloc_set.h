// alloc_set.h -- the arithmetic of handing out fresh slots of given sizes from
// the pool set, then the arena (alloc_set_gpu.hip: allocset_class,
// allocset_cscan, allocset_serve, allocset_ascan, allocset_place,
// allocset_commit): which entries reach the placement, and for one that does,
// rules S2..S4 of cio_write_dev_pool_set.h with new_cap := the entry's need --
// its class, the pool entry it takes (checked before it is handed out) or the
// arena-bound capacity and slot, and where an arena-bound slot lands.  Written
// per entry and without reference to an image, so that a grow out of the set
// can call the same text with new_cap = the reference's new capacity.  No HIP
// type, so that the same text compiles for the device and, stand-alone on the
// host, under ASan + UBSan (tools/alloc_check.cpp, `make alloccheck`).  Not
// installed.
#ifndef CIOA_ALLOC_SET_H
#define CIOA_ALLOC_SET_H

#include <stdint.h>

#include "grow_dev.h"
#include "pool_set.h"

namespace cioa {

constexpr uint64_t kAllocMinNeed = kReadHdr;           // a slot holds at least a chunk header
constexpr uint32_t kAllocAccepted = kGrowMoved;        // the entry has a slot: (off, cap) are its outputs

// Does entry i reach the placement?  gated: dev_gate is given.  The new
// capacity it asks for, 0 when it does not reach.
CIOA_PLACE_FN uint64_t alloc_new_cap(bool gated, int32_t gate, uint64_t need)
{
    return (!gated || gate == 0) && need >= kAllocMinNeed ? need : 0;
}

// S3 / S4 for one entry that reaches the placement asking new_cap, of class cls
// (kSetNone: none), the j-th of its class; F = the entries its class serves
// (set_serves).  Returns kSetServed (off, cap: the pool entry, with its whole
// capacity), kSetArena (cap: the arena-bound capacity, aslot: its slot; off is
// placed later), or 0: the pool entry failed S3's check and is consumed.
// set_offs / set_caps are read at one index, inside the class's entries.
CIOA_PLACE_FN uint32_t alloc_serve(const uint64_t *set, const uint64_t *set_offs, const uint64_t *set_caps,
                                   uint64_t stride, uint32_t cls, uint64_t j, uint64_t F, uint64_t new_cap,
                                   uint64_t dev_bytes, uint64_t align, uint64_t &off, uint64_t &cap, uint64_t &aslot)
{
    off = kPlaceOver;
    cap = 0;
    aslot = 0;
    if (cls != kSetNone && j < F) {               // F <= the class's capacity <= stride: inside the arrays
        const uint64_t e = cls * stride + (F - 1 - j);
        const uint64_t eo = set_offs[e], ec = set_caps[e];
        if (!set_entry_ok(eo, ec, dev_bytes, set[4 * cls + kPoolCls], align)) {
            return 0;
        }
        off = eo;
        cap = ec;
        return kSetServed;
    }
    cap = set_arena_cap(set, cls, new_cap);
    aslot = grow_slot(cap, align);
    return kSetArena;
}

// Where an entry lands, after the scan of the arena-bound slots: `before` the
// slots in front of it, code / off / cap what alloc_serve left.  Returns the
// code with grow's bits (kAllocAccepted: the entry has its slot; kGrowTop*: it
// writes the top, etop) and, for an accepted arena-bound entry, its offset.
CIOA_PLACE_FN uint32_t alloc_place(uint32_t code, uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align,
                                   uint64_t before, uint64_t cap, bool last, uint64_t &off, uint64_t &etop)
{
    const uint64_t slot = (code & kSetArena) ? grow_slot(cap, align) : 0;
    uint64_t at;
    const uint32_t g = grow_place_code(top, end, dev_bytes, align, before, slot, last, at);
    etop = (g & kGrowTopAt) ? at : (g & kGrowTopEnd) ? at + slot : 0;       // fits: no wrap
    if (code & kSetServed) {
        return code | (g & ~kGrowMoved) | kAllocAccepted;
    }
    if (g & kGrowMoved) {
        off = at;
    }
    return code | g;
}

}  // namespace cioa

#endif
