// coalesce.h -- the arithmetic of coalescing the free slots of a pool set in
// HBM (coalesce_gpu.hip: coal_gather, coal_ends, coal_mscan, coal_survive,
// coal_sscan, coal_compact, coal_link, coal_rscan, coal_groups, coal_class,
// coal_final, coal_commit): when an entry is well-formed and what its sort key
// is, when a sorted entry collides with those before it, when a survivor
// continues the run of the one before it, where the next group of a run starts
// (a galloping lower bound over the sorted offsets) and what one run's groups
// are, the class of an output, the verdict and dev_total, and where the
// per-call words and the workgroups' columns lie in the writer's scratch.  No
// HIP type, so that the same text compiles for the device and, stand-alone on
// the host, under ASan + UBSan (tools/coalesce_check.cpp, `make
// coalescecheck`).  Not installed.
#ifndef CIOA_COALESCE_H
#define CIOA_COALESCE_H

#include <stdint.h>

#include "pool_set.h"

namespace cioa {

constexpr uint32_t kCoalBlock = kSetBlock;             // positions per workgroup of every kernel of the chain
// What coal_link and coal_groups leave per survivor (bits; the class of an output in bits 8..11, kSetClsShift).
constexpr uint32_t kCoalCand = 1;        // a candidate: cap < T
constexpr uint32_t kCoalStart = 2;       // the first survivor of a run, or a non-candidate: a new run id starts here
constexpr uint32_t kCoalGroup = 4;       // the first entry of a group of two or more: it carries the group's capacity
constexpr uint32_t kCoalAbsorbed = 8;    // a later entry of such a group: no output

// dev_total[0].
constexpr uint64_t kCoalOk = 0, kCoalUnsound = 1, kCoalOverflow = 2;

// The per-call words behind the class table (64-bit words from
// set_words_at(nb)), and behind them four columns of nb words each: the
// workgroups' largest ends, survivor counts, run starts and packed counts.
constexpr uint32_t kCoalWValid = 0;      // the well-formed entries: the sorted positions below it hold a key
constexpr uint32_t kCoalWSurv = 1;       // the survivors
constexpr uint32_t kCoalWVerdict = 2;    // dev_total[0]
constexpr uint32_t kCoalWMask = 3;       // the classes whose set[4k] changes
constexpr uint32_t kCoalWCount = 4;      // c_k, kPoolSetMax words
constexpr uint32_t kCoalWords = 4 + kPoolSetMax;
constexpr uint32_t kCoalColMax = 0, kCoalColSurv = 1, kCoalColRun = 2, kCoalColCnt = 3, kCoalCols = 4;

CIOA_SORT_FN uint32_t coal_col_at(uint32_t col, uint32_t nb)
{
    return set_words_at(nb) + kCoalWords + col * nb;
}
// The sort's histogram table, kSortRadix 32-bit words per workgroup, holds the
// class table, the words and the columns of a batch of any nb >= 1.
static_assert(kPoolSetMax + kCoalWords + kCoalCols <= kSortRadix / 2, "the sort's table holds a coalesce batch's words");

// ONE workgroup's packed counts (each at most kCoalBlock): groups, entries in
// groups, classless outputs; one workgroup scan adds all three.  The sums over
// the grid are taken field by field: they do not fit a field.
constexpr uint32_t kCoalCntShift = 20;
CIOA_PLACE_FN uint64_t coal_cnt_pack(uint64_t groups, uint64_t absorbed, uint64_t classless)
{
    return groups | (absorbed << kCoalCntShift) | (classless << (2 * kCoalCntShift));
}
CIOA_PLACE_FN uint64_t coal_cnt_field(uint64_t packed, uint32_t f)
{
    return (packed >> (f * kCoalCntShift)) & ((1ull << kCoalCntShift) - 1);
}

// The sentinel key of an ill-formed entry or an unused position, one above the
// largest key a well-formed entry can have ((dev_bytes - 1) / align: its cap is
// at least 1).  The host refuses a call in which it does not fit 32 bits.
CIOA_SORT_FN uint64_t coal_key_bound(uint64_t dev_bytes, uint64_t align)
{
    return (dev_bytes - 1) / align + 1;
}

// C1: cap >= 1, off + cap <= dev_bytes without a wrap, off a multiple of align.
CIOA_PLACE_FN bool coal_wellformed(uint64_t off, uint64_t cap, uint64_t dev_bytes, uint64_t align)
{
    return cap != 0 && off + cap >= off && off + cap <= dev_bytes && (off & (align - 1)) == 0;
}

// The key of position (k, j) of a sound set: off / align of a well-formed entry
// below the class's count, else the sentinel.  Equal offsets have equal keys
// and the sort is stable, so the sorted order is C2's.
CIOA_PLACE_FN uint32_t coal_key(bool entry, uint64_t off, uint64_t cap, uint64_t dev_bytes, uint64_t align,
                                uint32_t sentinel)
{
    return entry && coal_wellformed(off, cap, dev_bytes, align) ? (uint32_t) (off / align) : sentinel;
}

// C2: M is the largest off + cap of the entries before this one (0: none).
CIOA_PLACE_FN bool coal_collides(uint64_t off, uint64_t M)
{
    return off < M;
}

// off + cap of a well-formed entry rounded up to align: at most dev_bytes +
// align - 1 < 2^45, no wrap.
CIOA_PLACE_FN uint64_t coal_slot_end(uint64_t off, uint64_t cap, uint64_t align)
{
    return (off + cap + (align - 1)) & ~(align - 1);
}

// C3: does a survivor continue the run of the survivor before it?
CIOA_PLACE_FN bool coal_links(uint64_t prev_off, uint64_t prev_cap, uint64_t off, uint64_t cap, uint64_t T,
                              uint64_t align)
{
    return prev_cap < T && cap < T && coal_slot_end(prev_off, prev_cap, align) == off;
}

// A survivor's run id: the run starts before its workgroup (the column, scanned)
// plus those up to it inside its workgroup.
CIOA_PLACE_FN uint64_t coal_run_id(const uint64_t *col, const uint32_t *local, uint64_t s)
{
    return col[s / kCoalBlock] + local[s];
}

// The first index in (g, n) whose offset is >= target: a gallop from g + 1,
// then a binary search, over offsets that rise strictly.  n when there is none.
CIOA_PLACE_FN uint64_t coal_lower_bound(const uint64_t *offs, uint64_t n, uint64_t g, uint64_t target)
{
    uint64_t lo = g + 1, step = 1;
    if (lo >= n || offs[lo] >= target) {
        return lo < n ? lo : n;
    }
    uint64_t hi = lo + step;                  // offs[lo] < target throughout
    while (hi < n && offs[hi] < target) {
        lo = hi;
        step <<= 1;
        hi = lo + step;
    }
    if (hi > n) {
        hi = n;
    }
    while (lo + 1 < hi) {                     // offs[lo] < target, and offs[hi] >= target or hi == n
        const uint64_t mid = lo + (hi - lo) / 2;
        if (offs[mid] < target) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return hi;
}

// The first index above g whose run id differs from rid (the ids do not fall):
// the same search over the ids.
CIOA_PLACE_FN uint64_t coal_run_end(const uint64_t *col, const uint32_t *local, uint64_t n, uint64_t g, uint64_t rid)
{
    uint64_t lo = g, step = 1, hi = g + 1;    // id(lo) == rid throughout
    while (hi < n && coal_run_id(col, local, hi) == rid) {
        lo = hi;
        step <<= 1;
        hi = lo + step;
    }
    if (hi > n) {
        hi = n;
    }
    while (lo + 1 < hi) {
        const uint64_t mid = lo + (hi - lo) / 2;
        if (coal_run_id(col, local, mid) == rid) {
            lo = mid;
        } else {
            hi = mid;
        }
    }
    return hi;
}

// C4's step: the start of the group behind the one that starts at g -- the
// first entry of g's run with off >= off(g) + T and off a multiple of P; n when
// the run has none.  off(g) + T saturates: no offset reaches 2^64 - 1.
CIOA_PLACE_FN uint64_t coal_next_start(const uint64_t *offs, const uint64_t *col, const uint32_t *local, uint64_t n,
                                       uint64_t g, uint64_t rid, uint64_t T, uint64_t P)
{
    uint64_t t = coal_lower_bound(offs, n, g, place_add(offs[g], T));
    while (t < n && coal_run_id(col, local, t) == rid && (offs[t] & (P - 1)) != 0) {
        t += 1;
    }
    return t < n && coal_run_id(col, local, t) == rid ? t : n;
}

// C4 over ONE run, by the thread of its first survivor `head`: every group of
// two or more entries gets kCoalGroup and the group's capacity at its first
// entry and kCoalAbsorbed at the others.  A group of one entry IS that entry,
// unchanged, and is marked nowhere.  Loads per group, one store per entry of a
// group; entries outside groups are not touched.
CIOA_PLACE_FN void coal_walk_run(const uint64_t *offs, const uint64_t *caps, const uint64_t *col,
                                 const uint32_t *local, uint64_t n, uint64_t head, uint64_t T, uint64_t P,
                                 uint64_t *ocap, uint32_t *code)
{
    const uint64_t rid = coal_run_id(col, local, head);
    uint64_t g = head;
    while (g < n && coal_run_id(col, local, g) == rid && (offs[g] & (P - 1)) != 0) {
        g += 1;                               // the entries before g_0 stay single
    }
    while (g < n && coal_run_id(col, local, g) == rid) {
        uint64_t e = coal_next_start(offs, col, local, n, g, rid, T, P);
        if (e == n) {                         // the last group: to the run's end, if that covers T bytes
            e = coal_run_end(col, local, n, g, rid);
            if (offs[e - 1] + caps[e - 1] - offs[g] < T) {
                return;
            }
        }
        if (e - g >= 2) {
            ocap[g] = offs[e - 1] + caps[e - 1] - offs[g];
            code[g] |= kCoalGroup;
            for (uint64_t u = g + 1; u < e; ++u) {
                code[u] |= kCoalAbsorbed;
            }
        }
        g = e;
    }
}

// C6 / C7 in one place, by one thread: from the classes' output counts c[], the
// well-formed entries V, the survivors S, the groups, the entries in them and
// the classless outputs, the verdict, dev_total[0 .. 5 + n_cls) and the mask of
// the set words that change.
CIOA_PLACE_FN uint64_t coal_totals(const uint64_t *set, uint32_t n_cls, bool sound, const uint64_t *c, uint64_t V,
                                   uint64_t S, uint64_t groups, uint64_t absorbed, uint64_t classless,
                                   uint64_t *total, uint64_t &mask)
{
    mask = 0;
    if (!sound) {
        total[0] = kCoalUnsound;
        for (uint32_t w = 1; w < 5 + n_cls; ++w) {
            total[w] = 0;
        }
        return kCoalUnsound;
    }
    uint64_t entries = 0, verdict = kCoalOk;
    for (uint32_t k = 0; k < n_cls; ++k) {
        entries += set[4 * k + kPoolCount];   // each <= stride, n_cls * stride < 2^32
        if (c[k] > set[4 * k + kPoolCap]) {
            verdict = kCoalOverflow;
        }
        mask |= c[k] != set[4 * k + kPoolCount] ? 1ull << k : 0;
        total[5 + k] = c[k];
    }
    total[0] = verdict;
    total[1] = entries - V + classless;
    total[2] = V - S;
    total[3] = groups;
    total[4] = absorbed;
    if (verdict != kCoalOk) {
        mask = 0;
    }
    return verdict;
}

}  // namespace cioa

#endif
