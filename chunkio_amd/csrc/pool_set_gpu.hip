// pool_set_gpu.hip -- the size-classed pool set in HBM: releasing drained
// slots into the class that fits each, and growing images out of the set
// before the arena is touched, for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_write_dev_pool_set.h; DESIGN.md §23.
//
// A release into the set is a serial chain of kernels on the caller's stream:
//
//   relset_headers  one thread per entry: rules 0..3 and 4' (is it among the
//                   first m, does an image still live there, the gate, the
//                   write path's image check, the set's soundness, the entry's
//                   class), then the K-WAY COUNTING SCAN: a lane's rank among
//                   the entries of its class in its wave from three ballots
//                   over the class index, a [wave][class] table in LDS scanned
//                   along the wave index, and the workgroup's K totals into
//                   the class-major table
//   relset_scan     ONE workgroup: per class the exclusive scan of the
//                   workgroups' totals; dev_total; what every set[4k] becomes
//                   and whether it changes, from the words as they were
//   relset_place    one thread per entry: accepted iff its rank in its class
//                   lies below the class's room; its index in the set's
//                   arrays; the fill's region; with CIOA_RELEASE_COMPACT the
//                   workgroup scan of the kept flags -- the SECOND SCAN: the
//                   accepted entries are no prefix of those that reach
//   relset_kscan    COMPACT: ONE workgroup, the scan of the kept totals
//   relset_kmove    COMPACT: every kept entry to its new position IN WRITER
//                   SCRATCH, the vacated positions prepared there
//   planner, fill   with CIOA_RELEASE_ZERO: devplan's four kernels over the
//                   slots and grow's byte-balanced zero fill, unchanged
//   relset_commit   one thread per entry: the push, bytes 0..1 of the slot, the
//                   scratch copied back over the list, dev_count[0]; thread k
//                   of workgroup 0 writes set[4k] when it changes
//
// A grow out of the set:
//
//   grow's front    grow_clear, grow_need (records), grow_headers, unchanged
//                   (grow_launch_front, grow_dev_gpu.hip): statuses, prev_*,
//                   the used bytes and the reference's new capacity per image
//   growset_class   one thread per image: S1, S2 and the K-way counting scan
//   growset_cscan   ONE workgroup: per class the scan of the totals;
//                   dev_total[1], dev_total[2 + k]; the set words' end values
//   growset_serve   one thread per image: S3 (the pool entry, checked before a
//                   byte of it is touched) or S4 (the arena-bound capacity and
//                   slot), and the workgroup scan of the arena-bound slots --
//                   grow's scan over this part alone
//   growset_ascan   ONE workgroup: the scan of the slot totals; dev_total[0]
//   growset_place   one thread per image: grow_place_code over the arena-bound
//                   part, the copy and tail regions, who writes the top and
//                   what
//   planner, append_copy, planner, grow_zero   as in grow, unchanged
//   growset_commit  one thread per image: dev_img_offs / dev_img_caps in
//                   place, the top (one thread), set[4k] (thread k of
//                   workgroup 0), the planner's status
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another, there is no atomic, and no kernel that writes a set word, the
// top or dev_count[0] reads it.  The class table and the per-call words live
// in the sort's histogram table (stab), which neither chain uses otherwise:
// kPoolSetMax + 17 64-bit words against the 128 it has per workgroup.  The
// arithmetic is pool_set.h, the text tools/pool_set_check.cpp runs on the
// host; the workgroup scans are block_scan_gpu.h's (block_scan_excl,
// totals_scan) and set_scan_gpu.h's (class_rank, class_scan), the latter
// shared with coalesce_gpu.hip.  Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "pool_set.h"
#include "set_scan_gpu.h"
#include "chunkio_amd/cio_write_dev_pool_set.h"

using namespace cioa;

namespace {

// ---------------------------------------------------------------- release into the set

// code[i] takes kRelIn, kRelReach and the class, ord[i] the entry's rank in its
// class inside its workgroup, tab the workgroup's K counts.
__global__ void __launch_bounds__(kSetBlock)
relset_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ offs,
               const uint64_t *__restrict__ caps, uint32_t n, uint32_t nb, const uint64_t *__restrict__ count,
               const int32_t *__restrict__ gate, const uint64_t *__restrict__ live,
               const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride, int32_t *__restrict__ status,
               uint64_t *__restrict__ ord, uint32_t *__restrict__ code, uint64_t *__restrict__ tab)
{
    __shared__ uint32_t wcount[kSetWaves * kPoolSetMax];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    const uint64_t m = pool_m(n, count != nullptr, count ? count[0] : 0);
    int32_t st = CIO_OK;
    uint32_t c = 0, cls = kSetNone;
    if (i < m) {
        c = kRelIn;
        const uint64_t off = offs[i];
        if (live && live[i] == off) {
            // an image still lives there: kept
        } else if (gate && gate[i] != CIO_OK) {
            st = CIO_ERROR;                       // the slot is not read
        } else {
            const uint64_t cap = caps[i];
            uint32_t meta;                        // the image's lengths: checked, not used
            uint64_t content;
            if (set_sound(set, n_cls, stride) && image_ok(base, dev_bytes, off, cap, meta, content)) {
                cls = set_release_class(set, n_cls, off, cap);
            }
            if (cls != kSetNone) {
                c |= kRelReach | (cls << kSetClsShift);
            } else {
                st = CIO_ERROR;
            }
        }
    }
    const uint32_t rank = class_rank(wcount, cls, tab, nb);
    if (i < n) {
        status[i] = st;
        ord[i] = rank;
        code[i] = c;
    }
}

// words: the per-call words behind the table.
__global__ void __launch_bounds__(kSetBlock)
relset_scan(uint64_t *tab, uint32_t nb, uint32_t n, const uint64_t *__restrict__ count,
            const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kSetBlock];
    __shared__ uint64_t reach[kPoolSetMax];
    class_scan(sh, reach, tab, nb, n_cls);
    if (threadIdx.x == 0) {
        uint64_t *words = tab + set_words_at(nb);
        const bool sound = set_sound(set, n_cls, stride);
        uint64_t all = 0, kept = pool_m(n, count != nullptr, count ? count[0] : 0), mask = 0;
        for (uint32_t k = 0; k < n_cls; ++k) {
            const uint64_t r = reach[k], room = set_room(set, k, sound);
            bool changed;
            words[kSetWEnd + k] = set_release_end(set[4 * k + kPoolCount], room, r, changed);
            mask |= changed ? 1ull << k : 0;
            total[2 + k] = r;
            all += r;
            kept -= r < room ? r : room;
        }
        words[kSetWMask] = mask;
        total[0] = all;
        total[1] = kept;
    }
}

// code[i] gains kRelAccepted; slot[i] the entry's index in the set's arrays;
// zoff[i], zlen[i] the slot of an accepted entry (0, 0 otherwise: the fill's
// planner reads all n).  compact: ord[i] becomes the number of kept entries
// before i in its workgroup, rtot the workgroup's kept count.
__global__ void __launch_bounds__(kSetBlock)
relset_place(uint32_t n, uint32_t nb, const uint64_t *__restrict__ tab, const uint64_t *__restrict__ set,
             uint64_t stride, const uint64_t *__restrict__ offs, const uint64_t *__restrict__ caps,
             int32_t *__restrict__ status, uint64_t *__restrict__ ord, uint32_t *__restrict__ code,
             uint64_t *__restrict__ slot, uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen, int compact,
             uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kSetBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    uint64_t kept = 0;
    if (i < n) {
        uint32_t c = code[i];
        uint64_t zo = 0, zl = 0;
        if (c & kRelReach) {                      // the set is sound
            const uint32_t k = (c >> kSetClsShift) & 15u;
            const uint64_t before = tab[set_tab_at(k, blockIdx.x, nb)] + ord[i];
            if (before < set_room(set, k, true)) {
                c |= kRelAccepted;
                slot[i] = k * stride + set[4 * k + kPoolCount] + before;
                zo = offs[i];
                zl = caps[i];
                code[i] = c;
            } else {
                status[i] = CIO_ERROR;            // cut: the entry is kept, and not offered to a lower class
            }
        }
        kept = (c & kRelIn) && !(c & kRelAccepted) ? 1 : 0;
        zoff[i] = zo;
        zlen[i] = zl;
    }
    if (compact) {
        uint64_t total;
        const uint64_t excl = block_scan_excl(sh, threadIdx.x, kept, total);
        if (threadIdx.x == 0) {
            rtot[blockIdx.x] = total;
        }
        if (i < n) {
            ord[i] = excl;
        }
    }
}

__global__ void __launch_bounds__(kSetBlock)
relset_kscan(uint64_t *__restrict__ rtot, uint32_t nb)
{
    __shared__ uint64_t sh[kSetBlock];
    (void) totals_scan(sh, rtot, nb);
}

// koff, kcap, kimg take the list as it will be: total[1] kept entries in front,
// (0, 0, 0xffffffff) behind them up to m.
__global__ void __launch_bounds__(kSetBlock)
relset_kmove(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ offs,
             const uint64_t *__restrict__ caps, const uint32_t *__restrict__ img, const uint64_t *__restrict__ ord,
             const uint32_t *__restrict__ code, const uint64_t *__restrict__ total, uint64_t *__restrict__ koff,
             uint64_t *__restrict__ kcap, uint32_t *__restrict__ kimg)
{
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (!(c & kRelIn)) {
        return;
    }
    if (!(c & kRelAccepted)) {
        const uint64_t p = rtot[blockIdx.x] + ord[i];     // <= i
        koff[p] = offs[i];
        kcap[p] = caps[i];
        if (img) {
            kimg[p] = img[i];
        }
    }
    if (i >= total[1]) {                          // vacated: no kept entry lands at or behind the kept total
        koff[i] = 0;
        kcap[i] = 0;
        kimg[i] = kPoolNoImage;
    }
}

// hdr: the fill's planner's header, or NULL without CIOA_RELEASE_ZERO.  A
// planner that published an empty batch filled nothing: no entry is accepted,
// nothing is marked, and neither the set nor the list is written.
__global__ void __launch_bounds__(kSetBlock)
relset_commit(uint8_t *base, uint64_t *__restrict__ offs, uint64_t *__restrict__ caps, uint32_t *__restrict__ img,
              uint32_t n, uint64_t *count, int32_t *__restrict__ status, const uint32_t *__restrict__ code,
              const uint64_t *__restrict__ slot, const uint64_t *__restrict__ zoff,
              const uint64_t *__restrict__ zlen, const unsigned long long *__restrict__ hdr, int compact,
              const uint64_t *__restrict__ koff, const uint64_t *__restrict__ kcap,
              const uint32_t *__restrict__ kimg, uint64_t *__restrict__ set_offs, uint64_t *__restrict__ set_caps,
              uint64_t *set, uint32_t n_cls, const uint64_t *__restrict__ words, uint64_t *total)
{
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    const bool bad = hdr && hdr[kDevHdrStatus] != 0;
    if (!bad && i < n_cls && ((words[kSetWMask] >> i) & 1u)) {
        set[4 * i + kPoolCount] = words[kSetWEnd + i];    // the word's one writer
    }
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (c == 0) {
        return;
    }
    if (bad) {
        if (c & kRelAccepted) {
            status[i] = CIO_ERROR;
        }
        if (i == 0) {                             // every entry among the first m is kept; nobody writes the count
            total[1] = pool_m(n, count != nullptr, count ? count[0] : 0);
        }
        return;
    }
    if (c & kRelAccepted) {
        const uint64_t off = zoff[i], k = slot[i];
        set_offs[k] = off;
        set_caps[k] = zlen[i];
        base[off] = 0;                            // no magic: a stale reference fails every image check
        base[off + 1] = 0;
    }
    if (compact) {
        offs[i] = koff[i];
        caps[i] = kcap[i];
        if (img) {
            img[i] = kimg[i];
        }
        if (i == 0) {
            count[0] = total[1];
        }
    }
}

// ---------------------------------------------------------------- growing out of the set

// gcap[i]: grow_headers' new capacity (0: the image does not reach rule 4).
// code[i] takes the class, ord[i] the image's rank in its class inside its
// workgroup, tab the workgroup's K counts.
__global__ void __launch_bounds__(kSetBlock)
growset_class(uint32_t n, uint32_t nb, const uint64_t *__restrict__ gcap, const uint64_t *__restrict__ set,
              uint32_t n_cls, uint64_t stride, uint64_t align, uint64_t *__restrict__ ord,
              uint32_t *__restrict__ code, uint64_t *__restrict__ tab)
{
    __shared__ uint32_t wcount[kSetWaves * kPoolSetMax];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    uint32_t cls = kSetNone;
    if (i < n) {
        const uint64_t ncap = gcap[i];
        if (ncap != 0) {
            cls = set_grow_class(set, n_cls, set_usable(set, n_cls, stride, align), ncap);
        }
    }
    const uint32_t rank = class_rank(wcount, cls, tab, nb);
    if (i < n) {
        ord[i] = rank;
        code[i] = cls << kSetClsShift;
    }
}

__global__ void __launch_bounds__(kSetBlock)
growset_cscan(uint64_t *tab, uint32_t nb, const uint64_t *__restrict__ set, uint32_t n_cls,
              uint64_t stride, uint64_t align, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kSetBlock];
    __shared__ uint64_t images[kPoolSetMax];
    class_scan(sh, images, tab, nb, n_cls);
    if (threadIdx.x == 0) {
        uint64_t *words = tab + set_words_at(nb);
        const uint32_t usable = set_usable(set, n_cls, stride, align);
        uint64_t taken = 0, mask = 0;
        for (uint32_t k = 0; k < n_cls; ++k) {
            const uint64_t r = images[k], F = set_serves(set, k, usable);
            bool changed;
            words[kSetWEnd + k] = set_grow_end(set[4 * k + kPoolCount], F, r, changed);
            mask |= changed ? 1ull << k : 0;
            total[2 + k] = r;
            taken += r < F ? r : F;
        }
        words[kSetWMask] = mask;
        total[1] = taken;
    }
}

// S3 / S4.  code[i] gains kSetServed or kSetArena; gcap[i] becomes the capacity
// of the slot the image takes (0: none -- not grown, or its pool entry failed
// the check); dst[i] the pool entry's offset of a served image; ord[i] the sum
// of the arena-bound slots before i in its workgroup, rtot the workgroup's.
__global__ void __launch_bounds__(kSetBlock)
growset_serve(uint32_t n, uint32_t nb, const uint64_t *__restrict__ tab, const uint64_t *__restrict__ set,
              uint32_t n_cls, uint64_t stride, uint64_t align, uint64_t dev_bytes,
              const uint64_t *__restrict__ set_offs, const uint64_t *__restrict__ set_caps,
              int32_t *__restrict__ status, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
              uint64_t *__restrict__ dst, uint64_t *__restrict__ gcap, uint64_t *__restrict__ ord,
              uint32_t *__restrict__ code, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kSetBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    uint64_t aslot = 0;
    if (i < n) {
        const uint64_t ncap = gcap[i];
        if (ncap != 0) {
            uint32_t c = code[i];
            const uint32_t cls = (c >> kSetClsShift) & 15u;
            bool pooled = false;
            if (cls != kSetNone) {
                const uint64_t j = tab[set_tab_at(cls, blockIdx.x, nb)] + ord[i];
                const uint64_t F = set_serves(set, cls, set_usable(set, n_cls, stride, align));
                if (j < F) {                      // F <= the class's capacity <= stride: inside the arrays
                    pooled = true;
                    const uint64_t e = cls * stride + (F - 1 - j);
                    const uint64_t eo = set_offs[e], ec = set_caps[e];
                    if (set_entry_ok(eo, ec, dev_bytes, set[4 * cls + kPoolCls], align)) {
                        c |= kSetServed;
                        dst[i] = eo;
                        gcap[i] = ec;             // its WHOLE capacity
                    } else {                      // consumed; the image stays valid where it was
                        status[i] = CIO_ERROR;
                        soff[i] = 0;
                        slen[i] = 0;
                        gcap[i] = 0;
                    }
                }
            }
            if (!pooled) {
                const uint64_t cap = set_arena_cap(set, cls, ncap);
                c |= kSetArena;
                gcap[i] = cap;
                aslot = grow_slot(cap, align);
            }
            code[i] = c;
        }
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, threadIdx.x, aslot, total);
    if (threadIdx.x == 0) {
        rtot[blockIdx.x] = total;
    }
    if (i < n) {
        ord[i] = excl;
    }
}

__global__ void __launch_bounds__(kSetBlock)
growset_ascan(uint64_t *__restrict__ rtot, uint32_t nb, const uint64_t *__restrict__ arena, uint64_t align,
              uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kSetBlock];
    const uint64_t slots = totals_scan(sh, rtot, nb);
    if (threadIdx.x == 0) {
        total[0] = grow_total(arena[0], align, slots);
    }
}

// code[i] gains grow's bits; etop[i]: the top the entry with a kGrowTop* bit
// writes, from the words as they were.
__global__ void __launch_bounds__(kSetBlock)
growset_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ arena, uint64_t dev_bytes,
              uint64_t align, int32_t *__restrict__ status, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
              uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap, const uint64_t *__restrict__ ord,
              uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen, uint64_t *__restrict__ etop,
              uint32_t *__restrict__ code)
{
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint32_t c = code[i];
    const uint64_t cap = gcap[i];
    const uint64_t slot = (c & kSetArena) ? grow_slot(cap, align) : 0;
    const uint64_t before = place_add(rtot[blockIdx.x], ord[i]);
    uint64_t off;
    const uint32_t g = grow_place_code(arena[0], arena[1], dev_bytes, align, before, slot, i + 1 == n, off);
    if (g & (kGrowTopAt | kGrowTopEnd)) {
        etop[i] = (g & kGrowTopAt) ? off : off + slot;    // fits: no wrap
    }
    c |= g;
    if (c & kSetServed) {
        c |= kGrowMoved;
        off = dst[i];
    } else if (slot != 0 && !(g & kGrowMoved)) {
        status[i] = CIO_ERROR;                    // cut: the image stays valid where it is
        soff[i] = 0;
        slen[i] = 0;
    }
    code[i] = c;
    if (c & kGrowMoved) {
        const uint64_t used = slen[i];
        dst[i] = off;
        zoff[i] = off + used;
        zlen[i] = cap - used;
        return;
    }
    zoff[i] = 0;
    zlen[i] = 0;
}

// hdr: the last planner's header.  A planner that published an empty batch
// copied nothing: the grown images are rejected where they were, and neither
// the top nor a set word is written.
__global__ void __launch_bounds__(kSetBlock)
growset_commit(uint64_t *__restrict__ img_offs, uint64_t *__restrict__ img_caps, uint32_t n,
               int32_t *__restrict__ status, const uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap,
               const uint64_t *__restrict__ etop, const uint32_t *__restrict__ code,
               const unsigned long long *__restrict__ hdr, uint64_t *__restrict__ arena, uint64_t *set,
               uint32_t n_cls, const uint64_t *__restrict__ words)
{
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    const bool bad = hdr[kDevHdrStatus] != 0;
    if (!bad && i < n_cls && ((words[kSetWMask] >> i) & 1u)) {
        set[4 * i + kPoolCount] = words[kSetWEnd + i];    // the word's one writer
    }
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (c & kGrowMoved) {
        if (bad) {
            status[i] = CIO_ERROR;
        } else {
            img_offs[i] = dst[i];
            img_caps[i] = gcap[i];
        }
    }
    if (!bad && (c & (kGrowTopAt | kGrowTopEnd))) {
        arena[0] = etop[i];
    }
}

struct SetArgs {
    uint64_t *offs, *caps, *words;
    size_t n_cls;
    uint64_t stride;
};

// The set's own checks: the values first (an empty batch included), the
// pointers where the call checks its own.
int check_set_values(const char *who, const SetArgs &t)
{
    if (t.n_cls < 1 || t.n_cls > CIOA_POOL_SET_MAX) {
        return fail_who(who, "n_cls must be in 1 .. 8");
    }
    if (t.stride == 0) {
        return fail_who(who, "stride must not be 0");
    }
    return 0;
}

struct RelArgs {
    cio_dev_writer *w;
    void *dev_base;
    uint64_t dev_bytes;
    uint64_t *offs, *caps;
    uint32_t *img;
    size_t n;
    uint64_t *count;
    const int32_t *gate;
    const uint64_t *live;
    int flags;
    SetArgs set;
    uint64_t *total;
    int32_t *status;
};

const char kRel[] = "cio_file_release_set_batch_dev";

// The argument checks, before any device call: cio_file_release_batch_dev's
// and the set's.  Returns 1 when the call is a no-op (an empty batch), 0 to go
// on, CIO_ERROR.
int check_release(const RelArgs &a)
{
    if (a.flags & ~(CIOA_RELEASE_ZERO | CIOA_RELEASE_COMPACT)) {
        return fail("cio_file_release_set_batch_dev: unknown flags");
    }
    if ((a.flags & CIOA_RELEASE_COMPACT) && !a.count) {
        return fail("cio_file_release_set_batch_dev: CIOA_RELEASE_COMPACT needs dev_count");
    }
    if ((a.flags & CIOA_RELEASE_COMPACT) && a.live) {
        return fail("cio_file_release_set_batch_dev: CIOA_RELEASE_COMPACT does not go with dev_live_offs");
    }
    if (check_set_values(kRel, a.set) != 0) {
        return CIO_ERROR;
    }
    if (!a.w) {
        return fail("cio_file_release_set_batch_dev: null writer");
    }
    if (a.n == 0) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.set.offs || !a.set.caps || !a.set.words || !a.total || !a.status) {
        return fail("cio_file_release_set_batch_dev: null pointer");
    }
    if (a.n > a.w->max_chunks) {
        return fail("cio_file_release_set_batch_dev: more entries than the writer was created for");
    }
    return 0;
}

int launch_release(const RelArgs &a, hipStream_t s)
{
    cio_dev_writer *w = a.w;
    uint8_t *base = reinterpret_cast<uint8_t *>(a.dev_base);
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kSetBlock), n_cls = (uint32_t) a.set.n_cls;
    const int compact = (a.flags & CIOA_RELEASE_COMPACT) != 0;
    const bool zero = (a.flags & CIOA_RELEASE_ZERO) != 0;
    // writer arenas: newlen the entry's code, groom its rank (then its kept ordinal), dst its index in the set's
    // arrays, roff / rlen the fill's regions, goffs / glens / gimg the compacted list, rtot the kept totals, stab
    // the class table and the per-call words
    uint64_t *tab = reinterpret_cast<uint64_t *>(w->stab);
    const uint64_t *words = tab + set_words_at(nb);
    hipLaunchKernelGGL(relset_headers, dim3(nb), dim3(kSetBlock), 0, s, base, a.dev_bytes, a.offs, a.caps, n, nb,
                       a.count, a.gate, a.live, a.set.words, n_cls, a.set.stride, a.status, w->groom, w->newlen, tab);
    hipLaunchKernelGGL(relset_scan, dim3(1), dim3(kSetBlock), 0, s, tab, nb, n, a.count, a.set.words, n_cls,
                       a.set.stride, a.total);
    hipLaunchKernelGGL(relset_place, dim3(nb), dim3(kSetBlock), 0, s, n, nb, tab, a.set.words, a.set.stride, a.offs,
                       a.caps, a.status, w->groom, w->newlen, w->dst, w->roff, w->rlen, compact, w->rtot);
    if (compact) {
        hipLaunchKernelGGL(relset_kscan, dim3(1), dim3(kSetBlock), 0, s, w->rtot, nb);
        hipLaunchKernelGGL(relset_kmove, dim3(nb), dim3(kSetBlock), 0, s, n, w->rtot, a.offs, a.caps, a.img,
                           w->groom, w->newlen, a.total, w->goffs, w->glens, w->gimg);
    }
    HIP_TRY(hipGetLastError(), "release into the set: placement kernels launch");
    if (zero && (devplan_launch_planner(w->dp, a.dev_bytes, w->roff, w->rlen, a.n, nullptr, s) != CIO_OK ||
                 launch_zero_fill(w, a.dev_base, w->roff, w->rlen, a.n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(relset_commit, dim3(nb), dim3(kSetBlock), 0, s, base, a.offs, a.caps, a.img, n, a.count,
                       a.status, w->newlen, w->dst, w->roff, w->rlen,
                       zero ? w->dp->hdr : (const unsigned long long *) nullptr, compact, w->goffs, w->glens, w->gimg,
                       a.set.offs, a.set.caps, a.set.words, n_cls, words, a.total);
    HIP_TRY(hipGetLastError(), "release into the set: commit kernel launch");
    return CIO_OK;
}

int launch_grow_set(const GrowArgs &a, const SetArgs &t, hipStream_t s)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kSetBlock), n_cls = (uint32_t) t.n_cls;
    if (grow_launch_front(a, s) != CIO_OK) {
        return CIO_ERROR;
    }
    // writer arenas beside the front's (soff, slen, gcap): newlen the image's code, groom its rank (then the
    // arena-bound slots before it), dst the new offset, roff / rlen the tail regions, goffs the top the ending
    // entry writes, rtot the slot totals, stab the class table and the per-call words
    uint64_t *tab = reinterpret_cast<uint64_t *>(w->stab);
    const uint64_t *words = tab + set_words_at(nb);
    hipLaunchKernelGGL(growset_class, dim3(nb), dim3(kSetBlock), 0, s, n, nb, w->gcap, t.words, n_cls, t.stride,
                       a.align, w->groom, w->newlen, tab);
    hipLaunchKernelGGL(growset_cscan, dim3(1), dim3(kSetBlock), 0, s, tab, nb, t.words, n_cls, t.stride, a.align,
                       a.total);
    hipLaunchKernelGGL(growset_serve, dim3(nb), dim3(kSetBlock), 0, s, n, nb, tab, t.words, n_cls, t.stride, a.align,
                       a.dev_bytes, t.offs, t.caps, a.status, w->soff, w->slen, w->dst, w->gcap, w->groom,
                       w->newlen, w->rtot);
    hipLaunchKernelGGL(growset_ascan, dim3(1), dim3(kSetBlock), 0, s, w->rtot, nb, a.arena, a.align, a.total);
    hipLaunchKernelGGL(growset_place, dim3(nb), dim3(kSetBlock), 0, s, n, w->rtot, a.arena, a.dev_bytes, a.align,
                       a.status, w->soff, w->slen, w->dst, w->gcap, w->groom, w->roff, w->rlen, w->goffs, w->newlen);
    HIP_TRY(hipGetLastError(), "grow out of the set: placement kernels launch");
    if (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK ||
        launch_copy(w, a.dev_base, a.dev_base, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if ((a.flags & CIOA_GROW_ZERO) &&
        (devplan_launch_planner(w->dp, a.dev_bytes, w->roff, w->rlen, a.n, nullptr, s) != CIO_OK ||
         launch_zero_fill(w, a.dev_base, w->roff, w->rlen, a.n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(growset_commit, dim3(nb), dim3(kSetBlock), 0, s, a.offs, a.caps, n, a.status, w->dst, w->gcap,
                       w->goffs, w->newlen, w->dp->hdr, a.arena, t.words, n_cls, words);
    HIP_TRY(hipGetLastError(), "grow out of the set: commit kernel launch");
    return CIO_OK;
}

int grow_set(const GrowArgs &a, bool records, const SetArgs &t, void *stream)
{
    if (check_set_values(a.who, t) != 0) {
        return CIO_ERROR;
    }
    const int rc = grow_check_args(a, records);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    if (!t.offs || !t.caps || !t.words) {
        return fail_who(a.who, "null pointer");
    }
    return launch_grow_set(a, t, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int cio_file_release_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   uint64_t *dev_offs, uint64_t *dev_caps, uint32_t *dev_img, size_t n,
                                   uint64_t *dev_count, const int32_t *dev_gate, const uint64_t *dev_live_offs,
                                   int flags,
                                   uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set, size_t n_cls,
                                   uint64_t stride,
                                   uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const RelArgs a = {w, dev_base, dev_bytes, dev_offs, dev_caps, dev_img, n, dev_count, dev_gate, dev_live_offs,
                       flags, {dev_set_offs, dev_set_caps, dev_set, n_cls, stride}, dev_total, dev_status};
    const int rc = check_release(a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_release(a, reinterpret_cast<hipStream_t>(stream));
}

int cio_file_grow_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                const uint64_t *dev_need, uint64_t *dev_arena,
                                uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set, size_t n_cls,
                                uint64_t stride,
                                uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const GrowArgs a = {"cio_file_grow_set_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_need,
                        nullptr, nullptr, 0, dev_arena, realloc_size, page, align, flags, dev_prev_offs,
                        dev_prev_caps, dev_total, dev_status};
    const SetArgs t = {dev_set_offs, dev_set_caps, dev_set, n_cls, stride};
    return grow_set(a, false, t, stream);
}

int cio_file_grow_set_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                        uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                        const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                        uint64_t *dev_arena,
                                        uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                                        size_t n_cls, uint64_t stride,
                                        uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                        uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                        uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const GrowArgs a = {"cio_file_grow_set_records_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                        nullptr, dev_rec_img, dev_rec_lens, n_rec, dev_arena, realloc_size, page, align, flags,
                        dev_prev_offs, dev_prev_caps, dev_total, dev_status};
    const SetArgs t = {dev_set_offs, dev_set_caps, dev_set, n_cls, stride};
    return grow_set(a, true, t, stream);
}

}  // extern "C"
