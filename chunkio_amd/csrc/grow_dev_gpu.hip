// grow_dev_gpu.hip -- growing chunk images in HBM out of a caller-provided
// arena ahead of an append, for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_write_dev_grow.h; DESIGN.md §18.
//
// A grow batch is a serial chain of kernels on the caller's stream:
//
//   grow_clear     records variant; one thread per image: the per-image need
//   grow_need      arena and the header word re-zeroed, then one thread per
//                  record: the index check (an index >= n_img is published in
//                  the header word) and need[img] += min(len, 2^32), a plain
//                  atomicAdd (integer addition does not depend on order)
//   grow_headers   one thread per image: the entry values into prev_*, rules
//                  1..4 (the image check of the write path, the length field,
//                  the arena, room, the reference's growth rule), the slot, a
//                  workgroup scan of the slots and the workgroup's total
//   grow_scan      ONE workgroup, looping over however many totals there are:
//                  their exclusive scan, and dev_total
//   grow_place     one thread per image: the new offset, whether the slot fits
//                  the arena, the status; into the writer's arenas the copy
//                  region (source [old_off, + used), destination new_off) and
//                  the tail region [new_off + used, new_off + new_cap), both
//                  zero-length for every image that is not grown; and who
//                  writes the arena's top
//   planner        devplan's four kernels over the copy regions
//   append_copy    the write path's copy kernel (write_dev_gpu.hip), unchanged:
//                  source buffer = destination buffer = dev_base; the regions
//                  are disjoint (an image inside the arena's free part is
//                  rejected) and neither base pointer is __restrict__
//   planner        with CIOA_GROW_ZERO, over the tail regions
//   grow_zero      with CIOA_GROW_ZERO: the byte-balanced fill
//   grow_commit    one thread per image: dev_img_offs / dev_img_caps in place,
//                  the arena's top (exactly one thread), the planner's status
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another.  The planner's own checks cannot fire: every region lies inside
// an image grow_headers found inside dev_bytes or inside an arena slot below
// end <= dev_bytes, and both planner runs see a batch that is empty or not
// together (a grown image has used >= 24 and new_cap > used).
//
// The arithmetic is grow_dev.h, the text tools/grow_check.cpp runs on the
// host.  Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "grow_dev.h"
#include "block_scan_gpu.h"
#include "chunkio_amd/cio_write_dev_grow.h"

using namespace cioa;

namespace {

constexpr uint32_t kZeroThreads = 256;                 // 4 waves per workgroup, the copy kernel's shape
constexpr uint32_t kZeroWaves = kZeroThreads / kWave;

__global__ void __launch_bounds__(256)
grow_clear(unsigned long long *__restrict__ need, uint32_t n, uint32_t *__restrict__ ghdr)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i < n) {
        need[i] = 0;
    }
    if (i == 0) {
        ghdr[0] = 0;
    }
}

__global__ void __launch_bounds__(256)
grow_need(const uint32_t *__restrict__ rec_img, const uint64_t *__restrict__ rec_lens, uint32_t n_rec,
          uint32_t n_img, unsigned long long *need, uint32_t *ghdr)
{
    const uint32_t r = blockIdx.x * 256u + threadIdx.x;
    if (r >= n_rec) {
        return;
    }
    const uint32_t img = rec_img[r];
    if (img >= n_img) {
        atomicOr(ghdr, 1u);                   // the whole call is rejected
        return;
    }
    atomicAdd(need + img, (unsigned long long) umin(rec_lens[r], kGrowLenClamp));
}

// dst[i] takes the exclusive sum of the slots before entry i in its workgroup
// and rtot[blockIdx.x] the workgroup's total; slen[i] the used bytes and
// gcap[i] the new capacity of an image that is to grow, 0 otherwise.
__global__ void __launch_bounds__(kGrowBlock)
grow_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
             const uint64_t *__restrict__ img_caps, uint32_t n, const uint64_t *__restrict__ need,
             const uint32_t *__restrict__ ghdr, const uint64_t *__restrict__ arena, uint64_t realloc_size,
             uint64_t page, uint64_t align, uint64_t *__restrict__ prev_offs, uint64_t *__restrict__ prev_caps,
             int32_t *__restrict__ status, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
             uint64_t *__restrict__ dst, uint64_t *__restrict__ gcap, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kGrowBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kGrowBlock + tid;
    int32_t st = CIO_OK;
    uint64_t off = 0, used = 0, ncap = 0;
    if (i < n) {
        off = img_offs[i];
        const uint64_t cap = img_caps[i], nd = need[i];
        if (prev_offs) {
            prev_offs[i] = off;
            prev_caps[i] = cap;
        }
        if (ghdr && ghdr[0] != 0) {
            st = CIO_ERROR;
        } else if (nd != 0) {                 // an image without a need is not read
            uint32_t meta = 0;
            uint64_t content = 0;
            if (!image_ok(base, dev_bytes, off, cap, meta, content)) {
                st = CIO_ERROR;
            } else {
                used = kReadHdr + meta + content;
                if (grow_decide(off, cap, used, content, nd, arena[0], arena[1], realloc_size, page, ncap) ==
                    kGrowReject) {
                    st = CIO_ERROR;
                }
            }
        }
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, tid, grow_slot(ncap, align), total);
    if (tid == 0) {
        rtot[blockIdx.x] = total;
    }
    if (i < n) {
        status[i] = st;
        soff[i] = ncap ? off : 0;
        slen[i] = ncap ? used : 0;
        dst[i] = excl;
        gcap[i] = ncap;
    }
}

// rtot[j] becomes the sum of the totals before workgroup j; total[0] the
// batch's dev_total.
__global__ void __launch_bounds__(kGrowBlock)
grow_scan(uint64_t *__restrict__ rtot, uint32_t nb, const uint64_t *__restrict__ arena, uint64_t align,
          uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kGrowBlock];
    uint64_t carry = 0;                       // totals_scan, written out (block_scan_gpu.h)
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        carry = totals_pass(sh, rtot, nb, base, carry);
    }
    if (threadIdx.x == 0) {
        total[0] = grow_total(arena[0], align, carry);
    }
}

__global__ void __launch_bounds__(kGrowBlock)
grow_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ arena, uint64_t dev_bytes,
           uint64_t align, int32_t *__restrict__ status, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
           uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap, uint64_t *__restrict__ zoff,
           uint64_t *__restrict__ zlen, uint32_t *__restrict__ code)
{
    const uint64_t i = (uint64_t) blockIdx.x * kGrowBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t before = place_add(rtot[blockIdx.x], dst[i]);
    const uint64_t ncap = gcap[i], slot = grow_slot(ncap, align);
    uint64_t off;
    const uint32_t c = grow_place_code(arena[0], arena[1], dev_bytes, align, before, slot, i + 1 == n, off);
    code[i] = c;
    dst[i] = off;
    if (c & kGrowMoved) {
        const uint64_t used = slen[i];
        zoff[i] = off + used;
        zlen[i] = ncap - used;
        return;
    }
    if (slot != 0) {
        status[i] = CIO_ERROR;                // cut: the image stays valid where it is
    }
    soff[i] = 0;
    slen[i] = 0;
    zoff[i] = 0;
    zlen[i] = 0;
}

// Region i: zlen[i] bytes at base + zoff[i] become zero.  The planner's image
// of the regions gives the balance, as for append_copy: wave w of the grid
// takes steps [w S / W, (w + 1) S / W), whatever regions they belong to.
__global__ void __launch_bounds__(kZeroThreads)
grow_zero(uint8_t *base, const ChunkDesc *__restrict__ desc, const uint64_t *__restrict__ zoff,
          const uint64_t *__restrict__ zlen, const unsigned long long *__restrict__ hdr, uint32_t n)
{
    if (hdr[kDevHdrStatus] != 0) {
        return;
    }
    const uint64_t gtid = (uint64_t) blockIdx.x * kZeroThreads + threadIdx.x;
    if (hdr[kDevHdrNtiny] != 0) {
        fill_tiny(base, zoff, zlen, n, gtid, (uint64_t) gridDim.x * kZeroThreads);
    }
    const uint64_t w = __builtin_amdgcn_readfirstlane((uint32_t) (gtid / kWave));
    fill_wave(base, desc, zoff, zlen, n, hdr[kDevHdrS], (uint64_t) gridDim.x * kZeroWaves, w,
              threadIdx.x & (kWave - 1));
}

// hdr: the last planner's header.  A planner that published an empty batch
// copied nothing: the grown images are rejected where they were and the top
// stays.
__global__ void __launch_bounds__(kGrowBlock)
grow_commit(uint64_t *__restrict__ img_offs, uint64_t *__restrict__ img_caps, uint32_t n,
            int32_t *__restrict__ status, const uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap,
            const uint32_t *__restrict__ code, const unsigned long long *__restrict__ hdr,
            uint64_t *__restrict__ arena, uint64_t align)
{
    const uint64_t i = (uint64_t) blockIdx.x * kGrowBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (c == 0) {
        return;
    }
    const bool bad = hdr[kDevHdrStatus] != 0;
    if (c & kGrowMoved) {
        if (bad) {
            status[i] = CIO_ERROR;
        } else {
            img_offs[i] = dst[i];
            img_caps[i] = gcap[i];
        }
    }
    if (!bad && (c & (kGrowTopAt | kGrowTopEnd))) {
        arena[0] = (c & kGrowTopAt) ? dst[i] : dst[i] + grow_slot(gcap[i], align);
    }
}

// The argument checks, before any device call.  Returns 1 when the call is a
// no-op (an empty batch), 0 to go on, CIO_ERROR.
int check_grow(const GrowArgs &a, bool records)
{
    if (a.flags & ~CIOA_GROW_ZERO) {
        return fail_who(a.who, "unknown flags");
    }
    if (a.realloc_size == 0) {
        return fail_who(a.who, "realloc_size must not be 0");
    }
    if (!pow2(a.page)) {
        return fail_who(a.who, "page must be a power of two");
    }
    if (!pow2(a.align) || a.align > 4096) {
        return fail_who(a.who, "align must be a power of two in 1 .. 4096");
    }
    if ((a.prev_offs == nullptr) != (a.prev_caps == nullptr)) {
        return fail_who(a.who, "dev_prev_offs and dev_prev_caps go together");
    }
    if (!a.w) {
        return fail_who(a.who, "null writer");
    }
    if (a.n == 0 || (records && a.n_rec == 0)) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.arena || !a.total || !a.status ||
        (records ? !a.rec_img || !a.rec_lens : !a.need)) {
        return fail_who(a.who, "null pointer");
    }
    if (a.n > a.w->max_chunks) {
        return fail_who(a.who, "more images than the writer was created for");
    }
    if (records && a.n_rec > a.w->max_chunks) {
        return fail_who(a.who, "more records than the writer was created for");
    }
    return 0;
}

// Measurement: the sections of cioa_debug_grow_events (SectionEvents).
enum { kSecNone = 0, kSecNeed, kSecBook, kSecCopy, kSecZero, kSecCommit };

int launch_grow(const GrowArgs &a, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kGrowBlock);
    if (grow_launch_front(a, s, ev) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(grow_scan, dim3(1), dim3(kGrowBlock), 0, s, w->rtot, nb, a.arena, a.align, a.total);
    hipLaunchKernelGGL(grow_place, dim3(nb), dim3(kGrowBlock), 0, s, n, w->rtot, a.arena, a.dev_bytes, a.align,
                       a.status, w->soff, w->slen, w->dst, w->gcap, w->roff, w->rlen, w->newlen);
    HIP_TRY(hipGetLastError(), "grow: placement kernels launch");
    if (mark(ev, kSecBook, false, s) != CIO_OK || mark(ev, kSecCopy, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK ||
        launch_copy(w, a.dev_base, a.dev_base, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (mark(ev, kSecCopy, false, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (a.flags & CIOA_GROW_ZERO) {
        if (devplan_launch_planner(w->dp, a.dev_bytes, w->roff, w->rlen, a.n, nullptr, s) != CIO_OK ||
            mark(ev, kSecZero, true, s) != CIO_OK) {
            return CIO_ERROR;
        }
        if (launch_zero_fill(w, a.dev_base, w->roff, w->rlen, a.n, s) != CIO_OK ||
            mark(ev, kSecZero, false, s) != CIO_OK) {
            return CIO_ERROR;
        }
    }
    if (mark(ev, kSecCommit, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(grow_commit, dim3(nb), dim3(kGrowBlock), 0, s, a.offs, a.caps, n, a.status, w->dst, w->gcap,
                       w->newlen, w->dp->hdr, a.arena, a.align);
    HIP_TRY(hipGetLastError(), "grow: commit kernel launch");
    return mark(ev, kSecCommit, false, s);
}

}  // namespace

int cioa::grow_check_args(const GrowArgs &a, bool records)
{
    return check_grow(a, records);
}

// grow_clear and, where there are records, grow_need: the records-to-need sums
// of the grow calls and of the rotate calls (rotate_dev_gpu.hip).
int cioa::launch_need_sums(const cio_dev_writer *w, const uint32_t *rec_img, const uint64_t *rec_lens, size_t n_img,
                           size_t n_rec, hipStream_t s)
{
    unsigned long long *acc = reinterpret_cast<unsigned long long *>(w->gneed);
    hipLaunchKernelGGL(grow_clear, dim3(blocks_of(n_img, 256)), dim3(256), 0, s, acc, (uint32_t) n_img, w->growhdr);
    if (n_rec != 0) {
        hipLaunchKernelGGL(grow_need, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, rec_img, rec_lens,
                           (uint32_t) n_rec, (uint32_t) n_img, acc, w->growhdr);
    }
    HIP_TRY(hipGetLastError(), "need sums kernels launch");
    return CIO_OK;
}

// The head of launch_grow, and of the variant that takes its slots from a pool
// set first (pool_set_gpu.hip): the need sums of the records variant and
// grow_headers.  No event lies between grow_headers and grow_scan, so the
// bookkeeping section opens here and closes in the caller.
int cioa::grow_launch_front(const GrowArgs &a, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kGrowBlock);
    const uint64_t *need = a.need;
    if (mark(ev, kSecNeed, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (!need) {
        if (launch_need_sums(w, a.rec_img, a.rec_lens, a.n, a.n_rec, s) != CIO_OK) {
            return CIO_ERROR;
        }
        need = w->gneed;
    }
    if (mark(ev, kSecNeed, false, s) != CIO_OK || mark(ev, kSecBook, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(grow_headers, dim3(nb), dim3(kGrowBlock), 0, s, reinterpret_cast<uint8_t *>(a.dev_base),
                       a.dev_bytes, a.offs, a.caps, n, need, a.need ? (const uint32_t *) nullptr : w->growhdr,
                       a.arena, a.realloc_size, a.page, a.align, a.prev_offs, a.prev_caps, a.status, w->soff,
                       w->slen, w->dst, w->gcap, w->rtot);
    HIP_TRY(hipGetLastError(), "grow: front kernels launch");
    return CIO_OK;
}

// One launch of grow_zero over the planner's image of (zoff, zlen): region i,
// zlen[i] bytes at dev_base + zoff[i], becomes zero.  The rollback's fill as
// well (tx_dev_gpu.hip).
int cioa::launch_zero_fill(const cio_dev_writer *w, void *dev_base, const uint64_t *zoff, const uint64_t *zlen, size_t n,
                           hipStream_t s)
{
    hipLaunchKernelGGL(grow_zero, dim3(w->copy_grid), dim3(kZeroThreads), 0, s, reinterpret_cast<uint8_t *>(dev_base),
                       w->dp->p->desc, zoff, zlen, w->dp->hdr, (uint32_t) n);
    HIP_TRY(hipGetLastError(), "zero fill kernel launch");
    return CIO_OK;
}

extern "C" {

int cio_file_grow_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                            const uint64_t *dev_need, uint64_t *dev_arena,
                            uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                            uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                            uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const GrowArgs a = {"cio_file_grow_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_need,
                        nullptr, nullptr, 0, dev_arena, realloc_size, page, align, flags, dev_prev_offs,
                        dev_prev_caps, dev_total, dev_status};
    const int rc = check_grow(a, false);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_grow(a, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int cio_file_grow_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                    uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                    const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                    uint64_t *dev_arena,
                                    uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                    uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                    uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const GrowArgs a = {"cio_file_grow_records_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                        nullptr, dev_rec_img, dev_rec_lens, n_rec, dev_arena, realloc_size, page, align, flags,
                        dev_prev_offs, dev_prev_caps, dev_total, dev_status};
    const int rc = check_grow(a, true);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_grow(a, reinterpret_cast<hipStream_t>(stream), nullptr);
}

/* Measurement hook (not in the public header; tools/grow_dev_ab.py): a whole
 * grow call -- the records variant when dev_need is NULL -- with the two HIP
 * events around ONE section of its chain: 1 the need kernels, 2 grow_headers +
 * grow_scan + grow_place, 3 the copy's planner and append_copy, 4 grow_zero
 * alone (its planner runs before the first event), 5 grow_commit. */
int cioa_debug_grow_events(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes, uint64_t *dev_img_offs,
                           uint64_t *dev_img_caps, size_t n, const uint64_t *dev_need, const uint32_t *dev_rec_img,
                           const uint64_t *dev_rec_lens, size_t n_rec, uint64_t *dev_arena, uint64_t realloc_size,
                           uint64_t page, uint64_t align, int flags, uint64_t *dev_total, int32_t *dev_status,
                           void *stream, int section, void *ev_start, void *ev_stop)
{
    const GrowArgs a = {"cioa_debug_grow_events", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_need,
                        dev_rec_img, dev_rec_lens, n_rec, dev_arena, realloc_size, page, align, flags, nullptr,
                        nullptr, dev_total, dev_status};
    if (!ev_start || !ev_stop || section < kSecNeed || section > kSecCommit || (section == kSecNeed && dev_need) ||
        (section == kSecZero && !(flags & CIOA_GROW_ZERO)) || check_grow(a, dev_need == nullptr) != 0) {
        return fail("cioa_debug_grow_events: bad argument");
    }
    const SectionEvents ev = {section, reinterpret_cast<hipEvent_t>(ev_start), reinterpret_cast<hipEvent_t>(ev_stop)};
    return launch_grow(a, reinterpret_cast<hipStream_t>(stream), &ev);
}

}  // extern "C"
