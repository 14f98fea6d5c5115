// alloc_set_gpu.hip -- fresh slots of given sizes out of the size-classed pool
// set in HBM, then the arena, and the device steps of a load behind it (the
// copy's regions and the adopt step), for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_persist_dev.h; DESIGN.md §26.
//
// An allocation is a serial chain of kernels on the caller's stream, the shape
// of a grow out of the set (pool_set_gpu.hip) without an image in front:
//
//   allocset_class   one thread per entry: does it reach the placement (the
//                    gate, need >= 24), S1, S2 and the K-way counting scan
//   allocset_cscan   ONE workgroup: per class the scan of the totals;
//                    dev_total[1], dev_total[2 + k]; the set words' end values
//   allocset_serve   one thread per entry: S3 (the pool entry, checked before
//                    it is handed out) or S4 (the arena-bound capacity and
//                    slot), and the workgroup scan of the arena-bound slots
//   allocset_ascan   ONE workgroup: the scan of the slot totals; dev_total[0]
//   allocset_place   one thread per entry: grow_place_code over the arena-bound
//                    part, the fill's region, who writes the top and what
//   planner, fill    with CIOA_ALLOC_ZERO: devplan's four kernels over the
//                    slots and grow's byte-balanced zero fill, unchanged
//   allocset_commit  one thread per entry: dev_out_offs, dev_out_caps and
//                    dev_status, the top (one thread), set[4k] (thread k of
//                    workgroup 0)
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another, there is no atomic, and no kernel that writes a set word or the
// top reads it.  The class table and the per-call words live in the sort's
// histogram table (stab), as in pool_set_gpu.hip.  The arithmetic is
// alloc_set.h over pool_set.h and grow_dev.h, the text tools/alloc_check.cpp
// runs on the host; the scans are set_scan_gpu.h's and block_scan_gpu.h's.
// Plain C++ and vector stores throughout.
//
// allocset_cscan and allocset_ascan are growset_cscan and growset_ascan line
// for line, and allocset_commit is growset_commit without the images: this
// change was not to touch pool_set_gpu.hip.  When the grow out of the set
// adopts alloc_set.h, the three pairs fold into one each.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "alloc_set.h"
#include "set_scan_gpu.h"
#include "chunkio_amd/cio_persist_dev.h"

using namespace cioa;

namespace {

// gcap[i]: the capacity the entry asks for (0: it does not reach the
// placement).  code[i] takes the class, ord[i] the entry's rank in its class
// inside its workgroup, tab the workgroup's K counts.
__global__ void __launch_bounds__(kSetBlock)
allocset_class(uint32_t n, uint32_t nb, const uint64_t *__restrict__ need, const int32_t *__restrict__ gate,
               const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride, uint64_t align,
               uint64_t *__restrict__ gcap, uint64_t *__restrict__ ord, uint32_t *__restrict__ code,
               uint64_t *__restrict__ tab)
{
    __shared__ uint32_t wcount[kSetWaves * kPoolSetMax];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    uint32_t cls = kSetNone;
    uint64_t ncap = 0;
    if (i < n) {
        ncap = alloc_new_cap(gate != nullptr, gate ? gate[i] : 0, need[i]);
        if (ncap != 0) {
            cls = set_grow_class(set, n_cls, set_usable(set, n_cls, stride, align), ncap);
        }
    }
    const uint32_t rank = class_rank(wcount, cls, tab, nb);
    if (i < n) {
        gcap[i] = ncap;
        ord[i] = rank;
        code[i] = cls << kSetClsShift;
    }
}

__global__ void __launch_bounds__(kSetBlock)
allocset_cscan(uint64_t *tab, uint32_t nb, const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride,
               uint64_t align, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kSetBlock];
    __shared__ uint64_t entries[kPoolSetMax];
    class_scan(sh, entries, tab, nb, n_cls);
    if (threadIdx.x == 0) {
        uint64_t *words = tab + set_words_at(nb);
        const uint32_t usable = set_usable(set, n_cls, stride, align);
        uint64_t taken = 0, mask = 0;
        for (uint32_t k = 0; k < n_cls; ++k) {
            const uint64_t r = entries[k], F = set_serves(set, k, usable);
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

// code[i] gains kSetServed or kSetArena; dst[i], gcap[i] the slot of a served
// entry, gcap[i] the capacity of an arena-bound one (0: no slot); ord[i] the
// sum of the arena-bound slots before i in its workgroup, rtot the workgroup's.
__global__ void __launch_bounds__(kSetBlock)
allocset_serve(uint32_t n, uint32_t nb, const uint64_t *__restrict__ tab, const uint64_t *__restrict__ set,
               uint32_t n_cls, uint64_t stride, uint64_t align, uint64_t dev_bytes,
               const uint64_t *__restrict__ set_offs, const uint64_t *__restrict__ set_caps,
               uint64_t *__restrict__ dst, uint64_t *__restrict__ gcap, uint64_t *__restrict__ ord,
               uint32_t *__restrict__ code, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kSetBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    uint64_t aslot = 0;
    if (i < n) {
        const uint64_t ncap = gcap[i];
        uint64_t off = kPlaceOver, cap = 0;
        if (ncap != 0) {
            uint32_t c = code[i];
            const uint32_t cls = (c >> kSetClsShift) & 15u;
            uint64_t j = 0, F = 0;
            if (cls != kSetNone) {
                j = tab[set_tab_at(cls, blockIdx.x, nb)] + ord[i];
                F = set_serves(set, cls, set_usable(set, n_cls, stride, align));
            }
            c |= alloc_serve(set, set_offs, set_caps, stride, cls, j, F, ncap, dev_bytes, align, off, cap, aslot);
            code[i] = c;
        }
        dst[i] = off;
        gcap[i] = cap;
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
allocset_ascan(uint64_t *__restrict__ rtot, uint32_t nb, const uint64_t *__restrict__ arena, uint64_t align,
               uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kSetBlock];
    const uint64_t slots = totals_scan(sh, rtot, nb);
    if (threadIdx.x == 0) {
        total[0] = grow_total(arena[0], align, slots);
    }
}

// code[i] gains grow's bits; dst[i] the offset of an accepted entry; zoff[i],
// zlen[i] its slot (0, 0 otherwise: the fill's planner reads all n); etop[i]
// the top the entry with a kGrowTop* bit writes, from the words as they were.
__global__ void __launch_bounds__(kSetBlock)
allocset_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ arena, uint64_t dev_bytes,
               uint64_t align, uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap,
               const uint64_t *__restrict__ ord, uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen,
               uint64_t *__restrict__ etop, uint32_t *__restrict__ code)
{
    const uint64_t i = (uint64_t) blockIdx.x * kSetBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t cap = gcap[i];
    uint64_t off = dst[i], top;
    const uint32_t c = alloc_place(code[i], arena[0], arena[1], dev_bytes, align, place_add(rtot[blockIdx.x], ord[i]),
                                   cap, i + 1 == n, off, top);
    code[i] = c;
    etop[i] = top;
    const bool acc = (c & kAllocAccepted) != 0;
    dst[i] = off;
    zoff[i] = acc ? off : 0;
    zlen[i] = acc ? cap : 0;
}

// hdr: the fill's planner's header, or NULL without CIOA_ALLOC_ZERO.  A
// planner that published an empty batch filled nothing: no entry is accepted,
// and neither the top nor a set word is written.
__global__ void __launch_bounds__(kSetBlock)
allocset_commit(uint32_t n, const uint64_t *__restrict__ dst, const uint64_t *__restrict__ gcap,
                const uint64_t *__restrict__ etop, const uint32_t *__restrict__ code,
                const unsigned long long *__restrict__ hdr, uint64_t *__restrict__ arena, uint64_t *set,
                uint32_t n_cls, const uint64_t *__restrict__ words, uint64_t *__restrict__ out_offs,
                uint64_t *__restrict__ out_caps, int32_t *__restrict__ status)
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
    const bool acc = !bad && (c & kAllocAccepted);
    out_offs[i] = acc ? dst[i] : kPlaceOver;
    out_caps[i] = acc ? gcap[i] : 0;
    status[i] = acc ? CIO_OK : CIO_ERROR;
    if (!bad && (c & (kGrowTopAt | kGrowTopEnd))) {
        arena[0] = etop[i];
    }
}

// ---------------------------------------------------------------- the device steps of a load

// One thread per file of a round, behind verify and the allocation: the copy's
// regions (file i's bytes in the stage to its slot; nothing for a file without
// a slot) and, with CIOA_LOAD_ZERO, the fill's ([size, cap) of the slot).
__global__ void __launch_bounds__(256)
load_regions(uint32_t n, const uint64_t *__restrict__ soffs, const uint64_t *__restrict__ sizes,
             const int32_t *__restrict__ ast, const uint64_t *__restrict__ aoffs,
             const uint64_t *__restrict__ acaps, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
             uint64_t *__restrict__ dst, uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const bool ok = ast[i] == CIO_OK;             // then sizes[i] >= 24 and acaps[i] >= sizes[i]
    soff[i] = ok ? soffs[i] : 0;
    slen[i] = ok ? sizes[i] : 0;
    dst[i] = ok ? aoffs[i] : 0;
    zoff[i] = ok ? aoffs[i] + sizes[i] : 0;
    zlen[i] = ok ? acaps[i] - sizes[i] : 0;
}

// The adopt step, one thread per file of a round, behind the copy: image i is
// what the host read in full (pre[i] == CIO_OK), verify accepted (vst[i] ==
// CIO_OK) AND the allocation placed (ast[i] == CIO_OK).  A header whose
// content length field is 0 gets the length verify inferred written to bytes
// 10..13 of the HBM copy, as the reference's read-write load does; the slot's
// capacity no longer says where the content ends.  The field lies in front of
// the CRC's region.  An image that verified but found no slot, or whose copy's
// planner published an empty batch (hdr), is CIO_ERROR.
__global__ void __launch_bounds__(256)
adopt_images(uint8_t *base, uint32_t n, const int32_t *__restrict__ pre, const int32_t *__restrict__ vst,
             const int32_t *__restrict__ ast, const uint64_t *__restrict__ aoffs,
             const uint64_t *__restrict__ acaps, const uint32_t *__restrict__ vcrc,
             const uint64_t *__restrict__ vcontent, const unsigned long long *__restrict__ hdr,
             uint64_t *__restrict__ img_offs, uint64_t *__restrict__ img_caps, uint32_t *__restrict__ crc_cur,
             int32_t *__restrict__ status)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const int32_t h = pre[i], v = vst[i];
    const bool ok = h == CIO_OK && v == CIO_OK && ast[i] == CIO_OK && hdr[kDevHdrStatus] == 0;
    if (ok) {
        uint8_t *p = base + aoffs[i];             // the allocation's slot: inside dev_bytes, >= 24 bytes
        if (be32(p + 10) == 0 && vcontent[i] != 0) {
            put_be32(p + 10, (uint32_t) vcontent[i]);
        }
    }
    img_offs[i] = ok ? aoffs[i] : kPlaceOver;
    img_caps[i] = ok ? acaps[i] : 0;
    crc_cur[i] = ok ? vcrc[i] : 0;
    status[i] = ok ? CIO_OK : h != CIO_OK ? h : v != CIO_OK ? v : CIO_ERROR;
}

const char kWho[] = "cio_file_alloc_set_batch_dev";

}  // namespace

int cioa::load_launch_back(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes, const void *dev_stage,
                           uint64_t stage_bytes, size_t n, bool zero, const LoadRound &r, hipStream_t s)
{
    const uint32_t nb = blocks_of(n, 256);
    hipLaunchKernelGGL(load_regions, dim3(nb), dim3(256), 0, s, (uint32_t) n, r.soffs, r.sizes, r.ast, r.aoffs,
                       r.acaps, w->soff, w->slen, w->dst, w->roff, w->rlen);
    HIP_TRY(hipGetLastError(), "load: region kernel launch");
    if (devplan_launch_planner(w->dp, stage_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
        launch_copy(w, dev_base, dev_stage, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(adopt_images, dim3(nb), dim3(256), 0, s, reinterpret_cast<uint8_t *>(dev_base), (uint32_t) n,
                       r.pre, r.vst, r.ast, r.aoffs, r.acaps, r.vcrc, r.vcontent, w->dp->hdr, r.img_offs, r.img_caps,
                       r.crc_cur, r.status);
    HIP_TRY(hipGetLastError(), "load: adopt kernel launch");
    if (zero && (devplan_launch_planner(w->dp, dev_bytes, w->roff, w->rlen, n, nullptr, s) != CIO_OK ||
                 launch_zero_fill(w, dev_base, w->roff, w->rlen, n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    return CIO_OK;
}

extern "C" int cio_file_alloc_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                            const uint64_t *dev_need, const int32_t *dev_gate, size_t n,
                                            uint64_t *dev_arena,
                                            uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                                            size_t n_cls, uint64_t stride,
                                            uint64_t align, int flags,
                                            uint64_t *dev_out_offs, uint64_t *dev_out_caps,
                                            uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    if (flags & ~CIOA_ALLOC_ZERO) {
        return fail_who(kWho, "unknown flags");
    }
    if (!pow2(align) || align > 4096) {
        return fail_who(kWho, "align must be a power of two in 1 .. 4096");
    }
    if (n_cls > CIOA_POOL_SET_MAX) {
        return fail_who(kWho, "n_cls must be in 0 .. 8");
    }
    if (n_cls != 0 && stride == 0) {
        return fail_who(kWho, "stride must not be 0");
    }
    if (!w) {
        return fail_who(kWho, "null writer");
    }
    if (n == 0) {
        return CIO_OK;
    }
    if (!dev_base || !dev_need || !dev_arena || !dev_out_offs || !dev_out_caps || !dev_total || !dev_status ||
        (n_cls != 0 && (!dev_set_offs || !dev_set_caps || !dev_set))) {
        return fail_who(kWho, "null pointer");
    }
    if (n > w->max_chunks) {
        return fail_who(kWho, "more entries than the writer was created for");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint32_t cnt = (uint32_t) n, nb = blocks_of(n, kSetBlock), k = (uint32_t) n_cls;
    // writer arenas: gcap the capacity asked for, then taken; newlen the entry's code; groom its rank (then the
    // arena-bound slots before it); dst its offset; roff / rlen the fill's regions; goffs the top the ending entry
    // writes; rtot the slot totals; stab the class table and the per-call words
    uint64_t *tab = reinterpret_cast<uint64_t *>(w->stab);
    const uint64_t *words = tab + set_words_at(nb);
    hipLaunchKernelGGL(allocset_class, dim3(nb), dim3(kSetBlock), 0, s, cnt, nb, dev_need, dev_gate, dev_set, k, stride,
                       align, w->gcap, w->groom, w->newlen, tab);
    hipLaunchKernelGGL(allocset_cscan, dim3(1), dim3(kSetBlock), 0, s, tab, nb, dev_set, k, stride, align, dev_total);
    hipLaunchKernelGGL(allocset_serve, dim3(nb), dim3(kSetBlock), 0, s, cnt, nb, tab, dev_set, k, stride, align,
                       dev_bytes, dev_set_offs, dev_set_caps, w->dst, w->gcap, w->groom, w->newlen, w->rtot);
    hipLaunchKernelGGL(allocset_ascan, dim3(1), dim3(kSetBlock), 0, s, w->rtot, nb, dev_arena, align, dev_total);
    hipLaunchKernelGGL(allocset_place, dim3(nb), dim3(kSetBlock), 0, s, cnt, w->rtot, dev_arena, dev_bytes, align,
                       w->dst, w->gcap, w->groom, w->roff, w->rlen, w->goffs, w->newlen);
    HIP_TRY(hipGetLastError(), "allocation out of the set: placement kernels launch");
    const bool zero = (flags & CIOA_ALLOC_ZERO) != 0;
    if (zero && (devplan_launch_planner(w->dp, dev_bytes, w->roff, w->rlen, n, nullptr, s) != CIO_OK ||
                 launch_zero_fill(w, dev_base, w->roff, w->rlen, n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(allocset_commit, dim3(nb), dim3(kSetBlock), 0, s, cnt, w->dst, w->gcap, w->goffs, w->newlen,
                       zero ? w->dp->hdr : (const unsigned long long *) nullptr, dev_arena, dev_set, k, words,
                       dev_out_offs, dev_out_caps, dev_status);
    HIP_TRY(hipGetLastError(), "allocation out of the set: commit kernel launch");
    return CIO_OK;
}
