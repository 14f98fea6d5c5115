// read_dev_gpu.hip -- the read path of chunk images in HBM, for CDNA4 (gfx950,
// MI355X): a record of every image -- its metadata, its content, or the whole
// image trimmed to its used bytes -- gathered into an output buffer, at places
// the caller gives or at places a device-side scan computes, and the metadata
// compare.  C ABI in include/chunkio_amd/cio_read_dev.h; DESIGN.md §15.
//
// A read batch is a serial chain of kernels on the caller's stream:
//
//   read_headers   one thread per image: the image check of the write path,
//                  the gate, the record by `what`, its length; into the
//                  writer's arenas the record's region in the image buffer
//                  (zero-length for a rejected entry, so the batch keeps its
//                  indexing and nothing of that entry is copied).  Placed: the
//                  slot checks, and the destination.  Packed: a workgroup scan
//                  of the slot sizes and the workgroup's total.
//   read_scan      packed only; ONE workgroup, looping over however many
//                  totals there are: their exclusive scan, and dev_total.
//   read_place     packed only; one thread per image: the final offset, the
//                  capacity and overflow rules.  After it status, out_lens and
//                  the arenas are final.
//   planner        devplan's four kernels over the records' regions in the
//                  IMAGE buffer: desc[i].g / nsteps is the byte-balanced
//                  partition the copy reads.
//   append_copy    the write path's copy kernel (write_dev_gpu.hip), unchanged:
//                  source = the image buffer, destination = dev_out.
//   read_nul       with CIOA_READ_NUL, one thread per image: the terminator.
//
// With dev_out == NULL the chain ends after read_place (after read_headers in
// placed mode): a size query.  Kernel boundaries are the only grid-wide
// synchronisation; no workgroup waits on another.  The planner's own checks
// cannot fire: every region lies inside an image that read_headers found
// inside dev_bytes, and no image holds 2^32 steps.
//
// The placement arithmetic (record selection, slot size, the scan's combine
// step, the capacity and overflow rules) is read_dev_place.h, the text that
// tools/place_check.cpp runs on the host.  Plain C++ throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "read_dev_place.h"
#include "block_scan_gpu.h"
#include "write_dev_copy.h"
#include "chunkio_amd/cio_read_dev.h"

using namespace cioa;

namespace {

constexpr uint32_t kCmpThreads = 256;                  // 4 waves, one image each
constexpr uint32_t kCmpWaves = kCmpThreads / kWave;

// PACKED: dst[i] takes the exclusive sum of the slots before entry i in its
// workgroup and rtot[blockIdx.x] the workgroup's total.  Placed: dst[i] is
// final; out_offs == NULL is the size query (no slot checks).
template <bool PACKED>
__global__ void __launch_bounds__(kReadBlock)
read_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
             const uint64_t *__restrict__ img_caps, uint32_t n, int what, const int32_t *gate, uint64_t nul,
             uint64_t align, const uint64_t *out_offs, const uint64_t *__restrict__ out_caps, uint64_t out_bytes,
             int32_t *status, uint64_t *__restrict__ out_lens, uint64_t *__restrict__ soff,
             uint64_t *__restrict__ slen, uint64_t *__restrict__ dst, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[PACKED ? kReadBlock : 1];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kReadBlock + tid;
    bool ok = false;
    uint64_t first = 0, len = 0, d = 0, off = 0;
    if (i < n) {
        off = img_offs[i];
        uint32_t meta = 0;
        uint64_t content = 0;
        ok = (!gate || gate[i] == CIO_OK) && image_ok(base, dev_bytes, off, img_caps[i], meta, content);
        if (ok) {
            place_select(what, meta, content, first, len);
            if (!PACKED && out_offs) {
                d = out_offs[i];
                ok = placed_fits(d, out_caps[i], out_bytes, len, nul);
            }
        }
    }
    uint64_t slot = 0;
    if (PACKED) {
        slot = ok ? place_slot(len, nul, align) : 0;
        uint64_t total;
        const uint64_t excl = block_scan_excl(sh, tid, slot, total);
        if (tid == 0) {
            rtot[blockIdx.x] = total;
        }
        d = excl;
    }
    if (i < n) {
        status[i] = ok ? CIO_OK : CIO_ERROR;
        out_lens[i] = ok ? len : 0;
        soff[i] = ok ? off + first : 0;
        slen[i] = ok ? len : 0;
        dst[i] = PACKED || ok ? d : 0;
    }
}

// rtot[j] becomes the sum of the totals before workgroup j; total[0] the sum
// of all (kPlaceOver when it left 64 bits).
__global__ void __launch_bounds__(kReadBlock)
read_scan(uint64_t *__restrict__ rtot, uint32_t nb, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kReadBlock];
    uint64_t carry = 0;                       // totals_scan, written out (block_scan_gpu.h)
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        carry = totals_pass(sh, rtot, nb, base, carry);
    }
    if (threadIdx.x == 0) {
        total[0] = carry;
    }
}

__global__ void __launch_bounds__(kReadBlock)
read_place(uint32_t n, const uint64_t *__restrict__ rtot, uint64_t nul, uint64_t align, uint64_t out_bytes,
           int32_t *__restrict__ status, uint64_t *__restrict__ out_offs, uint64_t *__restrict__ out_lens,
           uint64_t *__restrict__ soff, uint64_t *__restrict__ slen, uint64_t *__restrict__ dst)
{
    const uint64_t i = (uint64_t) blockIdx.x * kReadBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t before = place_add(rtot[blockIdx.x], dst[i]);
    out_offs[i] = before;
    if (status[i] == CIO_OK && place_fits(before, place_slot(slen[i], nul, align), out_bytes)) {
        dst[i] = before;
        return;
    }
    status[i] = CIO_ERROR;
    out_lens[i] = 0;
    soff[i] = 0;
    slen[i] = 0;
    dst[i] = 0;
}

__global__ void __launch_bounds__(256)
read_nul(uint8_t *out, uint32_t n, const int32_t *__restrict__ status, const uint64_t *__restrict__ slen,
         const uint64_t *__restrict__ dst, const unsigned long long *__restrict__ hdr)
{
    const uint64_t i = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK || hdr[kDevHdrStatus] != 0) {
        return;
    }
    out[dst[i] + slen[i]] = 0;
}

// One wave per image: the image check, the candidate's checks, the lengths,
// then the bytes -- 16 per lane and load on both sides, at any alignment (one
// unaligned 16-byte vector load each, as the append copy's source side), the
// last m & 15 bytes one per lane -- and a wave vote.
__global__ void __launch_bounds__(kCmpThreads)
meta_cmp(const uint8_t *__restrict__ base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
         const uint64_t *__restrict__ img_caps, uint32_t n, const uint8_t *__restrict__ cand, uint64_t cand_bytes,
         const uint64_t *__restrict__ cand_offs, const uint64_t *__restrict__ cand_lens,
         int32_t *__restrict__ result, int32_t *__restrict__ status)
{
    const uint64_t i = (uint64_t) blockIdx.x * kCmpWaves + threadIdx.x / kWave;
    const uint32_t lane = threadIdx.x & (kWave - 1);
    if (i >= n) {
        return;
    }
    const uint64_t off = img_offs[i], coff = cand_offs[i], clen = cand_lens[i];
    uint32_t meta = 0;
    uint64_t content = 0;
    const bool ok = image_ok(base, dev_bytes, off, img_caps[i], meta, content) && clen <= 65535u &&
                    range_ok(coff, clen, cand_bytes);
    bool differ = !ok || clen != meta;
    if (!differ && meta != 0) {
        const uint8_t *a = base + off + kReadHdr, *b = cand + coff;
        const uint32_t m16 = meta & ~15u;
        bool d = false;
        for (uint32_t x = lane * kGran; x < m16; x += kRow) {
            const u32x4 va = reinterpret_cast<const Unaligned16 *>(a + x)->v;
            const u32x4 vb = reinterpret_cast<const Unaligned16 *>(b + x)->v;
            d |= ((va[0] ^ vb[0]) | (va[1] ^ vb[1]) | (va[2] ^ vb[2]) | (va[3] ^ vb[3])) != 0;
        }
        if (m16 + lane < meta) {
            d |= a[m16 + lane] != b[m16 + lane];
        }
        differ = __ballot(d) != 0;
    }
    if (lane == 0) {
        result[i] = differ ? -1 : 0;
        status[i] = ok ? CIO_OK : CIO_ERROR;
    }
}

struct ReadArgs {
    const char *who;
    cio_dev_writer *w;
    const void *dev_base;
    uint64_t dev_bytes;
    const uint64_t *offs, *caps;
    size_t n;
    int what;
    const int32_t *gate;
    void *dev_out;
    uint64_t out_bytes;
    int flags;
    uint64_t *out_lens;
    int32_t *status;
};

// The argument checks the two read calls share, before any device call.
// Returns 1 when the call is a no-op (n == 0), 0 to go on, CIO_ERROR.
int check_read(const ReadArgs &a, bool pointers_ok)
{
    if (a.what != CIOA_READ_META && a.what != CIOA_READ_CONTENT && a.what != CIOA_READ_IMAGE) {
        return fail_who(a.who, "unknown what");
    }
    if (a.flags & ~CIOA_READ_NUL) {
        return fail_who(a.who, "unknown flags");
    }
    if (!a.w) {
        return fail_who(a.who, "null writer");
    }
    if (a.n == 0) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.out_lens || !a.status || !pointers_ok) {
        return fail_who(a.who, "null pointer");
    }
    if (a.n > a.w->max_chunks) {
        return fail_who(a.who, "more images than the writer was created for");
    }
    return 0;
}

// The planner, the copy and the terminators of a batch whose arenas are final;
// ev0 / ev1 (measurement): events around the copy kernel alone.
int launch_gather(const ReadArgs &a, hipStream_t s, hipEvent_t ev0, hipEvent_t ev1)
{
    cio_dev_writer *w = a.w;
    if (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (ev0) {
        HIP_TRY(hipEventRecord(ev0, s), "hipEventRecord");
    }
    if (launch_copy(w, a.dev_out, a.dev_base, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (ev1) {
        HIP_TRY(hipEventRecord(ev1, s), "hipEventRecord");
    }
    if (a.flags & CIOA_READ_NUL) {
        hipLaunchKernelGGL(read_nul, dim3(blocks_of(a.n, 256)), dim3(256), 0, s,
                           reinterpret_cast<uint8_t *>(a.dev_out), (uint32_t) a.n, a.status, w->slen, w->dst,
                           w->dp->hdr);
        HIP_TRY(hipGetLastError(), "read: terminator kernel launch");
    }
    return CIO_OK;
}

int read_packed(const ReadArgs &a, uint64_t align, uint64_t *out_offs, uint64_t *total, hipStream_t s,
                hipEvent_t ev0, hipEvent_t ev1)
{
    cio_dev_writer *w = a.w;
    const uint8_t *base = reinterpret_cast<const uint8_t *>(a.dev_base);
    const uint32_t nb = blocks_of(a.n, kReadBlock);
    const uint64_t nul = (a.flags & CIOA_READ_NUL) ? 1 : 0;
    const uint64_t room = a.dev_out ? a.out_bytes : ~0ull;   // a size query places as if unbounded
    hipLaunchKernelGGL(read_headers<true>, dim3(nb), dim3(kReadBlock), 0, s, base, a.dev_bytes, a.offs, a.caps,
                       (uint32_t) a.n, a.what, a.gate, nul, align, (const uint64_t *) nullptr,
                       (const uint64_t *) nullptr, room, a.status, a.out_lens, w->soff, w->slen, w->dst, w->rtot);
    hipLaunchKernelGGL(read_scan, dim3(1), dim3(kReadBlock), 0, s, w->rtot, nb, total);
    hipLaunchKernelGGL(read_place, dim3(nb), dim3(kReadBlock), 0, s, (uint32_t) a.n, w->rtot, nul, align, room,
                       a.status, out_offs, a.out_lens, w->soff, w->slen, w->dst);
    HIP_TRY(hipGetLastError(), "cio_file_read_packed_batch_dev: placement kernels launch");
    return a.dev_out ? launch_gather(a, s, ev0, ev1) : CIO_OK;
}

bool align_ok(uint64_t align)
{
    return align >= 1 && align <= 4096 && (align & (align - 1)) == 0;
}

}  // namespace

extern "C" {

int cio_file_read_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            int what, const int32_t *dev_gate,
                            void *dev_out, uint64_t out_bytes,
                            const uint64_t *dev_out_offs, const uint64_t *dev_out_caps,
                            int flags, uint64_t *dev_out_lens, int32_t *dev_status, void *stream)
{
    const ReadArgs a = {"cio_file_read_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, what,
                        dev_gate, dev_out, out_bytes, flags, dev_out_lens, dev_status};
    const int rc = check_read(a, !dev_out || (dev_out_offs && dev_out_caps));
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint64_t nul = (flags & CIOA_READ_NUL) ? 1 : 0;
    hipLaunchKernelGGL(read_headers<false>, dim3(blocks_of(n, kReadBlock)), dim3(kReadBlock), 0, s,
                       reinterpret_cast<const uint8_t *>(dev_base), dev_bytes, dev_img_offs, dev_img_caps,
                       (uint32_t) n, what, dev_gate, nul, (uint64_t) 1, dev_out ? dev_out_offs : nullptr,
                       dev_out ? dev_out_caps : nullptr, out_bytes, dev_status, dev_out_lens, w->soff, w->slen,
                       w->dst, w->rtot);
    HIP_TRY(hipGetLastError(), "cio_file_read_batch_dev: header kernel launch");
    return dev_out ? launch_gather(a, s, nullptr, nullptr) : CIO_OK;
}

int cio_file_read_packed_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                   const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                   int what, const int32_t *dev_gate,
                                   void *dev_out, uint64_t out_bytes, uint64_t align,
                                   int flags, uint64_t *dev_out_offs, uint64_t *dev_out_lens,
                                   uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const ReadArgs a = {"cio_file_read_packed_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                        what, dev_gate, dev_out, out_bytes, flags, dev_out_lens, dev_status};
    if (!align_ok(align)) {
        return fail("cio_file_read_packed_batch_dev: align must be a power of two in 1 .. 4096");
    }
    const int rc = check_read(a, dev_out_offs && dev_total);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return read_packed(a, align, dev_out_offs, dev_total, reinterpret_cast<hipStream_t>(stream), nullptr, nullptr);
}

int cio_meta_cmp_batch_dev(const void *dev_base, uint64_t dev_bytes,
                           const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                           const void *dev_cand, uint64_t cand_bytes,
                           const uint64_t *dev_cand_offs, const uint64_t *dev_cand_lens,
                           int32_t *dev_result, int32_t *dev_status, void *stream)
{
    if (n == 0) {
        return CIO_OK;
    }
    if (!dev_base || !dev_img_offs || !dev_img_caps || (!dev_cand && cand_bytes != 0) || !dev_cand_offs ||
        !dev_cand_lens || !dev_result || !dev_status) {
        return fail("cio_meta_cmp_batch_dev: null pointer");
    }
    if (n >= 0xffffffffull) {
        return fail("cio_meta_cmp_batch_dev: n must be below 2^32 - 1");
    }
    hipLaunchKernelGGL(meta_cmp, dim3(blocks_of(n, kCmpWaves)), dim3(kCmpThreads), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<const uint8_t *>(dev_base), dev_bytes,
                       dev_img_offs, dev_img_caps, (uint32_t) n, reinterpret_cast<const uint8_t *>(dev_cand),
                       cand_bytes, dev_cand_offs, dev_cand_lens, dev_result, dev_status);
    HIP_TRY(hipGetLastError(), "cio_meta_cmp_batch_dev: kernel launch");
    return CIO_OK;
}

/* Measurement hook (not in the public header; tools/read_dev_ab.py): a whole
 * cio_file_read_packed_batch_dev with the two HIP events around its copy
 * kernel ALONE (the header, placement and planner kernels run before the first
 * event, the terminators after the second). */
int cioa_debug_read_dev_copy_events(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                    const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                    int what, void *dev_out, uint64_t out_bytes, uint64_t align, int flags,
                                    uint64_t *dev_out_offs, uint64_t *dev_out_lens, uint64_t *dev_total,
                                    int32_t *dev_status, void *stream, void *ev_start, void *ev_stop)
{
    const ReadArgs a = {"cioa_debug_read_dev_copy_events", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                        what, nullptr, dev_out, out_bytes, flags, dev_out_lens, dev_status};
    if (!align_ok(align) || !dev_out || !ev_start || !ev_stop || n == 0 ||
        check_read(a, dev_out_offs && dev_total) != 0) {
        return fail("cioa_debug_read_dev_copy_events: bad argument");
    }
    return read_packed(a, align, dev_out_offs, dev_total, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<hipEvent_t>(ev_start), reinterpret_cast<hipEvent_t>(ev_stop));
}

}  // extern "C"
