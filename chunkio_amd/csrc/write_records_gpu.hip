// write_records_gpu.hip -- the grouped append to chunk images in HBM, for CDNA4
// (gfx950, MI355X): many records per image in one call.  C ABI in
// include/chunkio_amd/cio_write_dev_records.h; DESIGN.md §16.
//
// The records arrive grouped by image (dev_rec_img non-decreasing): a run of
// records per image, appended in order.  A device-side SEGMENTED scan turns
// (record -> image) into destinations inside the images, decides which records
// fit, and gives each image its new length and the one range to checksum.  A
// serial chain of kernels on the caller's stream:
//
//   rec_images       one thread per image: does it have a run (a binary search
//                    in dev_rec_img); for one that has, the image check of the
//                    write path, its room and its append base.  An image
//                    without a run is not read.  The defaults: CRC region
//                    [base, + 0), dev_img_status by the check.
//   rec_scan_local   one thread per record, kRecBlock to a workgroup: run
//                    heads, the order and index check, the record's value (its
//                    length, or saturated for a bad source); the workgroup's
//                    segmented exclusive scan and its aggregate.
//   rec_scan_groups  ONE workgroup looping over the aggregates kRecBlock at a
//                    time: their segmented exclusive scan, and the batch's
//                    malformed flag reduced into a header word.
//   rec_place        one thread per record: adds the carry, decides acceptance;
//                    dev_rec_status, and into the writer's arenas the record's
//                    source region (zero-length if rejected) and destination.
//                    The last accepted record of a run writes the image's new
//                    content length and CRC region [base, + accepted total).
//   planner, append_copy   unchanged (§13, §14), over the n_rec record regions.
//   planner, CRC     with CIO_CHECKSUM: over the n_img appended regions IN THE
//                    IMAGE BUFFER, seeds = dev_crc_cur, output in writer
//                    scratch.
//   rec_finish       one thread per image: crc_cur, bytes 2..9, bytes 10..13 of
//                    an image with an accepted byte; every dev_img_status to
//                    CIO_ERROR for a malformed batch.
//
// Kernel boundaries are the only grid-wide synchronisation: no workgroup waits
// on another, there are no tickets and no look-back.  A malformed batch is
// published the way the planner publishes a rejected geometry: every region
// zero-length, so the copy and the CRC read and write nothing.  The planner's
// own checks cannot fire: every source region lies inside src_bytes and is
// shorter than 2^32 bytes, the accepted bytes of an image fit its room, and
// every CRC region lies inside an image that rec_images found inside
// dev_bytes.
//
// The arithmetic (run heads, record values, the scan's operator, room,
// acceptance) is write_dev_records.h, the text tools/records_check.cpp runs on
// the host.  Plain C++ throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "write_dev_records.h"
#include "chunkio_amd/cio_write_dev_records.h"

using namespace cioa;

namespace {

// Image i has a run when i occurs in rec_img: a lower bound in the sorted
// array.  (Over a malformed array the answer may be wrong; every status of
// such a batch is overwritten, and the image check guards every read.)
__global__ void __launch_bounds__(256)
rec_images(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
           const uint64_t *__restrict__ img_caps, uint32_t n_img, const uint32_t *__restrict__ rec_img,
           uint32_t n_rec, int32_t *__restrict__ img_status, uint64_t *__restrict__ roff,
           uint64_t *__restrict__ rlen, uint64_t *__restrict__ room, uint32_t *__restrict__ newlen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_img) {
        return;
    }
    uint32_t lo = 0, hi = n_rec;
    while (lo < hi) {
        const uint32_t mid = lo + (hi - lo) / 2;
        if (rec_img[mid] < i) {
            lo = mid + 1;
        } else {
            hi = mid;
        }
    }
    bool ok = true;
    uint64_t b = 0, rm = 0;
    uint32_t content32 = 0;
    if (lo < n_rec && rec_img[lo] == i) {
        const uint64_t off = img_offs[i], cap = img_caps[i];
        uint32_t meta = 0;
        uint64_t content = 0;
        ok = image_ok(base, dev_bytes, off, cap, meta, content);
        if (ok) {
            b = off + kRecHdr + meta + content;
            rm = rec_room(cap, meta, content);
            content32 = (uint32_t) content;
        }
    }
    img_status[i] = ok ? CIO_OK : CIO_ERROR;
    roff[i] = b;
    rlen[i] = 0;
    room[i] = rm;
    newlen[i] = content32;
}

// The segmented inclusive scan of v over the kRecBlock threads of a workgroup
// with rec_combine, through LDS; returns the exclusive result of thread tid,
// total: the combination over the workgroup.
__device__ __forceinline__ RecSeg block_seg_scan_excl(uint32_t *shf, uint64_t *shs, uint32_t tid, RecSeg v,
                                                      RecSeg &total)
{
    shf[tid] = v.flag;
    shs[tid] = v.sum;
    __syncthreads();
    for (uint32_t off = 1; off < kRecBlock; off <<= 1) {
        RecSeg x = rec_none();
        if (tid >= off) {
            x.flag = shf[tid - off];
            x.sum = shs[tid - off];
        }
        const RecSeg mine = {shf[tid], shs[tid]};
        __syncthreads();
        const RecSeg y = rec_combine(x, mine);
        shf[tid] = y.flag;
        shs[tid] = y.sum;
        __syncthreads();
    }
    RecSeg excl = rec_none();
    if (tid) {
        excl.flag = shf[tid - 1];
        excl.sum = shs[tid - 1];
    }
    total.flag = shf[kRecBlock - 1];
    total.sum = shs[kRecBlock - 1];
    __syncthreads();
    return excl;
}

// lflag[r], lsum[r]: the combination of the records of r's workgroup before r.
// gflag[wg]: bit 0 the aggregate's flag, bit 1 "malformed in this workgroup";
// gsum[wg]: the aggregate's sum.
__global__ void __launch_bounds__(kRecBlock)
rec_scan_local(const uint32_t *__restrict__ rec_img, const uint64_t *__restrict__ rec_offs,
               const uint64_t *__restrict__ rec_lens, uint32_t n_rec, uint32_t n_img, uint64_t src_bytes,
               uint64_t *__restrict__ lflag, uint64_t *__restrict__ lsum, uint32_t *__restrict__ gflag,
               uint64_t *__restrict__ gsum)
{
    __shared__ uint32_t shf[kRecBlock];
    __shared__ uint64_t shs[kRecBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t r = (uint64_t) blockIdx.x * kRecBlock + tid;
    RecSeg v = rec_none();
    int bad = 0;
    if (r < n_rec) {
        const uint32_t img = rec_img[r], prev = r ? rec_img[r - 1] : 0;
        bad = rec_malformed(r, img, prev, n_img);
        v.flag = rec_head(r, img, prev);
        v.sum = rec_value(rec_offs[r], rec_lens[r], src_bytes);
    }
    RecSeg total;
    const RecSeg excl = block_seg_scan_excl(shf, shs, tid, v, total);
    const int anybad = __syncthreads_or(bad);
    if (r < n_rec) {
        lflag[r] = excl.flag;
        lsum[r] = excl.sum;
    }
    if (tid == 0) {
        gflag[blockIdx.x] = total.flag | (anybad ? 2u : 0u);
        gsum[blockIdx.x] = total.sum;
    }
}

// (gflag[j] bit 0, gsum[j]) becomes the combination of the aggregates before
// workgroup j; ghdr[0] whether any workgroup found the grouping malformed.
__global__ void __launch_bounds__(kRecBlock)
rec_scan_groups(uint32_t *__restrict__ gflag, uint64_t *__restrict__ gsum, uint32_t nb, uint32_t *__restrict__ ghdr)
{
    __shared__ uint32_t shf[kRecBlock];
    __shared__ uint64_t shs[kRecBlock];
    const uint32_t tid = threadIdx.x;
    RecSeg carry = rec_none();                // the aggregates before `base` (the same in every thread)
    int bad = 0;
    for (uint32_t base = 0; base < nb; base += kRecBlock) {
        const uint32_t j = base + tid;
        RecSeg v = rec_none();
        if (j < nb) {
            const uint32_t f = gflag[j];
            bad |= (int) (f >> 1);
            v.flag = f & 1u;
            v.sum = gsum[j];
        }
        RecSeg pass;
        const RecSeg excl = block_seg_scan_excl(shf, shs, tid, v, pass);
        if (j < nb) {
            const RecSeg c = rec_combine(carry, excl);
            gflag[j] = c.flag;
            gsum[j] = c.sum;
        }
        carry = rec_combine(carry, pass);
    }
    const int anybad = __syncthreads_or(bad);
    if (tid == 0) {
        ghdr[0] = anybad ? 1u : 0u;
    }
}

// lflag / lsum are the arenas soff / dst: read first, then overwritten with
// the record's final source offset and destination.
__global__ void __launch_bounds__(kRecBlock)
rec_place(const uint32_t *__restrict__ rec_img, const uint64_t *__restrict__ rec_offs,
          const uint64_t *__restrict__ rec_lens, uint32_t n_rec, uint64_t src_bytes,
          const uint32_t *__restrict__ gflag, const uint64_t *__restrict__ gsum, const uint32_t *__restrict__ ghdr,
          const int32_t *__restrict__ img_status, const uint64_t *__restrict__ room, const uint64_t *roff,
          uint64_t *rlen, uint32_t *newlen, int32_t *__restrict__ rec_status, uint64_t *soff,
          uint64_t *__restrict__ slen, uint64_t *dst)
{
    const uint64_t r = (uint64_t) blockIdx.x * kRecBlock + threadIdx.x;
    if (r >= n_rec) {
        return;
    }
    bool accept = false;
    uint64_t so = 0, sl = 0, d = 0;
    if (ghdr[0] == 0) {                       // otherwise rec_img[r] may be no image of the batch
        const uint32_t img = rec_img[r];
        const RecSeg carry = {gflag[blockIdx.x], gsum[blockIdx.x]};
        const RecSeg local = {(uint32_t) soff[r], dst[r]};
        const uint64_t before = rec_before(rec_head(r, img, r ? rec_img[r - 1] : 0), carry, local);
        const uint64_t off = rec_offs[r], v = rec_value(off, rec_lens[r], src_bytes), rm = room[img];
        const bool ok = img_status[img] == CIO_OK;
        accept = rec_accept(ok, before, v, rm);
        if (accept) {
            so = v ? off : 0;
            sl = v;
            d = roff[img] + before;
            // the run's last accepted record: the run ends here, or the next record does not fit
            const uint64_t end = before + v;
            bool last = r + 1 == n_rec || rec_img[r + 1] != img;
            if (!last) {
                last = !rec_accept(ok, end, rec_value(rec_offs[r + 1], rec_lens[r + 1], src_bytes), rm);
            }
            if (last && end != 0) {
                rlen[img] = end;
                newlen[img] += (uint32_t) end;    // rec_images left the content length there; end <= room
            }
        }
    }
    rec_status[r] = accept ? CIO_OK : CIO_ERROR;
    soff[r] = so;
    slen[r] = sl;
    dst[r] = d;
}

// crc: the CRC launch's output, or NULL without CIO_CHECKSUM; hdr: the last
// planner's header.
__global__ void __launch_bounds__(256)
rec_finish(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n_img, int32_t *__restrict__ img_status,
           const uint64_t *__restrict__ rlen, const uint32_t *__restrict__ newlen, const uint32_t *__restrict__ crc,
           const unsigned long long *__restrict__ hdr, const uint32_t *__restrict__ ghdr,
           uint32_t *__restrict__ crc_cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n_img) {
        return;
    }
    if (ghdr[0] != 0) {
        img_status[i] = CIO_ERROR;            // malformed grouping: the whole batch
        return;
    }
    if (img_status[i] != CIO_OK || rlen[i] == 0) {
        return;
    }
    if (hdr[kDevHdrStatus] != 0) {
        img_status[i] = CIO_ERROR;            // the planner published an empty batch
        return;
    }
    uint8_t *p = base + img_offs[i];
    if (crc) {
        const uint32_t c = crc[i];
        crc_cur[i] = c;
        p[2] = (uint8_t) c;                   // raw state in an 8-byte crc_t, host byte order
        p[3] = (uint8_t) (c >> 8);
        p[4] = (uint8_t) (c >> 16);
        p[5] = (uint8_t) (c >> 24);
        p[6] = p[7] = p[8] = p[9] = 0;
    }
    const uint32_t nl = newlen[i];
    p[10] = (uint8_t) (nl >> 24);
    p[11] = (uint8_t) (nl >> 16);
    p[12] = (uint8_t) (nl >> 8);
    p[13] = (uint8_t) nl;
}

// The four bookkeeping kernels: after them dev_rec_status, the record regions
// (soff, slen, dst) and the images' CRC regions (roff, rlen) are final.
int launch_bookkeeping(cio_dev_writer *w, const uint8_t *base, uint64_t dev_bytes, const uint64_t *img_offs,
                       const uint64_t *img_caps, size_t n_img, uint64_t src_bytes, const uint32_t *rec_img,
                       const uint64_t *rec_offs, const uint64_t *rec_lens, size_t n_rec, int32_t *img_status,
                       int32_t *rec_status, hipStream_t s)
{
    const uint32_t nb = blocks_of(n_rec, kRecBlock);
    hipLaunchKernelGGL(rec_images, dim3(blocks_of(n_img, 256)), dim3(256), 0, s, base, dev_bytes, img_offs, img_caps,
                       (uint32_t) n_img, rec_img, (uint32_t) n_rec, img_status, w->roff, w->rlen, w->groom,
                       w->newlen);
    hipLaunchKernelGGL(rec_scan_local, dim3(nb), dim3(kRecBlock), 0, s, rec_img, rec_offs, rec_lens,
                       (uint32_t) n_rec, (uint32_t) n_img, src_bytes, w->soff, w->dst, w->gflag, w->gsum);
    hipLaunchKernelGGL(rec_scan_groups, dim3(1), dim3(kRecBlock), 0, s, w->gflag, w->gsum, nb, w->ghdr);
    hipLaunchKernelGGL(rec_place, dim3(nb), dim3(kRecBlock), 0, s, rec_img, rec_offs, rec_lens, (uint32_t) n_rec,
                       src_bytes, w->gflag, w->gsum, w->ghdr, img_status, w->groom, w->roff, w->rlen, w->newlen,
                       rec_status, w->soff, w->slen, w->dst);
    HIP_TRY(hipGetLastError(), "cio_file_write_records_batch_dev: bookkeeping kernels launch");
    return CIO_OK;
}

}  // namespace

namespace cioa {

// The argument checks of the grouped and the ungrouped append (declared in
// cio_gpu_internal.h): 0 go on, 1 a no-op, CIO_ERROR refused with a message
// under the caller's name.
int check_records(const char *who, const cio_dev_writer *w, const void *dev_base, const uint64_t *offs,
                  const uint64_t *caps, size_t n_img, const void *dev_src, const uint32_t *rec_img,
                  const uint64_t *rec_offs, const uint64_t *rec_lens, size_t n_rec, int flags,
                  const uint32_t *crc_cur, const int32_t *img_status, const int32_t *rec_status)
{
    if (flags & ~CIO_CHECKSUM) {
        return fail_who(who, "unknown flags");
    }
    if (!w) {
        return fail_who(who, "null writer");
    }
    if (n_img == 0 || n_rec == 0) {
        return 1;
    }
    if (!dev_base || !offs || !caps || !dev_src || !rec_img || !rec_offs || !rec_lens || !img_status ||
        !rec_status || ((flags & CIO_CHECKSUM) && !crc_cur)) {
        return fail_who(who, "null pointer");
    }
    if (n_img > w->max_chunks) {
        return fail_who(who, "more images than the writer was created for");
    }
    if (n_rec > w->max_chunks) {
        return fail_who(who, "more records than the writer was created for");
    }
    return 0;
}

}  // namespace cioa

extern "C" {

int cio_file_write_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                     const void *dev_src, uint64_t src_bytes,
                                     const uint32_t *dev_rec_img, const uint64_t *dev_rec_offs,
                                     const uint64_t *dev_rec_lens, size_t n_rec,
                                     int flags, uint32_t *dev_crc_cur, int32_t *dev_img_status,
                                     int32_t *dev_rec_status, void *stream)
{
    static const char who[] = "cio_file_write_records_batch_dev";
    const int rc = check_records(who, w, dev_base, dev_img_offs, dev_img_caps, n_img, dev_src, dev_rec_img,
                                 dev_rec_offs, dev_rec_lens, n_rec, flags, dev_crc_cur, dev_img_status,
                                 dev_rec_status);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const bool checksum = (flags & CIO_CHECKSUM) != 0;
    if (launch_bookkeeping(w, base, dev_bytes, dev_img_offs, dev_img_caps, n_img, src_bytes, dev_rec_img,
                           dev_rec_offs, dev_rec_lens, n_rec, dev_img_status, dev_rec_status, s) != CIO_OK ||
        devplan_launch_planner(w->dp, src_bytes, w->soff, w->slen, n_rec, nullptr, s) != CIO_OK ||
        launch_copy(w, dev_base, dev_src, n_rec, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum &&
        (devplan_launch_planner(w->dp, dev_bytes, w->roff, w->rlen, n_img, nullptr, s) != CIO_OK ||
         devplan_crc_launch(w->dp->p, w->dp->hdr, dev_base, dev_crc_cur, w->crc, n_img, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(rec_finish, dim3(blocks_of(n_img, 256)), dim3(256), 0, s, base, dev_img_offs,
                       (uint32_t) n_img, dev_img_status, w->rlen, w->newlen, checksum ? w->crc : nullptr,
                       w->dp->hdr, w->ghdr, dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_write_records_batch_dev: finish kernel launch");
    return CIO_OK;
}

/* Measurement hook (not in the public header; tools/write_records_ab.py): the
 * four bookkeeping kernels of a cio_file_write_records_batch_dev ALONE between
 * two HIP events.  Nothing of the images changes. */
int cioa_debug_write_records_book_events(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                         const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                         uint64_t src_bytes, const uint32_t *dev_rec_img,
                                         const uint64_t *dev_rec_offs, const uint64_t *dev_rec_lens, size_t n_rec,
                                         int32_t *dev_img_status, int32_t *dev_rec_status, void *stream,
                                         void *ev_start, void *ev_stop)
{
    if (!ev_start || !ev_stop ||
        check_records("cioa_debug_write_records_book_events", w, dev_base, dev_img_offs, dev_img_caps, n_img,
                      dev_base, dev_rec_img, dev_rec_offs, dev_rec_lens, n_rec, 0, nullptr, dev_img_status,
                      dev_rec_status) != 0) {
        return fail("cioa_debug_write_records_book_events: bad argument");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_start), s), "hipEventRecord");
    if (launch_bookkeeping(w, reinterpret_cast<const uint8_t *>(dev_base), dev_bytes, dev_img_offs, dev_img_caps,
                           n_img, src_bytes, dev_rec_img, dev_rec_offs, dev_rec_lens, n_rec, dev_img_status,
                           dev_rec_status, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_stop), s), "hipEventRecord");
    return CIO_OK;
}

}  // extern "C"
