// rotate_dev_gpu.hip -- rotating full chunk images in HBM: sealing them where
// they lie and reopening them, with the same metadata, in a slot of a
// caller-provided arena, for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_write_dev_rotate.h; DESIGN.md §19.
//
// A rotate batch is a serial chain of kernels on the caller's stream:
//
//   grow_clear      records variant; grow's need sums (launch_need_sums,
//   grow_need       grow_dev_gpu.hip), unchanged: the per-image need arena and
//                   the header word re-zeroed (a kernel of its own: zeroing
//                   inside the sums would race with the sums of other
//                   workgroups), then one thread per record: the index check (an
//                   index >= n_img is published in the header word) and
//                   need[img] += min(len, 2^32), a plain atomicAdd.
//                   (rotate_sums_wave, the same sums with a wave-level
//                   pre-reduction -- a segmented scan over the wave
//                   sums every run of equal indices, the last lane of a run
//                   issues ONE atomicAdd -- is measured through the hook and not
//                   launched by the calls: DESIGN.md §19.)
//   rotate_headers  one thread per image: rules 1..4 (the image check of the
//                   write path, the arena, full or not, the metadata against
//                   new_cap), the CRC state after the fresh image's two length
//                   bytes, a workgroup scan of the images that reach the
//                   placement and the workgroup's total
//   rotate_scan     ONE workgroup, looping over however many totals there are:
//                   their exclusive scan, and dev_total
//   rotate_place    one thread per image: the fresh image's offset, its list
//                   index, whether both fit, the status; into the writer's
//                   arenas the metadata region (source old_off + 24, destination
//                   new_off + 24), zero-length for every image that is not
//                   rotated; and who writes the arena's top and the list's count
//   planner         devplan's four kernels over the metadata regions
//   append_copy     the write path's copy kernel (write_dev_gpu.hip), unchanged:
//                   source buffer = destination buffer = dev_base; the regions
//                   are disjoint (an image inside the arena's free part is
//                   rejected)
//   CRC             with CIO_CHECKSUM: the device-planned stream kernel over the
//                   SOURCE metadata, seeds = the states after the length bytes,
//                   output in writer scratch
//   rotate_commit   one thread per image: the seal of the old image, the list
//                   entry, the fresh 24-byte header, crc_cur, dev_img_offs /
//                   dev_img_caps in place, the top and the count (exactly one
//                   thread each), the planner's status
//
// Every image that reaches the placement has the same slot, new_cap rounded up
// to align, so the scan counts images and the sum of the slots in front of one
// is its ordinal times the slot (rot_slots): one scan gives both the offset and
// the list index.
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another.  The planner's own checks cannot fire: every region lies inside
// an image rotate_headers found inside dev_bytes.
//
// The arithmetic is rotate_dev.h, the text tools/rotate_check.cpp runs on the
// host.  Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "rotate_dev.h"
#include "block_scan_gpu.h"
#include "chunkio_amd/cio_write_dev_rotate.h"

using namespace cioa;

namespace {

// The need sums (grow_need, grow_dev_gpu.hip: one plain atomicAdd per record)
// with a wave-level pre-reduction; launched by the measurement hook only
// (section 6).  It missed one of the two conditions set for it (DESIGN.md §19,
// leg (e)), so it is not what ships.  Every lane of every wave takes part in the shuffles:
// a lane without a record holds the key kRotNoImage and the length 0, and
// never issues.
__global__ void __launch_bounds__(kRotSumBlock)
rotate_sums_wave(const uint32_t *__restrict__ rec_img, const uint64_t *__restrict__ rec_lens, uint32_t n_rec,
            uint32_t n_img, unsigned long long *need, uint32_t *ghdr)
{
    const uint32_t r = blockIdx.x * kRotSumBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kRotLanes - 1);
    uint32_t key = kRotNoImage;
    uint64_t v = 0;
    if (r < n_rec) {
        const uint32_t img = rec_img[r];
        if (img >= n_img) {
            atomicOr(ghdr, 1u);                   // the whole call is rejected
        } else {
            key = img;
            v = umin(rec_lens[r], kGrowLenClamp);
        }
    }
    const uint32_t prev = (uint32_t) __shfl_up((int) key, 1);
    const bool head = rot_run_head(lane, key, prev);
    bool f = head;
#pragma unroll
    for (uint32_t d = 1; d < kRotLanes; d <<= 1) {
        const uint64_t v_up = (uint64_t) __shfl_up((unsigned long long) v, d);
        const bool f_up = __shfl_up((int) f, d) != 0;
        rot_seg_step(lane, d, v, f, v_up, f_up);
    }
    const bool next_head = __shfl_down((int) head, 1) != 0;
    if ((lane + 1 == kRotLanes || next_head) && key < n_img) {
        atomicAdd(need + key, (unsigned long long) v);
    }
}

// ord[i] takes the number of images before entry i in its workgroup that reach
// the placement and rtot[blockIdx.x] the workgroup's count; hlen[i] the bytes
// 24 + meta of an image that reaches the placement, 0 otherwise; seed[i] the
// CRC state after the fresh image's bytes 22..23.
__global__ void __launch_bounds__(kRotBlock)
rotate_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
               const uint64_t *__restrict__ img_caps, uint32_t n, const uint64_t *__restrict__ need,
               const uint32_t *__restrict__ ghdr, const uint64_t *__restrict__ arena, uint64_t limit,
               uint64_t new_cap, int32_t *__restrict__ status, uint64_t *__restrict__ hlen,
               uint64_t *__restrict__ ord, uint32_t *__restrict__ seed, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kRotBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kRotBlock + tid;
    int32_t st = CIO_OK;
    uint64_t hl = 0;
    uint32_t meta = 0;
    if (i < n) {
        const uint64_t nd = need ? need[i] : 0;
        if (ghdr && ghdr[0] != 0) {
            st = CIO_ERROR;
        } else if (nd != 0 || limit != 0) {       // otherwise the image is not read
            const uint64_t off = img_offs[i], cap = img_caps[i];
            uint64_t content = 0;
            if (!image_ok(base, dev_bytes, off, cap, meta, content)) {
                st = CIO_ERROR;
            } else {
                const int verdict = rot_decide(off, cap, meta, content, nd, limit, new_cap, arena[0], arena[1]);
                if (verdict == kRotReject) {
                    st = CIO_ERROR;
                } else if (verdict == kRotFull) {
                    hl = kReadHdr + meta;
                }
            }
        }
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, tid, hl ? 1 : 0, total);
    if (tid == 0) {
        rtot[blockIdx.x] = total;
    }
    if (i < n) {
        status[i] = st;
        hlen[i] = hl;
        ord[i] = excl;
        seed[i] = rot_len_seed(hl ? meta : 0);
    }
}

// rtot[j] becomes the sum of the counts before workgroup j; total[0], total[1]
// the batch's dev_total.
__global__ void __launch_bounds__(kRotBlock)
rotate_scan(uint64_t *__restrict__ rtot, uint32_t nb, const uint64_t *__restrict__ arena, uint64_t new_cap,
            uint64_t align, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kRotBlock];
    uint64_t carry = 0;                       // totals_scan, written out (block_scan_gpu.h)
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        carry = totals_pass(sh, rtot, nb, base, carry);
    }
    if (threadIdx.x == 0) {
        total[0] = rot_total(arena[0], align, carry, grow_round_up(new_cap, align));
        total[1] = carry;
    }
}

// roff[i], rk[i]: the entry's place and list index (rot_place_code), for the
// accepted images and for the entry that writes the top and the count.
__global__ void __launch_bounds__(kRotBlock)
rotate_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ arena,
             const uint64_t *__restrict__ out_count, uint64_t dev_bytes, uint64_t new_cap, uint64_t align,
             const uint64_t *__restrict__ img_offs, int32_t *__restrict__ status, const uint64_t *__restrict__ hlen,
             const uint64_t *__restrict__ ord, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
             uint64_t *__restrict__ dst, uint64_t *__restrict__ roff, uint64_t *__restrict__ rk,
             uint32_t *__restrict__ code)
{
    const uint64_t i = (uint64_t) blockIdx.x * kRotBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t before = place_add(rtot[blockIdx.x], ord[i]);
    const uint64_t hl = hlen[i];
    uint64_t off, k;
    const uint32_t c = rot_place_code(arena[0], arena[1], dev_bytes, align, grow_round_up(new_cap, align),
                                      out_count[0], out_count[1], before, hl != 0, i + 1 == n, off, k);
    code[i] = c;
    roff[i] = off;
    rk[i] = k;
    if (c & kRotAccepted) {
        soff[i] = img_offs[i] + kReadHdr;
        slen[i] = hl - kReadHdr;
        dst[i] = off + kReadHdr;
        return;
    }
    if (hl != 0) {
        status[i] = CIO_ERROR;                // cut: the image stays valid where it is, unsealed
    }
    soff[i] = 0;
    slen[i] = 0;
    dst[i] = 0;
}

// hdr: the planner's header.  A planner that published an empty batch copied
// nothing: the accepted images are rejected where they were, unsealed, and the
// top and the count stay.  crc: the CRC launch's output over the metadata, or
// NULL without CIO_CHECKSUM.
__global__ void __launch_bounds__(kRotBlock)
rotate_commit(uint8_t *base, uint64_t *__restrict__ img_offs, uint64_t *__restrict__ img_caps, uint32_t n,
              int32_t *__restrict__ status, const uint64_t *__restrict__ hlen, const uint64_t *__restrict__ roff,
              const uint64_t *__restrict__ rk, const uint32_t *__restrict__ code,
              const uint32_t *__restrict__ seed, const uint32_t *__restrict__ crc,
              const unsigned long long *__restrict__ hdr, uint32_t *__restrict__ crc_cur, uint64_t new_cap,
              uint64_t align, uint64_t *__restrict__ arena, uint64_t *__restrict__ out_offs,
              uint64_t *__restrict__ out_caps, uint32_t *__restrict__ out_img, uint64_t *__restrict__ out_count)
{
    const uint64_t i = (uint64_t) blockIdx.x * kRotBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (c == 0) {
        return;
    }
    const bool bad = hdr[kDevHdrStatus] != 0;
    if (c & kRotAccepted) {
        if (bad) {
            status[i] = CIO_ERROR;
        } else {
            const uint64_t old_off = img_offs[i], new_off = roff[i], k = rk[i];
            const uint32_t meta = (uint32_t) (hlen[i] - kReadHdr);
            if (crc) {                            // the seal: htonl(crc_finalize) in an 8-byte crc_t
                uint8_t *p = base + old_off;
                const uint32_t fin = crc_cur[i] ^ 0xffffffffu;
                p[2] = (uint8_t) (fin >> 24);
                p[3] = (uint8_t) (fin >> 16);
                p[4] = (uint8_t) (fin >> 8);
                p[5] = (uint8_t) fin;
                p[6] = p[7] = p[8] = p[9] = 0;
                crc_cur[i] = meta ? crc[i] : seed[i];
            }
            out_offs[k] = old_off;
            out_caps[k] = img_caps[i];
            out_img[k] = (uint32_t) i;
            rot_fresh_header(base + new_off, meta, crc != nullptr);
            img_offs[i] = new_off;
            img_caps[i] = new_cap;
        }
    }
    if (!bad && (c & (kRotEndAt | kRotEndLast))) {
        uint64_t top, count;
        rot_end_values(c, roff[i], rk[i], grow_round_up(new_cap, align), top, count);
        arena[0] = top;
        out_count[0] = count;
    }
}

// The argument checks, before any device call.  Returns 1 when the call is a
// no-op (an empty batch), 0 to go on, CIO_ERROR.
int check_rotate(const RotArgs &a, bool records)
{
    if (a.flags & ~CIO_CHECKSUM) {
        return fail_who(a.who, "unknown flags");
    }
    if (a.new_cap < kReadHdr) {
        return fail_who(a.who, "new_cap must be at least 24");
    }
    if (!pow2(a.align) || a.align > 4096) {
        return fail_who(a.who, "align must be a power of two in 1 .. 4096");
    }
    if (!a.w) {
        return fail_who(a.who, "null writer");
    }
    if (a.n == 0 || (records && a.n_rec == 0)) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.arena || !a.out_offs || !a.out_caps || !a.out_img ||
        !a.out_count || !a.total || !a.status || ((a.flags & CIO_CHECKSUM) && !a.crc_cur) ||
        (records && (!a.rec_img || !a.rec_lens))) {
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

// Measurement: the sections of cioa_debug_rotate_events (SectionEvents).
enum { kSecNone = 0, kSecSums, kSecBook, kSecCopy, kSecCrc, kSecCommit, kSecSumsWave };

int launch_rotate(const RotArgs &a, bool records, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    uint8_t *base = reinterpret_cast<uint8_t *>(a.dev_base);
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kRotBlock);
    const bool checksum = (a.flags & CIO_CHECKSUM) != 0;
    if (rotate_launch_front(a, records, s, ev) != CIO_OK) {
        return CIO_ERROR;
    }
    // writer arenas: gcap 24 + meta of an image that reaches the placement, groom its ordinal, roff / rlen its
    // place and list index, newlen the place kernel's code
    hipLaunchKernelGGL(rotate_place, dim3(nb), dim3(kRotBlock), 0, s, n, w->rtot, a.arena, a.out_count, a.dev_bytes,
                       a.new_cap, a.align, a.offs, a.status, w->gcap, w->groom, w->soff, w->slen, w->dst, w->roff,
                       w->rlen, w->newlen);
    HIP_TRY(hipGetLastError(), "rotate: placement kernels launch");
    if (mark(ev, kSecBook, false, s) != CIO_OK || mark(ev, kSecCopy, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK ||
        launch_copy(w, a.dev_base, a.dev_base, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (mark(ev, kSecCopy, false, s) != CIO_OK || mark(ev, kSecCrc, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum && devplan_crc_launch(w->dp->p, w->dp->hdr, a.dev_base, w->seed, w->crc, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (mark(ev, kSecCrc, false, s) != CIO_OK || mark(ev, kSecCommit, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(rotate_commit, dim3(nb), dim3(kRotBlock), 0, s, base, a.offs, a.caps, n, a.status, w->gcap,
                       w->roff, w->rlen, w->newlen, w->seed, checksum ? w->crc : (const uint32_t *) nullptr,
                       w->dp->hdr, a.crc_cur, a.new_cap, a.align, a.arena, a.out_offs, a.out_caps, a.out_img,
                       a.out_count);
    HIP_TRY(hipGetLastError(), "rotate: commit kernel launch");
    return mark(ev, kSecCommit, false, s);
}

}  // namespace

int cioa::rotate_check_args(const RotArgs &a, bool records)
{
    return check_rotate(a, records);
}

// The head of launch_rotate, and of the variant that takes its slots from a
// pool first (pool_dev_gpu.hip): the need sums of the records variant,
// rotate_headers and rotate_scan.  No event lies between rotate_scan and
// rotate_place, so the bookkeeping section opens here and closes in the caller.
int cioa::rotate_launch_front(const RotArgs &a, bool records, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kRotBlock);
    const uint64_t *need = a.need;
    const bool wave = ev && ev->section == kSecSumsWave;
    if (mark(ev, kSecSums, true, s) != CIO_OK || mark(ev, kSecSumsWave, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (records) {
        // section 6: the clear alone, then the pre-reduced sums in grow_need's place
        if (launch_need_sums(w, a.rec_img, a.rec_lens, a.n, wave ? 0 : a.n_rec, s) != CIO_OK) {
            return CIO_ERROR;
        }
        if (wave) {
            hipLaunchKernelGGL(rotate_sums_wave, dim3(blocks_of(a.n_rec, kRotSumBlock)), dim3(kRotSumBlock), 0, s,
                               a.rec_img, a.rec_lens, (uint32_t) a.n_rec, n,
                               reinterpret_cast<unsigned long long *>(w->gneed), w->growhdr);
            HIP_TRY(hipGetLastError(), "rotate: sums kernels launch");
        }
        need = w->gneed;
    }
    if (mark(ev, kSecSums, false, s) != CIO_OK || mark(ev, kSecSumsWave, false, s) != CIO_OK ||
        mark(ev, kSecBook, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(rotate_headers, dim3(nb), dim3(kRotBlock), 0, s, reinterpret_cast<const uint8_t *>(a.dev_base),
                       a.dev_bytes, a.offs, a.caps, n, need, records ? w->growhdr : (const uint32_t *) nullptr,
                       a.arena, a.limit, a.new_cap, a.status, w->gcap, w->groom, w->seed, w->rtot);
    hipLaunchKernelGGL(rotate_scan, dim3(1), dim3(kRotBlock), 0, s, w->rtot, nb, a.arena, a.new_cap, a.align,
                       a.total);
    HIP_TRY(hipGetLastError(), "rotate: header kernels launch");
    return CIO_OK;
}

extern "C" {

int cio_file_rotate_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                              uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                              const uint64_t *dev_need, uint64_t limit,
                              uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                              uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                              uint64_t *dev_out_count, int flags,
                              uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const RotArgs a = {"cio_file_rotate_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_need,
                       nullptr, nullptr, 0, limit, new_cap, align, dev_arena, dev_out_offs, dev_out_caps,
                       dev_out_img, dev_out_count, flags, dev_crc_cur, dev_total, dev_status};
    const int rc = check_rotate(a, false);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_rotate(a, false, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int cio_file_rotate_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                      uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                      const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                      uint64_t limit,
                                      uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                      uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                      uint64_t *dev_out_count, int flags,
                                      uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const RotArgs a = {"cio_file_rotate_records_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                       nullptr, dev_rec_img, dev_rec_lens, n_rec, limit, new_cap, align, dev_arena, dev_out_offs,
                       dev_out_caps, dev_out_img, dev_out_count, flags, dev_crc_cur, dev_total, dev_status};
    const int rc = check_rotate(a, true);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_rotate(a, true, reinterpret_cast<hipStream_t>(stream), nullptr);
}

/* Measurement hook (not in the public header; tools/rotate_dev_ab.py): a whole
 * rotate call -- the records variant when dev_rec_img is not NULL -- with the
 * two HIP events around ONE section of its chain: 1 grow_clear + grow_need,
 * 2 rotate_headers + rotate_scan + rotate_place, 3 the planner and append_copy,
 * 4 the CRC launch, 5 rotate_commit, 6 grow_clear + rotate_sums_wave (the
 * pre-reduced sums INSTEAD of grow_need; nothing else launches that kernel). */
int cioa_debug_rotate_events(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes, uint64_t *dev_img_offs,
                             uint64_t *dev_img_caps, size_t n, const uint64_t *dev_need,
                             const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                             uint64_t limit, uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                             uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                             uint64_t *dev_out_count, int flags, uint32_t *dev_crc_cur, uint64_t *dev_total,
                             int32_t *dev_status, void *stream, int section, void *ev_start, void *ev_stop)
{
    const bool records = dev_rec_img != nullptr;
    const RotArgs a = {"cioa_debug_rotate_events", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_need,
                       dev_rec_img, dev_rec_lens, n_rec, limit, new_cap, align, dev_arena, dev_out_offs,
                       dev_out_caps, dev_out_img, dev_out_count, flags, dev_crc_cur, dev_total, dev_status};
    if (!ev_start || !ev_stop || section < kSecSums || section > kSecSumsWave ||
        ((section == kSecSums || section == kSecSumsWave) && !records) ||
        (section == kSecCrc && !(flags & CIO_CHECKSUM)) || check_rotate(a, records) != 0) {
        return fail("cioa_debug_rotate_events: bad argument");
    }
    const SectionEvents ev = {section, reinterpret_cast<hipEvent_t>(ev_start), reinterpret_cast<hipEvent_t>(ev_stop)};
    return launch_rotate(a, records, reinterpret_cast<hipStream_t>(stream), &ev);
}

}  // extern "C"
