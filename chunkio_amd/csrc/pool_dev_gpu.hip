// pool_dev_gpu.hip -- recycling drained chunk slots in HBM: releasing them to a
// caller-owned pool (with an in-place compaction of the list of finished
// chunks) and rotating full images into pool slots before the arena is touched,
// for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_write_dev_pool.h; DESIGN.md §22.
//
// A release batch is a serial chain of kernels on the caller's stream:
//
//   release_headers  one thread per entry: rules 0..5 (is it among the first m,
//                    does an image still live there, the gate, the write path's
//                    image check, the pool's class and alignment), a workgroup
//                    scan of the entries that reach the placement and the
//                    workgroup's total
//   release_scan     ONE workgroup, looping over however many totals there are:
//                    their exclusive scan, and dev_total
//   release_place    one thread per entry: the pool index, whether the pool
//                    takes it, the status, who writes the pool's count; the
//                    fill's region (the whole slot of an accepted entry,
//                    zero-length otherwise); with CIOA_RELEASE_COMPACT every
//                    kept entry goes to its new position IN WRITER SCRATCH and
//                    the vacated positions are prepared there
//   planner, fill    with CIOA_RELEASE_ZERO: devplan's four kernels over the
//                    slots and grow's byte-balanced zero fill, unchanged
//   release_commit   one thread per entry: the push, bytes 0..1 of the slot, the
//                    pool's count (exactly one thread), the scratch copied back
//                    over the list and dev_count[0] (exactly one thread), the
//                    planner's status
//
// A rotate batch from the pool is rotate's chain with its own place and commit:
// the need sums, rotate_headers and rotate_scan run unchanged
// (rotate_launch_front, rotate_dev_gpu.hip); rotpool_place gives ordinal j <
// F pool entry count - 1 - j and every later ordinal arena slot j - F, and
// rewrites dev_total[0]; the planner, append_copy and the CRC launch follow as
// in rotate; rotpool_commit is rotate_commit with the slot's own capacity and
// the three end words.
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another.  The arithmetic is pool_dev.h, the text tools/pool_check.cpp runs
// on the host.  Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "pool_dev.h"
#include "block_scan_gpu.h"
#include "chunkio_amd/cio_write_dev_pool.h"

using namespace cioa;

namespace {

// code[i] takes kRelIn and kRelReach, ord[i] the number of entries before i in
// its workgroup that reach the placement, rtot[blockIdx.x] the workgroup's
// count.
__global__ void __launch_bounds__(kPoolBlock)
release_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ offs,
                const uint64_t *__restrict__ caps, uint32_t n, const uint64_t *__restrict__ count,
                const int32_t *__restrict__ gate, const uint64_t *__restrict__ live,
                const uint64_t *__restrict__ pool, int32_t *__restrict__ status, uint64_t *__restrict__ ord,
                uint32_t *__restrict__ code, uint64_t *__restrict__ rtot)
{
    __shared__ uint64_t sh[kPoolBlock];
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kPoolBlock + tid;
    const uint64_t m = pool_m(n, count != nullptr, count ? count[0] : 0);
    int32_t st = CIO_OK;
    uint32_t c = 0;
    if (i < m) {
        c = kRelIn;
        const uint64_t off = offs[i];
        if (live && live[i] == off) {
            // an image still lives there: kept
        } else if (gate && gate[i] != CIO_OK) {
            st = CIO_ERROR;                       // the slot is not read
        } else {
            const uint64_t cap = caps[i];
            const uint64_t cls = pool[kPoolCls], pal = pool[kPoolAlign];
            uint32_t meta;                        // the image's lengths: checked, not used
            uint64_t content;
            if (pool_sound(pool[kPoolCount], pool[kPoolCap], cls, pal) &&
                image_ok(base, dev_bytes, off, cap, meta, content) && pool_takes(off, cap, cls, pal)) {
                c |= kRelReach;
            } else {
                st = CIO_ERROR;
            }
        }
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, tid, (c & kRelReach) ? 1 : 0, total);
    if (tid == 0) {
        rtot[blockIdx.x] = total;
    }
    if (i < n) {
        status[i] = st;
        ord[i] = excl;
        code[i] = c;
    }
}

// rtot[j] becomes the sum of the counts before workgroup j; total[0], total[1]
// the batch's dev_total.
__global__ void __launch_bounds__(kPoolBlock)
release_scan(uint64_t *__restrict__ rtot, uint32_t nb, uint32_t n, const uint64_t *__restrict__ count,
             const uint64_t *__restrict__ pool, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kPoolBlock];
    uint64_t carry = 0;                       // totals_scan, written out (block_scan_gpu.h)
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        carry = totals_pass(sh, rtot, nb, base, carry);
    }
    if (threadIdx.x == 0) {
        const uint64_t m = pool_m(n, count != nullptr, count ? count[0] : 0);
        total[0] = carry;
        total[1] = pool_kept_total(m, carry,
                                   pool_room(pool[kPoolCount], pool[kPoolCap], pool[kPoolCls], pool[kPoolAlign]));
    }
}

// code[i] gains the placement's bits; slot[i] the entry's pool index; zoff[i],
// zlen[i] the slot of an accepted entry (0, 0 otherwise: the fill's planner
// reads all n).  compact: koff, kcap, kimg take the list as it will be.
__global__ void __launch_bounds__(kPoolBlock)
release_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ count,
              const uint64_t *__restrict__ pool, const uint64_t *__restrict__ offs,
              const uint64_t *__restrict__ caps, const uint32_t *__restrict__ img, int32_t *__restrict__ status,
              const uint64_t *__restrict__ ord, uint32_t *__restrict__ code, uint64_t *__restrict__ slot,
              uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen, int compact,
              const uint64_t *__restrict__ total, uint64_t *__restrict__ koff, uint64_t *__restrict__ kcap,
              uint32_t *__restrict__ kimg)
{
    const uint64_t i = (uint64_t) blockIdx.x * kPoolBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    uint32_t c = code[i];
    uint64_t zo = 0, zl = 0;
    if (c & kRelIn) {
        const uint64_t m = pool_m(n, count != nullptr, count ? count[0] : 0);
        const uint64_t have = pool[kPoolCount];
        const uint64_t room = pool_room(have, pool[kPoolCap], pool[kPoolCls], pool[kPoolAlign]);
        const uint64_t before = place_add(rtot[blockIdx.x], ord[i]);
        uint64_t sl;
        c |= pool_release_code(have, room, before, (c & kRelReach) != 0, i + 1 == m, sl);
        slot[i] = sl;
        code[i] = c;
        if (c & kRelAccepted) {
            zo = offs[i];
            zl = caps[i];
        } else if (c & kRelReach) {
            status[i] = CIO_ERROR;                // cut: the entry is kept
        }
        if (compact) {
            if (!(c & kRelAccepted)) {
                const uint64_t p = pool_kept_pos(i, before, room);
                koff[p] = offs[i];
                kcap[p] = caps[i];
                if (img) {
                    kimg[p] = img[i];
                }
            }
            if (i >= total[1]) {                  // vacated: no kept entry lands at or behind the kept total
                koff[i] = 0;
                kcap[i] = 0;
                kimg[i] = kPoolNoImage;
            }
        }
    }
    zoff[i] = zo;
    zlen[i] = zl;
}

// hdr: the fill's planner's header, or NULL without CIOA_RELEASE_ZERO.  A
// planner that published an empty batch filled nothing: no entry is accepted,
// nothing is marked, and neither the pool nor the list is written.
__global__ void __launch_bounds__(kPoolBlock)
release_commit(uint8_t *base, uint64_t *__restrict__ offs, uint64_t *__restrict__ caps, uint32_t *__restrict__ img,
               uint32_t n, uint64_t *count, int32_t *__restrict__ status, const uint32_t *__restrict__ code,
               const uint64_t *__restrict__ slot, const uint64_t *__restrict__ zoff,
               const uint64_t *__restrict__ zlen, const unsigned long long *__restrict__ hdr, int compact,
               const uint64_t *__restrict__ koff, const uint64_t *__restrict__ kcap,
               const uint32_t *__restrict__ kimg, uint64_t *__restrict__ pool_offs,
               uint64_t *__restrict__ pool_caps, uint64_t *pool, uint64_t *total)
{
    const uint64_t i = (uint64_t) blockIdx.x * kPoolBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t c = code[i];
    if (c == 0) {
        return;
    }
    if (hdr && hdr[kDevHdrStatus] != 0) {
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
        pool_offs[k] = off;
        pool_caps[k] = zlen[i];
        base[off] = 0;                            // no magic: a stale reference fails every image check
        base[off + 1] = 0;
    }
    if (c & (kRelEndAt | kRelEndLast)) {
        pool[kPoolCount] = pool_release_end(c, slot[i]);
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

// rotate_place with the pool in front of the arena.  roff[i], rk[i], rcap[i]:
// the fresh image's place, list index and capacity; for the entry with a
// kRotEnd* bit etop[i], epool[i]: the top and the pool count it writes (the
// list's count follows from rk[i], as in rot_end_values).  Thread 0 replaces
// rotate_scan's dev_total[0] by the pool rule's.
__global__ void __launch_bounds__(kPoolBlock)
rotpool_place(uint32_t n, const uint64_t *__restrict__ rtot, const uint64_t *__restrict__ arena,
              const uint64_t *__restrict__ out_count, const uint64_t *__restrict__ pool_offs,
              const uint64_t *__restrict__ pool_caps, const uint64_t *__restrict__ pool, uint64_t dev_bytes,
              uint64_t new_cap, uint64_t align, const uint64_t *__restrict__ img_offs,
              int32_t *__restrict__ status, const uint64_t *__restrict__ hlen, const uint64_t *__restrict__ ord,
              uint64_t *__restrict__ soff, uint64_t *__restrict__ slen, uint64_t *__restrict__ dst,
              uint64_t *__restrict__ roff, uint64_t *__restrict__ rk, uint64_t *__restrict__ rcap,
              uint64_t *__restrict__ etop, uint64_t *__restrict__ epool, uint32_t *__restrict__ code,
              uint64_t *__restrict__ total)
{
    const uint64_t i = (uint64_t) blockIdx.x * kPoolBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t top = arena[0], have0 = out_count[0], pcount = pool[kPoolCount];
    const uint64_t slot = grow_round_up(new_cap, align);
    const uint64_t F = pool_usable(pcount, pool[kPoolCap], pool[kPoolCls], pool[kPoolAlign], new_cap, align);
    if (i == 0) {
        total[0] = pool_rot_total(top, align, total[1], F, slot);
    }
    const uint64_t before = place_add(rtot[blockIdx.x], ord[i]);
    const uint64_t hl = hlen[i];
    uint64_t off, k, cap = new_cap;
    uint32_t c = pool_rot_place_code(top, arena[1], dev_bytes, align, slot, have0, out_count[1], F, before, hl != 0,
                                     i + 1 == n, off, k);
    if ((c & kRotAccepted) && before < F) {
        off = pool_offs[pcount - 1 - before];
        cap = pool_caps[pcount - 1 - before];
    }
    if (c & (kRotEndAt | kRotEndLast)) {
        uint64_t ntop, ncount, npool;
        c |= pool_rot_end_values(c, before, F, top, align, slot, have0, pcount, ntop, ncount, npool);
        etop[i] = ntop;                           // the new count is k, or k + 1 behind the entry's own image
        epool[i] = npool;
    }
    code[i] = c;
    roff[i] = off;
    rk[i] = k;
    rcap[i] = cap;
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

// rotate_commit with the fresh image's own capacity (a pool entry's whole
// capacity, new_cap in the arena) and the end words of rotpool_place.
__global__ void __launch_bounds__(kPoolBlock)
rotpool_commit(uint8_t *base, uint64_t *__restrict__ img_offs, uint64_t *__restrict__ img_caps, uint32_t n,
               int32_t *__restrict__ status, const uint64_t *__restrict__ hlen, const uint64_t *__restrict__ roff,
               const uint64_t *__restrict__ rk, const uint64_t *__restrict__ rcap,
               const uint64_t *__restrict__ etop, const uint64_t *__restrict__ epool,
               const uint32_t *__restrict__ code, const uint32_t *__restrict__ seed,
               const uint32_t *__restrict__ crc, const unsigned long long *__restrict__ hdr,
               uint32_t *__restrict__ crc_cur, uint64_t *__restrict__ arena, uint64_t *__restrict__ out_offs,
               uint64_t *__restrict__ out_caps, uint32_t *__restrict__ out_img, uint64_t *__restrict__ out_count,
               uint64_t *__restrict__ pool)
{
    const uint64_t i = (uint64_t) blockIdx.x * kPoolBlock + threadIdx.x;
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
            img_caps[i] = rcap[i];
        }
    }
    if (!bad && (c & (kRotEndAt | kRotEndLast))) {
        out_count[0] = (c & kRotAccepted) ? rk[i] + 1 : rk[i];
        if (c & kRotPoolTop) {
            arena[0] = etop[i];
        }
        if (c & kRotPoolPop) {
            pool[kPoolCount] = epool[i];
        }
    }
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
    uint64_t *pool_offs, *pool_caps, *pool, *total;
    int32_t *status;
};

// The argument checks, before any device call.  Returns 1 when the call is a
// no-op (an empty batch), 0 to go on, CIO_ERROR.
int check_release(const RelArgs &a)
{
    if (a.flags & ~(CIOA_RELEASE_ZERO | CIOA_RELEASE_COMPACT)) {
        return fail("cio_file_release_batch_dev: unknown flags");
    }
    if ((a.flags & CIOA_RELEASE_COMPACT) && !a.count) {
        return fail("cio_file_release_batch_dev: CIOA_RELEASE_COMPACT needs dev_count");
    }
    if ((a.flags & CIOA_RELEASE_COMPACT) && a.live) {
        return fail("cio_file_release_batch_dev: CIOA_RELEASE_COMPACT does not go with dev_live_offs");
    }
    if (!a.w) {
        return fail("cio_file_release_batch_dev: null writer");
    }
    if (a.n == 0) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.pool_offs || !a.pool_caps || !a.pool || !a.total || !a.status) {
        return fail("cio_file_release_batch_dev: null pointer");
    }
    if (a.n > a.w->max_chunks) {
        return fail("cio_file_release_batch_dev: more entries than the writer was created for");
    }
    return 0;
}

int launch_release(const RelArgs &a, hipStream_t s)
{
    cio_dev_writer *w = a.w;
    uint8_t *base = reinterpret_cast<uint8_t *>(a.dev_base);
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kPoolBlock);
    const int compact = (a.flags & CIOA_RELEASE_COMPACT) != 0;
    const bool zero = (a.flags & CIOA_RELEASE_ZERO) != 0;
    // writer arenas: newlen the entry's code, groom its ordinal, dst its pool index, roff / rlen the fill's
    // regions, goffs / glens / gimg the compacted list
    hipLaunchKernelGGL(release_headers, dim3(nb), dim3(kPoolBlock), 0, s, base, a.dev_bytes, a.offs, a.caps, n,
                       a.count, a.gate, a.live, a.pool, a.status, w->groom, w->newlen, w->rtot);
    hipLaunchKernelGGL(release_scan, dim3(1), dim3(kPoolBlock), 0, s, w->rtot, nb, n, a.count, a.pool, a.total);
    hipLaunchKernelGGL(release_place, dim3(nb), dim3(kPoolBlock), 0, s, n, w->rtot, a.count, a.pool, a.offs, a.caps,
                       a.img, a.status, w->groom, w->newlen, w->dst, w->roff, w->rlen, compact, a.total, w->goffs,
                       w->glens, w->gimg);
    HIP_TRY(hipGetLastError(), "release: placement kernels launch");
    if (zero && (devplan_launch_planner(w->dp, a.dev_bytes, w->roff, w->rlen, a.n, nullptr, s) != CIO_OK ||
                 launch_zero_fill(w, a.dev_base, w->roff, w->rlen, a.n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(release_commit, dim3(nb), dim3(kPoolBlock), 0, s, base, a.offs, a.caps, a.img, n, a.count,
                       a.status, w->newlen, w->dst, w->roff, w->rlen,
                       zero ? w->dp->hdr : (const unsigned long long *) nullptr, compact, w->goffs, w->glens, w->gimg,
                       a.pool_offs, a.pool_caps, a.pool, a.total);
    HIP_TRY(hipGetLastError(), "release: commit kernel launch");
    return CIO_OK;
}

int launch_rotate_pool(const RotArgs &a, bool records, uint64_t *pool_offs, uint64_t *pool_caps, uint64_t *pool,
                       hipStream_t s)
{
    cio_dev_writer *w = a.w;
    uint8_t *base = reinterpret_cast<uint8_t *>(a.dev_base);
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kPoolBlock);
    const bool checksum = (a.flags & CIO_CHECKSUM) != 0;
    if (rotate_launch_front(a, records, s) != CIO_OK) {
        return CIO_ERROR;
    }
    // writer arenas beside rotate's: goffs the fresh image's capacity, gneed / glens the ending entry's top and
    // pool count (the records variant's sums in gneed are consumed by rotate_headers)
    hipLaunchKernelGGL(rotpool_place, dim3(nb), dim3(kPoolBlock), 0, s, n, w->rtot, a.arena, a.out_count, pool_offs,
                       pool_caps, pool, a.dev_bytes, a.new_cap, a.align, a.offs, a.status, w->gcap, w->groom,
                       w->soff, w->slen, w->dst, w->roff, w->rlen, w->goffs, w->gneed, w->glens, w->newlen, a.total);
    HIP_TRY(hipGetLastError(), "rotate from the pool: placement kernel launch");
    if (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK ||
        launch_copy(w, a.dev_base, a.dev_base, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum && devplan_crc_launch(w->dp->p, w->dp->hdr, a.dev_base, w->seed, w->crc, a.n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(rotpool_commit, dim3(nb), dim3(kPoolBlock), 0, s, base, a.offs, a.caps, n, a.status, w->gcap,
                       w->roff, w->rlen, w->goffs, w->gneed, w->glens, w->newlen, w->seed,
                       checksum ? w->crc : (const uint32_t *) nullptr, w->dp->hdr, a.crc_cur, a.arena, a.out_offs,
                       a.out_caps, a.out_img, a.out_count, pool);
    HIP_TRY(hipGetLastError(), "rotate from the pool: commit kernel launch");
    return CIO_OK;
}

int rotate_pool(const RotArgs &a, bool records, uint64_t *pool_offs, uint64_t *pool_caps, uint64_t *pool,
                void *stream)
{
    const int rc = rotate_check_args(a, records);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    if (!pool_offs || !pool_caps || !pool) {
        return fail_who(a.who, "null pointer");
    }
    return launch_rotate_pool(a, records, pool_offs, pool_caps, pool, reinterpret_cast<hipStream_t>(stream));
}

}  // namespace

extern "C" {

int cio_file_release_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                               uint64_t *dev_offs, uint64_t *dev_caps, uint32_t *dev_img, size_t n,
                               uint64_t *dev_count, const int32_t *dev_gate, const uint64_t *dev_live_offs, int flags,
                               uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                               uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const RelArgs a = {w, dev_base, dev_bytes, dev_offs, dev_caps, dev_img, n, dev_count, dev_gate, dev_live_offs,
                       flags, dev_pool_offs, dev_pool_caps, dev_pool, dev_total, dev_status};
    const int rc = check_release(a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_release(a, reinterpret_cast<hipStream_t>(stream));
}

int cio_file_rotate_pool_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                   const uint64_t *dev_need, uint64_t limit,
                                   uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                   uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                                   uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                   uint64_t *dev_out_count, int flags,
                                   uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream)
{
    const RotArgs a = {"cio_file_rotate_pool_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n,
                       dev_need, nullptr, nullptr, 0, limit, new_cap, align, dev_arena, dev_out_offs, dev_out_caps,
                       dev_out_img, dev_out_count, flags, dev_crc_cur, dev_total, dev_status};
    return rotate_pool(a, false, dev_pool_offs, dev_pool_caps, dev_pool, stream);
}

int cio_file_rotate_pool_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                           uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                           const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                           uint64_t limit,
                                           uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                           uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                                           uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                           uint64_t *dev_out_count, int flags,
                                           uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status,
                                           void *stream)
{
    const RotArgs a = {"cio_file_rotate_pool_records_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps,
                       n, nullptr, dev_rec_img, dev_rec_lens, n_rec, limit, new_cap, align, dev_arena, dev_out_offs,
                       dev_out_caps, dev_out_img, dev_out_count, flags, dev_crc_cur, dev_total, dev_status};
    return rotate_pool(a, true, dev_pool_offs, dev_pool_caps, dev_pool, stream);
}

}  // extern "C"
