// tx_dev_gpu.hip -- transactions on chunk images in HBM: begin, roll back,
// commit, and the per-image condition of an all-or-nothing append, for CDNA4
// (gfx950, MI355X).  C ABI in include/chunkio_amd/cio_write_dev_tx.h;
// DESIGN.md §20.
//
//   tx_begin             one thread per image: one 16-byte state access and,
//                        for an entry that is not active, one header read
//   tx_rollback          the rollback without CIOA_TX_ZERO / CIOA_TX_RECOMPUTE,
//                        whole: one thread per image decides and writes
//   tx_commit            one thread per image: the image check, the seal's
//                        bytes 2..9, active = 0
//
// With CIOA_TX_ZERO or CIOA_TX_RECOMPUTE a rollback is a serial chain on the
// caller's stream:
//
//   tx_rollback_headers  one thread per image: the verdict and, into the
//                        writer's arenas, the dropped range and the CRC region
//                        [22, 24 + meta + tx.content_len), both zero-length for
//                        every entry that is not rolled back
//   planner + fill       with CIOA_TX_ZERO: devplan's four kernels over the
//                        dropped ranges, then grow's byte-balanced zero fill
//   planner + CRC        with CIOA_TX_RECOMPUTE: the same over the CRC regions,
//                        then the device-planned stream kernel seeded with
//                        crc_init(), output in writer scratch
//   tx_rollback_commit   one thread per image: the planner's status, the
//                        header bytes, crc_cur, the state
//
// The condition (no writer, no scratch: dev_cond itself carries everything):
//
//   tx_cond_clear        one thread per image: CIO_OK, or the image's own
//                        status folded in
//   tx_cond_records      one thread per record: a failing record publishes
//                        CIO_ERROR with atomicMin, unless the previous lane
//                        holds a failing record of the same image (one
//                        __shfl_up; no LDS, no barrier, every lane reaches the
//                        shuffle); an index outside the batch publishes a
//                        marker below CIO_ERROR in dev_cond[0]
//   tx_cond_apply        one thread per image 1 ..: the marker makes it
//   tx_cond_last         CIO_ERROR; then ONE thread turns the marker itself
//                        into CIO_ERROR (a kernel of its own: the other
//                        workgroups of tx_cond_apply still read the word)
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another.  The planner's own checks cannot fire: every region lies inside
// an image tx_rollback_headers found inside dev_bytes.
//
// The per-thread text is tx_dev.h, which tools/tx_check.cpp runs on the host.
// Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "tx_dev.h"
#include "chunkio_amd/cio_write_dev_tx.h"

using namespace cioa;

static_assert(sizeof(cio_dev_tx_state) == sizeof(TxState) && sizeof(TxState) == 16, "the state entry is 16 bytes");
static_assert(kTxOk == CIO_OK && kTxError == CIO_ERROR && kTxChecksum == CIO_CHECKSUM &&
                  kTxRecompute == CIOA_TX_RECOMPUTE && kTxZero == CIOA_TX_ZERO,
              "tx_dev.h restates the public constants");

namespace {

__global__ void __launch_bounds__(kTxBlock)
tx_begin(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
         const uint64_t *__restrict__ img_caps, uint32_t n, const uint32_t *__restrict__ crc_cur, TxState *tx,
         int32_t *__restrict__ status)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    status[i] = tx_begin_one(base, dev_bytes, img_offs, img_caps, i, crc_cur, tx);
}

__global__ void __launch_bounds__(kTxBlock)
tx_rollback(uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
            const uint64_t *__restrict__ img_caps, uint32_t n, const int32_t *__restrict__ cond, int flags,
            uint32_t *__restrict__ crc_cur, TxState *tx, int32_t *__restrict__ status)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    status[i] = tx_rollback_one(base, dev_bytes, img_offs, img_caps, i, cond, flags, crc_cur, tx);
}

__global__ void __launch_bounds__(kTxBlock)
tx_rollback_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
                    const uint64_t *__restrict__ img_caps, uint32_t n, const int32_t *__restrict__ cond, int flags,
                    const TxState *tx, int32_t *__restrict__ status, uint32_t *__restrict__ code,
                    uint64_t *__restrict__ zoff, uint64_t *__restrict__ zlen, uint64_t *__restrict__ coff,
                    uint64_t *__restrict__ clen)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    status[i] = tx_rollback_regions(base, dev_bytes, img_offs, img_caps, i, cond, flags, tx, code, zoff, zlen, coff,
                                    clen);
}

// hdr: the last planner's header.  With CIOA_TX_RECOMPUTE that is the CRC's,
// and every rolled-back entry has a region in it; with CIOA_TX_ZERO alone the
// fill's, and an entry that drops nothing does not depend on it.
__global__ void __launch_bounds__(kTxBlock)
tx_rollback_commit(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n, int flags,
                   const uint32_t *__restrict__ code, const uint64_t *__restrict__ zlen,
                   const uint32_t *__restrict__ crc, const unsigned long long *__restrict__ hdr,
                   uint32_t *__restrict__ crc_cur, TxState *tx, int32_t *__restrict__ status)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i >= n || code[i] != kTxRoll) {
        return;
    }
    const bool bad = hdr[kDevHdrStatus] != 0 && (crc != nullptr || zlen[i] != 0);
    status[i] = tx_rollback_finish(base, img_offs, i, flags, bad, crc, crc_cur, tx);
}

__global__ void __launch_bounds__(kTxBlock)
tx_commit(uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
          const uint64_t *__restrict__ img_caps, uint32_t n, const int32_t *__restrict__ cond, int flags,
          const uint32_t *__restrict__ crc_cur, TxState *tx, int32_t *__restrict__ status)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    status[i] = tx_commit_one(base, dev_bytes, img_offs, img_caps, i, cond, flags, crc_cur, tx);
}

__global__ void __launch_bounds__(kTxBlock)
tx_cond_clear(const int32_t *__restrict__ img_status, uint32_t n_img, int32_t *__restrict__ cond)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    if (i < n_img) {
        cond[i] = tx_cond_clear_one(img_status, i);
    }
}

// Every lane of every wave takes part in the shuffle: a lane without a failing
// record holds the key kTxNoImage and never issues.
__global__ void __launch_bounds__(kTxBlock)
tx_cond_records(const uint32_t *__restrict__ rec_img, const int32_t *__restrict__ rec_status, uint32_t n_rec,
                uint32_t n_img, int32_t *cond)
{
    const uint64_t r = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x;
    const uint32_t lane = threadIdx.x & (kTxLanes - 1);
    bool malformed;
    const uint32_t key = tx_cond_key(rec_img, rec_status, r, n_rec, n_img, malformed);
    const uint32_t prev = (uint32_t) __shfl_up((int) key, 1);
    if (tx_cond_issues(lane, key, prev)) {
        atomicMin(cond + key, kTxError);
    }
    if (malformed) {
        atomicMin(cond, kTxMalformed);            // the whole batch fails
    }
}

__global__ void __launch_bounds__(kTxBlock)
tx_cond_apply(uint32_t n_img, int32_t *cond)
{
    const uint64_t i = (uint64_t) blockIdx.x * kTxBlock + threadIdx.x + 1;
    if (i < n_img) {
        cond[i] = tx_cond_apply_one(cond[i], cond[0]);
    }
}

__global__ void __launch_bounds__(kTxLanes)
tx_cond_last(int32_t *cond)
{
    if (threadIdx.x == 0) {
        cond[0] = tx_cond_apply_one(cond[0], cond[0]);
    }
}

struct TxArgs {
    const char *who;
    cio_dev_writer *w;
    void *dev_base;
    uint64_t dev_bytes;
    const uint64_t *offs, *caps;
    size_t n;
    int flags, allowed;
    const uint32_t *crc_cur;
    cio_dev_tx_state *tx;
    int32_t *status;
};

// The argument checks, before any device call.  Returns 1 when the call is a
// no-op (an empty batch), 0 to go on, CIO_ERROR.
int check_tx(const TxArgs &a)
{
    if (a.flags & ~a.allowed) {
        return fail_who(a.who, "unknown flags");
    }
    if ((a.flags & CIOA_TX_RECOMPUTE) && !(a.flags & CIO_CHECKSUM)) {
        return fail_who(a.who, "CIOA_TX_RECOMPUTE needs CIO_CHECKSUM");
    }
    if (!a.w) {
        return fail_who(a.who, "null writer");
    }
    if (a.n == 0) {
        return 1;
    }
    if (!a.dev_base || !a.offs || !a.caps || !a.tx || !a.status || ((a.flags & CIO_CHECKSUM) && !a.crc_cur)) {
        return fail_who(a.who, "null pointer");
    }
    if (reinterpret_cast<uintptr_t>(a.tx) & 15u) {
        return fail_who(a.who, "dev_tx must be 16-byte aligned");
    }
    if (a.n > a.w->max_chunks) {
        return fail_who(a.who, "more images than the writer was created for");
    }
    return 0;
}

int launch_rollback(const TxArgs &a, const int32_t *cond, uint32_t *crc_cur, hipStream_t s)
{
    cio_dev_writer *w = a.w;
    uint8_t *base = reinterpret_cast<uint8_t *>(a.dev_base);
    TxState *tx = reinterpret_cast<TxState *>(a.tx);
    const uint32_t n = (uint32_t) a.n, nb = blocks_of(a.n, kTxBlock);
    if (!(a.flags & (CIOA_TX_ZERO | CIOA_TX_RECOMPUTE))) {
        hipLaunchKernelGGL(tx_rollback, dim3(nb), dim3(kTxBlock), 0, s, base, a.dev_bytes, a.offs, a.caps, n, cond,
                           a.flags, crc_cur, tx, a.status);
        HIP_TRY(hipGetLastError(), "tx rollback: kernel launch");
        return CIO_OK;
    }
    const bool recompute = (a.flags & CIOA_TX_RECOMPUTE) != 0;
    // writer arenas: newlen the verdict, roff / rlen the dropped range, soff / slen the CRC region
    hipLaunchKernelGGL(tx_rollback_headers, dim3(nb), dim3(kTxBlock), 0, s, base, a.dev_bytes, a.offs, a.caps, n, cond,
                       a.flags, tx, a.status, w->newlen, w->roff, w->rlen, w->soff, w->slen);
    HIP_TRY(hipGetLastError(), "tx rollback: header kernel launch");
    if ((a.flags & CIOA_TX_ZERO) &&
        (devplan_launch_planner(w->dp, a.dev_bytes, w->roff, w->rlen, a.n, nullptr, s) != CIO_OK ||
         launch_zero_fill(w, a.dev_base, w->roff, w->rlen, a.n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    if (recompute &&
        (devplan_launch_planner(w->dp, a.dev_bytes, w->soff, w->slen, a.n, nullptr, s) != CIO_OK ||
         devplan_crc_launch(w->dp->p, w->dp->hdr, a.dev_base, nullptr, w->crc, a.n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(tx_rollback_commit, dim3(nb), dim3(kTxBlock), 0, s, base, a.offs, n, a.flags, w->newlen,
                       w->rlen, recompute ? w->crc : (const uint32_t *) nullptr, w->dp->hdr, crc_cur, tx, a.status);
    HIP_TRY(hipGetLastError(), "tx rollback: commit kernel launch");
    return CIO_OK;
}

}  // namespace

extern "C" {

int cio_file_tx_begin_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n, int flags,
                                const uint32_t *dev_crc_cur, cio_dev_tx_state *dev_tx, int32_t *dev_status,
                                void *stream)
{
    const TxArgs a = {"cio_file_tx_begin_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, flags,
                      CIO_CHECKSUM, dev_crc_cur, dev_tx, dev_status};
    const int rc = check_tx(a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipLaunchKernelGGL(tx_begin, dim3(blocks_of(n, kTxBlock)), dim3(kTxBlock), 0, reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t *>(dev_base), dev_bytes, dev_img_offs, dev_img_caps,
                       (uint32_t) n, (flags & CIO_CHECKSUM) ? dev_crc_cur : (const uint32_t *) nullptr,
                       reinterpret_cast<TxState *>(dev_tx), dev_status);
    HIP_TRY(hipGetLastError(), "cio_file_tx_begin_batch_dev: kernel launch");
    return CIO_OK;
}

int cio_file_tx_rollback_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                   const int32_t *dev_cond, int flags, uint32_t *dev_crc_cur,
                                   cio_dev_tx_state *dev_tx, int32_t *dev_status, void *stream)
{
    const TxArgs a = {"cio_file_tx_rollback_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, flags,
                      CIO_CHECKSUM | CIOA_TX_RECOMPUTE | CIOA_TX_ZERO, dev_crc_cur, dev_tx, dev_status};
    const int rc = check_tx(a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_rollback(a, dev_cond, dev_crc_cur, reinterpret_cast<hipStream_t>(stream));
}

int cio_file_tx_commit_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                 const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                 const int32_t *dev_cond, int flags, uint32_t *dev_crc_cur,
                                 cio_dev_tx_state *dev_tx, int32_t *dev_status, void *stream)
{
    const TxArgs a = {"cio_file_tx_commit_batch_dev", w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, flags,
                      CIO_CHECKSUM, dev_crc_cur, dev_tx, dev_status};
    const int rc = check_tx(a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipLaunchKernelGGL(tx_commit, dim3(blocks_of(n, kTxBlock)), dim3(kTxBlock), 0,
                       reinterpret_cast<hipStream_t>(stream), reinterpret_cast<uint8_t *>(dev_base), dev_bytes,
                       dev_img_offs, dev_img_caps, (uint32_t) n, dev_cond, flags, dev_crc_cur,
                       reinterpret_cast<TxState *>(dev_tx), dev_status);
    HIP_TRY(hipGetLastError(), "cio_file_tx_commit_batch_dev: kernel launch");
    return CIO_OK;
}

int cio_file_tx_cond_records_batch_dev(const uint32_t *dev_rec_img, const int32_t *dev_rec_status, size_t n_rec,
                                       const int32_t *dev_img_status, size_t n_img, int32_t *dev_cond, void *stream)
{
    static const char who[] = "cio_file_tx_cond_records_batch_dev";
    if (n_img == 0) {
        return CIO_OK;
    }
    if (!dev_cond || (n_rec != 0 && (!dev_rec_img || !dev_rec_status))) {
        return fail_who(who, "null pointer");
    }
    if (n_img >= 0xffffffffull || n_rec >= 0xffffffffull) {
        return fail_who(who, "more than 2^32 - 2 images or records");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(tx_cond_clear, dim3(blocks_of(n_img, kTxBlock)), dim3(kTxBlock), 0, s, dev_img_status,
                       (uint32_t) n_img, dev_cond);
    if (n_rec != 0) {
        hipLaunchKernelGGL(tx_cond_records, dim3(blocks_of(n_rec, kTxBlock)), dim3(kTxBlock), 0, s, dev_rec_img,
                           dev_rec_status, (uint32_t) n_rec, (uint32_t) n_img, dev_cond);
        if (n_img > 1) {
            hipLaunchKernelGGL(tx_cond_apply, dim3(blocks_of(n_img - 1, kTxBlock)), dim3(kTxBlock), 0, s,
                               (uint32_t) n_img, dev_cond);
        }
        hipLaunchKernelGGL(tx_cond_last, dim3(1), dim3(kTxLanes), 0, s, dev_cond);
    }
    HIP_TRY(hipGetLastError(), "cio_file_tx_cond_records_batch_dev: kernel launch");
    return CIO_OK;
}

}  // extern "C"
