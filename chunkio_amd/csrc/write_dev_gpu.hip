// write_dev_gpu.hip -- chunkio's write lifecycle for chunk images in HBM, for
// CDNA4 (gfx950, MI355X): initialise, append, seal, and -- on what is already
// in an image -- replace the metadata and write_at.  C ABI in
// include/chunkio_amd/cio_write_dev.h and cio_write_dev_move.h; DESIGN.md §14.
//
// An append batch is a serial chain of kernels on the caller's stream:
//
//   write_headers  one thread per image: the checks, and -- into the writer's
//                  arenas -- the record's validated source region, its
//                  destination offset and the new content length.  A rejected
//                  entry gets a zero-length region, so the batch keeps its
//                  indexing and nothing of that entry is copied or CRC'd.
//   planner        devplan's four kernels over the source regions.  They run
//                  for the CRC anyway; desc[i].g / nsteps is the exclusive
//                  scan of the records' 4 KiB steps, which is exactly the
//                  byte-balanced partition the copy needs, so the copy reads
//                  it instead of running a scan of its own.
//   append_copy    the hot path: every wave takes an even share of the S
//                  steps, whatever records they belong to.
//   CRC            the device-planned stream kernel over the SOURCE records,
//                  seeds = crc_cur, output in writer scratch (not in place).
//   write_finish   one thread per image: crc_cur, bytes 2..9, bytes 10..13.
//
// Init is the same chain over the metadata records (seed = the CRC state after
// the two length bytes, computed per thread); seal with CIOA_SEAL_RECOMPUTE is
// verify-on-load's chain (header kernel, planner + CRC over the image regions)
// with a finish kernel that stores instead of comparing.
//
// Replacing the metadata (cio_file_write_metadata_batch_dev) shifts the content
// of every image onto itself by new - old metadata length:
//
//   meta_headers   the checks; the move's regions (old content, delta), the
//                  metadata records as an append copy's, the CRC region on the
//                  NEW layout and its seed (the state after the new bytes 22..23)
//   planner        over the move's source regions
//   move_save      } the in-place, overlapping, byte-balanced move:
//   move_shift     } write_dev_move.h
//   planner, append_copy    the metadata records to byte 24 (after the shift:
//                  a longer metadata lands on the old content's first bytes)
//   planner, CRC   over [img + 24, + m + content) of the moved image
//   meta_finish    accepted entries only: bytes 22..23, crc_cur
//
// No kernel before meta_finish touches a rejected image: its regions have
// length zero.  write_at (cio_file_write_at_batch_dev) is the seal-recompute
// chain over the kept prefix [img + 22, + 2 + meta + at) into the writer's seed
// arena, then the append chain with the CRC launch seeded from there.
//
// The planner's own checks (a region outside dev_bytes, a region of 2^32
// steps, a batch of 2^40 steps) cannot fire in those chains' region passes:
// every region lies inside an image the header kernel found inside dev_bytes.
//
// The image check and the layout it rests on are image_dev.h.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "write_dev_copy.h"
#include "write_dev_move.h"
#include "read_dev_place.h"
#include "write_dev_records.h"
#include "sort_records.h"
#include "chunkio_amd/cio_write_dev.h"
#include "chunkio_amd/cio_write_dev_move.h"

using namespace cioa;

namespace {

constexpr uint32_t kCopyThreads = 256;                 // 4 waves per workgroup
constexpr uint32_t kCopyWaves = kCopyThreads / kWave;
constexpr uint32_t kCopyWgPerCu = 8;                   // 32 waves per CU in flight
constexpr uint64_t kMaxContent = 0xffffffffull;        // the length field is 32 bits
constexpr uint32_t kMoveWgPerCu = 4;                   // 32 waves per CU, 128 KiB of loads in flight

// crc_update over one byte, bit by bit (raw state, reflected polynomial).
__device__ __forceinline__ uint32_t crc_byte(uint32_t crc, uint32_t b)
{
    crc ^= b;
    for (int k = 0; k < 8; ++k) {
        crc = (crc >> 1) ^ (CIOA_POLY & (0u - (crc & 1u)));
    }
    return crc;
}

// ---------------------------------------------------------------- init

__global__ void __launch_bounds__(256)
init_headers(uint64_t dev_bytes, const uint64_t *__restrict__ img_offs, const uint64_t *__restrict__ img_caps,
             uint32_t n, const uint64_t *__restrict__ meta_offs, const uint64_t *__restrict__ meta_lens,
             uint64_t meta_src_bytes, int32_t *__restrict__ status, uint64_t *__restrict__ soff,
             uint64_t *__restrict__ slen, uint64_t *__restrict__ dst, uint32_t *__restrict__ seed)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t off = img_offs[i], cap = img_caps[i];
    const uint64_t moff = meta_offs ? meta_offs[i] : 0, m = meta_lens ? meta_lens[i] : 0;
    bool ok = range_ok(off, cap, dev_bytes) && cap >= kReadHdr;
    if (ok && m != 0) {
        ok = m <= 65535u && kReadHdr + m <= cap && range_ok(moff, m, meta_src_bytes);
    }
    status[i] = ok ? CIO_OK : CIO_ERROR;
    soff[i] = ok && m ? moff : 0;
    slen[i] = ok ? m : 0;
    dst[i] = ok ? off + kReadHdr : 0;
    // crc_update(crc_init(), bytes 22..23): 0xBE26ED00 without metadata
    seed[i] = crc_byte(crc_byte(0xffffffffu, (uint32_t) (m >> 8) & 0xffu), (uint32_t) m & 0xffu);
}

// crc: the CRC launch's output over the metadata, or NULL when there was none
// (then the seed is already the state); hdr: the planner's header, or NULL
// when no planner ran.
__global__ void __launch_bounds__(256)
init_finish(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n, int32_t *__restrict__ status,
            const uint64_t *__restrict__ slen, const uint32_t *__restrict__ seed, const uint32_t *__restrict__ crc,
            const unsigned long long *__restrict__ hdr, int checksum, uint32_t *__restrict__ crc_cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK) {
        return;
    }
    if (hdr && hdr[kDevHdrStatus] != 0) {
        status[i] = CIO_ERROR;                // the planner published an empty batch: nothing was copied
        return;
    }
    uint8_t *p = base + img_offs[i];
    const uint32_t m = (uint32_t) slen[i];
    p[0] = 0xc1;
    p[1] = 0x00;
    p[2] = checksum ? 0xff : 0;
    p[3] = checksum ? 0x12 : 0;
    p[4] = checksum ? 0xd9 : 0;
    p[5] = checksum ? 0x41 : 0;
    for (uint32_t k = 6; k < 22; ++k) {
        p[k] = 0;
    }
    p[22] = (uint8_t) (m >> 8);
    p[23] = (uint8_t) m;
    if (checksum) {
        crc_cur[i] = crc ? crc[i] : seed[i];
    }
}

// ---------------------------------------------------------------- write

__global__ void __launch_bounds__(256)
write_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
              const uint64_t *__restrict__ img_caps, uint32_t n, const uint64_t *__restrict__ src_offs,
              const uint64_t *__restrict__ src_lens, uint64_t src_bytes, int32_t *__restrict__ status,
              uint64_t *__restrict__ soff, uint64_t *__restrict__ slen, uint64_t *__restrict__ dst,
              uint32_t *__restrict__ newlen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t count = src_lens[i];
    int32_t st = CIO_OK;
    uint64_t so = 0, sl = 0, d = 0;
    uint32_t nl = 0;
    if (count != 0) {                         // cio_file_write: count == 0 does nothing
        const uint64_t off = img_offs[i], cap = img_caps[i], s = src_offs[i];
        uint32_t meta = 0;
        uint64_t content = 0;
        if (image_ok(base, dev_bytes, off, cap, meta, content) && count <= kMaxContent &&
            content + count <= kMaxContent && kReadHdr + meta + content + count <= cap &&
            range_ok(s, count, src_bytes)) {
            so = s;
            sl = count;
            d = off + kReadHdr + meta + content;
            nl = (uint32_t) (content + count);
        } else {
            st = CIO_ERROR;
        }
    }
    status[i] = st;
    soff[i] = so;
    slen[i] = sl;
    dst[i] = d;
    newlen[i] = nl;
}

__global__ void __launch_bounds__(256)
write_finish(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n, int32_t *__restrict__ status,
             const uint64_t *__restrict__ slen, const uint32_t *__restrict__ newlen,
             const uint32_t *__restrict__ crc, const unsigned long long *__restrict__ hdr, int checksum,
             uint32_t *__restrict__ crc_cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK || slen[i] == 0) {
        return;
    }
    if (hdr[kDevHdrStatus] != 0) {
        status[i] = CIO_ERROR;                // the planner published an empty batch: nothing was copied
        return;
    }
    uint8_t *p = base + img_offs[i];
    if (checksum) {
        const uint32_t c = crc[i];
        crc_cur[i] = c;
        p[2] = (uint8_t) c;                   // raw state in an 8-byte crc_t, host byte order
        p[3] = (uint8_t) (c >> 8);
        p[4] = (uint8_t) (c >> 16);
        p[5] = (uint8_t) (c >> 24);
        p[6] = p[7] = p[8] = p[9] = 0;
    }
    put_be32(p + 10, newlen[i]);
}

// ---------------------------------------------------------------- seal

// Validates; with CIOA_SEAL_RECOMPUTE (soff, slen not NULL) the emitted CRC
// region is [img + 22, + 2 + meta + content), zero-length for a rejected image.
__global__ void __launch_bounds__(256)
seal_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
             const uint64_t *__restrict__ img_caps, uint32_t n, int32_t *__restrict__ status,
             uint64_t *__restrict__ soff, uint64_t *__restrict__ slen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t off = img_offs[i];
    uint32_t meta = 0;
    uint64_t content = 0;
    const bool ok = image_ok(base, dev_bytes, off, img_caps[i], meta, content);
    status[i] = ok ? CIO_OK : CIO_ERROR;
    if (soff) {
        soff[i] = ok ? off + 22 : 0;
        slen[i] = ok ? 2ull + meta + content : 0;
    }
}

// crc / hdr: the recomputed states and the planner's header, or NULL.
__global__ void __launch_bounds__(256)
seal_finish(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n, int32_t *__restrict__ status,
            const uint32_t *__restrict__ crc, const unsigned long long *__restrict__ hdr,
            uint32_t *__restrict__ crc_cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK) {
        return;
    }
    if (hdr && hdr[kDevHdrStatus] != 0) {
        status[i] = CIO_ERROR;
        return;
    }
    uint32_t c = crc_cur[i];
    if (crc) {
        c = crc[i];
        crc_cur[i] = c;
    }
    uint8_t *p = base + img_offs[i];
    put_be32(p + 2, c ^ 0xffffffffu);         // htonl(crc_finalize) in an 8-byte crc_t
    p[6] = p[7] = p[8] = p[9] = 0;
}

// ---------------------------------------------------------------- the append copy
// (record_of, copy_units, copy_wave and copy_tiny: write_dev_copy.h)

// Record i: slen[i] bytes from src_base + soff[i] to dst_base + dst[i].  The
// planner's image of the source regions gives the balance: S steps in all,
// record i holding steps [desc[i].g, + desc[i].nsteps).  Wave w of the grid
// takes steps [w S / W, (w + 1) S / W), so one 4 MiB record among thousands of
// 4 KiB ones spreads over as many waves as its bytes call for.  Records of
// fewer than 4 bytes have no step (the CRC kernel's tiny list); they are
// copied bytewise up front.
__global__ void __launch_bounds__(kCopyThreads)
append_copy(uint8_t *dst_base, const uint8_t *src_base, const ChunkDesc *__restrict__ desc,
            const uint64_t *__restrict__ soff, const uint64_t *__restrict__ slen,
            const uint64_t *__restrict__ dst, const unsigned long long *__restrict__ hdr, uint32_t n)
{
    if (hdr[kDevHdrStatus] != 0) {
        return;
    }
    const uint64_t gtid = (uint64_t) blockIdx.x * kCopyThreads + threadIdx.x;
    const uint64_t nthreads = (uint64_t) gridDim.x * kCopyThreads;
    if (hdr[kDevHdrNtiny] != 0) {
        copy_tiny(dst_base, src_base, soff, slen, dst, n, gtid, nthreads);
    }
    const uint64_t w = __builtin_amdgcn_readfirstlane((uint32_t) (gtid / kWave));
    copy_wave(dst_base, src_base, desc, soff, slen, dst, n, hdr[kDevHdrS], (uint64_t) gridDim.x * kCopyWaves, w,
              threadIdx.x & (kWave - 1));
}

// ---------------------------------------------------------------- write_at

// As write_headers, with the content cut to at[i] first; also the CRC region
// of the kept prefix, [img + 22, + 2 + meta + at), zero-length for an entry
// that is rejected or has no record.
__global__ void __launch_bounds__(256)
write_at_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
                 const uint64_t *__restrict__ img_caps, uint32_t n, const uint64_t *__restrict__ at_offs,
                 const uint64_t *__restrict__ src_offs, const uint64_t *__restrict__ src_lens, uint64_t src_bytes,
                 int32_t *__restrict__ status, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen,
                 uint64_t *__restrict__ dst, uint32_t *__restrict__ newlen, uint64_t *__restrict__ roff,
                 uint64_t *__restrict__ rlen)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t count = src_lens[i];
    int32_t st = CIO_OK;
    uint64_t so = 0, sl = 0, d = 0, ro = 0, rl = 0;
    uint32_t nl = 0;
    if (count != 0) {
        const uint64_t off = img_offs[i], cap = img_caps[i], s = src_offs[i], at = at_offs[i];
        uint32_t meta = 0;
        uint64_t content = 0;
        if (image_ok(base, dev_bytes, off, cap, meta, content) && at <= content && count <= kMaxContent &&
            at + count <= kMaxContent && kReadHdr + meta + at + count <= cap &&
            range_ok(s, count, src_bytes)) {
            so = s;
            sl = count;
            d = off + kReadHdr + meta + at;
            nl = (uint32_t) (at + count);
            ro = off + 22;
            rl = 2ull + meta + at;
        } else {
            st = CIO_ERROR;
        }
    }
    status[i] = st;
    soff[i] = so;
    slen[i] = sl;
    dst[i] = d;
    newlen[i] = nl;
    roff[i] = ro;
    rlen[i] = rl;
}

// ---------------------------------------------------------------- write_metadata

__global__ void __launch_bounds__(256)
meta_headers(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
             const uint64_t *__restrict__ img_caps, uint32_t n, const uint64_t *__restrict__ meta_offs,
             const uint64_t *__restrict__ meta_lens, uint64_t meta_src_bytes, int32_t *__restrict__ status,
             uint64_t *__restrict__ soff, uint64_t *__restrict__ slen, uint64_t *__restrict__ dst,
             uint64_t *__restrict__ msrc, uint64_t *__restrict__ mlen, int64_t *__restrict__ mdelta,
             uint64_t *__restrict__ roff, uint64_t *__restrict__ rlen, uint32_t *__restrict__ seed)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t off = img_offs[i], cap = img_caps[i], moff = meta_offs[i], m = meta_lens[i];
    uint32_t old = 0;
    uint64_t content = 0;
    const bool ok = image_ok(base, dev_bytes, off, cap, old, content) && m <= 65535u &&
                    kReadHdr + m + content <= cap && range_ok(moff, m, meta_src_bytes);
    const int64_t delta = ok ? (int64_t) m - (int64_t) old : 0;
    status[i] = ok ? CIO_OK : CIO_ERROR;
    soff[i] = ok && m ? moff : 0;
    slen[i] = ok ? m : 0;
    dst[i] = ok ? off + kReadHdr : 0;
    msrc[i] = ok ? off + kReadHdr + old : 0;
    mlen[i] = delta != 0 ? content : 0;       // m == old: the metadata is rewritten in place, nothing moves
    mdelta[i] = delta;
    roff[i] = ok ? off + kReadHdr : 0;
    rlen[i] = ok ? m + content : 0;
    seed[i] = crc_byte(crc_byte(0xffffffffu, (uint32_t) (m >> 8) & 0xffu), (uint32_t) m & 0xffu);
}

// crc: the CRC launch's output, or NULL without CIO_CHECKSUM; hdr: the last
// planner's header; the new metadata length is slen[i].
__global__ void __launch_bounds__(256)
meta_finish(uint8_t *base, const uint64_t *__restrict__ img_offs, uint32_t n, int32_t *__restrict__ status,
            const uint64_t *__restrict__ slen, const uint32_t *__restrict__ crc,
            const unsigned long long *__restrict__ hdr, uint32_t *__restrict__ crc_cur)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK) {
        return;
    }
    if (hdr[kDevHdrStatus] != 0) {
        status[i] = CIO_ERROR;
        return;
    }
    uint8_t *p = base + img_offs[i];
    const uint32_t m = (uint32_t) slen[i];
    p[22] = (uint8_t) (m >> 8);
    p[23] = (uint8_t) m;
    if (crc) {
        crc_cur[i] = crc[i];
    }
}

// ---------------------------------------------------------------- the in-place move
// (move_window, move_range, the tile and move_tiny: write_dev_move.h)

// The save kernel's tiles, dealt to the workgroup's waves in turn: nothing it
// reads is written in this kernel, so a wave loads and stores at once.
struct SaveTile {
    uint32_t lane, wave, next;
    __device__ __forceinline__ void tile(uint8_t *d, const uint8_t *s, uint64_t len)
    {
        if (next == wave) {
            MoveRegs r;
            tile_load(r, d, s, len, lane);
            tile_store(r, d, len, lane);
        }
        next = next + 1 == kMoveWaves ? 0 : next + 1;
    }
    __device__ __forceinline__ void end() const {}
};

// The shift kernel's tiles, kMoveWaves to a phase, one per wave: every lane of
// the workgroup has its loads in registers before any lane stores.  The walk
// that deals the tiles is the same in every lane, so every lane reaches every
// barrier.  "In registers" means the loads have RETURNED: __syncthreads()
// alone lets plain global loads stay in flight across the barrier on this
// target (the wait for them is placed at their first use, after it), so the
// wait is stated before the barrier.  It costs nothing: the stores need the
// same data.
struct ShiftTile {
    uint32_t lane, wave, pending;
    bool mine;
    uint8_t *d;
    const uint8_t *s;
    uint64_t len;
    __device__ __forceinline__ void tile(uint8_t *d_, const uint8_t *s_, uint64_t len_)
    {
        if (pending == wave) {
            mine = true;
            d = d_;
            s = s_;
            len = len_;
        }
        if (++pending == kMoveWaves) {
            end();
        }
    }
    __device__ __forceinline__ void end()
    {
        if (pending == 0) {
            return;
        }
        MoveRegs r;
        if (mine) {
            tile_load(r, d, s, len, lane);
        }
        __builtin_amdgcn_s_waitcnt(0x0f70);   // vmcnt(0); expcnt and lgkmcnt not waited for
        __syncthreads();
        if (mine) {
            tile_store(r, d, len, lane);
        }
        mine = false;
        pending = 0;
    }
};

// Segment blockIdx.x of gridDim.x: its even share of the S steps, walked window
// by window.  Every condition here is the same in all lanes of the workgroup.
template <bool SAVE, class Ex>
__device__ __forceinline__ void move_segment(uint8_t *base, uint8_t *arena, const ChunkDesc *desc,
                                             const uint64_t *msrc, const uint64_t *mlen, const int64_t *mdelta,
                                             uint32_t n, uint64_t S, Ex &ex)
{
    __shared__ MoveRec win[kMoveWindow];
    uint64_t t = ((uint64_t) blockIdx.x * S) / gridDim.x;
    const uint64_t t1 = (((uint64_t) blockIdx.x + 1) * S) / gridDim.x;
    if (t >= t1) {
        return;
    }
    uint8_t *slots = arena + (uint64_t) blockIdx.x * kMoveSegBytes;
    uint32_t c = record_of(desc, n, t);
    while (t < t1 && c < n) {
        const uint32_t nw = min(kMoveWindow, n - c);
        __syncthreads();                      // nobody reads the window before it is replaced
        if (threadIdx.x < nw) {
            win[threadIdx.x] = move_rec(desc, msrc, mlen, mdelta, c + threadIdx.x);
        }
        __syncthreads();
        move_window<SAVE>(base, slots, win, c, nw, t, t1, c, ex);
    }
    ex.end();                                 // the last phase, if it is not full
}

// One workgroup per segment; arena: gridDim.x * kMoveSegBytes.
__global__ void __launch_bounds__(kMoveThreads)
move_save(uint8_t *base, uint8_t *arena, const ChunkDesc *__restrict__ desc, const uint64_t *__restrict__ msrc,
          const uint64_t *__restrict__ mlen, const int64_t *__restrict__ mdelta,
          const unsigned long long *__restrict__ hdr, uint32_t n)
{
    if (hdr[kDevHdrStatus] != 0) {
        return;
    }
    SaveTile ex = {threadIdx.x & (kWave - 1), (uint32_t) __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), 0};
    move_segment<true>(base, arena, desc, msrc, mlen, mdelta, n, hdr[kDevHdrS], ex);
}

__global__ void __launch_bounds__(kMoveThreads)
move_shift(uint8_t *base, uint8_t *arena, const ChunkDesc *__restrict__ desc, const uint64_t *__restrict__ msrc,
           const uint64_t *__restrict__ mlen, const int64_t *__restrict__ mdelta,
           const unsigned long long *__restrict__ hdr, uint32_t n)
{
    if (hdr[kDevHdrStatus] != 0) {
        return;
    }
    if (hdr[kDevHdrNtiny] != 0) {
        move_tiny(base, msrc, mlen, mdelta, n, (uint64_t) blockIdx.x * kMoveThreads + threadIdx.x,
                  (uint64_t) gridDim.x * kMoveThreads);
    }
    ShiftTile ex = {threadIdx.x & (kWave - 1), (uint32_t) __builtin_amdgcn_readfirstlane(threadIdx.x / kWave), 0,
                    false, nullptr, nullptr, 0};
    move_segment<false>(base, arena, desc, msrc, mlen, mdelta, n, hdr[kDevHdrS], ex);
}

uint32_t blocks256(size_t n)
{
    return (uint32_t) ((n + 255) / 256);
}

}  // namespace

// struct cio_dev_writer: cio_gpu_internal.h (the read path shares it).

int cioa::launch_copy(const cio_dev_writer *w, void *dev_base, const void *dev_src, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(append_copy, dim3(w->copy_grid), dim3(kCopyThreads), 0, s,
                       reinterpret_cast<uint8_t *>(dev_base), reinterpret_cast<const uint8_t *>(dev_src),
                       w->dp->p->desc, w->soff, w->slen, w->dst, w->dp->hdr, (uint32_t) n);
    HIP_TRY(hipGetLastError(), "append_copy launch");
    return CIO_OK;
}

namespace {

// The argument checks every entry point shares, before any device call.
// Returns 1 when the call is a no-op (n == 0), 0 to go on, CIO_ERROR.
int check_args(const char *who, const cio_dev_writer *w, const void *dev_base, const uint64_t *offs,
               const uint64_t *caps, size_t n, int flags, int allowed, const uint32_t *crc_cur,
               const int32_t *status, bool source_ok = true)
{
    if (flags & ~allowed) {
        return fail_who(who, "unknown flags");
    }
    if ((flags & CIOA_SEAL_RECOMPUTE) && !(flags & CIO_CHECKSUM)) {
        return fail_who(who, "CIOA_SEAL_RECOMPUTE needs CIO_CHECKSUM");
    }
    if (!w) {
        return fail_who(who, "null writer");
    }
    if (n == 0) {
        return 1;
    }
    if (!dev_base || !offs || !caps || !status || ((flags & CIO_CHECKSUM) && !crc_cur) || !source_ok) {
        return fail_who(who, "null pointer");
    }
    if (n > w->max_chunks) {
        return fail_who(who, "more images than the writer was created for");
    }
    return 0;
}

int launch_meta_headers(const cio_dev_writer *w, const uint8_t *base, uint64_t dev_bytes, const uint64_t *offs,
                        const uint64_t *caps, size_t n, uint64_t meta_src_bytes, const uint64_t *meta_offs,
                        const uint64_t *meta_lens, int32_t *status, hipStream_t s)
{
    hipLaunchKernelGGL(meta_headers, dim3(blocks256(n)), dim3(256), 0, s, base, dev_bytes, offs, caps, (uint32_t) n,
                       meta_offs, meta_lens, meta_src_bytes, status, w->soff, w->slen, w->dst, w->msrc, w->mlen,
                       w->mdelta, w->roff, w->rlen, w->seed);
    HIP_TRY(hipGetLastError(), "cio_file_write_metadata_batch_dev: header kernel launch");
    return CIO_OK;
}

// move_save and move_shift over the planner's image of (msrc, mlen).
int launch_move(const cio_dev_writer *w, uint8_t *base, size_t n, hipStream_t s)
{
    hipLaunchKernelGGL(move_save, dim3(w->move_grid), dim3(kMoveThreads), 0, s, base, w->arena, w->dp->p->desc,
                       w->msrc, w->mlen, w->mdelta, w->dp->hdr, (uint32_t) n);
    hipLaunchKernelGGL(move_shift, dim3(w->move_grid), dim3(kMoveThreads), 0, s, base, w->arena, w->dp->p->desc,
                       w->msrc, w->mlen, w->mdelta, w->dp->hdr, (uint32_t) n);
    HIP_TRY(hipGetLastError(), "move launch");
    return CIO_OK;
}

}  // namespace

extern "C" {

void cio_dev_writer_destroy(cio_dev_writer *w)
{
    if (!w) {
        return;
    }
    cio_crc32_devplan_destroy(w->dp);
    (void) hipFree(w->soff);
    (void) hipFree(w->slen);
    (void) hipFree(w->dst);
    (void) hipFree(w->newlen);
    (void) hipFree(w->seed);
    (void) hipFree(w->crc);
    (void) hipFree(w->roff);
    (void) hipFree(w->rlen);
    (void) hipFree(w->msrc);
    (void) hipFree(w->mlen);
    (void) hipFree(w->mdelta);
    (void) hipFree(w->arena);
    (void) hipFree(w->rtot);
    (void) hipFree(w->groom);
    (void) hipFree(w->gsum);
    (void) hipFree(w->gflag);
    (void) hipFree(w->ghdr);
    (void) hipFree(w->skey[0]);
    (void) hipFree(w->skey[1]);
    (void) hipFree(w->sidx[0]);
    (void) hipFree(w->sidx[1]);
    (void) hipFree(w->stab);
    (void) hipFree(w->gimg);
    (void) hipFree(w->goffs);
    (void) hipFree(w->glens);
    (void) hipFree(w->gst);
    (void) hipFree(w->gneed);
    (void) hipFree(w->gcap);
    (void) hipFree(w->growhdr);
    delete w;
}

int cio_dev_writer_create(cio_dev_writer **out, size_t max_chunks)
{
    return cio_dev_writer_create_ex(out, max_chunks, 0);
}

uint32_t cio_dev_writer_move_segments(const cio_dev_writer *w)
{
    return w ? w->move_grid : 0;
}

int cio_dev_writer_create_ex(cio_dev_writer **out, size_t max_chunks, int flags)
{
    if (!out) {
        return fail("cio_dev_writer_create: null argument");
    }
    *out = nullptr;
    if (max_chunks == 0 || max_chunks >= 0xffffffffull) {
        return fail("cio_dev_writer_create: max_chunks must be 1 .. 2^32 - 2");
    }
    if (flags & ~CIOA_WRITER_MOVE) {
        return fail("cio_dev_writer_create_ex: unknown flags");
    }
    DeviceState *st;
    if (device_state(&st) != CIO_OK) {
        return CIO_ERROR;
    }
    cio_dev_writer *w = new cio_dev_writer();
    w->max_chunks = (uint32_t) max_chunks;
    w->copy_grid = (uint32_t) st->cus * kCopyWgPerCu;
    if (cio_crc32_devplan_create(&w->dp, max_chunks) != CIO_OK) {
        cio_dev_writer_destroy(w);
        return CIO_ERROR;
    }
    hipError_t e;
    if ((e = hipMalloc(&w->soff, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->slen, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->dst, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->newlen, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->seed, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->crc, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->roff, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->rlen, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->rtot, ((max_chunks + kReadBlock - 1) / kReadBlock) * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->groom, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->gsum, ((max_chunks + kRecBlock - 1) / kRecBlock) * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->gflag, ((max_chunks + kRecBlock - 1) / kRecBlock) * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->ghdr, 2 * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->skey[0], max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->skey[1], max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->sidx[0], max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->sidx[1], max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->stab, (size_t) kSortRadix * sort_blocks(max_chunks) * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->gimg, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&w->goffs, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->glens, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->gst, max_chunks * sizeof(int32_t))) != hipSuccess ||
        (e = hipMalloc(&w->gneed, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->gcap, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&w->growhdr, sizeof(uint32_t))) != hipSuccess) {
        cio_dev_writer_destroy(w);
        return fail("cio_dev_writer_create: device allocation", e);
    }
    if (flags & CIOA_WRITER_MOVE) {
        const uint32_t grid = (uint32_t) st->cus * kMoveWgPerCu;
        if ((e = hipMalloc(&w->msrc, max_chunks * sizeof(uint64_t))) != hipSuccess ||
            (e = hipMalloc(&w->mlen, max_chunks * sizeof(uint64_t))) != hipSuccess ||
            (e = hipMalloc(&w->mdelta, max_chunks * sizeof(int64_t))) != hipSuccess ||
            (e = hipMalloc(&w->arena, (size_t) grid * kMoveSegBytes)) != hipSuccess) {
            cio_dev_writer_destroy(w);
            return fail("cio_dev_writer_create_ex: device allocation", e);
        }
        w->move_grid = grid;
    }
    *out = w;
    return CIO_OK;
}

int cio_file_init_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            const void *dev_meta_src, uint64_t meta_src_bytes,
                            const uint64_t *dev_meta_offs, const uint64_t *dev_meta_lens,
                            int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream)
{
    static const char who[] = "cio_file_init_batch_dev";
    const int rc = check_args(who, w, dev_base, dev_img_offs, dev_img_caps, n, flags, CIO_CHECKSUM, dev_crc_cur,
                              dev_status, !dev_meta_src || (dev_meta_offs && dev_meta_lens));
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const uint32_t nb = blocks256(n);
    const int checksum = (flags & CIO_CHECKSUM) != 0;
    const bool meta = dev_meta_src != nullptr;
    hipLaunchKernelGGL(init_headers, dim3(nb), dim3(256), 0, s, dev_bytes, dev_img_offs, dev_img_caps, (uint32_t) n,
                       meta ? dev_meta_offs : nullptr, meta ? dev_meta_lens : nullptr, meta_src_bytes, dev_status,
                       w->soff, w->slen, w->dst, w->seed);
    HIP_TRY(hipGetLastError(), "cio_file_init_batch_dev: header kernel launch");
    if (meta) {
        if (devplan_launch_planner(w->dp, meta_src_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
            launch_copy(w, dev_base, dev_meta_src, n, s) != CIO_OK) {
            return CIO_ERROR;
        }
        if (checksum && devplan_crc_launch(w->dp->p, w->dp->hdr, dev_meta_src, w->seed, w->crc, n, s) != CIO_OK) {
            return CIO_ERROR;
        }
    }
    hipLaunchKernelGGL(init_finish, dim3(nb), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n, dev_status,
                       w->slen, w->seed, meta && checksum ? w->crc : nullptr, meta ? w->dp->hdr : nullptr, checksum,
                       dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_init_batch_dev: finish kernel launch");
    return CIO_OK;
}

int cio_file_write_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                             const void *dev_src, uint64_t src_bytes,
                             const uint64_t *dev_src_offs, const uint64_t *dev_src_lens,
                             int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream)
{
    static const char who[] = "cio_file_write_batch_dev";
    const int rc = check_args(who, w, dev_base, dev_img_offs, dev_img_caps, n, flags, CIO_CHECKSUM, dev_crc_cur,
                              dev_status, dev_src && dev_src_offs && dev_src_lens);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const uint32_t nb = blocks256(n);
    const int checksum = (flags & CIO_CHECKSUM) != 0;
    hipLaunchKernelGGL(write_headers, dim3(nb), dim3(256), 0, s, base, dev_bytes, dev_img_offs, dev_img_caps,
                       (uint32_t) n, dev_src_offs, dev_src_lens, src_bytes, dev_status, w->soff, w->slen, w->dst,
                       w->newlen);
    HIP_TRY(hipGetLastError(), "cio_file_write_batch_dev: header kernel launch");
    if (devplan_launch_planner(w->dp, src_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
        launch_copy(w, dev_base, dev_src, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum && devplan_crc_launch(w->dp->p, w->dp->hdr, dev_src, dev_crc_cur, w->crc, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(write_finish, dim3(nb), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n, dev_status,
                       w->slen, w->newlen, w->crc, w->dp->hdr, checksum, dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_write_batch_dev: finish kernel launch");
    return CIO_OK;
}

int cio_file_seal_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream)
{
    static const char who[] = "cio_file_seal_batch_dev";
    const int rc = check_args(who, w, dev_base, dev_img_offs, dev_img_caps, n, flags,
                              CIO_CHECKSUM | CIOA_SEAL_RECOMPUTE, dev_crc_cur, dev_status);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const uint32_t nb = blocks256(n);
    const bool recompute = (flags & CIOA_SEAL_RECOMPUTE) != 0;
    hipLaunchKernelGGL(seal_headers, dim3(nb), dim3(256), 0, s, base, dev_bytes, dev_img_offs, dev_img_caps,
                       (uint32_t) n, dev_status, recompute ? w->soff : nullptr, recompute ? w->slen : nullptr);
    HIP_TRY(hipGetLastError(), "cio_file_seal_batch_dev: header kernel launch");
    if (!(flags & CIO_CHECKSUM)) {
        return CIO_OK;
    }
    if (recompute &&
        (devplan_launch_planner(w->dp, dev_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
         devplan_crc_launch(w->dp->p, w->dp->hdr, dev_base, nullptr, w->crc, n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(seal_finish, dim3(nb), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n, dev_status,
                       recompute ? w->crc : nullptr, recompute ? w->dp->hdr : nullptr, dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_seal_batch_dev: finish kernel launch");
    return CIO_OK;
}

int cio_file_write_at_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                const uint64_t *dev_at_offs,
                                const void *dev_src, uint64_t src_bytes,
                                const uint64_t *dev_src_offs, const uint64_t *dev_src_lens,
                                int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream)
{
    static const char who[] = "cio_file_write_at_batch_dev";
    const int rc = check_args(who, w, dev_base, dev_img_offs, dev_img_caps, n, flags, CIO_CHECKSUM, dev_crc_cur,
                              dev_status, dev_at_offs && dev_src && dev_src_offs && dev_src_lens);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const uint32_t nb = blocks256(n);
    const int checksum = (flags & CIO_CHECKSUM) != 0;
    hipLaunchKernelGGL(write_at_headers, dim3(nb), dim3(256), 0, s, base, dev_bytes, dev_img_offs, dev_img_caps,
                       (uint32_t) n, dev_at_offs, dev_src_offs, dev_src_lens, src_bytes, dev_status, w->soff,
                       w->slen, w->dst, w->newlen, w->roff, w->rlen);
    HIP_TRY(hipGetLastError(), "cio_file_write_at_batch_dev: header kernel launch");
    // the crc_reset recompute over the kept prefix, into the seed arena
    if (checksum &&
        (devplan_launch_planner(w->dp, dev_bytes, w->roff, w->rlen, n, nullptr, s) != CIO_OK ||
         devplan_crc_launch(w->dp->p, w->dp->hdr, dev_base, nullptr, w->seed, n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    if (devplan_launch_planner(w->dp, src_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
        launch_copy(w, dev_base, dev_src, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum && devplan_crc_launch(w->dp->p, w->dp->hdr, dev_src, w->seed, w->crc, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(write_finish, dim3(nb), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n, dev_status,
                       w->slen, w->newlen, w->crc, w->dp->hdr, checksum, dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_write_at_batch_dev: finish kernel launch");
    return CIO_OK;
}

int cio_file_write_metadata_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                      const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                      const void *dev_meta_src, uint64_t meta_src_bytes,
                                      const uint64_t *dev_meta_offs, const uint64_t *dev_meta_lens,
                                      int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream)
{
    static const char who[] = "cio_file_write_metadata_batch_dev";
    const int rc = check_args(who, w, dev_base, dev_img_offs, dev_img_caps, n, flags, CIO_CHECKSUM, dev_crc_cur,
                              dev_status, dev_meta_src && dev_meta_offs && dev_meta_lens);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    if (w->move_grid == 0) {
        return fail("cio_file_write_metadata_batch_dev: the writer was created without CIOA_WRITER_MOVE");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    const int checksum = (flags & CIO_CHECKSUM) != 0;
    if (launch_meta_headers(w, base, dev_bytes, dev_img_offs, dev_img_caps, n, meta_src_bytes, dev_meta_offs,
                            dev_meta_lens, dev_status, s) != CIO_OK ||
        devplan_launch_planner(w->dp, dev_bytes, w->msrc, w->mlen, n, nullptr, s) != CIO_OK ||
        launch_move(w, base, n, s) != CIO_OK ||
        devplan_launch_planner(w->dp, meta_src_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
        launch_copy(w, dev_base, dev_meta_src, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (checksum &&
        (devplan_launch_planner(w->dp, dev_bytes, w->roff, w->rlen, n, nullptr, s) != CIO_OK ||
         devplan_crc_launch(w->dp->p, w->dp->hdr, dev_base, w->seed, w->crc, n, s) != CIO_OK)) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(meta_finish, dim3(blocks256(n)), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n,
                       dev_status, w->slen, checksum ? w->crc : nullptr, w->dp->hdr, dev_crc_cur);
    HIP_TRY(hipGetLastError(), "cio_file_write_metadata_batch_dev: finish kernel launch");
    return CIO_OK;
}

/* Measurement hook (not in the public header; tools/write_dev_move_ab.py): the
 * header kernel and the move's planner of a cio_file_write_metadata_batch_dev,
 * then move_save + move_shift ALONE between two HIP events.  No metadata copy,
 * no CRC and no finish kernel: the content lands at its new place, the headers
 * stay as they were, so the same call can be timed again over the same images. */
int cioa_debug_write_dev_move_events(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                     uint64_t meta_src_bytes, const uint64_t *dev_meta_offs,
                                     const uint64_t *dev_meta_lens, int32_t *dev_status, void *stream,
                                     void *ev_start, void *ev_stop)
{
    if (!w || !dev_base || !dev_img_offs || !dev_img_caps || !dev_meta_offs || !dev_meta_lens || !dev_status ||
        !ev_start || !ev_stop || n == 0 || n > w->max_chunks || w->move_grid == 0) {
        return fail("cioa_debug_write_dev_move_events: bad argument");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    uint8_t *base = reinterpret_cast<uint8_t *>(dev_base);
    if (launch_meta_headers(w, base, dev_bytes, dev_img_offs, dev_img_caps, n, meta_src_bytes, dev_meta_offs,
                            dev_meta_lens, dev_status, s) != CIO_OK ||
        devplan_launch_planner(w->dp, dev_bytes, w->msrc, w->mlen, n, nullptr, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_start), s), "hipEventRecord");
    if (launch_move(w, base, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_stop), s), "hipEventRecord");
    return CIO_OK;
}

/* Measurement hook (not in the public header; tools/write_dev_ab.py): the
 * header kernel and the planner of a cio_file_write_batch_dev, then the append
 * copy kernel ALONE between two HIP events (cio_gpu_event_create).  No CRC and
 * no finish kernel: the record bytes land, the headers stay as they were, so
 * the same call can be timed again over the same images. */
int cioa_debug_write_dev_copy_events(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                     const void *dev_src, uint64_t src_bytes, const uint64_t *dev_src_offs,
                                     const uint64_t *dev_src_lens, int32_t *dev_status, void *stream,
                                     void *ev_start, void *ev_stop)
{
    if (!w || !dev_base || !dev_img_offs || !dev_img_caps || !dev_src || !dev_src_offs || !dev_src_lens ||
        !dev_status || !ev_start || !ev_stop || n == 0 || n > w->max_chunks) {
        return fail("cioa_debug_write_dev_copy_events: bad argument");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    hipLaunchKernelGGL(write_headers, dim3(blocks256(n)), dim3(256), 0, s, reinterpret_cast<const uint8_t *>(dev_base),
                       dev_bytes, dev_img_offs, dev_img_caps, (uint32_t) n, dev_src_offs, dev_src_lens, src_bytes,
                       dev_status, w->soff, w->slen, w->dst, w->newlen);
    HIP_TRY(hipGetLastError(), "cioa_debug_write_dev_copy_events: header kernel launch");
    if (devplan_launch_planner(w->dp, src_bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_start), s), "hipEventRecord");
    if (launch_copy(w, dev_base, dev_src, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_stop), s), "hipEventRecord");
    return CIO_OK;
}

}  // extern "C"
