// devplan_gpu.hip -- device-planned CRC-32 batches and verify-on-load of chunk
// images in HBM, for CDNA4 (gfx950, MI355X).  C ABI in
// include/chunkio_amd/cio_crc32_gpu.h (cio_crc32_devplan_*) and
// include/chunkio_amd/cio_verify.h (cio_file_verify_batch_dev).
//
// cio_crc32_plan_create builds the stream kernel's work partition on the host
// (cioa::plan_build, crc_plan.cpp) from HOST offsets and lengths.  Here the
// same partition -- byte for byte -- is written by four small kernels from
// offsets and lengths that live in device memory, so a batch whose geometry
// the host never sees (a length read from a chunk header in HBM, a captured
// graph replayed over changing lengths) is CRC'd without a round trip:
//
//   plan_chunks1   one thread per chunk: aligned start, head, virtual length,
//                  step count and the bounds / size checks; a workgroup scan
//                  of steps and tiny-chunk ranks; per-workgroup totals; and
//                  the piece slots of pfac re-zeroed (fold_chunk skips an
//                  empty wave's stale partial by its zero factor)
//   plan_scan      ONE workgroup: exclusive scan of the workgroup totals,
//                  the batch checks (S < 2^40, S W < 2^52), the header
//   plan_chunks2   one thread per chunk: global first step g, first / last
//                  wave and piece count, the tiny list, and the fold factor
//                  of the piece in the chunk's first wave
//   plan_waves     one thread per wave: first chunk (binary search over the
//                  chunk ends), WaveStart, the LDS-fold flags, the last
//                  piece's factor, and the fold factor of the piece of the
//                  wave's first chunk
//
// Every piece (wave w, chunk k) either starts its chunk (w is the chunk's
// first wave) or starts its wave (k is the wave's first chunk), so the two
// O(1) writers above cover every piece slot.  Kernel boundaries are the only
// grid-wide synchronisation: no workgroup waits on another.
//
// The verify kernels restate cio_verify.c's per-chunk header checks
// (cio_file_format_check, src/cio_file.c:187-294, through a read-only map with
// taint 0) and its 8-byte CRC compare, one thread per image.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "cio_gpu_internal.h"
#include "image_dev.h"
#include "chunkio_amd/cio_verify.h"

using namespace cioa;

namespace {

constexpr uint32_t cx_multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        if ((a >> i) & 1u) {
            p ^= b;
        }
        b = (b & 1u) ? (b >> 1) ^ CIOA_POLY : (b >> 1);
    }
    return p;
}

// x^(8 * 4096 * 2^j) mod P, j < 52: the 4 KiB-multiple part of a fold factor
// by square-and-multiply over the bits of the step count.
constexpr int kX4kBits = 52;
struct X4kPow {
    uint32_t v[kX4kBits];
    constexpr X4kPow() : v{}
    {
        uint32_t sq = 0x00800000u;            // x^8
        for (int i = 0; i < 12; ++i) {
            sq = cx_multmodp(sq, sq);         // x^(8 * 4096)
        }
        for (int j = 0; j < kX4kBits; ++j) {
            v[j] = sq;
            sq = cx_multmodp(sq, sq);
        }
    }
};
__device__ const X4kPow d_x4k{};

// a(x) * b(x) mod P(x), reflected bit order (bit 31 = x^0).
__device__ __forceinline__ uint32_t multmodp(uint32_t a, uint32_t b)
{
    uint32_t p = 0;
    for (int i = 31; i >= 0; --i) {
        p ^= b & (0u - ((a >> i) & 1u));
        b = (b >> 1) ^ (CIOA_POLY & (0u - (b & 1u)));
    }
    return p;
}

// x^(8 d) mod P: a field element, so the same word as the host's factor().
__device__ uint32_t factor(uint64_t d, const uint32_t *x8)
{
    uint32_t r = x8[d & (uint64_t) (kStep - 1)];
    uint64_t m = d / kStep;                   // < 2^52
    for (int j = 0; m != 0 && j < kX4kBits; ++j, m >>= 1) {
        if (m & 1u) {
            r = multmodp(d_x4k.v[j], r);
        }
    }
    return r;
}

// The even split of S steps over W waves, in exact integer arithmetic (the
// host's ((uint64_t) w * S) / W; the planner validates S W < 2^52).
__device__ __forceinline__ uint64_t split(uint64_t w, uint64_t S, uint64_t W)
{
    return (w * S) / W;
}

// The wave whose range holds step t < S: the largest w with split(w) <= t,
// i.e. w S < (t + 1) W.  Its range is never empty.
__device__ __forceinline__ uint64_t wave_of(uint64_t t, uint64_t S, uint64_t W)
{
    return ((t + 1) * W - 1) / S;
}

// First and last wave and the piece count of a chunk of ns > 0 steps from
// global step g.  With S >= W no wave is empty and every wave of [w0, w1]
// holds a piece; with S < W a non-empty wave holds exactly one step, so the
// chunk has one piece per step whatever empty waves lie between them.
__device__ __forceinline__ void chunk_waves(uint64_t g, uint32_t ns, uint64_t S, uint64_t W, uint32_t &w0,
                                            uint32_t &w1, uint32_t &np)
{
    w0 = (uint32_t) wave_of(g, S, W);
    w1 = (uint32_t) wave_of(g + ns - 1, S, W);
    np = S >= W ? w1 - w0 + 1 : ns;
}

// Fold factor of the piece of chunk d in wave w: x^(8 * chunk bytes after it).
__device__ __forceinline__ uint32_t piece_factor(const ChunkDesc &d, uint64_t w, uint64_t S, uint64_t W,
                                                 const uint32_t *x8)
{
    const uint64_t g1 = split(w + 1, S, W);
    const uint64_t steps = min(g1 - d.g, (uint64_t) d.nsteps);
    const uint64_t pend = min(steps * (uint64_t) kStep, d.vlen);
    return factor(d.vlen - pend, x8);
}

// Inclusive scan over the kPlanBlock threads of a workgroup, through LDS.
template <typename T>
__device__ __forceinline__ T block_scan(T *sh, uint32_t tid, T v)
{
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kPlanBlock; off <<= 1) {
        const T x = tid >= off ? sh[tid - off] : (T) 0;
        __syncthreads();
        sh[tid] += x;
        __syncthreads();
    }
    const T r = sh[tid];
    __syncthreads();
    return r;
}

__global__ void __launch_bounds__(kPlanBlock)
plan_chunks1(const uint64_t *__restrict__ offs, const uint64_t *__restrict__ lens, uint32_t n, uint32_t W,
             uint64_t dev_bytes, ChunkDesc *__restrict__ desc, PlanBlockSum *__restrict__ bsum,
             uint32_t *__restrict__ pfac)
{
    __shared__ uint64_t sh64[kPlanBlock];
    __shared__ uint32_t sh32[kPlanBlock];
    __shared__ unsigned long long s_bytes;
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    const uint64_t i = (uint64_t) blockIdx.x * kPlanBlock + tid;
    if (tid == 0) {
        s_bytes = 0;
        s_err = 0;
    }
    // Every piece slot the CRC kernel may read for this n is re-zeroed: the
    // plan is reused with another geometry on every exec.
    const uint64_t nslots = (uint64_t) W + n + 1;
    for (uint64_t j = i; j < nslots; j += (uint64_t) gridDim.x * kPlanBlock) {
        pfac[j] = 0u;
    }
    __syncthreads();

    ChunkDesc d = {};
    uint32_t err = 0, tiny = 0;
    uint64_t len = 0;
    if (i < n) {
        const uint64_t off = offs[i];
        len = lens[i];
        if (off + len < off || off + len > dev_bytes) {
            err = CIO_DEVPLAN_E_BOUNDS;
            len = 0;
        }
        const uint64_t amask = len > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
        d.a = off & ~amask;
        d.h = (uint32_t) (off & amask);
        d.vlen = d.h + len;
        uint64_t ns = len >= 4 ? (d.vlen + kStep - 1) / kStep : 0;
        if (ns > 0xffffffffull) {
            err |= CIO_DEVPLAN_E_CHUNK_TOO_LARGE;
            ns = 0;
        }
        d.nsteps = (uint32_t) ns;
        tiny = ns == 0 && err == 0;
    }
    const uint64_t steps_incl = block_scan(sh64, tid, (uint64_t) d.nsteps);
    const uint32_t tiny_incl = block_scan(sh32, tid, tiny);
    if (len) {
        atomicAdd(&s_bytes, (unsigned long long) len);
    }
    if (err) {
        atomicOr(&s_err, err);
    }
    if (i < n) {
        d.g = steps_incl - d.nsteps;          // within the workgroup; plan_chunks2 adds the base
        d.npieces = tiny_incl - tiny;         // rank among the workgroup's tiny chunks, until then
        desc[i] = d;
    }
    __syncthreads();
    if (tid == kPlanBlock - 1) {
        PlanBlockSum b;
        b.steps = steps_incl;
        b.bytes = s_bytes;
        b.ntiny = tiny_incl;
        b.err = s_err;
        bsum[blockIdx.x] = b;
    }
}

__global__ void __launch_bounds__(kPlanBlock)
plan_scan(PlanBlockSum *__restrict__ bsum, uint32_t nb, uint32_t W, unsigned long long *__restrict__ hdr,
          uint32_t *__restrict__ status)
{
    __shared__ uint64_t sh64[kPlanBlock];
    __shared__ uint32_t sh32[kPlanBlock];
    __shared__ unsigned long long s_bytes;
    __shared__ uint32_t s_err;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) {
        s_bytes = 0;
        s_err = 0;
    }
    __syncthreads();
    uint64_t steps = 0;      // totals of the workgroups before `base` (the same in every thread)
    uint32_t ntiny = 0;
    for (uint32_t base = 0; base < nb; base += kPlanBlock) {
        const uint32_t j = base + tid;
        PlanBlockSum b = {};
        if (j < nb) {
            b = bsum[j];
        }
        const uint64_t si = block_scan(sh64, tid, b.steps);
        const uint32_t ti = block_scan(sh32, tid, b.ntiny);
        if (b.bytes) {
            atomicAdd(&s_bytes, (unsigned long long) b.bytes);
        }
        if (b.err) {
            atomicOr(&s_err, b.err);
        }
        if (j < nb) {
            bsum[j].steps = steps + si - b.steps;
            bsum[j].ntiny = ntiny + ti - b.ntiny;
        }
        sh64[tid] = si;
        sh32[tid] = ti;
        __syncthreads();
        steps += sh64[kPlanBlock - 1];
        ntiny += sh32[kPlanBlock - 1];
        __syncthreads();
    }
    if (tid == 0) {
        uint32_t err = s_err;
        // The host's "batch too large": the kernels' split needs w S < 2^52.
        if (steps >= (1ull << 40) || W > 65536u || ((steps * (uint64_t) W) >> 52) != 0) {
            err |= CIO_DEVPLAN_E_BATCH_TOO_LARGE;
        }
        // A rejected batch is published empty: the CRC launch that follows
        // then has no step and no tiny chunk, reads no data, writes no output.
        hdr[kDevHdrS] = err ? 0ull : steps;
        hdr[kDevHdrNtiny] = err ? 0ull : ntiny;
        hdr[kDevHdrBytes] = err ? 0ull : s_bytes;
        hdr[kDevHdrStatus] = err;
        if (status) {
            *status = err;
        }
    }
}

__global__ void __launch_bounds__(kPlanBlock)
plan_chunks2(uint32_t n, uint32_t W, ChunkDesc *__restrict__ desc, const PlanBlockSum *__restrict__ bsum,
             const unsigned long long *__restrict__ hdr, uint32_t *__restrict__ tiny,
             uint32_t *__restrict__ pfac, const uint32_t *__restrict__ x8)
{
    const uint64_t i = (uint64_t) blockIdx.x * kPlanBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t S = hdr[kDevHdrS];
    const bool ok = hdr[kDevHdrStatus] == 0;
    const PlanBlockSum b = bsum[blockIdx.x];
    ChunkDesc d = desc[i];
    const uint32_t rank = b.ntiny + d.npieces;
    d.g += b.steps;
    d.npieces = 0;
    d.w0 = d.w1 = 0;
    d.pad = 0;
    if (d.nsteps != 0 && S != 0) {
        chunk_waves(d.g, d.nsteps, S, W, d.w0, d.w1, d.npieces);
        pfac[(uint64_t) d.w0 + i] = piece_factor(d, d.w0, S, W, x8);
    } else if (d.nsteps == 0 && ok) {
        tiny[rank] = (uint32_t) i;            // increasing: ranks follow the chunk order
    }
    desc[i] = d;
}

// First chunk whose end step is > t (t < S): never a tiny chunk, whose end
// is its predecessor's.
__device__ __forceinline__ uint32_t chunk_of(const ChunkDesc *desc, uint32_t n, uint64_t t)
{
    uint64_t lo = 0, hi = n;
    while (lo < hi) {
        const uint64_t mid = (lo + hi) >> 1;
        if (desc[mid].g + desc[mid].nsteps > t) {
            hi = mid;
        } else {
            lo = mid + 1;
        }
    }
    return (uint32_t) min(lo, (uint64_t) n - 1);
}

__device__ __forceinline__ bool wg_local(const ChunkDesc &d)
{
    return d.npieces > 1 && d.w0 / kWavesPerWg == d.w1 / kWavesPerWg;
}

__global__ void __launch_bounds__(256)
plan_waves(uint32_t n, uint32_t W, const ChunkDesc *__restrict__ desc,
           const unsigned long long *__restrict__ hdr, WaveStart *__restrict__ wstart,
           uint32_t *__restrict__ pfac, const uint32_t *__restrict__ x8)
{
    const uint32_t w = blockIdx.x * 256u + threadIdx.x;
    if (w >= W) {
        return;
    }
    const uint64_t S = hdr[kDevHdrS];
    const uint64_t nslots = (uint64_t) W + n + 1;
    WaveStart ws = {};
    uint32_t flags = 0, lastfac = 0;
    if (S == 0) {
        ws.d = desc[0];
    } else {
        const uint64_t g0 = split(w, S, W), g1 = split((uint64_t) w + 1, S, W);
        ws.c = chunk_of(desc, n, g0);
        ws.d = desc[ws.c];
        if (g0 < g1) {
            const ChunkDesc &first = ws.d;
            pfac[(uint64_t) w + ws.c] = piece_factor(first, w, S, W, x8);
            if (first.g < g0 && first.g + first.nsteps <= g1 && wg_local(first)) {
                flags |= kWfFold | ((w - first.w0) << 8);
            }
            const uint32_t lc = chunk_of(desc, n, g1 - 1);
            const ChunkDesc last = desc[lc];
            const bool nonfinal = last.g + last.nsteps > g1;
            if (nonfinal && wg_local(last)) {
                flags |= kWfPublish;
            }
            lastfac = nonfinal ? piece_factor(last, w, S, W, x8) : 0x80000000u;
        }
    }
    wstart[w] = ws;
    pfac[nslots + w] = flags;
    pfac[nslots + W + w] = lastfac;
}

// ---------------------------------------------------------------- verify-on-load

// cio_verify.c's per-chunk header checks (taint 0, read-only map), one image
// per thread.  Emits the CRC region [img + 22, + 2 + meta_len + content_len);
// a failed image gets a zero-length region so that the batch keeps its
// indexing.
__global__ void __launch_bounds__(256)
verify_headers(const uint8_t *__restrict__ base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
               const uint64_t *__restrict__ img_sizes, uint32_t n, int32_t *__restrict__ status,
               int32_t *__restrict__ error, uint32_t *__restrict__ crc_raw, uint32_t *__restrict__ meta_len,
               uint64_t *__restrict__ content_len, uint64_t *__restrict__ roffs, uint64_t *__restrict__ rlens)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint64_t off = img_offs[i], size = img_sizes[i];
    int32_t st = CIO_OK, er = 0;
    uint32_t meta = 0;
    uint64_t clen = 0, roff = 0, rlen = 0;
    if (off + size < off || off + size > dev_bytes) {
        st = CIO_ERROR;
    } else if (size == 0) {
        st = CIO_CORRUPTED;                   // a read-only open cannot prepare an empty file
        er = CIO_ERR_PERMISSION;
    } else if (size < 24) {
        st = CIO_CORRUPTED;                   // cio_file_st_get_content_len: before the magic check
        er = CIO_ERR_BAD_FILE_SIZE;
    } else {
        const uint8_t *p = base + off;
        const uint32_t m = ((uint32_t) p[22] << 8) | p[23];
        uint64_t len = be32(p + 10);
        if (len == 0 && size > 24ull + m && p[24ull + m] != 0x00) {
            len = size - 24ull - m;           // legacy inference; nothing is written back
        }
        if (p[0] != 0xc1 || p[1] != 0x00) {
            st = CIO_CORRUPTED;
            er = CIO_ERR_BAD_LAYOUT;
        } else {
            meta = m;
            clen = len;
            if (24ull + m + len > size) {
                st = CIO_CORRUPTED;
                er = CIO_ERR_BAD_FILE_SIZE;
            } else {
                roff = off + 22;
                rlen = 2ull + m + len;
            }
        }
    }
    status[i] = st;
    error[i] = er;
    crc_raw[i] = 0;
    if (meta_len) {
        meta_len[i] = meta;
    }
    if (content_len) {
        content_len[i] = clen;
    }
    roffs[i] = roff;
    rlens[i] = rlen;
}

// Image bytes 2..9 against htonl(crc_finalize(raw)) held in an 8-byte crc_t:
// the finalized CRC big-endian in bytes 2..5, zero in bytes 6..9.
__global__ void __launch_bounds__(256)
verify_verdicts(const uint8_t *__restrict__ base, const uint64_t *__restrict__ img_offs, uint32_t n,
                const uint32_t *__restrict__ raw, int32_t *__restrict__ status, int32_t *__restrict__ error,
                uint32_t *__restrict__ crc_raw)
{
    const uint32_t i = blockIdx.x * 256u + threadIdx.x;
    if (i >= n || status[i] != CIO_OK) {
        return;
    }
    const uint8_t *p = base + img_offs[i];
    const uint32_t fin = raw[i] ^ 0xffffffffu;
    if (be32(p + 2) != fin || be32(p + 6) != 0u) {
        status[i] = CIO_CORRUPTED;
        error[i] = CIO_ERR_BAD_CHECKSUM;
    } else {
        crc_raw[i] = raw[i];
    }
}

}  // namespace

int cioa::devplan_launch_planner(const cio_crc32_devplan *dp, uint64_t dev_bytes, const uint64_t *dev_offs,
                                 const uint64_t *dev_lens, size_t n, uint32_t *dev_status, hipStream_t s)
{
    const cio_crc32_plan *p = dp->p;
    const uint32_t nb = (uint32_t) ((n + kPlanBlock - 1) / kPlanBlock);
    hipLaunchKernelGGL(plan_chunks1, dim3(nb), dim3(kPlanBlock), 0, s, dev_offs, dev_lens, (uint32_t) n, p->W,
                       dev_bytes, p->desc, dp->bsum, p->pfac);
    hipLaunchKernelGGL(plan_scan, dim3(1), dim3(kPlanBlock), 0, s, dp->bsum, nb, p->W, dp->hdr, dev_status);
    hipLaunchKernelGGL(plan_chunks2, dim3(nb), dim3(kPlanBlock), 0, s, (uint32_t) n, p->W, p->desc, dp->bsum,
                       dp->hdr, p->tiny, p->pfac, p->st->x8);
    hipLaunchKernelGGL(plan_waves, dim3((p->W + 255u) / 256u), dim3(256), 0, s, (uint32_t) n, p->W, p->desc,
                       dp->hdr, p->wstart, p->pfac, p->st->x8);
    HIP_TRY(hipGetLastError(), "cio_crc32_devplan_exec: planner launch");
    return CIO_OK;
}

extern "C" {

void cio_crc32_devplan_destroy(cio_crc32_devplan *dp)
{
    if (!dp) {
        return;
    }
    cio_crc32_plan_destroy(dp->p);
    (void) hipFree(dp->bsum);
    (void) hipFree(dp->hdr);
    (void) hipFree(dp->roffs);
    (void) hipFree(dp->rlens);
    (void) hipFree(dp->rcrc);
    delete dp;
}

int cio_crc32_devplan_create(cio_crc32_devplan **out, size_t max_chunks)
{
    if (!out) {
        return fail("cio_crc32_devplan_create: null argument");
    }
    *out = nullptr;
    if (max_chunks == 0 || max_chunks >= 0xffffffffull) {
        return fail("cio_crc32_devplan_create: max_chunks must be 1 .. 2^32 - 2");
    }
    DeviceState *st;
    if (device_state(&st) != CIO_OK) {
        return CIO_ERROR;
    }
    cio_crc32_devplan *dp = new cio_crc32_devplan();
    cio_crc32_plan *p = dp->p = new cio_crc32_plan();
    plan_init(p, st, max_chunks);
    dp->max_chunks = (uint32_t) max_chunks;
    const size_t W = p->W, nb = (max_chunks + kPlanBlock - 1) / kPlanBlock;
    const size_t npart = W + max_chunks + 1 + 2 * W;
    hipError_t e;
    if ((e = hipMalloc(&p->desc, max_chunks * sizeof(ChunkDesc))) != hipSuccess ||
        (e = hipMalloc(&p->wstart, W * sizeof(WaveStart))) != hipSuccess ||
        (e = hipMalloc(&p->tiny, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&p->partials, npart * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMalloc(&p->counters, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&p->pfac, npart * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&dp->bsum, nb * sizeof(PlanBlockSum))) != hipSuccess ||
        (e = hipMalloc(&dp->hdr, kDevHdrWords * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMalloc(&dp->roffs, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&dp->rlens, max_chunks * sizeof(uint64_t))) != hipSuccess ||
        (e = hipMalloc(&dp->rcrc, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemset(p->partials, 0, npart * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(p->counters, 0, max_chunks * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemset(p->pfac, 0, npart * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemset(dp->hdr, 0, kDevHdrWords * sizeof(unsigned long long))) != hipSuccess) {
        cio_crc32_devplan_destroy(dp);
        return fail("cio_crc32_devplan_create: device allocation", e);
    }
    *out = dp;
    return CIO_OK;
}

int cio_crc32_devplan_exec(cio_crc32_devplan *dp, const void *dev_base, uint64_t dev_bytes,
                           const uint64_t *dev_offs, const uint64_t *dev_lens, size_t n,
                           const uint32_t *dev_seeds, uint32_t *dev_out, uint32_t *dev_status, void *stream)
{
    if (!dp) {
        return fail("cio_crc32_devplan_exec: null plan");
    }
    if (n == 0) {
        return CIO_OK;
    }
    if (!dev_base || !dev_offs || !dev_lens || !dev_out) {
        return fail("cio_crc32_devplan_exec: null pointer");
    }
    if (n > dp->max_chunks) {
        return fail("cio_crc32_devplan_exec: more chunks than the plan was created for");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    if (devplan_launch_planner(dp, dev_bytes, dev_offs, dev_lens, n, dev_status, s) != CIO_OK) {
        return CIO_ERROR;
    }
    return devplan_crc_launch(dp->p, dp->hdr, dev_base, dev_seeds, dev_out, n, s);
}

/* Measurement hook (not in the public header; tools/devplan_ab.py): the same
 * exec with HIP events (cio_gpu_event_create) recorded before the planner
 * kernels, between them and the CRC launch, and after it. */
int cioa_debug_devplan_exec_events(cio_crc32_devplan *dp, const void *dev_base, uint64_t dev_bytes,
                                   const uint64_t *dev_offs, const uint64_t *dev_lens, size_t n,
                                   uint32_t *dev_out, void *stream, void *ev_start, void *ev_planned,
                                   void *ev_stop)
{
    if (!dp || !dev_base || !dev_offs || !dev_lens || !dev_out || !ev_start || !ev_planned || !ev_stop ||
        n == 0 || n > dp->max_chunks) {
        return fail("cioa_debug_devplan_exec_events: bad argument");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_start), s), "hipEventRecord");
    if (devplan_launch_planner(dp, dev_bytes, dev_offs, dev_lens, n, nullptr, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_planned), s), "hipEventRecord");
    if (devplan_crc_launch(dp->p, dp->hdr, dev_base, nullptr, dev_out, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_stop), s), "hipEventRecord");
    return CIO_OK;
}

uint32_t cio_crc32_devplan_workgroups(const cio_crc32_devplan *dp)
{
    return dp ? dp->p->grid : 0;
}

int cio_file_verify_batch_dev(cio_crc32_devplan *dp, const void *dev_base, uint64_t dev_bytes,
                              const uint64_t *dev_img_offs, const uint64_t *dev_img_sizes, size_t n,
                              int flags, int32_t *dev_status, int32_t *dev_error,
                              uint32_t *dev_crc_raw, uint32_t *dev_meta_len,
                              uint64_t *dev_content_len, void *stream)
{
    if (flags & ~CIOA_VERIFY_CHECKSUM) {
        return fail("cio_file_verify_batch_dev: only CIOA_VERIFY_CHECKSUM is supported "
                    "(a device image cannot be written back or deleted)");
    }
    if (!dp) {
        return fail("cio_file_verify_batch_dev: null plan");
    }
    if (n == 0) {
        return CIO_OK;
    }
    if (!dev_base || !dev_img_offs || !dev_img_sizes || !dev_status || !dev_error || !dev_crc_raw) {
        return fail("cio_file_verify_batch_dev: null pointer");
    }
    if (n > dp->max_chunks) {
        return fail("cio_file_verify_batch_dev: more images than the plan was created for");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    const uint8_t *base = reinterpret_cast<const uint8_t *>(dev_base);
    const uint32_t nb = (uint32_t) ((n + 255) / 256);
    hipLaunchKernelGGL(verify_headers, dim3(nb), dim3(256), 0, s, base, dev_bytes, dev_img_offs, dev_img_sizes,
                       (uint32_t) n, dev_status, dev_error, dev_crc_raw, dev_meta_len, dev_content_len,
                       dp->roffs, dp->rlens);
    HIP_TRY(hipGetLastError(), "cio_file_verify_batch_dev: header kernel launch");
    if (!(flags & CIOA_VERIFY_CHECKSUM)) {
        return CIO_OK;
    }
    if (cio_crc32_devplan_exec(dp, dev_base, dev_bytes, dp->roffs, dp->rlens, n, nullptr, dp->rcrc, nullptr,
                               stream) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(verify_verdicts, dim3(nb), dim3(256), 0, s, base, dev_img_offs, (uint32_t) n, dp->rcrc,
                       dev_status, dev_error, dev_crc_raw);
    HIP_TRY(hipGetLastError(), "cio_file_verify_batch_dev: verdict kernel launch");
    return CIO_OK;
}

/* Test hook (not in the public header): run ONLY the planner kernels over the
 * device offs/lens, synchronise, and copy the plan image back: desc[n],
 * wstart[W], tiny[n] (the first hdr[kDevHdrNtiny] entries are the list),
 * pfac[W + n + 1 + 2 W], hdr[kDevHdrWords].  Any output may be NULL; *W_out
 * is the plan's wave count.  No CRC kernel runs. */
int cioa_debug_devplan_image(cio_crc32_devplan *dp, uint64_t dev_bytes, const uint64_t *dev_offs,
                             const uint64_t *dev_lens, size_t n, void *desc, void *wstart, uint32_t *tiny,
                             uint32_t *pfac, uint64_t *hdr, uint32_t *W_out)
{
    if (!dp) {
        return fail("cioa_debug_devplan_image: null plan");
    }
    const cio_crc32_plan *p = dp->p;
    if (W_out) {
        *W_out = p->W;
    }
    if (n == 0 || !dev_offs || !dev_lens) {
        return CIO_OK;
    }
    if (n > dp->max_chunks) {
        return fail("cioa_debug_devplan_image: more chunks than the plan was created for");
    }
    if (devplan_launch_planner(dp, dev_bytes, dev_offs, dev_lens, n, nullptr, nullptr) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipStreamSynchronize(nullptr), "cioa_debug_devplan_image: synchronise");
    const size_t W = p->W;
    if (desc) HIP_TRY(hipMemcpy(desc, p->desc, n * sizeof(ChunkDesc), hipMemcpyDeviceToHost), "copy desc");
    if (wstart) HIP_TRY(hipMemcpy(wstart, p->wstart, W * sizeof(WaveStart), hipMemcpyDeviceToHost), "copy wstart");
    if (tiny) HIP_TRY(hipMemcpy(tiny, p->tiny, n * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy tiny");
    if (pfac) HIP_TRY(hipMemcpy(pfac, p->pfac, (W + n + 1 + 2 * W) * sizeof(uint32_t), hipMemcpyDeviceToHost), "copy pfac");
    if (hdr) HIP_TRY(hipMemcpy(hdr, dp->hdr, kDevHdrWords * sizeof(uint64_t), hipMemcpyDeviceToHost), "copy header");
    return CIO_OK;
}

}  // extern "C"
