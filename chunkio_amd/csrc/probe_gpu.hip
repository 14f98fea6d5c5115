// probe_gpu.hip -- the kernels of libchunkio_amd.so that are not CRC: the
// read-only stream (the practical HBM-read ceiling of the CRC kernels' access
// pattern, with its run-time diagnostics) and the synthetic fill, with their
// host entry points.  C ABI in include/chunkio_amd/cio_crc32_gpu.h.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>
#include <algorithm>

#include "cio_gpu_internal.h"
#include "crc_wave.h"

using namespace cioa;

namespace {

// ---------------------------------------------------------------- read-only stream

// Practical HBM-read ceiling for the CRC kernel's access pattern: the same
// persistent grid (one 1024-thread workgroup per CU), the same even split of
// 4 KiB wave-steps and the same coalesced non-temporal 16-byte loads, with the
// CRC replaced by an XOR.  One 4-byte store per wave keeps the loads live.
__global__ void __launch_bounds__(kThreads, 1)
read_stream_kernel(const uint8_t *__restrict__ base, uint64_t S, uint32_t *__restrict__ sink, uint32_t B,
                   unsigned long long *stamps, uint32_t work)
{
    const unsigned long long t_entry = stamps ? __builtin_amdgcn_s_memrealtime() : 0;
    unsigned long long t_first = 0;
    const uint32_t W = gridDim.x * (kThreads / kWave);
    const uint32_t wave = __builtin_amdgcn_readfirstlane(blockIdx.x * (kThreads / kWave) + (threadIdx.x >> 6));
    const uint32_t lane = threadIdx.x & 63u;
    u32x4 acc = {0u, 0u, 0u, 0u};
    // diagnostic (CIO_GPU_RS_WORK=n): n rounds of 4 independent dependent
    // chains of full-rate VALU work (3 instructions per chain and round) on
    // each step's data, standing in for the CRC's arithmetic.
    auto burn = [&]() {
        uint32_t x0 = acc.x, x1 = acc.y, x2 = acc.z, x3 = acc.w;
        for (uint32_t k = 0; k < work; ++k) {
            x0 = __builtin_amdgcn_alignbit(x0, x0, 27) ^ (x0 + k);
            x1 = __builtin_amdgcn_alignbit(x1, x1, 27) ^ (x1 + k);
            x2 = __builtin_amdgcn_alignbit(x2, x2, 27) ^ (x2 + k);
            x3 = __builtin_amdgcn_alignbit(x3, x3, 27) ^ (x3 + k);
        }
        acc = u32x4{x0, x1, x2, x3};
    };
    // diagnostic (CIO_GPU_RS_LANE): lane l reads 32 or 64 contiguous bytes of
    // each half / whole step (2 or 4 dwordx4 loads at a 32 / 64-byte lane
    // stride) instead of 16 bytes of each 1 KiB row.
    const uint32_t lsh = work >> 16;
    work &= 0xffffu;
    auto step = [&](uint64_t g) {
        if (lsh == 0) {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(base + g * kStep + (uint64_t) lane * kGran);
#pragma unroll
            for (int q = 0; q < kSub; ++q) {
                acc ^= __builtin_nontemporal_load(p + q * kWave);
            }
        } else if (lsh == 1) {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(base + g * kStep + (uint64_t) lane * 32u);
            acc ^= __builtin_nontemporal_load(p);
            acc ^= __builtin_nontemporal_load(p + 1);
            acc ^= __builtin_nontemporal_load(p + 128);
            acc ^= __builtin_nontemporal_load(p + 129);
        } else {
            const u32x4 *p = reinterpret_cast<const u32x4 *>(base + g * kStep + (uint64_t) lane * 64u);
#pragma unroll
            for (int q = 0; q < kSub; ++q) {
                acc ^= __builtin_nontemporal_load(p + q);
            }
        }
        burn();
    };
    if (B == 0xffffffffu) {
        // diagnostic (CIO_GPU_RS_BLOCK=-1): the contiguous split with two
        // steps in flight per wave (the last two refills re-read the last step)
        const uint64_t g0 = wave_start(wave, S, W), g1 = wave_start((uint64_t) wave + 1, S, W);
        if (g0 < g1) {
            auto ld4 = [&](u32x4 *r, uint64_t g) {
                const u32x4 *p = reinterpret_cast<const u32x4 *>(base + min(g, g1 - 1) * kStep +
                                                                 (uint64_t) lane * kGran);
#pragma unroll
                for (int q = 0; q < kSub; ++q) {
                    r[q] = __builtin_nontemporal_load(p + q * kWave);
                }
            };
            u32x4 ra[kSub], rb[kSub];
            ld4(ra, g0);
            ld4(rb, g0 + 1);
            for (uint64_t g = g0; g < g1; g += 2) {
#pragma unroll
                for (int q = 0; q < kSub; ++q) {
                    acc ^= ra[q];
                }
                ld4(ra, g + 2);
                __builtin_amdgcn_sched_barrier(0);
                burn();
#pragma unroll
                for (int q = 0; q < kSub; ++q) {
                    acc ^= rb[q];
                }
                ld4(rb, g + 3);
                __builtin_amdgcn_sched_barrier(0);
                burn();
            }
        }
    } else if (B & 0x80000000u) {
        // diagnostic (CIO_GPU_RS_WGPOOL=k): the CRC kernel's split, but the
        // last k steps of every wave's range form a workgroup pool that the
        // workgroup's waves claim one step at a time (LDS atomic) once their
        // own ranges are done: intra-workgroup balancing, priced on the
        // read-only stream.
        __shared__ uint32_t pool_next;
        const uint32_t k = B & 0xffffu;
        if (threadIdx.x == 0) {
            pool_next = 0;
        }
        __syncthreads();
        auto static_end = [&](uint64_t w, uint64_t &e1) {
            const uint64_t a = wave_start(w, S, W), b = wave_start(w + 1, S, W);
            e1 = b;
            return b > a + k ? b - k : a;
        };
        uint64_t g1;
        const uint64_t g0 = wave_start(wave, S, W), gs = static_end(wave, g1);
        for (uint64_t g = g0; g < gs; ++g) {
            step(g);
        }
        const uint32_t first = blockIdx.x * (kThreads / kWave);
        for (;;) {
            uint32_t item = 0;
            if (lane == 0) {
                item = atomicAdd(&pool_next, 1u);
            }
            item = __builtin_amdgcn_readfirstlane(item);
            if (item >= (kThreads / kWave) * k) {
                break;
            }
            uint64_t o1;
            const uint64_t os = static_end(first + item / k, o1);
            const uint64_t g = os + item % k;
            if (g < o1) {
                step(g);
            }
        }
    } else if (B == 0) {
        // the CRC kernel's split: one contiguous range per wave
        const uint64_t g0 = wave_start(wave, S, W), g1 = wave_start((uint64_t) wave + 1, S, W);
        for (uint64_t g = g0; g < g1; ++g) {
            step(g);
            if (stamps && g == g0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                t_first = __builtin_amdgcn_s_memrealtime();
            }
        }
    } else {
        // diagnostic (CIO_GPU_RS_BLOCK=B): blocks of B steps dealt round-robin over the waves
        for (uint64_t b = wave; b * B < S; b += W) {
            for (uint64_t g = b * B; g < min(S, b * B + B); ++g) {
                step(g);
            }
        }
    }
    const uint32_t x = wave_xor(acc[0] ^ acc[1] ^ acc[2] ^ acc[3]);
    if (lane == 0) {
        sink[wave] = x;
    }
    if (stamps && lane == 0) {
        // Diagnostic (CIO_GPU_RS_STAMPS=1): 100 MHz global clock, per wave.
        uint32_t xcc_id;
        asm volatile("s_getreg_b32 %0, hwreg(HW_REG_XCC_ID)" : "=s"(xcc_id));
        stamps[4 * wave + 0] = t_entry;
        stamps[4 * wave + 1] = t_first;
        stamps[4 * wave + 2] = __builtin_amdgcn_s_memrealtime();
        stamps[4 * wave + 3] = xcc_id;
    }
}

// ---------------------------------------------------------------- synthetic fill

__device__ __forceinline__ uint64_t splitmix64(uint64_t x)
{
    uint64_t z = x + 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

__global__ void __launch_bounds__(256)
fill_kernel(uint8_t *__restrict__ base, const uint64_t *__restrict__ offs,
            const uint64_t *__restrict__ lens, const uint64_t *__restrict__ ids, uint64_t seed,
            uint32_t n)
{
    for (uint32_t i = blockIdx.x; i < n; i += gridDim.x) {
        const uint64_t off = offs[i], len = lens[i];
        if (len == 0) {
            continue;
        }
        const uint64_t id = ids ? ids[i] : (uint64_t) i;
        const uint64_t key = seed ^ (0x9E3779B97F4A7C15ull * (id + 1));
        const uint64_t first = off & ~15ull;
        const uint64_t ngran = ((off + len + 15) & ~15ull) - first;
        for (uint64_t gi = threadIdx.x; gi < ngran / 16; gi += blockDim.x) {
            const uint64_t gaddr = first + gi * 16;
            const int64_t t0 = (int64_t) gaddr - (int64_t) off;  // chunk-relative byte of granule start
            if (t0 >= 0 && (uint64_t) t0 + 16 <= len) {
                const uint64_t k0 = (uint64_t) t0 >> 3;
                const uint32_t sh = (uint32_t) (t0 & 7) * 8;
                const uint64_t w0 = splitmix64(key + k0), w1 = splitmix64(key + k0 + 1);
                uint64_t lo, hi;
                if (sh == 0) {
                    lo = w0; hi = w1;
                } else {
                    const uint64_t w2 = splitmix64(key + k0 + 2);
                    lo = (w0 >> sh) | (w1 << (64 - sh));
                    hi = (w1 >> sh) | (w2 << (64 - sh));
                }
                *reinterpret_cast<uint4 *>(base + gaddr) =
                    make_uint4((uint32_t) lo, (uint32_t) (lo >> 32), (uint32_t) hi, (uint32_t) (hi >> 32));
            } else {
                for (int b = 0; b < 16; ++b) {
                    const int64_t t = t0 + b;
                    if (t >= 0 && (uint64_t) t < len) {
                        const uint64_t w = splitmix64(key + ((uint64_t) t >> 3));
                        base[gaddr + b] = (uint8_t) (w >> (8 * (t & 7)));
                    }
                }
            }
        }
    }
}

}  // namespace

extern "C" {

int cio_gpu_fill_synthetic(void *dev_base, const uint64_t *offs, const uint64_t *lens,
                           const uint64_t *ids, size_t n, uint64_t seed, void *stream)
{
    if (n == 0) {
        return CIO_OK;
    }
    DeviceState *st;
    if (device_state(&st) != CIO_OK) {
        return CIO_ERROR;
    }
    uint64_t *d_meta = nullptr;
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    HIP_TRY(hipMalloc(&d_meta, 3 * n * sizeof(uint64_t)), "fill: hipMalloc");
    uint64_t *d_offs = d_meta, *d_lens = d_meta + n, *d_ids = ids ? d_meta + 2 * n : nullptr;
    hipError_t e = hipMemcpy(d_offs, offs, n * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_lens, lens, n * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess && ids) e = hipMemcpy(d_ids, ids, n * sizeof(uint64_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        const uint32_t grid = (uint32_t) std::min<size_t>(n, 65535);
        hipLaunchKernelGGL(fill_kernel, dim3(grid), dim3(256), 0, s,
                           reinterpret_cast<uint8_t *>(dev_base), d_offs, d_lens, d_ids, seed,
                           (uint32_t) n);
        e = hipGetLastError();
    }
    if (e == hipSuccess) {
        e = hipStreamSynchronize(s);
    }
    (void) hipFree(d_meta);
    if (e != hipSuccess) {
        return fail("fill_kernel", e);
    }
    return CIO_OK;
}

static unsigned long long *g_rs_stamps = nullptr;   // CIO_GPU_RS_STAMPS diagnostic
static uint32_t g_rs_waves = 0;

/* Diagnostic (not in the public header): per-wave (entry, first step, done,
 * xcc) stamps of the last CIO_GPU_RS_STAMPS=1 read-stream launch; returns the
 * number of waves. */
int cioa_debug_rs_stamps(unsigned long long *host, size_t cap)
{
    if (!g_rs_stamps) {
        return 0;
    }
    const size_t n = std::min(cap, (size_t) g_rs_waves * 4);
    if (hipMemcpy(host, g_rs_stamps, n * sizeof(unsigned long long), hipMemcpyDeviceToHost) != hipSuccess) {
        return 0;
    }
    return (int) g_rs_waves;
}

static int read_stream_impl(const void *dev_base, uint64_t bytes, void *stream, uint32_t workgroups = 0)
{
    DeviceState *st;
    if (device_state(&st) != CIO_OK) {
        return CIO_ERROR;
    }
    const uint32_t grid = workgroups ? workgroups : (uint32_t) st->cus;
    static thread_local uint32_t *sink = nullptr;
    if (!sink) {
        HIP_TRY(hipMalloc(&sink, 65536 * sizeof(uint32_t)), "read_stream: hipMalloc");
    }
    const uint64_t S = bytes / kStep;
    if (S == 0 || dev_base == nullptr) {
        return CIO_OK;
    }
    uint32_t B = 0;
    if (const char *r = cioa_diag_getenv("CIO_GPU_RS_BLOCK")) {
        B = (uint32_t) atoi(r);
    }
    if (const char *r = cioa_diag_getenv("CIO_GPU_RS_WGPOOL")) {
        const int k = atoi(r);
        if (k > 0 && k < 65536) {
            B = 0x80000000u | (uint32_t) k;
        }
    }
    unsigned long long *stamps = nullptr;
    if (const char *r = cioa_diag_getenv("CIO_GPU_RS_STAMPS")) {
        if (atoi(r) > 0) {
            if (!g_rs_stamps) {
                HIP_TRY(hipMalloc(&g_rs_stamps, 65536 * 4 * sizeof(unsigned long long)), "read_stream: hipMalloc");
            }
            stamps = g_rs_stamps;
            g_rs_waves = st->cus * (kThreads / kWave);
        }
    }
    uint32_t work = 0;
    if (const char *r = cioa_diag_getenv("CIO_GPU_RS_WORK")) {
        work = (uint32_t) std::max(0, std::min(65535, atoi(r)));
    }
    if (const char *r = cioa_diag_getenv("CIO_GPU_RS_LANE")) {
        // diagnostic: bytes per lane and step-row, 16 (coalesced rows), 32 or 64
        const int lb = atoi(r);
        work |= (lb == 64 ? 2u : lb == 32 ? 1u : 0u) << 16;
    }
    hipLaunchKernelGGL(read_stream_kernel, dim3(grid), dim3(kThreads), 0,
                       reinterpret_cast<hipStream_t>(stream),
                       reinterpret_cast<const uint8_t *>(dev_base), S, sink, B, stamps, work);
    HIP_TRY(hipGetLastError(), "read_stream_kernel launch");
    return CIO_OK;
}

int cio_gpu_read_stream(const void *dev_base, uint64_t bytes, void *stream)
{
    return read_stream_impl(dev_base, bytes, stream);
}

int cio_gpu_read_stream_grid(const void *dev_base, uint64_t bytes, uint32_t workgroups, void *stream)
{
    if (workgroups > 65536 / (kThreads / kWave)) {
        return fail("cio_gpu_read_stream_grid: more than 4096 workgroups");
    }
    return read_stream_impl(dev_base, bytes, stream, workgroups);
}

}  // extern "C"
