// crc_wave.h -- device helpers shared by the CRC kernels (crc32_gpu.hip) and
// the probe kernels (probe_gpu.hip): the even split of wave-steps over the
// persistent grid's waves, the wave-wide XOR and the 16-byte load type.
// Not installed.
#ifndef CIOA_CRC_WAVE_H
#define CIOA_CRC_WAVE_H

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace cioa {

// floor(x / d) for x < 2^52, d >= 1: a correctly rounded double quotient is
// within one of the integer quotient (x and d are exact in a double), and one
// compare-and-step fixes it.  A 64-bit integer division is a ~120-instruction
// SALU routine for wave-uniform operands; at kernel start 16 waves per CU
// running three of them on the CU's one scalar unit delayed the last wave's
// first HBM request by ~2.5 us.  This is ~20 VALU instructions per wave.
__device__ __forceinline__ uint64_t div_u52(uint64_t x, uint64_t d)
{
    uint64_t q = (uint64_t) ((double) x / (double) d);
    if (q * d > x) {
        q -= 1;
    } else if ((q + 1) * d <= x) {
        q += 1;
    }
    return q;
}

// floor(w * X / W), the even split of X units over W waves.  The plan
// guarantees S < 2^40 and W <= 2^12 (plan_create), so w * X < 2^52.  A full
// MI355X has W = 256 x 16 = 2^12 waves: then it is a uniform multiply and
// shift on the scalar unit, and the kernels' first HBM requests wait on no
// floating-point division.
__device__ __forceinline__ uint64_t split_point(uint64_t w, uint64_t X, uint64_t W)
{
    if ((W & (W - 1)) == 0) {
        return (w * X) >> __builtin_ctzll(W);
    }
    return div_u52(w * X, W);
}

__device__ __forceinline__ uint64_t wave_start(uint64_t w, uint64_t S, uint64_t W)
{
    return split_point(w, S, W);
}

typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// XOR over the 64 lanes of a wave (every lane active), wave-uniform result.
// DPP moves inside each 16-lane row (quad swaps, then the half-row and row
// mirrors) leave every lane holding its row's XOR; four lane reads combine
// the rows.  Plain VALU: __shfl_xor would be six ds_bpermute round trips
// through the LDS pipe that the CRC lookups are using.
__device__ __forceinline__ uint32_t wave_xor(uint32_t v)
{
    v ^= (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0xB1, 0xF, 0xF, false);    // quad_perm [1,0,3,2]
    v ^= (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x4E, 0xF, 0xF, false);    // quad_perm [2,3,0,1]
    v ^= (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x141, 0xF, 0xF, false);   // row_half_mirror
    v ^= (uint32_t) __builtin_amdgcn_update_dpp(0, (int) v, 0x140, 0xF, 0xF, false);   // row_mirror
    return (uint32_t) (__builtin_amdgcn_readlane((int) v, 0) ^ __builtin_amdgcn_readlane((int) v, 16) ^
                       __builtin_amdgcn_readlane((int) v, 32) ^ __builtin_amdgcn_readlane((int) v, 48));
}

}  // namespace cioa

#endif
