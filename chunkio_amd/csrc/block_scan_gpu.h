// block_scan_gpu.h -- the workgroup scan every unit that places chunk images
// in HBM shares (read_dev_gpu.hip, grow_dev_gpu.hip, rotate_dev_gpu.hip,
// pool_dev_gpu.hip, and through set_scan_gpu.h pool_set_gpu.hip and
// coalesce_gpu.hip): the exclusive scan of one value per thread through LDS,
// and the single-workgroup scan of a column of workgroup totals, pass by pass.
// Both combine with place_add (read_dev_place.h), over workgroups of
// kScanBlock threads -- kReadBlock, kGrowBlock, kRotBlock, kPoolBlock,
// kSetBlock and kCoalBlock are that width under the units' own names.  Device
// code: it needs HIP.  In an unnamed namespace: every unit inlines its own
// copy.  Not installed.
#ifndef CIOA_BLOCK_SCAN_GPU_H
#define CIOA_BLOCK_SCAN_GPU_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "read_dev_place.h"

namespace {

using namespace cioa;

constexpr uint32_t kScanBlock = kReadBlock;            // 1024: the width of every kernel that calls these

// Exclusive scan of v over the kScanBlock threads of a workgroup with
// place_add, through LDS; total: the sum over the workgroup.
__device__ __forceinline__ uint64_t block_scan_excl(uint64_t *sh, uint32_t tid, uint64_t v, uint64_t &total)
{
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kScanBlock; off <<= 1) {
        const uint64_t x = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] = place_add(x, sh[tid]);
        __syncthreads();
    }
    const uint64_t excl = tid ? sh[tid - 1] : 0;
    total = sh[kScanBlock - 1];
    __syncthreads();
    return excl;
}

// One pass of the scan of a column of workgroup totals, ONE workgroup: the
// kScanBlock totals from `base` on become the sums before them, `carry` being
// the sum of the totals before `base` (the same in every thread); returns the
// carry of the next pass.
__device__ __forceinline__ uint64_t totals_pass(uint64_t *sh, uint64_t *__restrict__ rtot, uint32_t nb, uint32_t base,
                                                uint64_t carry)
{
    const uint32_t tid = threadIdx.x, j = base + tid;
    uint64_t pass;
    const uint64_t excl = block_scan_excl(sh, tid, j < nb ? rtot[j] : 0, pass);
    if (j < nb) {
        rtot[j] = place_add(carry, excl);
    }
    return place_add(carry, pass);
}

// rtot[j] becomes the sum of the totals before workgroup j; returns their sum.
// ONE workgroup, looping over however many totals there are.  (read_scan,
// grow_scan, rotate_scan and release_scan write this loop out over
// totals_pass: with the loop statement inlined from here the compiler lays
// their exit block elsewhere and inverts the back edge's compare, and their
// device code is to stay what it was.)
__device__ __forceinline__ uint64_t totals_scan(uint64_t *sh, uint64_t *__restrict__ rtot, uint32_t nb)
{
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kScanBlock) {
        carry = totals_pass(sh, rtot, nb, base, carry);
    }
    return carry;
}

}  // namespace

#endif
