// set_scan_gpu.h -- the workgroup scans the kernels of the pool set
// (pool_set_gpu.hip) and of its coalescing (coalesce_gpu.hip) share beside
// block_scan_gpu.h's (which this header includes): the K-WAY COUNTING SCAN of
// a class index per thread (three ballots, a [wave][class] table in LDS, the
// workgroup's K totals into the class-major table), and the single-workgroup
// scan of that table.  Device code: it
// needs HIP, unlike pool_set.h, whose arithmetic it calls.  In an unnamed
// namespace, as it was inside pool_set_gpu.hip: every unit inlines its own
// copy, and that unit's device code is what it was.  Not installed.
#ifndef CIOA_SET_SCAN_GPU_H
#define CIOA_SET_SCAN_GPU_H

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "pool_set.h"
#include "block_scan_gpu.h"

namespace {

using namespace cioa;

// The K-way counting scan of one workgroup: every thread brings its class c
// (kSetNone: none).  Returns the number of entries before the thread in its
// workgroup with its class; tab gets the workgroup's count of every class.
__device__ __forceinline__ uint32_t class_rank(uint32_t *wcount, uint32_t c, uint64_t *__restrict__ tab, uint32_t nb)
{
    const uint32_t tid = threadIdx.x, lane = tid & (kSetWave - 1), wave = tid / kSetWave;
    const bool holds = c != kSetNone;
    if (tid < kSetWaves * kPoolSetMax) {
        wcount[tid] = 0;
    }
    uint64_t ballot[kSetBits];
    const uint64_t all = __ballot(holds);
    for (uint32_t bit = 0; bit < kSetBits; ++bit) {
        ballot[bit] = __ballot(holds && ((c >> bit) & 1u));
    }
    const uint64_t match = set_match(all, ballot, c);
    const uint32_t rank = sort_lane_rank(match, lane);
    __syncthreads();
    if (holds && rank == 0) {                 // the first lane of each class present in the wave
        wcount[wave * kPoolSetMax + c] = sort_popcount(match);
    }
    __syncthreads();
    if (tid < kPoolSetMax) {
        tab[set_tab_at(tid, blockIdx.x, nb)] = set_wave_scan(wcount, tid);
    }
    __syncthreads();
    return holds ? wcount[wave * kPoolSetMax + c] + rank : 0;
}

// tab[(k, j)] becomes the count of class k before workgroup j, for k < n_cls;
// reach[k] (LDS) the class's total.  ONE workgroup.  As the sort scans its
// histogram: one linear exclusive scan of the class-major table, whatever
// n_cls is, then every word less its class's first (set_class_excl).  The
// counts add up to at most n < 2^32: no sum wraps.
__device__ __forceinline__ void class_scan(uint64_t *sh, uint64_t *reach, uint64_t *tab, uint32_t nb, uint32_t n_cls)
{
    __shared__ uint64_t first[kPoolSetMax];
    const uint32_t tid = threadIdx.x, words = n_cls * nb;
    uint64_t carry = 0;                       // the counts before `base` (the same in every thread)
    for (uint32_t base = 0; base < words; base += kSetBlock) {
        const uint32_t j = base + tid;
        uint64_t pass;
        const uint64_t excl = block_scan_excl(sh, tid, j < words ? tab[j] : 0, pass);
        if (j < words) {
            tab[j] = carry + excl;
        }
        carry += pass;
    }
    __syncthreads();                          // the table's words, across the workgroup
    if (tid < n_cls) {
        first[tid] = tab[set_tab_at(tid, 0, nb)];
        reach[tid] = set_class_total(first[tid], tid + 1 < n_cls ? tab[set_tab_at(tid + 1, 0, nb)] : carry);
    }
    __syncthreads();
    for (uint32_t j = tid; j < words; j += kSetBlock) {
        tab[j] = set_class_excl(tab[j], first[j / nb]);
    }
    __syncthreads();
}

}  // namespace

#endif
