// check_scan.h -- what the stand-alone host checks (tools/*_check.cpp) share
// when they run the device kernels' scans workgroup by workgroup: the order in
// which the workgroups "run", block_scan_excl of block_scan_gpu.h over every
// "thread" of a workgroup of `width` threads, and totals_scan pass by pass.
// The combine step is place_add of read_dev_place.h, the text the kernels run.
#ifndef CIOA_TOOLS_CHECK_SCAN_H
#define CIOA_TOOLS_CHECK_SCAN_H

#include <stdint.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "read_dev_place.h"

// The workgroups 0 .. nb - 1 in order 0 ascending, 1 descending, 2 shuffled.
inline std::vector<uint32_t> order_of(uint32_t nb, int order, std::mt19937_64 &rng)
{
    std::vector<uint32_t> o(nb);
    std::iota(o.begin(), o.end(), 0u);
    if (order == 1) {
        std::reverse(o.begin(), o.end());
    } else if (order == 2) {
        std::shuffle(o.begin(), o.end(), rng);
    }
    return o;
}

// block_scan_excl, every "thread": sh holds the threads' values and is used
// up; excl[t] the sum before thread t, total the workgroup's.
inline void wg_scan(uint32_t width, std::vector<uint64_t> &sh, std::vector<uint64_t> &excl, uint64_t &total)
{
    std::vector<uint64_t> x(width);
    for (uint32_t off = 1; off < width; off <<= 1) {
        for (uint32_t t = 0; t < width; ++t) {
            x[t] = t >= off ? sh[t - off] : 0;
        }
        for (uint32_t t = 0; t < width; ++t) {
            sh[t] = cioa::place_add(x[t], sh[t]);
        }
    }
    for (uint32_t t = 0; t < width; ++t) {
        excl[t] = t ? sh[t - 1] : 0;
    }
    total = sh[width - 1];
}

// totals_scan, one workgroup, pass by pass: v[0 .. nb) becomes its exclusive
// scan; returns the sum.
inline uint64_t scan_totals(uint32_t width, uint64_t *v, uint32_t nb)
{
    std::vector<uint64_t> sh(width), excl(width);
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += width) {
        for (uint32_t t = 0; t < width; ++t) {
            sh[t] = base + t < nb ? v[base + t] : 0;
        }
        uint64_t pass;
        wg_scan(width, sh, excl, pass);
        for (uint32_t t = 0; t < width && base + t < nb; ++t) {
            v[base + t] = cioa::place_add(carry, excl[t]);
        }
        carry = cioa::place_add(carry, pass);
    }
    return carry;
}

#endif
