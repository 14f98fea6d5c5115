// sort_records.h -- the arithmetic of the ungrouped append's device sort
// (sort_records_gpu.hip: sort_hist, sort_scan, sort_scatter): a record's key
// and digit, the number of passes, where a workgroup's digit count lies in the
// histogram table, a lane's stable rank inside its wave from eight ballots, and
// the scan of the per-wave digit counts along the wave index.  No HIP type, so
// that the same text compiles for the device and, stand-alone on the host,
// under ASan + UBSan (tools/sort_check.cpp, `make sortcheck`).  Not installed.
#ifndef CIOA_SORT_RECORDS_H
#define CIOA_SORT_RECORDS_H

#include <stdint.h>

// Host and device: the launcher sizes its grids and arenas with the same text.
#ifdef __HIPCC__
#define CIOA_SORT_FN __host__ __device__ __forceinline__
#else
#define CIOA_SORT_FN inline
#endif

namespace cioa {

constexpr uint32_t kSortBlock = 1024;               // records per workgroup of the histogram and scatter kernels
constexpr uint32_t kSortBits = 8;                   // bits per pass
constexpr uint32_t kSortRadix = 1u << kSortBits;    // digit values
constexpr uint32_t kSortWave = 64;
constexpr uint32_t kSortWaves = kSortBlock / kSortWave;

// The key of a record for image img of a batch of n_img images: its image
// index, or the sentinel n_img for an index outside the batch.  The sentinel
// sorts last and is what the grouped chain then sees as malformed.
CIOA_SORT_FN uint32_t sort_key(uint32_t img, uint32_t n_img)
{
    return img < n_img ? img : n_img;
}

// Passes of kSortBits bits that cover every key 0 .. n_img, the sentinel
// included: ceil(bit_length(n_img) / 8), 1 .. 4.
CIOA_SORT_FN uint32_t sort_passes(uint32_t n_img)
{
    uint32_t bits = 0;
    for (uint32_t v = n_img; v != 0; v >>= 1) {
        bits += 1;
    }
    const uint32_t p = (bits + kSortBits - 1) / kSortBits;
    return p ? p : 1;
}

CIOA_SORT_FN uint32_t sort_digit(uint32_t key, uint32_t pass)
{
    return (key >> (pass * kSortBits)) & (kSortRadix - 1);
}

// Workgroups of a pass over n_rec records.
CIOA_SORT_FN uint32_t sort_blocks(uint64_t n_rec)
{
    return (uint32_t) ((n_rec + kSortBlock - 1) / kSortBlock);
}

// The histogram table is digit-major: one linear exclusive scan of its
// kSortRadix * nb words gives, for every (digit, workgroup), the number of
// records with a lower digit plus those with this digit in a lower workgroup:
// the first position of this workgroup's records of this digit.
CIOA_SORT_FN uint32_t sort_table_at(uint32_t digit, uint32_t wg, uint32_t nb)
{
    return digit * nb + wg;
}

// One step of the digit match inside a wave: ballot is the mask of the lanes
// whose digit has bit `bit` set; a lane keeps those that agree with its own
// digit in that bit.  Started from the mask of the lanes that hold a record
// and taken over bits 0 .. 7, match is the lanes with the lane's own digit.
CIOA_SORT_FN uint64_t sort_match_step(uint64_t match, uint64_t ballot, uint32_t digit, uint32_t bit)
{
    return match & (((digit >> bit) & 1u) ? ballot : ~ballot);
}

// The lanes of match below `lane`: the lane's stable rank among the records of
// its wave with its digit.
CIOA_SORT_FN uint32_t sort_lane_rank(uint64_t match, uint32_t lane)
{
    uint64_t below = match & ((1ull << lane) - 1);
    uint32_t n = 0;
    for (; below != 0; below &= below - 1) {
        n += 1;
    }
    return n;
}

CIOA_SORT_FN uint32_t sort_popcount(uint64_t m)
{
    uint32_t n = 0;
    for (; m != 0; m &= m - 1) {
        n += 1;
    }
    return n;
}

// wcount[wave * kSortRadix + digit] holds the records of `wave` with `digit`;
// the "thread" of `digit` turns its column into the exclusive sum along the
// wave index and returns the workgroup's count of the digit.  Digit-minor:
// the 64 lanes of a wave walk 64 consecutive words at every step.
CIOA_SORT_FN uint32_t sort_wave_scan(uint32_t *wcount, uint32_t digit)
{
    uint32_t sum = 0;
    for (uint32_t w = 0; w < kSortWaves; ++w) {
        const uint32_t c = wcount[w * kSortRadix + digit];
        wcount[w * kSortRadix + digit] = sum;
        sum += c;
    }
    return sum;
}

// A record's position after the pass: the scanned table entry of (its digit,
// its workgroup), the records of the digit in lower waves, its rank in its
// wave.  No term depends on the order in which anything ran.
CIOA_SORT_FN uint32_t sort_position(uint32_t table_base, uint32_t wave_before, uint32_t lane_rank)
{
    return table_base + wave_before + lane_rank;
}

}  // namespace cioa

#endif
