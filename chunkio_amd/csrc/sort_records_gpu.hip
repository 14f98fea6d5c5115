// sort_records_gpu.hip -- the ungrouped append to chunk images in HBM, for
// CDNA4 (gfx950, MI355X): records in any order.  C ABI in
// include/chunkio_amd/cio_write_dev_ungrouped.h; DESIGN.md §17.
//
// A stable LSD radix sort of (key, record index) by key = min(dev_rec_img[r],
// n_img), kSortBits bits per pass, sort_passes(n_img) passes, between two
// (key, index) arenas of the writer; then the grouped append (§16), unchanged,
// over the sorted list.  A serial chain of kernels on the caller's stream:
//
//   per pass:
//   sort_hist      one workgroup per kSortBlock records: the count of each
//                  digit in LDS (LDS atomics: a count does not depend on
//                  order), written digit-major, table[digit * nb + wg].
//   sort_scan      ONE workgroup looping over the kSortRadix * nb words
//                  kSortBlock at a time: their exclusive scan in place.
//   sort_scatter   one workgroup per kSortBlock records: each record's stable
//                  rank among the records of its workgroup with its digit --
//                  inside its wave a digit match from eight ballots and the
//                  count of the lower lanes, across the waves a [wave][digit]
//                  table in LDS scanned along the wave index -- and the store
//                  of (key, index) at table entry + rank.  No atomic decides a
//                  position.
//   then:
//   sort_gather    one thread per sorted position j: the grouped img / offs /
//                  lens arrays, and dev_rec_order[j], from the sorted indices.
//   cio_file_write_records_batch_dev   the grouped chain over those arrays,
//                  statuses into a writer arena.
//   sort_unpermute dev_rec_status[order[j]] = status[j].
//
// Pass 0 reads dev_rec_img itself and clamps; the record index is the thread's.
// Kernel boundaries are the only grid-wide synchronisation: no workgroup waits
// on another, there are no tickets and no look-back.  The arithmetic is
// sort_records.h, the text tools/sort_check.cpp runs on the host.  Plain C++
// throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "sort_records.h"
#include "chunkio_amd/cio_write_dev_ungrouped.h"

using namespace cioa;

namespace {

// Record r of the pass: its key, from the caller's array in pass 0.
__device__ __forceinline__ uint32_t load_key(const uint32_t *__restrict__ rec_img, const uint32_t *__restrict__ kin,
                                             uint32_t pass, uint32_t n_img, uint64_t r)
{
    return pass == 0 ? sort_key(rec_img[r], n_img) : kin[r];
}

__global__ void __launch_bounds__(kSortBlock)
sort_hist(const uint32_t *__restrict__ rec_img, const uint32_t *__restrict__ kin, uint32_t pass, uint32_t n_img,
          uint32_t n_rec, uint32_t nb, uint32_t *__restrict__ table)
{
    __shared__ uint32_t cnt[kSortRadix];
    const uint32_t tid = threadIdx.x;
    const uint64_t r = (uint64_t) blockIdx.x * kSortBlock + tid;
    if (tid < kSortRadix) {
        cnt[tid] = 0;
    }
    __syncthreads();
    if (r < n_rec) {
        atomicAdd(&cnt[sort_digit(load_key(rec_img, kin, pass, n_img, r), pass)], 1u);
    }
    __syncthreads();
    if (tid < kSortRadix) {
        table[sort_table_at(tid, blockIdx.x, nb)] = cnt[tid];
    }
}

// table[0 .. words) becomes its exclusive scan (32-bit: the total is n_rec).
__global__ void __launch_bounds__(kSortBlock)
sort_scan(uint32_t *__restrict__ table, uint32_t words)
{
    __shared__ uint32_t sh[kSortBlock];
    const uint32_t tid = threadIdx.x;
    uint32_t carry = 0;                       // the words before `base` (the same in every thread)
    for (uint32_t base = 0; base < words; base += kSortBlock) {
        const uint32_t j = base + tid;        // words <= 2^30: no wrap
        const uint32_t v = j < words ? table[j] : 0;
        sh[tid] = v;
        __syncthreads();
        for (uint32_t off = 1; off < kSortBlock; off <<= 1) {
            const uint32_t x = tid >= off ? sh[tid - off] : 0;
            __syncthreads();
            sh[tid] += x;
            __syncthreads();
        }
        const uint32_t incl = sh[tid], total = sh[kSortBlock - 1];
        __syncthreads();
        if (j < words) {
            table[j] = carry + incl - v;
        }
        carry += total;
    }
}

__global__ void __launch_bounds__(kSortBlock)
sort_scatter(const uint32_t *__restrict__ rec_img, const uint32_t *__restrict__ kin,
             const uint32_t *__restrict__ iin, uint32_t pass, uint32_t n_img, uint32_t n_rec, uint32_t nb,
             const uint32_t *__restrict__ table, uint32_t *__restrict__ kout, uint32_t *__restrict__ iout)
{
    __shared__ uint32_t wcount[kSortWaves * kSortRadix];    // [wave][digit]
    __shared__ uint32_t gbase[kSortRadix];
    const uint32_t tid = threadIdx.x, lane = tid & (kSortWave - 1), wave = tid / kSortWave;
    const uint64_t r = (uint64_t) blockIdx.x * kSortBlock + tid;
    const bool active = r < n_rec;
    for (uint32_t k = tid; k < kSortWaves * kSortRadix; k += kSortBlock) {
        wcount[k] = 0;
    }
    if (tid < kSortRadix) {
        gbase[tid] = table[sort_table_at(tid, blockIdx.x, nb)];
    }
    uint32_t key = 0, idx = 0, digit = 0;
    if (active) {
        key = load_key(rec_img, kin, pass, n_img, r);
        idx = pass == 0 ? (uint32_t) r : iin[r];
        digit = sort_digit(key, pass);
    }
    uint64_t match = __ballot(active);
    for (uint32_t bit = 0; bit < kSortBits; ++bit) {
        match = sort_match_step(match, __ballot(active && ((digit >> bit) & 1u)), digit, bit);
    }
    const uint32_t rank = sort_lane_rank(match, lane);
    __syncthreads();
    if (active && rank == 0) {                // the first lane of each digit present in the wave
        wcount[wave * kSortRadix + digit] = sort_popcount(match);
    }
    __syncthreads();
    if (tid < kSortRadix) {
        (void) sort_wave_scan(wcount, tid);
    }
    __syncthreads();
    if (active) {
        const uint32_t pos = sort_position(gbase[digit], wcount[wave * kSortRadix + digit], rank);
        if (pos < n_rec) {                    // holds by construction; no store outside the arenas
            kout[pos] = key;
            iout[pos] = idx;
        }
    }
}

__global__ void __launch_bounds__(256)
sort_gather(const uint32_t *__restrict__ keys, const uint32_t *__restrict__ idx,
            const uint64_t *__restrict__ rec_offs, const uint64_t *__restrict__ rec_lens, uint32_t n_rec,
            uint32_t *__restrict__ gimg, uint64_t *__restrict__ goffs, uint64_t *__restrict__ glens,
            uint32_t *__restrict__ order)
{
    const uint64_t j = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (j >= n_rec) {
        return;
    }
    const uint32_t r = idx[j];
    gimg[j] = keys[j];
    if (r < n_rec) {
        goffs[j] = rec_offs[r];
        glens[j] = rec_lens[r];
    }
    if (order) {
        order[j] = r;
    }
}

__global__ void __launch_bounds__(256)
sort_unpermute(const uint32_t *__restrict__ idx, const int32_t *__restrict__ gst, uint32_t n_rec,
               int32_t *__restrict__ rec_status)
{
    const uint64_t j = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (j >= n_rec) {
        return;
    }
    const uint32_t r = idx[j];
    if (r < n_rec) {
        rec_status[r] = gst[j];
    }
}

}  // namespace

// The sort's passes; *sorted: the arena pair (0 or 1) that holds the result.
// Declared in cio_gpu_internal.h: coalesce_gpu.hip sorts a pool set's entries
// by offset with it.
int cioa::sort_launch(cio_dev_writer *w, const uint32_t *rec_img, size_t n_img, size_t n_rec, int *sorted,
                      hipStream_t s)
{
    const uint32_t nb = sort_blocks(n_rec), passes = sort_passes((uint32_t) n_img);
    int in = 1;                               // pass 0 reads rec_img; no arena
    for (uint32_t p = 0; p < passes; ++p) {
        const int out = in ^ 1;
        hipLaunchKernelGGL(sort_hist, dim3(nb), dim3(kSortBlock), 0, s, rec_img, w->skey[in], p, (uint32_t) n_img,
                           (uint32_t) n_rec, nb, w->stab);
        hipLaunchKernelGGL(sort_scan, dim3(1), dim3(kSortBlock), 0, s, w->stab, kSortRadix * nb);
        hipLaunchKernelGGL(sort_scatter, dim3(nb), dim3(kSortBlock), 0, s, rec_img, w->skey[in], w->sidx[in], p,
                           (uint32_t) n_img, (uint32_t) n_rec, nb, w->stab, w->skey[out], w->sidx[out]);
        in = out;
    }
    HIP_TRY(hipGetLastError(), "the device sort (ungrouped append, coalesce): sort kernels launch");
    *sorted = in;
    return CIO_OK;
}

namespace {

int launch_gather(cio_dev_writer *w, int sorted, const uint64_t *rec_offs, const uint64_t *rec_lens, size_t n_rec,
                  uint32_t *order, hipStream_t s)
{
    hipLaunchKernelGGL(sort_gather, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, w->skey[sorted], w->sidx[sorted],
                       rec_offs, rec_lens, (uint32_t) n_rec, w->gimg, w->goffs, w->glens, order);
    HIP_TRY(hipGetLastError(), "cio_file_write_records_ungrouped_batch_dev: gather kernel launch");
    return CIO_OK;
}

int launch_unpermute(cio_dev_writer *w, int sorted, size_t n_rec, int32_t *rec_status, hipStream_t s)
{
    hipLaunchKernelGGL(sort_unpermute, dim3(blocks_of(n_rec, 256)), dim3(256), 0, s, w->sidx[sorted], w->gst,
                       (uint32_t) n_rec, rec_status);
    HIP_TRY(hipGetLastError(), "cio_file_write_records_ungrouped_batch_dev: unpermute kernel launch");
    return CIO_OK;
}

}  // namespace

extern "C" {

int cio_file_write_records_ungrouped_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                               const uint64_t *dev_img_offs, const uint64_t *dev_img_caps,
                                               size_t n_img, const void *dev_src, uint64_t src_bytes,
                                               const uint32_t *dev_rec_img, const uint64_t *dev_rec_offs,
                                               const uint64_t *dev_rec_lens, size_t n_rec, int flags,
                                               uint32_t *dev_crc_cur, int32_t *dev_img_status,
                                               int32_t *dev_rec_status, uint32_t *dev_rec_order, void *stream)
{
    static const char who[] = "cio_file_write_records_ungrouped_batch_dev";
    const int rc = check_records(who, w, dev_base, dev_img_offs, dev_img_caps, n_img, dev_src, dev_rec_img,
                                 dev_rec_offs, dev_rec_lens, n_rec, flags, dev_crc_cur, dev_img_status,
                                 dev_rec_status);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int sorted = 0;
    if (sort_launch(w, dev_rec_img, n_img, n_rec, &sorted, s) != CIO_OK ||
        launch_gather(w, sorted, dev_rec_offs, dev_rec_lens, n_rec, dev_rec_order, s) != CIO_OK ||
        cio_file_write_records_batch_dev(w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n_img, dev_src,
                                         src_bytes, w->gimg, w->goffs, w->glens, n_rec, flags, dev_crc_cur,
                                         dev_img_status, w->gst, stream) != CIO_OK) {
        return CIO_ERROR;
    }
    return launch_unpermute(w, sorted, n_rec, dev_rec_status, s);
}

/* Measurement hook (not in the public header; tools/write_records_ungrouped_ab.py):
 * the sort, gather and unpermute kernels of a
 * cio_file_write_records_ungrouped_batch_dev ALONE between two HIP events.
 * Nothing of the images changes; dev_rec_status takes whatever the writer's
 * status arena holds from its last ungrouped call. */
int cioa_debug_sort_records_events(cio_dev_writer *w, size_t n_img, const uint32_t *dev_rec_img,
                                   const uint64_t *dev_rec_offs, const uint64_t *dev_rec_lens, size_t n_rec,
                                   int32_t *dev_rec_status, uint32_t *dev_rec_order, void *stream, void *ev_start,
                                   void *ev_stop)
{
    if (!ev_start || !ev_stop || !w || n_img == 0 || n_rec == 0 || !dev_rec_img || !dev_rec_offs || !dev_rec_lens ||
        !dev_rec_status || n_img > w->max_chunks || n_rec > w->max_chunks) {
        return fail("cioa_debug_sort_records_events: bad argument");
    }
    hipStream_t s = reinterpret_cast<hipStream_t>(stream);
    int sorted = 0;
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_start), s), "hipEventRecord");
    if (sort_launch(w, dev_rec_img, n_img, n_rec, &sorted, s) != CIO_OK ||
        launch_gather(w, sorted, dev_rec_offs, dev_rec_lens, n_rec, dev_rec_order, s) != CIO_OK ||
        launch_unpermute(w, sorted, n_rec, dev_rec_status, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev_stop), s), "hipEventRecord");
    return CIO_OK;
}

}  // extern "C"
