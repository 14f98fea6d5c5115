// cio_gpu_internal.h -- declarations shared by the HIP translation units of
// libchunkio_amd.so (gpu_runtime.hip: errors, device state, plans, rings;
// crc32_gpu.hip: the CRC kernels and their launchers; probe_gpu.hip: the
// read-only stream and the synthetic fill; devplan_gpu.hip: the device
// planner; write_dev_gpu.hip: the write path of chunk images in HBM;
// read_dev_gpu.hip: their read path; write_records_gpu.hip: the grouped
// append; sort_records_gpu.hip: the ungrouped append's sort; grow_dev_gpu.hip:
// growing images out of an arena; rotate_dev_gpu.hip: rotating full images;
// tx_dev_gpu.hip: transactions on images; pool_dev_gpu.hip: recycling drained
// slots through a pool; pool_set_gpu.hip: the size-classed set of such pools;
// coalesce_gpu.hip: coalescing that set's adjacent free slots;
// alloc_set_gpu.hip: fresh slots out of that set and the device steps of a
// load; persist_host.hip: images down to chunk files and up again;
// route_gpu.hip: routing records to images by their metadata;
// host_pipeline.hip: the host-memory / file
// batch pipeline).
// Everything that needs no HIP type -- geometry, the plan image, the host
// planner of crc_plan.cpp -- is in cio_plan.h.  What the units of the chunk
// images share on the device is in two headers of its own: image_dev.h, the
// image check (no HIP type: the host checks run it too), and block_scan_gpu.h,
// the workgroup scan and the scan of the workgroup totals (set_scan_gpu.h adds
// the class-counting scans of the pool set).  What they share on the host is
// here: blocks_of, pow2, fail_who, SectionEvents / mark, and the launchers one
// unit exports to the others.  Not installed.
#ifndef CIOA_GPU_INTERNAL_H
#define CIOA_GPU_INTERNAL_H

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string>
#include <vector>

#include "cio_plan.h"

namespace cioa {

constexpr int kMaxDev = 64;          // device ordinals with per-device state

// The calling thread's last error message (cio_gpu_last_error).
extern thread_local std::string g_err;
// Record the message for cio_gpu_last_error(); returns CIO_ERROR.
int fail(const char *what, hipError_t e = hipSuccess);
// The same for an argument check's message under the caller's name: "who: what".
int fail_who(const char *who, const char *what);
// The calling thread's current device's state (built on first use).
int device_state(DeviceState **out);
// One launch of plan p over dev_base (chunk-id map cid: outputs and seeds by id).
int plan_exec_impl(const cio_crc32_plan *p, const void *dev_base, const uint32_t *dev_seeds,
                   uint32_t *dev_out, const uint32_t *cid, hipStream_t s,
                   hipEvent_t ev0 = nullptr, hipEvent_t ev1 = nullptr);

// The planner kernels (serial chain on s): everything plan_build writes, from
// device offs/lens, into dp's arenas.  n >= 1.
int devplan_launch_planner(const cio_crc32_devplan *dp, uint64_t dev_bytes, const uint64_t *dev_offs,
                           const uint64_t *dev_lens, size_t n, uint32_t *dev_status, hipStream_t s);
// One launch of the general stream kernel over the plan image in p's arrays,
// S and ntiny from the device header hdr (crc32_gpu.hip).
int devplan_crc_launch(const cio_crc32_plan *p, const unsigned long long *hdr, const void *dev_base,
                       const uint32_t *dev_seeds, uint32_t *dev_out, size_t n, hipStream_t s);

// Workgroups of `per` entries that cover n.
inline uint32_t blocks_of(size_t n, uint32_t per)
{
    return (uint32_t) ((n + per - 1) / per);
}

inline bool pow2(uint64_t v)
{
    return v != 0 && (v & (v - 1)) == 0;
}

// Measurement (the cioa_debug_*_events hooks): the two events go around ONE
// section of a launch chain.  mark() records ev0 (begin) or ev1 on s where
// `section` is the chosen one, and nothing where ev is NULL.
struct SectionEvents {
    int section;
    hipEvent_t ev0, ev1;
};
int mark(const SectionEvents *ev, int section, bool begin, hipStream_t s);

}  // namespace cioa

#define HIP_TRY(expr, what)                             \
    do {                                                   \
        hipError_t e_ = (expr);                            \
        if (e_ != hipSuccess) return cioa::fail(what, e_); \
    } while (0)

// A device-planned batch: plan_init's grid and knobs, arenas for max_chunks
// chunks (the plan image lives in `p`'s arrays), the planner's scratch and
// header, and the verify-on-load arrays (CRC regions and raw CRCs).
struct cio_crc32_devplan {
    cio_crc32_plan *p = nullptr;
    uint32_t max_chunks = 0;
    cioa::PlanBlockSum *bsum = nullptr;      // ceil(max_chunks / kPlanBlock)
    unsigned long long *hdr = nullptr;       // kDevHdrWords
    uint64_t *roffs = nullptr, *rlens = nullptr;   // cio_file_verify_batch_dev: CRC regions
    uint32_t *rcrc = nullptr;
};

// A writer of chunk images in HBM (cio_write_dev.h): the per-batch workspace of
// the write path (write_dev_gpu.hip, write_records_gpu.hip,
// sort_records_gpu.hip, grow_dev_gpu.hip, rotate_dev_gpu.hip, tx_dev_gpu.hip, pool_dev_gpu.hip) and of the read path
// (read_dev_gpu.hip).
struct cio_dev_writer {
    uint32_t max_chunks = 0;                 // first: the argument checks read it
    cio_crc32_devplan *dp = nullptr;
    uint32_t copy_grid = 0;
    uint32_t move_grid = 0;                  // segments of the in-place move; 0 without CIOA_WRITER_MOVE
    uint64_t *soff = nullptr, *slen = nullptr;   // validated source / CRC regions
    uint64_t *dst = nullptr;                 // destination offsets from dev_base
    uint32_t *newlen = nullptr;              // content length after the append
    uint32_t *seed = nullptr;                // init: the CRC state after bytes 22..23
    uint32_t *crc = nullptr;                 // the CRC launch's output
    uint64_t *roff = nullptr, *rlen = nullptr;   // write_at, write_metadata: the CRC region in the image
    uint64_t *msrc = nullptr, *mlen = nullptr;   // the move: old content (with CIOA_WRITER_MOVE)
    int64_t *mdelta = nullptr;               // new - old metadata length
    uint8_t *arena = nullptr;                // move_grid * kMoveSegBytes
    uint64_t *rtot = nullptr;                // packed read: slot totals, ceil(max_chunks / kReadBlock)
    uint64_t *groom = nullptr;               // grouped append: room per image
    uint64_t *gsum = nullptr;                // its scan's workgroup aggregates, ceil(max_chunks / kRecBlock)
    uint32_t *gflag = nullptr;
    uint32_t *ghdr = nullptr;                // one word: the batch's grouping is malformed
    uint32_t *skey[2] = {nullptr, nullptr};  // ungrouped append: the sort's (key, index) arenas, ping-pong
    uint32_t *sidx[2] = {nullptr, nullptr};
    uint32_t *stab = nullptr;                // its histogram table, kSortRadix * ceil(max_chunks / kSortBlock)
    uint32_t *gimg = nullptr;                // the grouped list handed to the grouped append
    uint64_t *goffs = nullptr, *glens = nullptr;
    int32_t *gst = nullptr;                  // its record statuses, in grouped order
    uint64_t *gneed = nullptr;               // grow: the bytes about to be appended per image (records variant)
    uint64_t *gcap = nullptr;                // the new capacity of an image that is to grow, 0 otherwise
    uint32_t *growhdr = nullptr;             // one word: a record's image index lies outside the batch
};

namespace cioa {

// One launch of append_copy (write_dev_gpu.hip) over the planner's image of
// (w->soff, w->slen): record i goes from dev_src + w->soff[i] to dev_dst +
// w->dst[i].  The read path's copy as well: source = the image buffer.
int launch_copy(const cio_dev_writer *w, void *dev_dst, const void *dev_src, size_t n, hipStream_t s);

// One launch of grow's byte-balanced zero fill (grow_dev_gpu.hip) over the
// planner's image of (zoff, zlen): region i, zlen[i] bytes at dev_base +
// zoff[i], becomes zero.  The transaction rollback's fill as well.
int launch_zero_fill(const cio_dev_writer *w, void *dev_base, const uint64_t *zoff, const uint64_t *zlen, size_t n,
                     hipStream_t s);

// The records-to-need sums of the grow and rotate calls' records variants
// (grow_clear and grow_need, grow_dev_gpu.hip): w->gneed[i] becomes the sum of
// min(rec_lens[r], 2^32) over the records of image i, and w->growhdr[0] whether
// an index lies outside the n_img images.  n_rec == 0: the clear alone.
int launch_need_sums(const cio_dev_writer *w, const uint32_t *rec_img, const uint64_t *rec_lens, size_t n_img,
                     size_t n_rec, hipStream_t s);

// The argument checks of cio_file_write_records_batch_dev and of the ungrouped
// call that runs it behind a sort (write_records_gpu.hip): 0 go on, 1 a no-op
// (an empty batch), CIO_ERROR refused, the message under the name `who`.
int check_records(const char *who, const cio_dev_writer *w, const void *dev_base, const uint64_t *offs,
                  const uint64_t *caps, size_t n_img, const void *dev_src, const uint32_t *rec_img,
                  const uint64_t *rec_offs, const uint64_t *rec_lens, size_t n_rec, int flags,
                  const uint32_t *crc_cur, const int32_t *img_status, const int32_t *rec_status);

// The arguments of a rotate call (rotate_dev_gpu.hip; the calls that take the
// fresh slots from a pool first, pool_dev_gpu.hip, share them).
struct RotArgs {
    const char *who;
    cio_dev_writer *w;
    void *dev_base;
    uint64_t dev_bytes;
    uint64_t *offs, *caps;
    size_t n;
    const uint64_t *need;                     // the need variant; may be NULL there too
    const uint32_t *rec_img;
    const uint64_t *rec_lens;
    size_t n_rec;
    uint64_t limit, new_cap, align;
    uint64_t *arena, *out_offs, *out_caps;
    uint32_t *out_img;
    uint64_t *out_count;
    int flags;
    uint32_t *crc_cur;
    uint64_t *total;
    int32_t *status;
};

// The argument checks of the rotate calls, before any device call
// (rotate_dev_gpu.hip): 0 go on, 1 a no-op (an empty batch), CIO_ERROR refused.
int rotate_check_args(const RotArgs &a, bool records);

// The head of a rotate batch, for the pool variant as well: the need sums
// (records), rotate_headers and rotate_scan.  Leaves in the writer's arenas
// gcap = 24 + meta of an image that reaches the placement (0 otherwise), groom
// its ordinal in its workgroup, rtot the workgroups' exclusive counts, seed the
// CRC states, and in a.total rotate's dev_total.  ev: the hook's marks around
// the sums, and the one that opens the bookkeeping (the caller closes it).
int rotate_launch_front(const RotArgs &a, bool records, hipStream_t s, const SectionEvents *ev = nullptr);

// The arguments of a grow call (grow_dev_gpu.hip; the calls that take the
// larger slots from a pool set first, pool_set_gpu.hip, share them).
struct GrowArgs {
    const char *who;
    cio_dev_writer *w;
    void *dev_base;
    uint64_t dev_bytes;
    uint64_t *offs, *caps;
    size_t n;
    const uint64_t *need;                     // NULL: the records variant
    const uint32_t *rec_img;
    const uint64_t *rec_lens;
    size_t n_rec;
    uint64_t *arena;
    uint64_t realloc_size, page, align;
    int flags;
    uint64_t *prev_offs, *prev_caps, *total;
    int32_t *status;
};

// The argument checks of the grow calls, before any device call
// (grow_dev_gpu.hip): 0 go on, 1 a no-op (an empty batch), CIO_ERROR refused.
int grow_check_args(const GrowArgs &a, bool records);

// The head of a grow batch, for the set variant as well: the need sums
// (records; a.need == NULL) and grow_headers.  Leaves the statuses of rules
// 1..4, prev_*, and in the writer's arenas soff / slen the old offset and the
// used bytes and gcap the reference's new capacity of an image that reaches
// rule 4 (all 0 otherwise).  ev: the hook's marks around the sums, and the one
// that opens the bookkeeping (the caller closes it).
int grow_launch_front(const GrowArgs &a, hipStream_t s, const SectionEvents *ev = nullptr);

// The ungrouped append's stable LSD radix sort (sort_records_gpu.hip), for the
// coalescing of a pool set as well: (key, index) of n_rec records by key =
// min(rec_img[r], n_img), sort_passes(n_img) passes between the writer's two
// (skey, sidx) arena pairs, the histogram table in stab.  *sorted: the pair
// that holds the result.  rec_img must be none of those arenas.
int sort_launch(cio_dev_writer *w, const uint32_t *rec_img, size_t n_img, size_t n_rec, int *sorted, hipStream_t s);

// The device arrays of one round of a load (persist_host.hip), n entries each:
// what the host uploads (the files' places in the stage, their sizes, whether
// each was read in full), what verify and the allocation leave, and the call's
// outputs for the round's files.
struct LoadRound {
    const uint64_t *soffs, *sizes;
    const int32_t *pre, *vst, *ast;
    const uint64_t *aoffs, *acaps;
    const uint32_t *vcrc;
    const uint64_t *vcontent;
    uint64_t *img_offs, *img_caps;
    uint32_t *crc_cur;
    int32_t *status;
};

// The back of a round of a load, behind verify and the allocation
// (alloc_set_gpu.hip): the copy from the stage into the slots, the adopt step,
// and with `zero` the fill of [size, cap) of every slot taken.
int load_launch_back(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes, const void *dev_stage,
                     uint64_t stage_bytes, size_t n, bool zero, const LoadRound &r, hipStream_t s);

}  // namespace cioa

#endif
