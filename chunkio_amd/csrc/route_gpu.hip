// route_gpu.hip -- routing records to chunk images in HBM by their metadata,
// for CDNA4 (gfx950, MI355X): a directory of the images keyed by the raw
// CRC-32 state of their metadata, and for every record of a batch the image
// whose metadata equals the record's tag.  C ABI in
// include/chunkio_amd/cio_route_dev.h; DESIGN.md §27.
//
// Both calls are a serial chain of kernels on the caller's stream.
//
// The build, over n_img images:
//
//   route_img_regions  one thread per image: the image check; into the
//                      writer's arenas the metadata's region in the image
//                      buffer, zero-length for an image that fails; the
//                      workgroup's count of the images that passed
//   planner + CRC      devplan's four kernels and the device-planned CRC
//                      launch over those regions, unseeded: the keys (R0).  A
//                      zero-length region gives the raw init state.
//   the sort           sort_records_gpu.hip's stable radix sort of (key, i)
//                      with the key cap 2^32 - 1: four passes, the key is the
//                      hash itself
//   route_dir_out      one thread per position: the two directory arrays
//   route_dir_hdr      ONE workgroup: the sum of the workgroups' counts, the
//                      header
//
// The route, over n_rec records:
//
//   route_tag_regions  one thread per record: R2; the tag's region in the tag
//                      buffer, zero-length for a malformed tag, so that the
//                      planner's bounds check has nothing to refuse
//   planner + CRC      the same two launches over the tag buffer: key(tag_r)
//   route_probe        ONE WAVE per record: the lower bound of the key in
//                      dev_dir_keys, then the walk over the positions of that
//                      key -- the gate, the image check, the lengths, and the
//                      bytes as meta_cmp compares them (16 per lane and load on
//                      both sides at any alignment, the last m & 15 one per
//                      lane, a wave vote).  Everything but the byte compare is
//                      wave-uniform.
//   route_count        one thread per record: the workgroup scan of (missed,
//                      matched), a missed record's rank in its workgroup
//   route_totals       ONE workgroup: the scan of the workgroups' counts,
//                      dev_total
//   route_list         with dev_miss_list: every missed record to its rank.
//                      No atomic: the list is ascending by construction.
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another.  No kernel writes the image buffer, and no load leaves an array
// whatever the directory holds: every index read from it is checked against
// n_img before it is used (R6).  The arithmetic is route.h, the text
// tools/route_check.cpp runs on the host; the workgroup scans are
// block_scan_gpu.h's.  Plain C++ and vector stores throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "route.h"
#include "block_scan_gpu.h"
#include "write_dev_copy.h"
#include "chunkio_amd/cio_route_dev.h"

using namespace cioa;

namespace {

constexpr uint32_t kProbeThreads = 256;                // 4 waves, one record each
constexpr uint32_t kProbeWaves = kProbeThreads / kWave;
constexpr size_t kSortAllKeys = 0xffffffffu;           // the sort's key cap: sort_key leaves every key as it is

static_assert(kRouteBlock == kScanBlock, "the route's scan kernels are block_scan_gpu.h's width");

// soff[i], slen[i]: the metadata of image i in the image buffer, (0, 0) when
// the image check fails; cnt[blockIdx.x]: the workgroup's images that passed.
__global__ void __launch_bounds__(kRouteBlock)
route_img_regions(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
                  const uint64_t *__restrict__ img_caps, uint32_t n, uint64_t *__restrict__ soff,
                  uint64_t *__restrict__ slen, uint64_t *__restrict__ cnt)
{
    __shared__ uint64_t sh[kRouteBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kRouteBlock + threadIdx.x;
    bool ok = false;
    if (i < n) {
        const uint64_t off = img_offs[i];
        uint32_t meta = 0;
        uint64_t content = 0;
        ok = image_ok(base, dev_bytes, off, img_caps[i], meta, content);
        soff[i] = ok && meta != 0 ? off + kReadHdr : 0;
        slen[i] = ok ? meta : 0;
    }
    uint64_t total;
    (void) block_scan_excl(sh, threadIdx.x, ok ? 1 : 0, total);
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(256)
route_dir_out(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx, uint32_t n,
              uint32_t *__restrict__ dir_keys, uint32_t *__restrict__ dir_imgs)
{
    const uint64_t j = (uint64_t) blockIdx.x * 256u + threadIdx.x;
    if (j < n) {
        dir_keys[j] = skey[j];
        dir_imgs[j] = sidx[j];
    }
}

// hdr = {n_img, the images that passed, 0, 0}; nb workgroup counts, 0 for an
// empty directory.
__global__ void __launch_bounds__(kRouteBlock)
route_dir_hdr(uint64_t *__restrict__ cnt, uint32_t nb, uint32_t n, uint32_t *__restrict__ hdr)
{
    __shared__ uint64_t sh[kRouteBlock];
    const uint64_t passed = totals_scan(sh, cnt, nb);
    if (threadIdx.x == 0) {
        hdr[0] = n;
        hdr[1] = (uint32_t) passed;
        hdr[2] = 0;
        hdr[3] = 0;
    }
}

// soff[r], slen[r]: tag r in the tag buffer, (0, 0) when it is malformed or
// empty.
__global__ void __launch_bounds__(kRouteBlock)
route_tag_regions(const uint64_t *__restrict__ tag_offs, const uint64_t *__restrict__ tag_lens, uint32_t n_rec,
                  uint64_t tag_bytes, uint64_t *__restrict__ soff, uint64_t *__restrict__ slen)
{
    const uint64_t r = (uint64_t) blockIdx.x * kRouteBlock + threadIdx.x;
    if (r >= n_rec) {
        return;
    }
    const uint64_t off = tag_offs[r], len = tag_lens[r];
    const bool ok = len != 0 && route_tag_ok(off, len, tag_bytes);
    soff[r] = ok ? off : 0;
    slen[r] = ok ? len : 0;
}

// R4's verdict on image i for a tag of len bytes at t, by one wave: true in
// every lane or in none.
__device__ __forceinline__ bool probe_pass(const uint8_t *base, uint64_t dev_bytes,
                                           const uint64_t *__restrict__ img_offs,
                                           const uint64_t *__restrict__ img_caps, const int32_t *gate, uint32_t i,
                                           const uint8_t *t, uint64_t len, uint32_t lane)
{
    if (gate && gate[i] != CIO_OK) {
        return false;
    }
    const uint64_t off = img_offs[i];
    uint32_t meta = 0;
    uint64_t content = 0;
    if (!image_ok(base, dev_bytes, off, img_caps[i], meta, content) || meta != len) {
        return false;
    }
    if (meta == 0) {
        return true;
    }
    const uint8_t *a = base + off + kReadHdr;
    const uint32_t m16 = meta & ~15u;
    bool d = false;
    for (uint32_t x = lane * kGran; x < m16; x += kRow) {
        const u32x4 va = reinterpret_cast<const Unaligned16 *>(a + x)->v;
        const u32x4 vb = reinterpret_cast<const Unaligned16 *>(t + x)->v;
        d |= ((va[0] ^ vb[0]) | (va[1] ^ vb[1]) | (va[2] ^ vb[2]) | (va[3] ^ vb[3])) != 0;
    }
    if (m16 + lane < meta) {
        d |= a[m16 + lane] != t[m16 + lane];
    }
    return __ballot(d) == 0;
}

// One wave per record.  keys: the CRC launch's output over the tags (not read
// when n_img == 0: nothing was launched).
__global__ void __launch_bounds__(kProbeThreads)
route_probe(const uint8_t *base, uint64_t dev_bytes, const uint64_t *__restrict__ img_offs,
            const uint64_t *__restrict__ img_caps, uint32_t n_img, const int32_t *gate,
            const uint32_t *__restrict__ dir_keys, const uint32_t *__restrict__ dir_imgs,
            const uint32_t *__restrict__ dir_hdr, const uint8_t *tags, uint64_t tag_bytes,
            const uint64_t *__restrict__ tag_offs, const uint64_t *__restrict__ tag_lens, uint32_t n_rec,
            const uint32_t *__restrict__ keys, uint32_t miss_img, uint32_t *__restrict__ rec_img,
            int32_t *__restrict__ rec_status)
{
    const uint32_t wave = (uint32_t) __builtin_amdgcn_readfirstlane((int) (threadIdx.x / kWave));
    const uint32_t lane = threadIdx.x & (kWave - 1);
    const uint64_t r = (uint64_t) blockIdx.x * kProbeWaves + wave;
    if (r >= n_rec) {
        return;
    }
    const uint64_t off = tag_offs[r], len = tag_lens[r];
    const bool dir_ok = dir_hdr[0] == n_img, tag_ok = route_tag_ok(off, len, tag_bytes);
    uint32_t found = kRouteNone;
    if (dir_ok && tag_ok && n_img != 0) {
        const uint8_t *t = tags + (len != 0 ? off : 0);
        found = route_match(dir_keys, dir_imgs, n_img, keys[r], [&](uint32_t i) {
            return probe_pass(base, dev_bytes, img_offs, img_caps, gate, i, t, len, lane);
        });
    }
    if (lane == 0) {
        const bool matched = found != kRouteNone;
        rec_img[r] = matched ? found : miss_img;
        rec_status[r] = route_status(dir_ok, tag_ok, matched);
    }
}

// rank[r]: the missed records before r in its workgroup; cnt[blockIdx.x]: the
// workgroup's packed (missed, matched).
__global__ void __launch_bounds__(kRouteBlock)
route_count(const int32_t *__restrict__ rec_status, uint32_t n_rec, uint32_t *__restrict__ rank,
            uint64_t *__restrict__ cnt)
{
    __shared__ uint64_t sh[kRouteBlock];
    const uint64_t r = (uint64_t) blockIdx.x * kRouteBlock + threadIdx.x;
    const uint64_t mine = r < n_rec ? route_count_pack(rec_status[r]) : 0;
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, threadIdx.x, mine, total);
    if (r < n_rec) {
        rank[r] = (uint32_t) route_count_missed(excl);
    }
    if (threadIdx.x == 0) {
        cnt[blockIdx.x] = total;
    }
}

// cnt[j] becomes the packed counts before workgroup j; total = {matched,
// missed, malformed}.
__global__ void __launch_bounds__(kRouteBlock)
route_totals(uint64_t *__restrict__ cnt, uint32_t nb, uint32_t n_rec, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kRouteBlock];
    const uint64_t all = totals_scan(sh, cnt, nb);
    if (threadIdx.x == 0) {
        const uint64_t matched = route_count_matched(all), missed = route_count_missed(all);
        total[0] = matched;
        total[1] = missed;
        total[2] = n_rec - matched - missed;
    }
}

__global__ void __launch_bounds__(kRouteBlock)
route_list(const int32_t *__restrict__ rec_status, uint32_t n_rec, const uint32_t *__restrict__ rank,
           const uint64_t *__restrict__ cnt, uint32_t *__restrict__ miss_list)
{
    const uint64_t r = (uint64_t) blockIdx.x * kRouteBlock + threadIdx.x;
    if (r >= n_rec || rec_status[r] != kRouteRetry) {
        return;
    }
    const uint64_t at = route_count_missed(cnt[blockIdx.x]) + rank[r];
    if (at < n_rec) {                             // at <= r holds by construction; no store outside the list
        miss_list[at] = (uint32_t) r;
    }
}

// Measurement: the sections of cioa_debug_route_build_events and
// cioa_debug_route_records_events (SectionEvents).  kSecFind is the sort in a
// build and the probe in a route; kSecOut what follows it.
enum { kSecNone = 0, kSecRegions, kSecPlan, kSecCrc, kSecFind, kSecOut };

// The keys of n regions (w->soff, w->slen) of `buf` into w->crc.
int launch_keys(cio_dev_writer *w, const void *buf, uint64_t bytes, size_t n, hipStream_t s,
                const SectionEvents *ev)
{
    if (mark(ev, kSecPlan, true, s) != CIO_OK ||
        devplan_launch_planner(w->dp, bytes, w->soff, w->slen, n, nullptr, s) != CIO_OK ||
        mark(ev, kSecPlan, false, s) != CIO_OK || mark(ev, kSecCrc, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    // a NULL tag buffer holds no byte, and every region is empty: any device address serves as the base
    if (devplan_crc_launch(w->dp->p, w->dp->hdr, buf ? buf : w->crc, nullptr, w->crc, n, s) != CIO_OK) {
        return CIO_ERROR;
    }
    return mark(ev, kSecCrc, false, s);
}

// What both calls check of the writer and the images, before any device call.
int check_common(const char *who, const cio_dev_writer *w, const void *dev_base, const uint64_t *offs,
                 const uint64_t *caps, size_t n_img, size_t n_rec, const void *keys, const void *imgs,
                 const void *hdr)
{
    if (!w) {
        return fail_who(who, "null writer");
    }
    if (n_img >= 0xffffffffull) {
        return fail_who(who, "n_img must be below 2^32 - 1");
    }
    if (n_img > w->max_chunks) {
        return fail_who(who, "more images than the writer was created for");
    }
    if (n_rec > w->max_chunks) {
        return fail_who(who, "more records than the writer was created for");
    }
    if (!hdr || (n_img != 0 && (!dev_base || !offs || !caps || !keys || !imgs))) {
        return fail_who(who, "null pointer");
    }
    return 0;
}


struct BuildArgs {
    cio_dev_writer *w;
    const void *dev_base;
    uint64_t dev_bytes;
    const uint64_t *offs, *caps;
    size_t n_img;
    uint32_t *keys, *imgs, *hdr;
};

struct RouteArgs {
    cio_dev_writer *w;
    const void *dev_base;
    uint64_t dev_bytes;
    const uint64_t *offs, *caps;
    size_t n_img;
    const int32_t *gate;
    const uint32_t *keys, *imgs, *hdr;
    const void *tags;
    uint64_t tag_bytes;
    const uint64_t *tag_offs, *tag_lens;
    size_t n_rec;
    uint32_t miss_img;
    int flags;
    uint32_t *rec_img;
    int32_t *rec_status;
    uint32_t *miss_list;
    uint64_t *total;
};

// The argument checks of the route call, before any device call: 0 go on, 1 a
// no-op (an empty batch), CIO_ERROR refused.
int check_route(const char *who, const RouteArgs &a)
{
    if (a.flags != 0) {
        return fail_who(who, "unknown flags");
    }
    if (check_common(who, a.w, a.dev_base, a.offs, a.caps, a.n_img, a.n_rec, a.keys, a.imgs, a.hdr) != 0) {
        return CIO_ERROR;
    }
    if (a.n_rec == 0) {
        return 1;
    }
    if ((!a.tags && a.tag_bytes != 0) || !a.tag_offs || !a.tag_lens || !a.rec_img || !a.rec_status || !a.total) {
        return fail_who(who, "null pointer");
    }
    return 0;
}

int launch_build(const BuildArgs &a, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n_img, nb = blocks_of(a.n_img, kRouteBlock);
    int sorted = 0;
    if (n != 0) {
        if (mark(ev, kSecRegions, true, s) != CIO_OK) {
            return CIO_ERROR;
        }
        hipLaunchKernelGGL(route_img_regions, dim3(nb), dim3(kRouteBlock), 0, s,
                           reinterpret_cast<const uint8_t *>(a.dev_base), a.dev_bytes, a.offs, a.caps, n, w->soff,
                           w->slen, w->rtot);
        HIP_TRY(hipGetLastError(), "cio_file_route_build_dev: region kernel launch");
        if (mark(ev, kSecRegions, false, s) != CIO_OK ||
            launch_keys(w, a.dev_base, a.dev_bytes, a.n_img, s, ev) != CIO_OK ||
            mark(ev, kSecFind, true, s) != CIO_OK ||
            sort_launch(w, w->crc, kSortAllKeys, a.n_img, &sorted, s) != CIO_OK ||
            mark(ev, kSecFind, false, s) != CIO_OK) {
            return CIO_ERROR;
        }
    }
    if (mark(ev, kSecOut, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    if (n != 0) {
        hipLaunchKernelGGL(route_dir_out, dim3(blocks_of(a.n_img, 256)), dim3(256), 0, s, w->skey[sorted],
                           w->sidx[sorted], n, a.keys, a.imgs);
    }
    hipLaunchKernelGGL(route_dir_hdr, dim3(1), dim3(kRouteBlock), 0, s, w->rtot, nb, n, a.hdr);
    HIP_TRY(hipGetLastError(), "cio_file_route_build_dev: directory kernels launch");
    return mark(ev, kSecOut, false, s);
}

int launch_route(const RouteArgs &a, hipStream_t s, const SectionEvents *ev)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) a.n_rec, nb = blocks_of(a.n_rec, kRouteBlock);
    if (a.n_img != 0) {                           // R8: without an image nothing can match; no key is needed
        if (mark(ev, kSecRegions, true, s) != CIO_OK) {
            return CIO_ERROR;
        }
        hipLaunchKernelGGL(route_tag_regions, dim3(nb), dim3(kRouteBlock), 0, s, a.tag_offs, a.tag_lens, n,
                           a.tag_bytes, w->soff, w->slen);
        HIP_TRY(hipGetLastError(), "cio_file_route_records_batch_dev: region kernel launch");
        if (mark(ev, kSecRegions, false, s) != CIO_OK ||
            launch_keys(w, a.tags, a.tag_bytes, a.n_rec, s, ev) != CIO_OK) {
            return CIO_ERROR;
        }
    }
    if (mark(ev, kSecFind, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(route_probe, dim3(blocks_of(a.n_rec, kProbeWaves)), dim3(kProbeThreads), 0, s,
                       reinterpret_cast<const uint8_t *>(a.dev_base), a.dev_bytes, a.offs, a.caps,
                       (uint32_t) a.n_img, a.gate, a.keys, a.imgs, a.hdr, reinterpret_cast<const uint8_t *>(a.tags),
                       a.tag_bytes, a.tag_offs, a.tag_lens, n, w->crc, a.miss_img, a.rec_img, a.rec_status);
    HIP_TRY(hipGetLastError(), "cio_file_route_records_batch_dev: probe kernel launch");
    if (mark(ev, kSecFind, false, s) != CIO_OK || mark(ev, kSecOut, true, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(route_count, dim3(nb), dim3(kRouteBlock), 0, s, a.rec_status, n, w->seed, w->rtot);
    hipLaunchKernelGGL(route_totals, dim3(1), dim3(kRouteBlock), 0, s, w->rtot, nb, n, a.total);
    if (a.miss_list) {
        hipLaunchKernelGGL(route_list, dim3(nb), dim3(kRouteBlock), 0, s, a.rec_status, n, w->seed, w->rtot,
                           a.miss_list);
    }
    HIP_TRY(hipGetLastError(), "cio_file_route_records_batch_dev: totals kernels launch");
    return mark(ev, kSecOut, false, s);
}

}  // namespace

extern "C" {

int cio_file_route_build_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                             uint32_t *dev_dir_keys, uint32_t *dev_dir_imgs, uint32_t *dev_dir_hdr, void *stream)
{
    const BuildArgs a = {w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n_img, dev_dir_keys, dev_dir_imgs,
                         dev_dir_hdr};
    if (check_common("cio_file_route_build_dev", w, dev_base, dev_img_offs, dev_img_caps, n_img, 0, dev_dir_keys,
                     dev_dir_imgs, dev_dir_hdr) != 0) {
        return CIO_ERROR;
    }
    return launch_build(a, reinterpret_cast<hipStream_t>(stream), nullptr);
}

int cio_file_route_records_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                     const int32_t *dev_img_gate,
                                     const uint32_t *dev_dir_keys, const uint32_t *dev_dir_imgs,
                                     const uint32_t *dev_dir_hdr,
                                     const void *dev_tags, uint64_t tag_bytes,
                                     const uint64_t *dev_tag_offs, const uint64_t *dev_tag_lens, size_t n_rec,
                                     uint32_t miss_img, int flags,
                                     uint32_t *dev_rec_img, int32_t *dev_rec_status,
                                     uint32_t *dev_miss_list, uint64_t *dev_total, void *stream)
{
    const RouteArgs a = {w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n_img, dev_img_gate, dev_dir_keys,
                         dev_dir_imgs, dev_dir_hdr, dev_tags, tag_bytes, dev_tag_offs, dev_tag_lens, n_rec, miss_img,
                         flags, dev_rec_img, dev_rec_status, dev_miss_list, dev_total};
    const int rc = check_route("cio_file_route_records_batch_dev", a);
    if (rc != 0) {
        return rc > 0 ? CIO_OK : rc;
    }
    return launch_route(a, reinterpret_cast<hipStream_t>(stream), nullptr);
}

/* Measurement hooks (not in the public header; tools/route_ab.py): a whole
 * cio_file_route_build_dev, or a whole cio_file_route_records_batch_dev without
 * a gate and a miss list, with the two HIP events around ONE section of its
 * chain: 1 the region kernel, 2 the planner's kernels, 3 the CRC launch, 4 the
 * sort (build) or the probe (route), 5 what follows it. */
int cioa_debug_route_build_events(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                  const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                  uint32_t *dev_dir_keys, uint32_t *dev_dir_imgs, uint32_t *dev_dir_hdr,
                                  void *stream, int section, void *ev_start, void *ev_stop)
{
    const BuildArgs a = {w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n_img, dev_dir_keys, dev_dir_imgs,
                         dev_dir_hdr};
    if (!ev_start || !ev_stop || section < kSecRegions || section > kSecOut || n_img == 0 ||
        check_common("cioa_debug_route_build_events", w, dev_base, dev_img_offs, dev_img_caps, n_img, 0,
                     dev_dir_keys, dev_dir_imgs, dev_dir_hdr) != 0) {
        return fail("cioa_debug_route_build_events: bad argument");
    }
    const SectionEvents ev = {section, reinterpret_cast<hipEvent_t>(ev_start), reinterpret_cast<hipEvent_t>(ev_stop)};
    return launch_build(a, reinterpret_cast<hipStream_t>(stream), &ev);
}

int cioa_debug_route_records_events(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                    const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                    const uint32_t *dev_dir_keys, const uint32_t *dev_dir_imgs,
                                    const uint32_t *dev_dir_hdr, const void *dev_tags, uint64_t tag_bytes,
                                    const uint64_t *dev_tag_offs, const uint64_t *dev_tag_lens, size_t n_rec,
                                    uint32_t miss_img, uint32_t *dev_rec_img, int32_t *dev_rec_status,
                                    uint64_t *dev_total, void *stream, int section, void *ev_start, void *ev_stop)
{
    const RouteArgs a = {w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n_img, nullptr, dev_dir_keys,
                         dev_dir_imgs, dev_dir_hdr, dev_tags, tag_bytes, dev_tag_offs, dev_tag_lens, n_rec, miss_img,
                         0, dev_rec_img, dev_rec_status, nullptr, dev_total};
    if (!ev_start || !ev_stop || section < kSecRegions || section > kSecOut || n_img == 0 ||
        check_route("cioa_debug_route_records_events", a) != 0) {
        return fail("cioa_debug_route_records_events: bad argument");
    }
    const SectionEvents ev = {section, reinterpret_cast<hipEvent_t>(ev_start), reinterpret_cast<hipEvent_t>(ev_stop)};
    return launch_route(a, reinterpret_cast<hipStream_t>(stream), &ev);
}

}  // extern "C"
