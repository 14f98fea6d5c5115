// coalesce_gpu.hip -- coalescing the adjacent free slots of the size-classed
// pool set in HBM, and dropping its duplicate and overlapping entries, for
// CDNA4 (gfx950, MI355X).  C ABI in include/chunkio_amd/cio_write_dev_coalesce.h;
// DESIGN.md §24.
//
// A serial chain of kernels on the caller's stream over the N = n_cls * stride
// positions of the set's arrays, kCoalBlock per workgroup:
//
//   coal_gather   one thread per position: the set's soundness, is the position
//                 an entry, C1, and the entry's 32-bit key off / align (the
//                 sentinel otherwise) into writer scratch
//   the sort      sort_records_gpu.hip's stable radix sort of (key, position),
//                 1 .. 4 passes for the key bound: C2's order
//   coal_ends     one thread per sorted position: (off, cap) into 64-bit
//                 scratch, the workgroup's exclusive prefix MAXIMUM of the
//                 ends, the number of well-formed entries
//   coal_mscan    ONE workgroup: the prefix maximum of the workgroups' maxima
//   coal_survive  C2's test off < M, and the workgroup scan of the survivors
//   coal_sscan    ONE workgroup: the scan of the survivor totals
//   coal_compact  every survivor to its rank: the survivors, dense, in order
//   coal_link     one thread per survivor: C3 -- candidate, continues the one
//                 before it -- and the workgroup scan of the run starts
//   coal_rscan    ONE workgroup: the scan of the run-start totals: run ids
//   coal_groups   the thread of a run's first survivor walks the run's GROUPS
//                 (C4): each next group start by a galloping lower bound over
//                 the sorted offsets, one store per entry of a group
//   coal_class    one thread per survivor: the output's class (C5) and §23's
//                 K-way counting scan over it; the workgroup's group,
//                 absorbed and classless counts
//   coal_final    ONE workgroup: the scan of the class table, the verdict,
//                 dev_total, c_k and the mask of the set words that change
//   coal_commit   not with CIOA_COALESCE_DRY: on verdict 0 every output to k *
//                 stride + its rank in its class; thread k of workgroup 0 writes
//                 set[4k] when it changes
//
// Kernel boundaries are the only grid-wide synchronisation; no workgroup waits
// on another, there is no atomic, and the one kernel that writes the set reads
// none of its words: everything it needs lies in writer scratch by then.  The
// class table, the per-call words and four columns of workgroup totals live in
// the sort's histogram table (stab), free once the sort is done.  The
// arithmetic is coalesce.h, the text tools/coalesce_check.cpp runs on the
// host; the workgroup scans are set_scan_gpu.h's.  Plain C++ and vector stores
// throughout.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "cio_gpu_internal.h"
#include "coalesce.h"
#include "set_scan_gpu.h"
#include "chunkio_amd/cio_write_dev_coalesce.h"

using namespace cioa;

namespace {

__device__ __forceinline__ uint64_t max64(uint64_t a, uint64_t b)
{
    return a > b ? a : b;
}

// Exclusive prefix maximum of v over the kCoalBlock threads of a workgroup
// (0 in front of the first), through LDS; total: the workgroup's maximum.
__device__ __forceinline__ uint64_t block_max_excl(uint64_t *sh, uint32_t tid, uint64_t v, uint64_t &total)
{
    sh[tid] = v;
    __syncthreads();
    for (uint32_t off = 1; off < kCoalBlock; off <<= 1) {
        const uint64_t x = tid >= off ? sh[tid - off] : 0;
        __syncthreads();
        sh[tid] = max64(x, sh[tid]);
        __syncthreads();
    }
    const uint64_t excl = tid ? sh[tid - 1] : 0;
    total = sh[kCoalBlock - 1];
    __syncthreads();
    return excl;
}

// key[p]: the sort key of position p = k * stride + j.
__global__ void __launch_bounds__(kCoalBlock)
coal_gather(const uint64_t *__restrict__ set_offs, const uint64_t *__restrict__ set_caps,
            const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride, uint32_t n, uint64_t dev_bytes,
            uint64_t align, uint32_t sentinel, uint32_t *__restrict__ key)
{
    const uint64_t p = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    if (p >= n) {
        return;
    }
    const uint64_t k = p / stride, j = p - k * stride;     // k < n_cls: p < n_cls * stride
    const bool entry = set_sound(set, n_cls, stride) && j < set[4 * k + kPoolCount];
    uint64_t off = 0, cap = 0;
    if (entry) {
        off = set_offs[p];
        cap = set_caps[p];
    }
    key[p] = coal_key(entry, off, cap, dev_bytes, align, sentinel);
}

// Sorted position i: eoff[i], ecap[i] its entry (0, 0 behind the well-formed
// ones), emax[i] the largest end before it in its workgroup, cmax the
// workgroup's largest; words[kCoalWValid] the well-formed entries (they are a
// prefix of the sorted order; the one thread at its end writes the word).
__global__ void __launch_bounds__(kCoalBlock)
coal_ends(const uint32_t *__restrict__ skey, const uint32_t *__restrict__ sidx,
          const uint64_t *__restrict__ set_offs, const uint64_t *__restrict__ set_caps, uint32_t n,
          uint32_t sentinel, uint64_t *__restrict__ eoff, uint64_t *__restrict__ ecap, uint64_t *__restrict__ emax,
          uint64_t *__restrict__ cmax, uint64_t *__restrict__ words)
{
    __shared__ uint64_t sh[kCoalBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    uint64_t off = 0, cap = 0;
    if (i < n) {
        const uint32_t p = sidx[i];
        const bool valid = skey[i] < sentinel && p < n;    // p < n holds by construction; no load outside the arrays
        if (valid) {
            off = set_offs[p];
            cap = set_caps[p];
        }
        eoff[i] = off;
        ecap[i] = cap;
        const bool next = i + 1 < n && skey[i + 1] < sentinel;
        if (valid && !next) {
            words[kCoalWValid] = i + 1;
        } else if (i == 0 && !valid) {
            words[kCoalWValid] = 0;
        }
    }
    uint64_t total;
    const uint64_t excl = block_max_excl(sh, threadIdx.x, off + cap, total);   // well-formed: no wrap
    if (i < n) {
        emax[i] = excl;
    }
    if (threadIdx.x == 0) {
        cmax[blockIdx.x] = total;
    }
}

// cmax[j] becomes the largest end before workgroup j.
__global__ void __launch_bounds__(kCoalBlock)
coal_mscan(uint64_t *__restrict__ cmax, uint32_t nb)
{
    __shared__ uint64_t sh[kCoalBlock];
    const uint32_t tid = threadIdx.x;
    uint64_t carry = 0;
    for (uint32_t base = 0; base < nb; base += kCoalBlock) {
        const uint32_t j = base + tid;
        uint64_t pass;
        const uint64_t excl = block_max_excl(sh, tid, j < nb ? cmax[j] : 0, pass);
        if (j < nb) {
            cmax[j] = max64(carry, excl);
        }
        carry = max64(carry, pass);
    }
}

// rank[i]: 2 * (the survivors before i in its workgroup) + 1 of a survivor, 0
// otherwise; csurv the workgroup's survivors.
__global__ void __launch_bounds__(kCoalBlock)
coal_survive(const uint32_t *__restrict__ skey, uint32_t n, uint32_t sentinel, const uint64_t *__restrict__ eoff,
             const uint64_t *__restrict__ emax, const uint64_t *__restrict__ cmax, uint32_t *__restrict__ rank,
             uint64_t *__restrict__ csurv)
{
    __shared__ uint64_t sh[kCoalBlock];
    const uint64_t i = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    bool surv = false;
    if (i < n) {
        surv = skey[i] < sentinel && !coal_collides(eoff[i], max64(cmax[blockIdx.x], emax[i]));
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, threadIdx.x, surv ? 1 : 0, total);
    if (i < n) {
        rank[i] = surv ? 2 * (uint32_t) excl + 1 : 0;
    }
    if (threadIdx.x == 0) {
        csurv[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(kCoalBlock)
coal_sscan(uint64_t *__restrict__ csurv, uint32_t nb, uint64_t *__restrict__ words)
{
    __shared__ uint64_t sh[kCoalBlock];
    const uint64_t all = totals_scan(sh, csurv, nb);
    if (threadIdx.x == 0) {
        words[kCoalWSurv] = all;
    }
}

// soff[s], scap[s]: survivor s, dense and in sorted order.
__global__ void __launch_bounds__(kCoalBlock)
coal_compact(uint32_t n, const uint32_t *__restrict__ rank, const uint64_t *__restrict__ csurv,
             const uint64_t *__restrict__ eoff, const uint64_t *__restrict__ ecap, uint64_t *__restrict__ soff,
             uint64_t *__restrict__ scap)
{
    const uint64_t i = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    if (i >= n) {
        return;
    }
    const uint32_t r = rank[i];
    if (r == 0) {
        return;
    }
    const uint64_t s = csurv[blockIdx.x] + (r >> 1);       // <= i
    if (s < n) {
        soff[s] = eoff[i];
        scap[s] = ecap[i];
    }
}

// code[s]: kCoalCand, kCoalStart; ocap[s] the survivor's own capacity; local[s]
// the run starts up to and including s in its workgroup, crun the workgroup's.
__global__ void __launch_bounds__(kCoalBlock)
coal_link(const uint64_t *__restrict__ words, const uint64_t *__restrict__ soff, const uint64_t *__restrict__ scap,
          const uint64_t *__restrict__ set, uint32_t target, uint64_t align, uint32_t *__restrict__ code,
          uint64_t *__restrict__ ocap, uint32_t *__restrict__ local, uint64_t *__restrict__ crun)
{
    __shared__ uint64_t sh[kCoalBlock];
    const uint64_t s = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    const uint64_t ns = words[kCoalWSurv];
    uint64_t start = 0;
    if (s < ns) {
        const uint64_t T = set[4 * target + kPoolCls], off = soff[s], cap = scap[s];
        const bool linked = s != 0 && coal_links(soff[s - 1], scap[s - 1], off, cap, T, align);
        start = linked ? 0 : 1;
        code[s] = (cap < T ? kCoalCand : 0) | (start ? kCoalStart : 0);
        ocap[s] = cap;
    }
    uint64_t total;
    const uint64_t excl = block_scan_excl(sh, threadIdx.x, start, total);
    if (s < ns) {
        local[s] = (uint32_t) (excl + start);
    }
    if (threadIdx.x == 0) {
        crun[blockIdx.x] = total;
    }
}

__global__ void __launch_bounds__(kCoalBlock)
coal_rscan(uint64_t *__restrict__ crun, uint32_t nb)
{
    __shared__ uint64_t sh[kCoalBlock];
    (void) totals_scan(sh, crun, nb);
}

// The walk of every run, by the thread of its first survivor.  The walks write
// kCoalGroup / kCoalAbsorbed into code words of their own run alone and leave
// the two bits this kernel's threads read as they are.
__global__ void __launch_bounds__(kCoalBlock)
coal_groups(const uint64_t *__restrict__ words, const uint64_t *__restrict__ soff, const uint64_t *__restrict__ scap,
            const uint64_t *__restrict__ crun, const uint32_t *__restrict__ local, const uint64_t *__restrict__ set,
            uint32_t target, uint64_t *ocap, uint32_t *code)
{
    const uint64_t s = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    const uint64_t ns = words[kCoalWSurv];
    if (s >= ns || (code[s] & (kCoalCand | kCoalStart)) != (kCoalCand | kCoalStart)) {
        return;
    }
    coal_walk_run(soff, scap, crun, local, ns, s, set[4 * target + kPoolCls], set[4 * target + kPoolAlign], ocap,
                  code);
}

// code[s] gains the output's class (kSetNone: no output, or classless); ord[s]
// its rank in its class inside its workgroup, tab the workgroup's K counts,
// ccnt its packed group / absorbed / classless counts.
__global__ void __launch_bounds__(kCoalBlock)
coal_class(const uint64_t *__restrict__ words, const uint64_t *__restrict__ soff, const uint64_t *__restrict__ ocap,
           const uint64_t *__restrict__ set, uint32_t n_cls, uint32_t nb, uint32_t *__restrict__ code,
           uint32_t *__restrict__ ord, uint64_t *__restrict__ tab, uint64_t *__restrict__ ccnt)
{
    __shared__ uint32_t wcount[kSetWaves * kPoolSetMax];
    __shared__ uint64_t sh[kCoalBlock];
    const uint64_t s = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    const uint64_t ns = words[kCoalWSurv];
    uint32_t c = 0, cls = kSetNone;
    uint64_t packed = 0;
    if (s < ns) {
        c = code[s];
        const bool out = !(c & kCoalAbsorbed);
        if (out) {
            cls = set_release_class(set, n_cls, soff[s], ocap[s]);
        }
        packed = coal_cnt_pack((c & kCoalGroup) ? 1 : 0, (c & (kCoalGroup | kCoalAbsorbed)) ? 1 : 0,
                               out && cls == kSetNone ? 1 : 0);
    }
    const uint32_t rank = class_rank(wcount, cls, tab, nb);
    uint64_t total;
    (void) block_scan_excl(sh, threadIdx.x, packed, total);
    if (s < ns) {
        ord[s] = rank;
        code[s] = c | (cls << kSetClsShift);
    }
    if (threadIdx.x == 0) {
        ccnt[blockIdx.x] = total;
    }
}

// The sum of field f of the nb packed words, over the workgroup.
__device__ __forceinline__ uint64_t field_sum(uint64_t *sh, const uint64_t *__restrict__ ccnt, uint32_t nb, uint32_t f)
{
    uint64_t mine = 0, total;
    for (uint32_t j = threadIdx.x; j < nb; j += kCoalBlock) {
        mine += coal_cnt_field(ccnt[j], f);
    }
    (void) block_scan_excl(sh, threadIdx.x, mine, total);
    return total;
}

__global__ void __launch_bounds__(kCoalBlock)
coal_final(uint64_t *tab, uint32_t nb, const uint64_t *__restrict__ set, uint32_t n_cls, uint64_t stride,
           const uint64_t *__restrict__ ccnt, uint64_t *words, uint64_t *__restrict__ total)
{
    __shared__ uint64_t sh[kCoalBlock];
    __shared__ uint64_t count[kPoolSetMax];
    class_scan(sh, count, tab, nb, n_cls);
    const uint64_t groups = field_sum(sh, ccnt, nb, 0), absorbed = field_sum(sh, ccnt, nb, 1),
                   classless = field_sum(sh, ccnt, nb, 2);
    if (threadIdx.x == 0) {
        uint64_t mask;
        words[kCoalWVerdict] = coal_totals(set, n_cls, set_sound(set, n_cls, stride), count, words[kCoalWValid],
                                           words[kCoalWSurv], groups, absorbed, classless, total, mask);
        words[kCoalWMask] = mask;
        for (uint32_t k = 0; k < n_cls; ++k) {
            words[kCoalWCount + k] = count[k];
        }
    }
}

// C6's second half.  Reads scratch alone: no word of the set or its arrays.
__global__ void __launch_bounds__(kCoalBlock)
coal_commit(const uint64_t *__restrict__ words, const uint64_t *__restrict__ soff, const uint64_t *__restrict__ ocap,
            const uint32_t *__restrict__ code, const uint32_t *__restrict__ ord, const uint64_t *__restrict__ tab,
            uint32_t nb, uint32_t n_cls, uint64_t stride, uint64_t *__restrict__ set_offs,
            uint64_t *__restrict__ set_caps, uint64_t *__restrict__ set)
{
    const uint64_t s = (uint64_t) blockIdx.x * kCoalBlock + threadIdx.x;
    if (words[kCoalWVerdict] != kCoalOk) {
        return;
    }
    if (s < n_cls && ((words[kCoalWMask] >> s) & 1u)) {
        set[4 * s + kPoolCount] = words[kCoalWCount + s];  // the word's one writer
    }
    if (s >= words[kCoalWSurv]) {
        return;
    }
    const uint32_t c = code[s], cls = (c >> kSetClsShift) & 15u;
    if ((c & kCoalAbsorbed) || cls >= n_cls) {
        return;
    }
    const uint64_t at = tab[set_tab_at(cls, blockIdx.x, nb)] + ord[s];
    if (at < stride) {                            // at < c_k <= the class's capacity <= stride: inside the arrays
        set_offs[cls * stride + at] = soff[s];
        set_caps[cls * stride + at] = ocap[s];
    }
}

struct CoalArgs {
    cio_dev_writer *w;
    uint64_t dev_bytes;
    uint64_t *offs, *caps, *words;
    size_t n_cls;
    uint64_t stride;
    size_t target;
    uint64_t align;
    int flags;
    uint64_t *total;
};

// The argument checks, before any device call: the values first, then the
// pointers, then what the writer holds.
int check_coalesce(const CoalArgs &a)
{
    if (a.flags & ~CIOA_COALESCE_DRY) {
        return fail("cio_file_coalesce_set_dev: unknown flags");
    }
    if (a.n_cls < 2 || a.n_cls > CIOA_POOL_SET_MAX) {
        return fail("cio_file_coalesce_set_dev: n_cls must be in 2 .. 8");
    }
    if (a.target < 1 || a.target > a.n_cls - 1) {
        return fail("cio_file_coalesce_set_dev: target must be in 1 .. n_cls - 1");
    }
    if (a.stride == 0) {
        return fail("cio_file_coalesce_set_dev: stride must not be 0");
    }
    if (a.align == 0 || (a.align & (a.align - 1)) != 0 || a.align > 4096) {
        return fail("cio_file_coalesce_set_dev: align must be a power of two in 1 .. 4096");
    }
    if (a.dev_bytes == 0) {
        return fail("cio_file_coalesce_set_dev: dev_bytes must not be 0");
    }
    if ((a.dev_bytes - 1) / a.align >= 0xffffffffull) {
        return fail("cio_file_coalesce_set_dev: dev_bytes / align does not fit the 32-bit sort key");
    }
    if (!a.w) {
        return fail("cio_file_coalesce_set_dev: null writer");
    }
    if (!a.offs || !a.caps || !a.words || !a.total) {
        return fail("cio_file_coalesce_set_dev: null pointer");
    }
    if (a.stride > a.w->max_chunks / a.n_cls) {
        return fail("cio_file_coalesce_set_dev: more set entries than the writer was created for");
    }
    return 0;
}

int launch_coalesce(const CoalArgs &a, hipStream_t s)
{
    cio_dev_writer *w = a.w;
    const uint32_t n = (uint32_t) (a.n_cls * a.stride), nb = blocks_of(n, kCoalBlock), n_cls = (uint32_t) a.n_cls;
    const uint32_t sentinel = (uint32_t) coal_key_bound(a.dev_bytes, a.align), target = (uint32_t) a.target;
    // writer arenas: newlen the keys, then the survivors' codes; skey / sidx the sort's; soff / slen the sorted
    // entries; groom the ends' prefix maxima; seed the survivor ranks, then the outputs' ranks in their classes;
    // roff / rlen the survivors; gcap the outputs' capacities; crc the run starts; stab, once the sort is done, the
    // class table, the per-call words and the four columns
    uint64_t *tab = reinterpret_cast<uint64_t *>(w->stab);
    uint64_t *words = tab + set_words_at(nb);
    uint64_t *cmax = tab + coal_col_at(kCoalColMax, nb), *csurv = tab + coal_col_at(kCoalColSurv, nb);
    uint64_t *crun = tab + coal_col_at(kCoalColRun, nb), *ccnt = tab + coal_col_at(kCoalColCnt, nb);
    hipLaunchKernelGGL(coal_gather, dim3(nb), dim3(kCoalBlock), 0, s, a.offs, a.caps, a.words, n_cls, a.stride, n,
                       a.dev_bytes, a.align, sentinel, w->newlen);
    HIP_TRY(hipGetLastError(), "cio_file_coalesce_set_dev: gather kernel launch");
    int sorted = 0;
    if (sort_launch(w, w->newlen, sentinel, n, &sorted, s) != CIO_OK) {
        return CIO_ERROR;
    }
    hipLaunchKernelGGL(coal_ends, dim3(nb), dim3(kCoalBlock), 0, s, w->skey[sorted], w->sidx[sorted], a.offs, a.caps,
                       n, sentinel, w->soff, w->slen, w->groom, cmax, words);
    hipLaunchKernelGGL(coal_mscan, dim3(1), dim3(kCoalBlock), 0, s, cmax, nb);
    hipLaunchKernelGGL(coal_survive, dim3(nb), dim3(kCoalBlock), 0, s, w->skey[sorted], n, sentinel, w->soff,
                       w->groom, cmax, w->seed, csurv);
    hipLaunchKernelGGL(coal_sscan, dim3(1), dim3(kCoalBlock), 0, s, csurv, nb, words);
    hipLaunchKernelGGL(coal_compact, dim3(nb), dim3(kCoalBlock), 0, s, n, w->seed, csurv, w->soff, w->slen, w->roff,
                       w->rlen);
    hipLaunchKernelGGL(coal_link, dim3(nb), dim3(kCoalBlock), 0, s, words, w->roff, w->rlen, a.words, target, a.align,
                       w->newlen, w->gcap, w->crc, crun);
    hipLaunchKernelGGL(coal_rscan, dim3(1), dim3(kCoalBlock), 0, s, crun, nb);
    hipLaunchKernelGGL(coal_groups, dim3(nb), dim3(kCoalBlock), 0, s, words, w->roff, w->rlen, crun, w->crc, a.words,
                       target, w->gcap, w->newlen);
    hipLaunchKernelGGL(coal_class, dim3(nb), dim3(kCoalBlock), 0, s, words, w->roff, w->gcap, a.words, n_cls, nb,
                       w->newlen, w->seed, tab, ccnt);
    hipLaunchKernelGGL(coal_final, dim3(1), dim3(kCoalBlock), 0, s, tab, nb, a.words, n_cls, a.stride, ccnt, words,
                       a.total);
    if (!(a.flags & CIOA_COALESCE_DRY)) {
        hipLaunchKernelGGL(coal_commit, dim3(nb), dim3(kCoalBlock), 0, s, words, w->roff, w->gcap, w->newlen, w->seed,
                           tab, nb, n_cls, a.stride, a.offs, a.caps, a.words);
    }
    HIP_TRY(hipGetLastError(), "cio_file_coalesce_set_dev: kernels launch");
    return CIO_OK;
}

}  // namespace

extern "C" {

int cio_file_coalesce_set_dev(cio_dev_writer *w, uint64_t dev_bytes,
                              uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                              size_t n_cls, uint64_t stride, size_t target, uint64_t align, int flags,
                              uint64_t *dev_total, void *stream)
{
    const CoalArgs a = {w, dev_bytes, dev_set_offs, dev_set_caps, dev_set, n_cls, stride, target, align, flags,
                        dev_total};
    const int rc = check_coalesce(a);
    if (rc != 0) {
        return rc;
    }
    return launch_coalesce(a, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
