// gpu_runtime.hip -- the process-wide GPU runtime of libchunkio_amd.so: the
// per-thread error message, per-device constant tables, CRC-32 plans (the
// choices of crc_plan.cpp, allocated and uploaded), the plan ring, and the
// event / stream helpers.  Host code only: no kernel lives here (the CRC
// kernels and their launchers are in crc32_gpu.hip).  C ABI in
// include/chunkio_amd/cio_crc32_gpu.h.

#include <hip/hip_runtime.h>
#include <stdint.h>
#include <string.h>
#include <stdio.h>
#include <stdlib.h>
#include <memory>
#include <mutex>
#include <vector>
#include <string>
#include <algorithm>

#include "cio_gpu_internal.h"

using namespace cioa;

namespace cioa {

thread_local std::string g_err;

int fail(const char *what, hipError_t e)
{
    char buf[512];
    if (e != hipSuccess) {
        snprintf(buf, sizeof(buf), "%s: %s", what, hipGetErrorString(e));
    } else {
        snprintf(buf, sizeof(buf), "%s", what);
    }
    g_err = buf;
    return CIO_ERROR;
}

int fail_who(const char *who, const char *what)
{
    const std::string msg = std::string(who) + ": " + what;
    return fail(msg.c_str());
}

int mark(const SectionEvents *ev, int section, bool begin, hipStream_t s)
{
    if (ev && ev->section == section) {
        HIP_TRY(hipEventRecord(begin ? ev->ev0 : ev->ev1, s), "hipEventRecord");
    }
    return CIO_OK;
}

}  // namespace cioa

extern "C" int cioa_fail_msg(const char *what, const char *detail)
{
    g_err = std::string(what) + (detail ? std::string(": ") + detail : std::string());
    return CIO_ERROR;
}

namespace cioa {

// One DeviceState per HIP device, allocated once and never moved: plans and
// in-flight host batches keep a pointer to it (a growing vector
// here reallocated under them when a second device was first used).
std::mutex g_mu;
std::unique_ptr<DeviceState> g_dev[kMaxDev];

int device_state(DeviceState **out)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "hipGetDevice");
    if (dev < 0 || dev >= kMaxDev) {
        return fail("device ordinal out of range");
    }
    std::lock_guard<std::mutex> lk(g_mu);
    if (!g_dev[dev]) {
        g_dev[dev].reset(new DeviceState());
    }
    DeviceState &st = *g_dev[dev];
    if (!st.ready) {
        hipDeviceProp_t prop;
        HIP_TRY(hipGetDeviceProperties(&prop, dev), "hipGetDeviceProperties");
        if (strncmp(prop.gcnArchName, "gfx950", 6) != 0) {
            char msg[256];
            snprintf(msg, sizeof(msg), "chunkio_amd kernels are built for gfx950, device is %s",
                     prop.gcnArchName);
            return fail(msg);
        }
        st.cus = prop.multiProcessorCount;
        static uint32_t slice[4][256], shift[4][256];
        std::vector<uint32_t> x8(kX8Count);
        cioa_gen_slice4(slice);
        cioa_gen_shift_table(shift, (uint64_t) (kStep - kGran));
        cioa_gen_xpow8_table(x8.data(), kX8Count, 1);
        HIP_TRY(hipMalloc(&st.slice, sizeof(slice)), "hipMalloc(slice)");
        HIP_TRY(hipMalloc(&st.shift, sizeof(shift)), "hipMalloc(shift)");
        HIP_TRY(hipMalloc(&st.x8, kX8Count * sizeof(uint32_t)), "hipMalloc(x8)");
        HIP_TRY(hipMemcpy(st.slice, slice, sizeof(slice), hipMemcpyHostToDevice), "upload slice");
        HIP_TRY(hipMemcpy(st.shift, shift, sizeof(shift), hipMemcpyHostToDevice), "upload shift");
        HIP_TRY(hipMemcpy(st.x8, x8.data(), kX8Count * sizeof(uint32_t), hipMemcpyHostToDevice),
                "upload x8");
        // x^-1 = (P(x) - 1) / x, reflected: P's low coefficients moved down one power.
        std::vector<uint32_t> xinv8(kStep);
        uint32_t xm8 = 0x80000000u;
        for (int i = 0; i < 8; ++i) {
            xm8 = cioa_multmodp(xm8, (CIOA_POLY << 1) | 1u);
        }
        xinv8[0] = 0x80000000u;
        for (int d = 1; d < kStep; ++d) {
            xinv8[d] = cioa_multmodp(xinv8[d - 1], xm8);
        }
        HIP_TRY(hipMalloc(&st.xinv8, kStep * sizeof(uint32_t)), "hipMalloc(xinv8)");
        HIP_TRY(hipMemcpy(st.xinv8, xinv8.data(), kStep * sizeof(uint32_t), hipMemcpyHostToDevice),
                "upload xinv8");
        st.ready = true;
    }
    *out = &st;
    return CIO_OK;
}

}  // namespace cioa

extern "C" {

const char *cio_gpu_last_error(void)
{
    return g_err.c_str();
}

const char *cio_gpu_version(void)
{
#define CIO_STR2(x) #x
#define CIO_STR(x) CIO_STR2(x)
    return "chunkio_amd crc32 v9 gfx950 stream(l64-lanes permlane-transpose issue-ahead<=64steps wave-aligned pre-shift prio-rotate "
           "coalesced-nt division-free-start slice4-lds32x perm direct-whole preshifted-partials wg-lds-fold "
           "head-align=" CIO_STR(CIO_HEAD_ALIGN) ") "
           "small(4x16B dpp-reduce bitop3-fold prio-rotate) "
           "host(nt-staging graduated-groups pread-bounce multi-device vpclmul-crc_update small-batch-route) "
           "sha1(2-schedule-waves 4-block-handover continuation)";
}

int cio_gpu_init(void)
{
    DeviceState *st;
    return device_state(&st);
}

void cio_crc32_plan_destroy(cio_crc32_plan *p)
{
    if (!p) {
        return;
    }
    (void) hipFree(p->desc);
    (void) hipFree(p->wstart);
    (void) hipFree(p->tiny);
    (void) hipFree(p->partials);
    (void) hipFree(p->counters);
    (void) hipFree(p->pfac);
    (void) hipFree(p->afac);
    (void) hipFree(p->stamps);
    delete p;
}

// The plan crc_plan.cpp chooses for the current device (plan_choose: kernel,
// grid, work partition), allocated and uploaded.
int cio_crc32_plan_create(cio_crc32_plan **out, const uint64_t *offs, const uint64_t *lens, size_t n)
{
    if (!out || (n && (!offs || !lens))) {
        return fail("cio_crc32_plan_create: null argument");
    }
    if (n >= 0xffffffffull) {
        return fail("cio_crc32_plan_create: too many chunks");
    }
    *out = nullptr;
    DeviceState *st;
    if (device_state(&st) != CIO_OK) {
        return CIO_ERROR;
    }
    cio_crc32_plan *p = new cio_crc32_plan();
    plan_init(p, st, n);
    PlanHost ph;
    if (const char *err = plan_choose(p, ph, offs, lens, n)) {
        delete p;
        return fail(err);
    }
    if (const char *r = cioa_diag_getenv("CIO_GPU_STAMPS")) {
        if (atoi(r) > 0 && hipMalloc(&p->stamps, (size_t) p->W * kStampWords * sizeof(unsigned long long)) != hipSuccess) {
            p->stamps = nullptr;
        }
    }
    hipError_t e;
    const size_t npart = ph.pfac.size();
    if ((e = hipMalloc(&p->desc, ph.desc.size() * sizeof(ChunkDesc))) != hipSuccess ||
        (e = hipMalloc(&p->wstart, ph.ws.size() * sizeof(WaveStart))) != hipSuccess ||
        (e = hipMalloc(&p->tiny, std::max<size_t>(1, ph.tiny.size()) * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&p->partials, npart * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMalloc(&p->counters, std::max<size_t>(1, n) * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMalloc(&p->pfac, npart * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemcpy(p->desc, ph.desc.data(), ph.desc.size() * sizeof(ChunkDesc), hipMemcpyHostToDevice)) != hipSuccess ||
        (e = hipMemcpy(p->wstart, ph.ws.data(), ph.ws.size() * sizeof(WaveStart), hipMemcpyHostToDevice)) != hipSuccess ||
        (ph.tiny.size() && (e = hipMemcpy(p->tiny, ph.tiny.data(), ph.tiny.size() * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess) ||
        (e = hipMemset(p->partials, 0, npart * sizeof(unsigned long long))) != hipSuccess ||
        (e = hipMemset(p->counters, 0, std::max<size_t>(1, n) * sizeof(uint32_t))) != hipSuccess ||
        (e = hipMemcpy(p->pfac, ph.pfac.data(), npart * sizeof(uint32_t), hipMemcpyHostToDevice)) != hipSuccess ||
        // (a wave-aligned plan launches with afac alone; the other arrays stay, unused)
        (p->aligned && ((e = hipMalloc(&p->afac, ph.afac.size() * sizeof(uint32_t))) != hipSuccess ||
                        (e = hipMemcpy(p->afac, ph.afac.data(), ph.afac.size() * sizeof(uint32_t),
                                       hipMemcpyHostToDevice)) != hipSuccess))) {
        cio_crc32_plan_destroy(p);
        return fail("cio_crc32_plan_create: device allocation/upload", e);
    }
    *out = p;
    return CIO_OK;
}

uint64_t cio_crc32_plan_bytes(const cio_crc32_plan *p)
{
    return p ? p->bytes : 0;
}

uint32_t cio_crc32_plan_workgroups(const cio_crc32_plan *p)
{
    return p ? p->grid : 0;
}

const char *cio_crc32_plan_kernel(const cio_crc32_plan *p)
{
    return (p && p->small) ? "crc32_small_kernel" : "crc32_stream_kernel";
}

int cio_crc32_plan_aligned(const cio_crc32_plan *p)
{
    return (p && p->aligned) ? 1 : 0;
}

int cio_crc32_plan_exec_events(const cio_crc32_plan *p, const void *dev_base,
                               const uint32_t *dev_seeds, uint32_t *dev_out, void *stream,
                               void *ev_piece_start, void *ev_piece_stop)
{
    return plan_exec_impl(p, dev_base, dev_seeds, dev_out, nullptr,
                          reinterpret_cast<hipStream_t>(stream),
                          reinterpret_cast<hipEvent_t>(ev_piece_start),
                          reinterpret_cast<hipEvent_t>(ev_piece_stop));
}

int cio_crc32_plan_exec(const cio_crc32_plan *p, const void *dev_base, const uint32_t *dev_seeds,
                        uint32_t *dev_out, void *stream)
{
    return plan_exec_impl(p, dev_base, dev_seeds, dev_out, nullptr,
                          reinterpret_cast<hipStream_t>(stream));
}

int cio_crc32_batch_dev(const void *dev_base, const uint64_t *offs, const uint64_t *lens,
                        const uint32_t *dev_seeds, uint32_t *dev_out, size_t n, void *stream)
{
    cio_crc32_plan *p = nullptr;
    if (cio_crc32_plan_create(&p, offs, lens, n) != CIO_OK) {
        return CIO_ERROR;
    }
    int rc = cio_crc32_plan_exec(p, dev_base, dev_seeds, dev_out, stream);
    if (rc == CIO_OK) {
        hipError_t e = hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream));
        if (e != hipSuccess) {
            rc = fail("cio_crc32_batch_dev: stream sync", e);
        }
    }
    cio_crc32_plan_destroy(p);
    return rc;
}

/* A ring of `depth` plans of one geometry, each on its own stream (see the
 * header): consecutive batches overlap at their kernel edges. */
struct cio_crc32_ring {
    std::vector<cio_crc32_plan *> plans;
    std::vector<hipStream_t> streams;
    std::vector<hipEvent_t> ready, done;    // per slot: caller's inputs, slot's last batch
    std::vector<bool> pending;              // slot has work the caller has not joined
    unsigned next = 0;
    int dev = 0;                            // device the plans and streams live on
};

// Makes `dev` current for one scope and restores the caller's device after:
// a ring's plans, streams and events belong to the device current at create.
struct RingDevice {
    int prev = -1;
    hipError_t e = hipSuccess;
    explicit RingDevice(int dev)
    {
        if ((e = hipGetDevice(&prev)) == hipSuccess && prev != dev) {
            e = hipSetDevice(dev);
        }
    }
    ~RingDevice()
    {
        int cur = -1;
        if (prev >= 0 && hipGetDevice(&cur) == hipSuccess && cur != prev) {
            (void) hipSetDevice(prev);
        }
    }
};

void cio_crc32_ring_destroy(cio_crc32_ring *r)
{
    if (!r) {
        return;
    }
    RingDevice on(r->dev);
    for (hipStream_t st : r->streams) {
        if (st) (void) hipStreamSynchronize(st);
    }
    for (size_t i = 0; i < r->plans.size(); i++) {
        cio_crc32_plan_destroy(r->plans[i]);
        if (r->ready[i]) (void) hipEventDestroy(r->ready[i]);
        if (r->done[i]) (void) hipEventDestroy(r->done[i]);
        if (r->streams[i]) (void) hipStreamDestroy(r->streams[i]);
    }
    delete r;
}

int cio_crc32_ring_create(cio_crc32_ring **out, const uint64_t *offs, const uint64_t *lens, size_t n, int depth)
{
    if (!out) {
        return fail("cio_crc32_ring_create: null argument");
    }
    *out = nullptr;
    if (depth < 1 || depth > 8) {
        return fail("cio_crc32_ring_create: depth must be 1..8");
    }
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "cio_crc32_ring_create: hipGetDevice");
    cio_crc32_ring *r = new cio_crc32_ring();
    r->dev = dev;
    r->plans.assign((size_t) depth, nullptr);
    r->streams.assign((size_t) depth, nullptr);
    r->ready.assign((size_t) depth, nullptr);
    r->done.assign((size_t) depth, nullptr);
    r->pending.assign((size_t) depth, false);
    for (int i = 0; i < depth; i++) {
        if (cio_crc32_plan_create(&r->plans[(size_t) i], offs, lens, n) != CIO_OK) {
            cio_crc32_ring_destroy(r);
            return CIO_ERROR;    // (the plan's message stands)
        }
        hipError_t e = hipStreamCreateWithFlags(&r->streams[(size_t) i], hipStreamNonBlocking);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&r->ready[(size_t) i], hipEventDisableTiming);
        if (e == hipSuccess) e = hipEventCreateWithFlags(&r->done[(size_t) i], hipEventDisableTiming);
        if (e != hipSuccess) {
            cio_crc32_ring_destroy(r);
            return fail("cio_crc32_ring_create", e);
        }
    }
    *out = r;
    return CIO_OK;
}

int cio_crc32_ring_exec(cio_crc32_ring *r, const void *dev_base, const uint32_t *dev_seeds, uint32_t *dev_out,
                        void *stream)
{
    if (!r) {
        return fail("cio_crc32_ring_exec: null ring");
    }
    RingDevice on(r->dev);
    HIP_TRY(on.e, "cio_crc32_ring_exec: hipSetDevice");
    const size_t i = r->next % r->plans.size();
    const hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
    // the batch waits for everything the caller queued before it (its inputs);
    // the slot's stream orders it after the slot's previous batch (scratch reuse)
    HIP_TRY(hipEventRecord(r->ready[i], caller), "cio_crc32_ring_exec: hipEventRecord");
    HIP_TRY(hipStreamWaitEvent(r->streams[i], r->ready[i], 0), "cio_crc32_ring_exec: hipStreamWaitEvent");
    if (plan_exec_impl(r->plans[i], dev_base, dev_seeds, dev_out, nullptr, r->streams[i]) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipEventRecord(r->done[i], r->streams[i]), "cio_crc32_ring_exec: hipEventRecord");
    r->pending[i] = true;
    r->next++;      // only a batch that was queued moves the ring on
    return CIO_OK;
}

int cio_crc32_ring_join(cio_crc32_ring *r, void *stream)
{
    if (!r) {
        return fail("cio_crc32_ring_join: null ring");
    }
    RingDevice on(r->dev);
    HIP_TRY(on.e, "cio_crc32_ring_join: hipSetDevice");
    const hipStream_t caller = reinterpret_cast<hipStream_t>(stream);
    for (size_t i = 0; i < r->plans.size(); i++) {
        if (r->pending[i]) {
            HIP_TRY(hipStreamWaitEvent(caller, r->done[i], 0), "cio_crc32_ring_join: hipStreamWaitEvent");
            r->pending[i] = false;
        }
    }
    return CIO_OK;
}

void *cio_gpu_event_create(void)
{
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) {
        return nullptr;
    }
    return ev;
}

void cio_gpu_event_destroy(void *ev)
{
    if (ev) {
        (void) hipEventDestroy(reinterpret_cast<hipEvent_t>(ev));
    }
}

int cio_gpu_event_record(void *ev, void *stream)
{
    HIP_TRY(hipEventRecord(reinterpret_cast<hipEvent_t>(ev), reinterpret_cast<hipStream_t>(stream)),
            "hipEventRecord");
    return CIO_OK;
}

float cio_gpu_event_elapsed_ms(void *start, void *stop)
{
    float ms = -1.0f;
    if (hipEventSynchronize(reinterpret_cast<hipEvent_t>(stop)) != hipSuccess) {
        return -1.0f;
    }
    if (hipEventElapsedTime(&ms, reinterpret_cast<hipEvent_t>(start),
                            reinterpret_cast<hipEvent_t>(stop)) != hipSuccess) {
        return -1.0f;
    }
    return ms;
}

int cio_gpu_stream_sync(void *stream)
{
    HIP_TRY(hipStreamSynchronize(reinterpret_cast<hipStream_t>(stream)), "hipStreamSynchronize");
    return CIO_OK;
}

}  // extern "C"
