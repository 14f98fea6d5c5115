// persist_host.hip -- the host pipelines that bring chunk images in HBM down to
// chunk files and up again (cio_file_load_paths_dev, cio_file_store_paths_dev;
// include/chunkio_amd/cio_persist_dev.h).  No kernel lives here:
// the device work is the existing calls (cio_file_verify_batch_dev,
// cio_file_alloc_set_batch_dev, cio_file_read_packed_batch_dev) and
// alloc_set_gpu.hip's load_launch_back.  The round arithmetic is
// persist_plan.h, the text tools/persist_check.cpp runs on the host.
//
// Both calls are host-synchronous and use the device stage whole: a round's
// file I/O does not overlap the previous round's device chain.  The pinned
// staging (sized to the largest round a call plans, not to the stage) and the
// per-round device arrays are kept between calls -- one set per process, grown
// on demand, under a mutex: two persist calls do not overlap --
// until cio_file_persist_trim() frees them.  The host threads of a call are
// started once per call and serve every round of it.

#include <hip/hip_runtime.h>
#include <stdint.h>

#include <atomic>
#include <chrono>
#include <condition_variable>
#include <functional>
#include <errno.h>
#include <fcntl.h>
#include <mutex>
#include <sys/stat.h>
#include <thread>
#include <unistd.h>
#include <vector>

#include "cio_gpu_internal.h"
#include "persist_plan.h"
#include "chunkio_amd/cio_persist_dev.h"
#include "chunkio_amd/cio_verify.h"

using namespace cioa;

namespace {

// What a persist call keeps between calls.
struct Scratch {
    std::mutex mu;
    uint8_t *pinned = nullptr;                // the round's bytes, then its small arrays
    size_t pinned_cap = 0;
    uint8_t *dev = nullptr;                   // the round's device arrays
    size_t dev_cap = 0;
    int dev_id = -1;
};
Scratch g_scratch;

int pinned_reserve(Scratch &sc, size_t bytes)
{
    if (bytes <= sc.pinned_cap) {
        return CIO_OK;
    }
    if (sc.pinned) {
        (void) hipHostFree(sc.pinned);
        sc.pinned = nullptr;
        sc.pinned_cap = 0;
    }
    HIP_TRY(hipHostMalloc(reinterpret_cast<void **>(&sc.pinned), bytes, hipHostMallocPortable),
            "persist: pinned staging allocation");
    sc.pinned_cap = bytes;
    return CIO_OK;
}

int dev_reserve(Scratch &sc, size_t bytes)
{
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev), "persist: hipGetDevice");
    if (dev == sc.dev_id && bytes <= sc.dev_cap) {
        return CIO_OK;
    }
    if (sc.dev) {
        (void) hipFree(sc.dev);
        sc.dev = nullptr;
        sc.dev_cap = 0;
    }
    HIP_TRY(hipMalloc(reinterpret_cast<void **>(&sc.dev), bytes), "persist: device scratch allocation");
    sc.dev_cap = bytes;
    sc.dev_id = dev;
    return CIO_OK;
}

// The host threads of one call: at most kPersistThreads - 1 beside the caller,
// started once and kept for every round of the call.  run(count, fn) calls
// fn(k) for every k in [0, count), items claimed one by one through a counter,
// and returns when all are done.
class Workers {
public:
    explicit Workers(size_t widest)
    {
        const size_t extra = widest < (size_t) kPersistThreads ? (widest ? widest - 1 : 0)
                                                               : (size_t) kPersistThreads - 1;
        pool_.reserve(extra);
        for (size_t t = 0; t < extra; ++t) {
            pool_.emplace_back([this] { loop(); });
        }
    }
    ~Workers()
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            stop_ = true;
        }
        cv_.notify_all();
        for (std::thread &t : pool_) {
            t.join();
        }
    }
    void run(size_t count, const std::function<void(size_t)> &fn)
    {
        {
            std::lock_guard<std::mutex> lk(mu_);
            fn_ = &fn;
            count_ = count;
            next_.store(0);
            busy_ = pool_.size();
            ++job_;
        }
        cv_.notify_all();
        work();
        std::unique_lock<std::mutex> lk(mu_);
        done_.wait(lk, [this] { return busy_ == 0; });
        fn_ = nullptr;
    }

private:
    void work()
    {
        for (size_t k = next_.fetch_add(1); k < count_; k = next_.fetch_add(1)) {
            (*fn_)(k);
        }
    }
    void loop()
    {
        uint64_t seen = 0;
        for (;;) {
            {
                std::unique_lock<std::mutex> lk(mu_);
                cv_.wait(lk, [&] { return stop_ || job_ != seen; });
                if (stop_) {
                    return;
                }
                seen = job_;
            }
            work();
            {
                std::lock_guard<std::mutex> lk(mu_);
                --busy_;
            }
            done_.notify_one();
        }
    }
    std::vector<std::thread> pool_;
    std::mutex mu_;
    std::condition_variable cv_, done_;
    const std::function<void(size_t)> *fn_ = nullptr;
    size_t count_ = 0, busy_ = 0;
    std::atomic<size_t> next_{0};
    uint64_t job_ = 0;
    bool stop_ = false;
};

// What the last load and the last store of the process spent where
// (cioa_debug_persist_timing): wall-clock seconds of the host parts, event
// milliseconds of the device parts, summed over the call's rounds.
struct PersistTiming {
    double rounds = 0, files_s = 0, copy_ms = 0, chain_ms = 0, wait_s = 0, query_s = 0;
};
PersistTiming g_load_t, g_store_t;

double now_s()
{
    return std::chrono::duration<double>(std::chrono::steady_clock::now().time_since_epoch()).count();
}

// Three events around the two device parts of a round (the transfer, the
// chain), created once per call.
struct RoundEvents {
    hipEvent_t e[3] = {nullptr, nullptr, nullptr};
    bool ok = false;
    RoundEvents()
    {
        ok = hipEventCreate(&e[0]) == hipSuccess && hipEventCreate(&e[1]) == hipSuccess &&
             hipEventCreate(&e[2]) == hipSuccess;
    }
    ~RoundEvents()
    {
        for (hipEvent_t x : e) {
            if (x) (void) hipEventDestroy(x);
        }
    }
    void mark(int k, hipStream_t s) { if (ok) (void) hipEventRecord(e[k], s); }
    void add(PersistTiming &t, bool copy_first)
    {
        float a = 0, b = 0;
        if (ok && hipEventElapsedTime(&a, e[0], e[1]) == hipSuccess &&
            hipEventElapsedTime(&b, e[1], e[2]) == hipSuccess) {
            t.copy_ms += copy_first ? a : b;
            t.chain_ms += copy_first ? b : a;
        }
    }
};

// All len bytes at off of fd into p; false on an error or a short file.
bool pread_all(int fd, uint8_t *p, uint64_t len, uint64_t off)
{
    while (len != 0) {
        const ssize_t r = pread(fd, p, len, (off_t) off);
        if (r < 0 && errno == EINTR) {
            continue;
        }
        if (r <= 0) {
            return false;
        }
        p += r;
        off += (uint64_t) r;
        len -= (uint64_t) r;
    }
    return true;
}

bool pwrite_all(int fd, const uint8_t *p, uint64_t len)
{
    uint64_t off = 0;
    while (len != 0) {
        const ssize_t r = pwrite(fd, p, len, (off_t) off);
        if (r < 0 && errno == EINTR) {
            continue;
        }
        if (r <= 0) {
            return false;
        }
        p += r;
        off += (uint64_t) r;
        len -= (uint64_t) r;
    }
    return true;
}

// File `path` of exactly `size` bytes into p.
bool read_file(const char *path, uint8_t *p, uint64_t size)
{
    const int fd = open(path, O_RDONLY | O_CLOEXEC);
    if (fd < 0) {
        return false;
    }
    struct stat sb;
    const bool ok = fstat(fd, &sb) == 0 && (uint64_t) sb.st_size == size && pread_all(fd, p, size, 0);
    (void) close(fd);
    return ok;
}

// The chunk file of one image: its used bytes, then zeros up to file_size from
// ftruncate.  A failure leaves no partial file.
bool write_file(const char *path, const uint8_t *p, uint64_t used, uint64_t file_size, bool sync)
{
    const int fd = open(path, O_WRONLY | O_CREAT | O_TRUNC | O_CLOEXEC, 0644);
    if (fd < 0) {
        return false;
    }
    bool ok = pwrite_all(fd, p, used < file_size ? used : file_size) && ftruncate(fd, (off_t) file_size) == 0;
    if (ok && sync) {
        ok = fdatasync(fd) == 0;
    }
    if (close(fd) != 0) {
        ok = false;
    }
    if (!ok) {
        (void) unlink(path);
    }
    return ok;
}

// [first, last) of every round: the rounds are runs of consecutive indices.
std::vector<std::pair<size_t, size_t>> round_ranges(const std::vector<uint32_t> &round_of, uint32_t rounds)
{
    std::vector<std::pair<size_t, size_t>> out(rounds, std::make_pair((size_t) 0, (size_t) 0));
    for (size_t i = 0; i < round_of.size(); ++i) {
        const uint32_t r = round_of[i];
        if (r == kPersistNoRound) {
            continue;
        }
        if (out[r].second == 0) {
            out[r].first = i;
        }
        out[r].second = i + 1;
    }
    return out;
}

size_t up8(size_t x)
{
    return (x + 7) & ~(size_t) 7;
}

const char kLoad[] = "cio_file_load_paths_dev";
const char kStore[] = "cio_file_store_paths_dev";

// ---------------------------------------------------------------- load

struct LoadArgs {
    cio_dev_writer *w;
    void *dev_base;
    uint64_t dev_bytes;
    const char *const *paths;
    size_t n;
    int flags;
    void *dev_stage;
    uint64_t stage_bytes;
    uint64_t *arena, *set_offs, *set_caps, *set;
    size_t n_cls;
    uint64_t stride, align;
    uint64_t *img_offs, *img_caps;
    uint32_t *crc_cur;
    int32_t *dev_status;
    int *status, *error;
    uint64_t *fs_sizes;
};

int load_run(const LoadArgs &a, hipStream_t s)
{
    const size_t n = a.n;
    std::vector<uint64_t> sizes(n, 0);
    std::vector<int32_t> pre(n, CIO_OK);
    Workers workers(n);
    RoundEvents ev;
    PersistTiming tm;
    double t0 = now_s();
    workers.run(n, [&](size_t i) {
        struct stat sb;
        if (stat(a.paths[i], &sb) != 0 || !S_ISREG(sb.st_mode)) {
            pre[i] = CIO_ERROR;
        } else {
            sizes[i] = (uint64_t) sb.st_size;
        }
    });
    std::vector<uint32_t> round_of(n);
    const uint32_t rounds = persist_rounds(sizes.data(), n, a.stage_bytes, round_of.data());
    const std::vector<std::pair<size_t, size_t>> ranges = round_ranges(round_of, rounds);
    size_t widest = 1, data_cap = 0;               // the most files and the most bytes of one round
    for (const auto &r : ranges) {
        widest = r.second - r.first > widest ? r.second - r.first : widest;
        size_t bytes = 0;
        for (size_t i = r.first; i < r.second; ++i) {
            bytes += (size_t) persist_slot(sizes[i]);
        }
        data_cap = bytes > data_cap ? bytes : data_cap;
    }
    tm.query_s = now_s() - t0;                    // the stat pass and the plan
    // every output has its final value for a file that no round takes
    for (size_t i = 0; i < n; ++i) {
        a.status[i] = CIO_ERROR;
        a.error[i] = 0;
        if (a.fs_sizes) {
            a.fs_sizes[i] = sizes[i];
        }
    }
    // pinned: the largest round's bytes | soffs | sizes | pre | vst | verr | ast; device: soffs | sizes | vcontent |
    // aoffs | acaps (64-bit), total (16 words), pre | vst | verr | ast | vcrc | vmeta (32-bit)
    const size_t m8 = widest * 8, m4 = up8(widest * 4);
    std::lock_guard<std::mutex> lock(g_scratch.mu);
    Scratch &sc = g_scratch;
    if (pinned_reserve(sc, data_cap + 2 * m8 + 4 * m4) != CIO_OK || dev_reserve(sc, 6 * m8 + 6 * m4 + 128) != CIO_OK) {
        return CIO_ERROR;
    }
    uint64_t *h_soffs = reinterpret_cast<uint64_t *>(sc.pinned + data_cap), *h_sizes = h_soffs + widest;
    int32_t *h_pre = reinterpret_cast<int32_t *>(sc.pinned + data_cap + 2 * m8);
    int32_t *h_vst = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(h_pre) + m4);
    int32_t *h_verr = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(h_vst) + m4);
    int32_t *h_ast = reinterpret_cast<int32_t *>(reinterpret_cast<uint8_t *>(h_verr) + m4);
    uint8_t *d = sc.dev;
    uint64_t *d_soffs = reinterpret_cast<uint64_t *>(d), *d_sizes = d_soffs + widest, *d_vcontent = d_sizes + widest,
             *d_aoffs = d_vcontent + widest, *d_acaps = d_aoffs + widest, *d_total = d_acaps + widest;
    d += 5 * m8 + 128;                        // d_total: 2 + CIOA_POOL_SET_MAX words
    int32_t *d_pre = reinterpret_cast<int32_t *>(d), *d_vst = reinterpret_cast<int32_t *>(d + m4),
            *d_verr = reinterpret_cast<int32_t *>(d + 2 * m4), *d_ast = reinterpret_cast<int32_t *>(d + 3 * m4);
    uint32_t *d_vcrc = reinterpret_cast<uint32_t *>(d + 4 * m4), *d_vmeta = reinterpret_cast<uint32_t *>(d + 5 * m4);

    {   // the device outputs of the files no round takes; the rounds overwrite their own
        std::vector<uint64_t> none(n, ~0ull);
        HIP_TRY(hipMemcpyAsync(a.img_offs, none.data(), n * 8, hipMemcpyHostToDevice, s), "load: output defaults");
        HIP_TRY(hipMemsetAsync(a.img_caps, 0, n * 8, s), "load: output defaults");
        HIP_TRY(hipMemsetAsync(a.crc_cur, 0, n * 4, s), "load: output defaults");
        HIP_TRY(hipMemsetAsync(a.dev_status, 0xff, n * 4, s), "load: output defaults");   // CIO_ERROR
        HIP_TRY(hipStreamSynchronize(s), "load: output defaults");
    }
    for (const auto &r : ranges) {
        const size_t i0 = r.first, m = r.second - r.first;
        uint64_t bytes = 0;
        for (size_t k = 0; k < m; ++k) {
            h_soffs[k] = bytes;
            h_sizes[k] = sizes[i0 + k];
            h_pre[k] = pre[i0 + k];
            bytes += persist_slot(sizes[i0 + k]);
        }
        t0 = now_s();
        workers.run(m, [&](size_t k) {
            if (h_pre[k] == CIO_OK && !read_file(a.paths[i0 + k], sc.pinned + h_soffs[k], h_sizes[k])) {
                h_pre[k] = CIO_ERROR;
            }
        });
        for (size_t k = 0; k < m; ++k) {
            if (h_pre[k] != CIO_OK) {
                h_sizes[k] = 0;                   // verify rejects it, so it takes no slot
            }
        }
        tm.files_s += now_s() - t0;
        ev.mark(0, s);
        if (bytes != 0) {
            HIP_TRY(hipMemcpyAsync(a.dev_stage, sc.pinned, bytes, hipMemcpyHostToDevice, s), "load: H2D of a round");
        }
        HIP_TRY(hipMemcpyAsync(d_soffs, h_soffs, m * 8, hipMemcpyHostToDevice, s), "load: H2D of a round's offsets");
        HIP_TRY(hipMemcpyAsync(d_sizes, h_sizes, m * 8, hipMemcpyHostToDevice, s), "load: H2D of a round's sizes");
        HIP_TRY(hipMemcpyAsync(d_pre, h_pre, m * 4, hipMemcpyHostToDevice, s), "load: H2D of a round's read results");
        ev.mark(1, s);
        if (cio_file_verify_batch_dev(a.w->dp, a.dev_stage, a.stage_bytes, d_soffs, d_sizes, m,
                                      a.flags & CIOA_VERIFY_CHECKSUM, d_vst, d_verr, d_vcrc, d_vmeta, d_vcontent,
                                      s) != CIO_OK ||
            cio_file_alloc_set_batch_dev(a.w, a.dev_base, a.dev_bytes, d_sizes, d_vst, m, a.arena, a.set_offs,
                                         a.set_caps, a.set, a.n_cls, a.stride, a.align, 0, d_aoffs, d_acaps, d_total,
                                         d_ast, s) != CIO_OK) {
            (void) hipStreamSynchronize(s);
            return CIO_ERROR;
        }
        const LoadRound lr = {d_soffs, d_sizes, d_pre, d_vst, d_ast, d_aoffs, d_acaps, d_vcrc, d_vcontent,
                              a.img_offs + i0, a.img_caps + i0, a.crc_cur + i0, a.dev_status + i0};
        if (load_launch_back(a.w, a.dev_base, a.dev_bytes, a.dev_stage, a.stage_bytes, m,
                             (a.flags & CIOA_LOAD_ZERO) != 0, lr, s) != CIO_OK) {
            (void) hipStreamSynchronize(s);
            return CIO_ERROR;
        }
        ev.mark(2, s);
        t0 = now_s();
        HIP_TRY(hipMemcpyAsync(h_vst, d_vst, m * 4, hipMemcpyDeviceToHost, s), "load: D2H of a round's verdicts");
        HIP_TRY(hipMemcpyAsync(h_verr, d_verr, m * 4, hipMemcpyDeviceToHost, s), "load: D2H of a round's verdicts");
        HIP_TRY(hipMemcpyAsync(h_ast, a.dev_status + i0, m * 4, hipMemcpyDeviceToHost, s),
                "load: D2H of a round's verdicts");
        HIP_TRY(hipStreamSynchronize(s), "load: a round's device chain");
        tm.wait_s += now_s() - t0;
        tm.rounds += 1;
        ev.add(tm, true);
        for (size_t k = 0; k < m; ++k) {
            const bool read = h_pre[k] == CIO_OK;
            a.status[i0 + k] = read ? h_ast[k] : CIO_ERROR;     // the adopt step's verdict
            a.error[i0 + k] = read && h_vst[k] != CIO_OK ? h_verr[k] : 0;
        }
    }
    g_load_t = tm;
    return CIO_OK;
}

// ---------------------------------------------------------------- store

struct StoreArgs {
    cio_dev_writer *w;
    const void *dev_base;
    uint64_t dev_bytes;
    const uint64_t *img_offs, *img_caps;
    size_t n;
    const int32_t *gate;
    const char *const *paths;
    int flags;
    uint64_t page;
    void *dev_stage;
    uint64_t stage_bytes;
    int *status;
    uint64_t *file_sizes;
    int32_t *dev_status;
};

int store_run(const StoreArgs &a, hipStream_t s)
{
    const size_t n = a.n;
    const size_t n8 = n * 8, n4 = up8(n * 4);
    const size_t head = (2 * n8 + n4 + 127) & ~(size_t) 127;
    Workers workers(n);
    RoundEvents ev;
    PersistTiming tm;
    double t0 = now_s();
    std::lock_guard<std::mutex> lock(g_scratch.mu);
    Scratch &sc = g_scratch;
    // pinned: lens | caps | statuses | the largest round's bytes; device: out_offs | out_lens | total | statuses
    if (pinned_reserve(sc, head) != CIO_OK || dev_reserve(sc, 2 * n8 + 64 + n4) != CIO_OK) {
        return CIO_ERROR;
    }
    uint64_t *h_lens = reinterpret_cast<uint64_t *>(sc.pinned), *h_caps = h_lens + n;
    int32_t *h_st = reinterpret_cast<int32_t *>(sc.pinned + 2 * n8);
    uint64_t *d_offs = reinterpret_cast<uint64_t *>(sc.dev), *d_lens = d_offs + n, *d_total = d_lens + n;
    int32_t *d_st = reinterpret_cast<int32_t *>(sc.dev + 2 * n8 + 64);
    // the size query: the call's one early synchronisation
    if (cio_file_read_packed_batch_dev(a.w, a.dev_base, a.dev_bytes, a.img_offs, a.img_caps, n, CIOA_READ_IMAGE, a.gate,
                                       nullptr, 0, kPersistAlign, 0, d_offs, d_lens, d_total, d_st, s) != CIO_OK) {
        return CIO_ERROR;
    }
    HIP_TRY(hipMemcpyAsync(h_lens, d_lens, n8, hipMemcpyDeviceToHost, s), "store: D2H of the lengths");
    HIP_TRY(hipMemcpyAsync(h_caps, a.img_caps, n8, hipMemcpyDeviceToHost, s), "store: D2H of the capacities");
    HIP_TRY(hipMemcpyAsync(h_st, d_st, n * 4, hipMemcpyDeviceToHost, s), "store: D2H of the statuses");
    HIP_TRY(hipStreamSynchronize(s), "store: the size query");
    std::vector<uint64_t> used(n), caps(h_caps, h_caps + n);
    std::vector<int32_t> st(h_st, h_st + n);
    for (size_t i = 0; i < n; ++i) {
        used[i] = st[i] == CIO_OK ? h_lens[i] : 0;
        a.status[i] = CIO_ERROR;
        if (a.file_sizes) {
            a.file_sizes[i] = 0;
        }
    }
    std::vector<uint32_t> round_of(n);
    const uint32_t rounds = persist_rounds(used.data(), n, a.stage_bytes, round_of.data());
    const bool trim = (a.flags & CIOA_STORE_TRIM) != 0, sync = (a.flags & CIOA_STORE_SYNC) != 0;
    const std::vector<std::pair<size_t, size_t>> ranges = round_ranges(round_of, rounds);
    size_t data_cap = 0;
    for (const auto &r : ranges) {
        size_t bytes = 0;
        for (size_t i = r.first; i < r.second; ++i) {
            bytes += (size_t) persist_slot(used[i]);
        }
        data_cap = bytes > data_cap ? bytes : data_cap;
    }
    if (pinned_reserve(sc, head + data_cap) != CIO_OK) {     // may move the buffer: lens, caps and statuses are copied
        return CIO_ERROR;
    }
    h_st = reinterpret_cast<int32_t *>(sc.pinned + 2 * n8);
    uint8_t *h_data = sc.pinned + head;
    tm.query_s = now_s() - t0;                    // the size query and the plan
    for (const auto &r : ranges) {
        const size_t i0 = r.first, m = r.second - r.first;
        std::vector<uint64_t> at(m);
        uint64_t bytes = 0;
        for (size_t k = 0; k < m; ++k) {
            at[k] = bytes;
            bytes += persist_slot(used[i0 + k]);
        }
        if (bytes == 0) {
            continue;                             // nothing but rejected entries
        }
        // the round's used bytes into the stage, 128-byte slots: the offsets are the host's sums
        ev.mark(0, s);
        if (cio_file_read_packed_batch_dev(a.w, a.dev_base, a.dev_bytes, a.img_offs + i0, a.img_caps + i0, m,
                                           CIOA_READ_IMAGE, a.gate ? a.gate + i0 : nullptr, a.dev_stage,
                                           a.stage_bytes, kPersistAlign, 0, d_offs, d_lens, d_total, d_st,
                                           s) != CIO_OK) {
            (void) hipStreamSynchronize(s);
            return CIO_ERROR;
        }
        ev.mark(1, s);
        t0 = now_s();
        HIP_TRY(hipMemcpyAsync(h_data, a.dev_stage, bytes, hipMemcpyDeviceToHost, s), "store: D2H of a round");
        HIP_TRY(hipMemcpyAsync(h_st, d_st, m * 4, hipMemcpyDeviceToHost, s), "store: D2H of a round's statuses");
        ev.mark(2, s);
        HIP_TRY(hipStreamSynchronize(s), "store: a round's device chain");
        tm.wait_s += now_s() - t0;
        tm.rounds += 1;
        ev.add(tm, false);
        t0 = now_s();
        workers.run(m, [&](size_t k) {
            const size_t i = i0 + k;
            if (st[i] != CIO_OK || h_st[k] != CIO_OK) {
                return;
            }
            const uint64_t fsz = persist_file_size(used[i], caps[i], trim, a.page);
            if (write_file(a.paths[i], h_data + at[k], used[i], fsz, sync)) {
                a.status[i] = CIO_OK;
                if (a.file_sizes) {
                    a.file_sizes[i] = fsz;
                }
            }
        });
        tm.files_s += now_s() - t0;
    }
    g_store_t = tm;
    for (size_t i = 0; i < n; ++i) {
        h_st[i] = a.status[i];
    }
    HIP_TRY(hipMemcpyAsync(a.dev_status, h_st, n * 4, hipMemcpyHostToDevice, s), "store: H2D of the statuses");
    HIP_TRY(hipStreamSynchronize(s), "store: H2D of the statuses");
    return CIO_OK;
}

}  // namespace

extern "C" {

void cio_file_persist_trim(void)
{
    std::lock_guard<std::mutex> lock(g_scratch.mu);
    Scratch &sc = g_scratch;
    if (sc.pinned) {
        (void) hipHostFree(sc.pinned);
    }
    if (sc.dev) {
        (void) hipFree(sc.dev);
    }
    sc.pinned = sc.dev = nullptr;
    sc.pinned_cap = sc.dev_cap = 0;
    sc.dev_id = -1;
}

/* Measurement hook (not in the public header; tools/persist_ab.py): what the
 * process's last load (which = 0) or store (1) spent where, summed over its
 * rounds -- out[0] rounds, [1] seconds in the file threads (pread / pwrite),
 * [2] event milliseconds of the rounds' transfers (H2D / D2H), [3] event
 * milliseconds of their device chains (verify, allocation, copy, adopt / the
 * packed read), [4] seconds the host waited for a round's stream, [5] seconds
 * before the first round (stat or the size query, and the plan). */
int cioa_debug_persist_timing(int which, double *out, int n)
{
    const PersistTiming t = which ? g_store_t : g_load_t;
    const double v[6] = {t.rounds, t.files_s, t.copy_ms, t.chain_ms, t.wait_s, t.query_s};
    for (int i = 0; i < n && i < 6; ++i) {
        out[i] = v[i];
    }
    return n < 6 ? n : 6;
}

uint64_t cio_file_persist_round_max(uint64_t stage_bytes)
{
    return persist_round_max(stage_bytes);
}

int cio_file_persist_rounds(const uint64_t *sizes, size_t n, uint64_t stage_bytes, uint32_t *round_of)
{
    if (n == 0) {
        return 0;
    }
    if (!sizes || !round_of) {
        return fail_who("cio_file_persist_rounds", "null pointer");
    }
    if (n >= 0x7fffffffull) {
        return fail_who("cio_file_persist_rounds", "n must be below 2^31 - 1");
    }
    return (int) persist_rounds(sizes, n, stage_bytes, round_of);
}

int cio_file_load_paths_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const char *const *paths, size_t n, int flags,
                            void *dev_stage, uint64_t stage_bytes,
                            uint64_t *dev_arena, uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                            size_t n_cls, uint64_t stride, uint64_t align,
                            uint64_t *dev_img_offs, uint64_t *dev_img_caps, uint32_t *dev_crc_cur,
                            int32_t *dev_status,
                            int *status, int *error, uint64_t *fs_sizes, void *stream)
{
    if (flags & ~(CIOA_VERIFY_CHECKSUM | CIOA_LOAD_ZERO)) {
        return fail_who(kLoad, "unknown flags");
    }
    if (!pow2(align) || align > 4096) {
        return fail_who(kLoad, "align must be a power of two in 1 .. 4096");
    }
    if (n_cls > CIOA_POOL_SET_MAX) {
        return fail_who(kLoad, "n_cls must be in 0 .. 8");
    }
    if (n_cls != 0 && stride == 0) {
        return fail_who(kLoad, "stride must not be 0");
    }
    if (!w) {
        return fail_who(kLoad, "null writer");
    }
    if (n == 0) {
        return CIO_OK;
    }
    if (stage_bytes == 0) {
        return fail_who(kLoad, "stage_bytes must not be 0");
    }
    if (!dev_base || !paths || !dev_stage || !dev_arena || !dev_img_offs || !dev_img_caps || !dev_crc_cur ||
        !dev_status || !status || !error || (n_cls != 0 && (!dev_set_offs || !dev_set_caps || !dev_set))) {
        return fail_who(kLoad, "null pointer");
    }
    if (n > w->max_chunks) {
        return fail_who(kLoad, "more files than the writer was created for");
    }
    for (size_t i = 0; i < n; ++i) {
        if (!paths[i]) {
            return fail_who(kLoad, "null path");
        }
    }
    const LoadArgs a = {w, dev_base, dev_bytes, paths, n, flags, dev_stage, stage_bytes, dev_arena, dev_set_offs,
                        dev_set_caps, dev_set, n_cls, stride, align, dev_img_offs, dev_img_caps, dev_crc_cur,
                        dev_status, status, error, fs_sizes};
    return load_run(a, reinterpret_cast<hipStream_t>(stream));
}

int cio_file_store_paths_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                             const int32_t *dev_gate, const char *const *paths, int flags, uint64_t page,
                             void *dev_stage, uint64_t stage_bytes,
                             int *status, uint64_t *file_sizes, int32_t *dev_status, void *stream)
{
    if (flags & ~(CIOA_STORE_TRIM | CIOA_STORE_SYNC)) {
        return fail_who(kStore, "unknown flags");
    }
    if (!pow2(page) || page > kPersistPageMax) {
        return fail_who(kStore, "page must be a power of two in 1 .. 2^30");
    }
    if (!w) {
        return fail_who(kStore, "null writer");
    }
    if (n == 0) {
        return CIO_OK;
    }
    if (stage_bytes == 0) {
        return fail_who(kStore, "stage_bytes must not be 0");
    }
    if (!dev_base || !dev_img_offs || !dev_img_caps || !paths || !dev_stage || !status || !dev_status) {
        return fail_who(kStore, "null pointer");
    }
    if (n > w->max_chunks) {
        return fail_who(kStore, "more images than the writer was created for");
    }
    for (size_t i = 0; i < n; ++i) {
        if (!paths[i]) {
            return fail_who(kStore, "null path");
        }
    }
    const StoreArgs a = {w, dev_base, dev_bytes, dev_img_offs, dev_img_caps, n, dev_gate, paths, flags, page,
                         dev_stage, stage_bytes, status, file_sizes, dev_status};
    return store_run(a, reinterpret_cast<hipStream_t>(stream));
}

}  // extern "C"
