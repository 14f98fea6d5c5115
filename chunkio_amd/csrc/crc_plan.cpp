// crc_plan.cpp -- the host planner of the CRC-32 stream kernels: the work
// partition a launch reads (plan_build) and every decision about which kernel
// and which grid a batch gets (plan_init, plan_choose).  Integer arithmetic
// over offsets and lengths: plain C++, no HIP header, no device.
// gpu_runtime.hip allocates and uploads what is decided here; the device
// planner of devplan_gpu.hip reproduces plan_build byte for byte.

#include <stdint.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <vector>

#include "cio_plan.h"

namespace cioa {

// Tuning knobs (environment, read at plan creation) and grid geometry.
void plan_init(cio_crc32_plan *p, DeviceState *st, size_t n)
{
    p->st = st;
    p->n = (uint32_t) n;
    if (const char *r = cioa_diag_getenv("CIO_GPU_PRIO")) {
        const int v = atoi(r);
        p->prio = (v == 0) ? 0 : 1;
    }
    // Lane layout of the CRC kernels (profiles/r03/ab_l64_*.txt): the
    // stream kernels take one 64-byte chain per lane (L64, permlane
    // transpose: cfg2 -5 %, cfg3 -1 %, 4 MiB chunks -1 to -2.5 %); the small
    // kernel keeps the 4-sub-chain layout (L64 there: cfg4k +1 %, 64 Ki x
    // 4 KiB -3.5 %).  CIO_GPU_L64=1 / 0 forces one layout on both.
    p->l64 = true;
    p->l64_small = false;
    if (const char *r = cioa_diag_getenv("CIO_GPU_L64")) {
        p->l64 = p->l64_small = atoi(r) != 0;
    }
    p->grid = (uint32_t) st->cus;
    // Test / A/B knob: another workgroup count (fewer than CUs: e.g. a wave
    // count that is not a power of two, which takes the kernels' f64 split
    // instead of the shift; more: workgroups that queue for a CU, up to 16
    // per CU).
    if (const char *r = cioa_diag_getenv("CIO_GPU_GRID")) {
        const int v = atoi(r);
        if (v >= 1 && v <= 16 * (int) p->grid) {
            p->grid = (uint32_t) v;
        }
    }
    p->W = p->grid * (kThreads / kWave);
}

// Virtual aligned chunks, wave-step numbering, the even split of the S steps
// over W waves, each wave's first chunk, per-chunk piece counts and per-slot
// fold factors.  Host only; returns an error message or nullptr.
const char *plan_build(PlanHost &ph, const uint64_t *offs, const uint64_t *lens, size_t n, uint32_t W)
{
    ph.desc.assign(n ? n : 1, ChunkDesc{});
    ph.tiny.clear();
    uint64_t S = 0, bytes = 0;
    for (size_t i = 0; i < n; i++) {
        ChunkDesc &d = ph.desc[i];
        const uint64_t amask = lens[i] > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
        d.a = offs[i] & ~amask;
        d.h = (uint32_t) (offs[i] & amask);
        d.vlen = d.h + lens[i];
        d.g = S;
        const uint64_t ns = lens[i] >= 4 ? (d.vlen + kStep - 1) / kStep : 0;
        if (ns > 0xffffffffull) {
            return "cio_crc32_plan_create: chunk too large";
        }
        d.nsteps = (uint32_t) ns;
        if (ns == 0) {
            ph.tiny.push_back((uint32_t) i);
        }
        S += ns;
        bytes += lens[i];
    }
    // The kernels' start-up divisions (div_u52) need w * S < 2^52 for w <= W
    // (W <= 2^12 on a full device: 2^40 wave-steps is 4 PiB, far past any
    // device's memory).
    if (S >= (1ull << 40) || W > 65536 || (S * (uint64_t) W) >> 52) {
        return "cio_crc32_plan_create: batch too large";
    }
    ph.S = S;
    ph.bytes = bytes;

    // Fold factors x^(8 d) for d = bytes after a piece = 4096 m + r: one
    // multiply of two table entries (x8 static, x4k per plan up to the
    // longest chunk) instead of a square-and-multiply per piece.
    static const std::vector<uint32_t> x8 = [] {
        std::vector<uint32_t> t(kStep);
        cioa_gen_xpow8_table(t.data(), kStep, 1);
        return t;
    }();
    uint64_t max_steps = 0;
    for (size_t i = 0; i < n; i++) {
        max_steps = std::max<uint64_t>(max_steps, ph.desc[i].nsteps);
    }
    std::vector<uint32_t> x4k;
    if (max_steps <= (1u << 20)) {
        x4k.resize(max_steps + 1);
        cioa_gen_xpow8_table(x4k.data(), x4k.size(), (uint64_t) kStep);
    }
    auto factor = [&](uint64_t d) {
        const uint64_t m = d / kStep, r = d % kStep;
        if (m == 0) {
            return x8[r];
        }
        return m < x4k.size() ? cioa_multmodp(x4k[m], x8[r]) : cioa_xpow8n(d);
    };

    std::vector<uint32_t> wc(W, 0), wl(W, 0);
    const size_t nslots = (size_t) W + n + 1;
    ph.pfac.assign(nslots + 2 * (size_t) W, 0u);
    if (S > 0) {
        size_t c = 0;
        for (uint32_t w = 0; w < W; w++) {
            const uint64_t g0 = ((uint64_t) w * S) / W;
            const uint64_t g1 = ((uint64_t) (w + 1) * S) / W;
            while (c < n && (ph.desc[c].nsteps == 0 || ph.desc[c].g + ph.desc[c].nsteps <= g0)) {
                c++;
            }
            wc[w] = (uint32_t) std::min(c, n - 1);
            if (g0 == g1) {
                continue;
            }
            for (size_t k = c; k < n && ph.desc[k].g < g1; k++) {
                ChunkDesc &d = ph.desc[k];
                if (d.nsteps) {
                    if (d.npieces == 0) {
                        d.w0 = w;
                    }
                    d.w1 = w;
                    wl[w] = (uint32_t) k;
                    d.npieces++;
                    const uint64_t pend = std::min(std::min(g1 - d.g, (uint64_t) d.nsteps) * (uint64_t) kStep,
                                                   d.vlen);
                    ph.pfac[w + k] = factor(d.vlen - pend);
                }
            }
        }
    }
    // Workgroup-local chunks: split, with every piece in one workgroup.
    auto local = [](const ChunkDesc &d) {
        return d.npieces > 1 && d.w0 / kWavesPerWg == d.w1 / kWavesPerWg;
    };
    for (uint32_t w = 0; S > 0 && w < W; w++) {
        const uint64_t g0 = ((uint64_t) w * S) / W;
        const uint64_t g1 = ((uint64_t) (w + 1) * S) / W;
        if (g0 == g1) {
            continue;
        }
        uint32_t f = 0;
        const ChunkDesc &first = ph.desc[wc[w]];
        if (first.g < g0 && first.g + first.nsteps <= g1 && local(first)) {
            f |= kWfFold | ((w - first.w0) << 8);
        }
        const ChunkDesc &last = ph.desc[wl[w]];
        const bool nonfinal = last.g + last.nsteps > g1;
        if (nonfinal && local(last)) {
            f |= kWfPublish;
        }
        ph.pfac[nslots + w] = f;
        // The last piece's factor (x^0 = 0x80000000 when it ends its chunk).
        ph.pfac[nslots + W + w] = nonfinal ? ph.pfac[w + wl[w]] : 0x80000000u;
    }
    ph.ws.assign(W, WaveStart{});
    for (uint32_t w = 0; w < W; w++) {
        ph.ws[w].c = wc[w];
        if (n) {
            ph.ws[w].d = ph.desc[wc[w]];
        }
    }
    return nullptr;
}

namespace {

// Uniform batch: n equal lengths >= 4 at offsets off0 + i * stride with
// stride a multiple of 16 (every chunk has the same misalignment).  The
// kernel then derives chunk descriptors arithmetically (CIO_GPU_UNIFORM=0
// disables).
void plan_uniform(cio_crc32_plan *p, const uint64_t *offs, const uint64_t *lens, size_t n, const PlanHost &ph)
{
    p->unsteps = 0;
    if (const char *r = cioa_diag_getenv("CIO_GPU_UNIFORM")) {
        if (!atoi(r)) {
            return;
        }
    }
    if (n == 0 || lens[0] < 4 || ph.desc[0].nsteps == 0) {
        return;
    }
    const uint64_t stride = n > 1 ? offs[1] - offs[0] : 0;
    if (n > 1 && (offs[1] < offs[0] || (stride & 15) != 0)) {
        return;
    }
    for (size_t i = 1; i < n; i++) {
        if (lens[i] != lens[0] || offs[i] != offs[0] + i * stride || ph.desc[i].h != ph.desc[0].h) {
            return;
        }
    }
    p->ustride = stride;
    p->ua0 = ph.desc[0].a;
    p->uvlen = ph.desc[0].vlen;
    p->uh = ph.desc[0].h;
    p->unsteps = ph.desc[0].nsteps;
}

}  // namespace

const char *plan_choose(cio_crc32_plan *p, PlanHost &ph, const uint64_t *offs, const uint64_t *lens, size_t n)
{
    if (const char *err = plan_build(ph, offs, lens, n, p->W)) {
        return err;
    }
    plan_uniform(p, offs, lens, n, ph);
    // All chunks within one wave-step (S = number of non-tiny chunks): a
    // small-chunk batch.  Read from ph as it stands at each decision below.
    auto small_batch = [&ph, n] { return ph.S > 0 && ph.S == (uint64_t) n - ph.tiny.size(); };
    // Long batches (>= 4 MiB per wave: cfg3's ~2400 steps per wave, cfg4's
    // 2048 at one GPU) split over 4 workgroups per CU: the extra workgroups
    // queue for a CU and start wherever one finishes, so the hardware evens
    // out the per-CU finish times (cfg3 -0.7 %, cfg4 -1.7 %; shorter ranges
    // lose: 1 MiB per wave +0.8 to +5.5 %, cfg2 +5 %:
    // profiles/r04/ab_grid_oversubscribed_r04q.txt, ab_grid_cfg4_r04x.txt).
    bool oversub = false;
    if (!cioa_diag_getenv("CIO_GPU_GRID") && ph.S >= 1024ull * p->W && 4ull * p->W <= 65536 &&
        !small_batch()) {    // (S >= 1024 W > 0 here)
        PlanHost ph4;
        if (plan_build(ph4, offs, lens, n, 4 * p->W) == nullptr) {
            p->grid *= 4;
            p->W *= 4;
            oversub = true;
            ph = std::move(ph4);
        }
    }
    // HBM channel camping (profiles/r05/camping/): when every wave's range is
    // the same multiple of 16 steps (64 KiB), all waves read addresses equal
    // modulo 64 KiB at the same moment and even the read-only stream loses
    // 5-10 % (16, 32, 64 steps per wave against 17, 33, 65).  One workgroup
    // fewer per 32 -- one per XCD, so the XCDs stay balanced -- makes the
    // ranges uneven and breaks the congruence.  Warm ABBA A/B
    // (ab_anticamp_abba_r05x.txt): stream kernel +4.1 to +4.6 % at 16-64
    // steps per wave, -1.0 % at 128 and 256; small-chunk kernel +10.9 to
    // +14.3 % at 16-64 chunks per wave, +3.9 % at 128.  CIO_GPU_ANTICAMP=0
    // keeps the full grid; CIO_GPU_ANTICAMP_MAX overrides the range cap.
    {
        const char *r = cioa_diag_getenv("CIO_GPU_ANTICAMP");
        const bool on = !(r && atoi(r) == 0);
        const char *mx = cioa_diag_getenv("CIO_GPU_ANTICAMP_MAX");     // A/B: longest range it applies to
        const uint64_t wmax = mx ? strtoull(mx, nullptr, 10) : small_batch() ? 128 : 64;
        const uint64_t w = p->W ? ph.S / p->W : 0;
        const bool any_grid = r && atoi(r) == 2;            // A/B: also on oversubscribed grids
        if (on && (!oversub || any_grid) && !cioa_diag_getenv("CIO_GPU_GRID") && p->grid % 32 == 0 && ph.S % p->W == 0 &&
            w % 16 == 0 &&
            w > 0 && w <= wmax) {
            const uint32_t g2 = p->grid / 32 * 31;
            PlanHost ph2;
            if (plan_build(ph2, offs, lens, n, g2 * (kThreads / kWave)) == nullptr) {
                p->grid = g2;
                p->W = g2 * (kThreads / kWave);
                ph = std::move(ph2);
            }
        }
    }
    p->S = ph.S;
    p->bytes = ph.bytes;
    p->ntiny = (uint32_t) ph.tiny.size();
    // Uniform batch of whole 4 KiB steps, 16-byte aligned, with short wave
    // ranges (<= 64 steps, e.g. cfg2's 25): the issue-ahead stream kernel.
    // Interleaved A/Bs (profiles/r03/ab_issue_ahead_*.txt): cfg2 -0.6 to
    // -1.8 %, 100- and 256-step ranges -0.3 to +0.6 % (neutral), so only
    // short ranges, where the first steps' start-up is a larger share, take
    // it.  CIO_GPU_AHEAD=1 forces it for any uniform aligned batch, 0 never.
    p->ahead = p->unsteps != 0 && p->uh == 0 && p->uvlen % kStep == 0;
    bool short_ranges = p->S <= 64ull * p->W;
    if (const char *r = cioa_diag_getenv("CIO_GPU_AHEAD")) {
        short_ranges = atoi(r) != 0;
    }
    p->ahead = p->ahead && short_ranges;

    // Wave-aligned batch: an issue-ahead batch on the full one-workgroup-per-CU
    // grid whose S steps split into exactly q per wave, with every chunk
    // exactly p = 2, 4, 8 or 16 consecutive waves (cfg2: q = 25, p = 4).  p
    // divides the 16 waves of a workgroup, so wave w holds piece w mod p of
    // chunk w / p, no chunk leaves its workgroup and a wave's only piece end
    // is its last step: crc32_aligned_kernel derives all of it from the
    // kernel arguments.  (p = 1, whole chunks per wave, stays on the issue-
    // ahead kernel, which writes such chunks out directly.)
    // CIO_GPU_ALIGNED=0 keeps the issue-ahead kernel.
    p->aligned = false;
    ph.afac.clear();
    {
        const char *r = cioa_diag_getenv("CIO_GPU_ALIGNED");
        const bool on = !(r && atoi(r) == 0);
        const uint64_t q = p->W ? p->S / p->W : 0;
        if (on && p->ahead && p->l64 && p->prio && p->ntiny == 0 && p->grid == (uint32_t) p->st->cus &&
            q >= 1 && q <= 64 && p->S == q * p->W && p->unsteps % q == 0) {
            const uint64_t np = p->unsteps / q;
            if (np == 2 || np == 4 || np == 8 || np == 16) {
                p->aligned = true;
                p->aq = (uint32_t) q;
                p->alg2p = np == 2 ? 1 : np == 4 ? 2 : np == 8 ? 3 : 4;
                // Piece i of a chunk ends q * 4096 * (p - 1 - i) bytes before
                // the chunk end, and lane l's 64-byte chain 64 (63 - l) bytes
                // before the piece end: one factor per (piece, lane) shifts a
                // lane's state to the chunk end.
                ph.afac.resize(np * kWave);
                for (uint64_t i = 0; i < np; i++) {
                    for (uint64_t l = 0; l < (uint64_t) kWave; l++) {
                        ph.afac[i * kWave + l] = cioa_xpow8n(q * kStep * (np - 1 - i) + 64 * (kWave - 1 - l));
                    }
                }
            }
        }
    }

    // The small-chunk kernel for a small-chunk batch (CIO_GPU_SMALL=0 disables).
    p->small = small_batch();
    if (const char *r = cioa_diag_getenv("CIO_GPU_SMALL")) {
        p->small = p->small && atoi(r) != 0;
    }
    return nullptr;
}

}  // namespace cioa

using namespace cioa;

extern "C" {

/* Test hook (not in the public header; host only, no device): the plan's
 * work split for W waves.  Per chunk: w0, w1, npieces (3 words); per wave:
 * the LDS-fold flags.  Returns 0, or -1 on a plan error. */
int cioa_debug_plan_layout(const uint64_t *offs, const uint64_t *lens, size_t n, uint32_t W,
                           uint32_t *chunk_words, uint32_t *wave_flags)
{
    PlanHost ph;
    if (plan_build(ph, offs, lens, n, W) != nullptr) {
        return -1;
    }
    for (size_t i = 0; i < n; i++) {
        chunk_words[3 * i + 0] = ph.desc[i].w0;
        chunk_words[3 * i + 1] = ph.desc[i].w1;
        chunk_words[3 * i + 2] = ph.desc[i].npieces;
    }
    const size_t nslots = (size_t) W + n + 1;
    for (uint32_t w = 0; w < W; w++) {
        wave_flags[w] = ph.pfac[nslots + w];
    }
    return 0;
}

/* Test hook (not in the public header; host only, no device): the host twin
 * of cioa_debug_devplan_image -- plan_build's arrays for the same inputs and
 * W, in the same layout; hdr = {S, ntiny, bytes, 0}.  -1 on a plan error. */
int cioa_debug_plan_image(const uint64_t *offs, const uint64_t *lens, size_t n, uint32_t W, void *desc,
                          void *wstart, uint32_t *tiny, uint32_t *pfac, uint64_t *hdr)
{
    PlanHost ph;
    if (plan_build(ph, offs, lens, n, W) != nullptr) {
        return -1;
    }
    memcpy(desc, ph.desc.data(), n * sizeof(ChunkDesc));
    memcpy(wstart, ph.ws.data(), (size_t) W * sizeof(WaveStart));
    if (!ph.tiny.empty()) {
        memcpy(tiny, ph.tiny.data(), ph.tiny.size() * sizeof(uint32_t));
    }
    memcpy(pfac, ph.pfac.data(), ph.pfac.size() * sizeof(uint32_t));
    hdr[kDevHdrS] = ph.S;
    hdr[kDevHdrNtiny] = ph.tiny.size();
    hdr[kDevHdrBytes] = ph.bytes;
    hdr[kDevHdrStatus] = 0;
    return 0;
}

/* Test hook (not in the public header; host only, no device): the kernel and
 * grid that cio_crc32_plan_create chooses for this batch on a device of `cus`
 * compute units (>= 1).  out_words[11]: grid, W, small, ahead, unsteps, l64,
 * l64_small, then S and ntiny as 64-bit values, low word first.  Returns 0,
 * or -1 on a plan error. */
int cioa_debug_plan_choice(const uint64_t *offs, const uint64_t *lens, size_t n, int cus, uint32_t *out_words)
{
    if (cus < 1 || n >= 0xffffffffull) {
        return -1;
    }
    DeviceState st;
    st.cus = cus;
    cio_crc32_plan p;
    PlanHost ph;
    plan_init(&p, &st, n);
    if (plan_choose(&p, ph, offs, lens, n) != nullptr) {
        return -1;
    }
    const uint64_t ntiny = p.ntiny;
    const uint32_t words[11] = {p.grid, p.W, p.small, p.ahead, p.unsteps, p.l64, p.l64_small,
                                (uint32_t) p.S, (uint32_t) (p.S >> 32), (uint32_t) ntiny, (uint32_t) (ntiny >> 32)};
    memcpy(out_words, words, sizeof(words));
    return 0;
}

/* Test hook (not in the public header; host only, no device): the wave-aligned
 * class of the same choice (cio_crc32_plan_aligned on a device).  out_words[3]:
 * aligned, steps per wave q, waves per chunk p (both 0 outside the class).
 * Returns 0, or -1 on a plan error. */
int cioa_debug_plan_aligned(const uint64_t *offs, const uint64_t *lens, size_t n, int cus, uint32_t *out_words)
{
    if (cus < 1 || n >= 0xffffffffull) {
        return -1;
    }
    DeviceState st;
    st.cus = cus;
    cio_crc32_plan p;
    PlanHost ph;
    plan_init(&p, &st, n);
    if (plan_choose(&p, ph, offs, lens, n) != nullptr) {
        return -1;
    }
    out_words[0] = p.aligned;
    out_words[1] = p.aligned ? p.aq : 0;
    out_words[2] = p.aligned ? 1u << p.alg2p : 0;
    return 0;
}

}  // extern "C"
