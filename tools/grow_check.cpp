// grow_check.cpp -- growing chunk images out of an arena (grow_dev.h: the text
// the kernels grow_headers, grow_scan, grow_place, grow_zero and grow_commit
// run), stand-alone on the host under ASan + UBSan: no GPU, no HIP.
// `make growcheck`.
//
// Bookkeeping: the header, scan, place and commit kernels are restated
// workgroup by workgroup -- the workgroup scan as the kernels do it, in log
// steps with place_add -- and run with the workgroups of each kernel in
// ascending, descending and random order (no workgroup may depend on another
// of its kernel).  Statuses, offsets, capacities, the total and the arena's
// top are compared with a sequential loop in 128-bit arithmetic.  The images
// are given by their fields (offset, capacity, used bytes, content length,
// validity): no data.
//
// Zero fill: random tail regions are partitioned as plan_chunks1 partitions
// them and zeroed wave by wave, lane by lane, in a buffer of EXACTLY the bytes
// the batch spans, so the sanitizer sees any access outside; the buffer is
// then compared byte for byte.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "grow_dev.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int OK = 0, ERR = -1;

struct Img {
    uint64_t off, cap, used, content, need;
    bool valid;                               // the write path's image check
};

struct Batch {
    std::vector<Img> img;
    uint64_t top, end, dev_bytes, realloc_size, page, align;
};

struct Result {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps;         // after the commit
    uint64_t total, top;
    bool operator==(const Result &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && total == o.total && top == o.top;
    }
};

Result kernels(const Batch &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.img.size();
    const uint32_t nb = (uint32_t) ((n + kGrowBlock - 1) / kGrowBlock);
    std::vector<uint64_t> dst(n), slen(n), gcap(n), rtot(nb), sh(kGrowBlock), excl(kGrowBlock);
    std::vector<uint32_t> code(n);
    Result r;
    r.status.assign(n, OK);
    r.offs.resize(n);
    r.caps.resize(n);
    uint64_t arena[2] = {b.top, b.end};
    // grow_headers
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kGrowBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kGrowBlock + t;
            uint64_t ncap = 0;
            if (i < n) {
                const Img &m = b.img[i];
                r.offs[i] = m.off;
                r.caps[i] = m.cap;
                if (m.need != 0) {
                    if (!m.valid || grow_decide(m.off, m.cap, m.used, m.content, m.need, arena[0], arena[1],
                                                b.realloc_size, b.page, ncap) == kGrowReject) {
                        r.status[i] = ERR;
                    }
                }
                slen[i] = ncap ? m.used : 0;
                gcap[i] = ncap;
            }
            sh[t] = grow_slot(ncap, b.align);
        }
        wg_scan(kGrowBlock, sh, excl, rtot[wg]);
        for (uint32_t t = 0; t < kGrowBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kGrowBlock + t;
            if (i < n) {
                dst[i] = excl[t];
            }
        }
    }
    // grow_scan: one workgroup, pass by pass
    const uint64_t carry = scan_totals(kGrowBlock, rtot.data(), nb);
    r.total = grow_total(arena[0], b.align, carry);
    // grow_place
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kGrowBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kGrowBlock + t;
            if (i >= n) {
                break;
            }
            const uint64_t before = place_add(rtot[wg], dst[i]);
            const uint64_t slot = grow_slot(gcap[i], b.align);
            uint64_t off;
            code[i] = grow_place_code(arena[0], arena[1], b.dev_bytes, b.align, before, slot, i + 1 == n, off);
            dst[i] = off;
            if (!(code[i] & kGrowMoved)) {
                if (slot != 0) {
                    r.status[i] = ERR;
                }
                slen[i] = 0;
            }
        }
    }
    // grow_commit: every thread reads the arena as the kernel's threads may --
    // before or after the one store to its top -- so no thread may use it
    int writers = 0;
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kGrowBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kGrowBlock + t;
            if (i >= n) {
                break;
            }
            const uint32_t c = code[i];
            if (c & kGrowMoved) {
                r.offs[i] = dst[i];
                r.caps[i] = gcap[i];
            }
            if (c & (kGrowTopAt | kGrowTopEnd)) {
                arena[0] = (c & kGrowTopAt) ? dst[i] : dst[i] + grow_slot(gcap[i], b.align);
                writers += 1 + ((c & kGrowTopAt) && (c & kGrowTopEnd));
            }
        }
    }
    r.top = writers > 1 ? ~b.top : arena[0];   // two writers: never equal to the reference
    return r;
}

u128 up128(u128 v, uint64_t a)
{
    return (v + (a - 1)) / a * a;
}

Result sequential(const Batch &b)
{
    const u128 over = (u128) kPlaceOver;
    const size_t n = b.img.size();
    Result r;
    r.status.assign(n, OK);
    const u128 base = std::min(up128(b.top, b.align), over);
    u128 run = 0, top = b.top;
    for (size_t i = 0; i < n; ++i) {
        const Img &m = b.img[i];
        r.offs.push_back(m.off);
        r.caps.push_back(m.cap);
        if (m.need == 0) {
            continue;
        }
        const bool overlap = b.top < b.end && (u128) m.off < b.end && (u128) b.top < (u128) m.off + m.cap;
        if (!m.valid || (u128) m.content + m.need > kGrowMaxContent || overlap) {
            r.status[i] = ERR;
            continue;
        }
        if ((u128) m.used + m.need <= m.cap) {
            continue;
        }
        u128 nw = (u128) m.cap + b.realloc_size;          // the reference's loop, in closed form
        if (nw < (u128) m.used + m.need) {
            const u128 lack = (u128) m.used + m.need - m.cap;
            nw = (u128) m.cap + (lack + b.realloc_size - 1) / b.realloc_size * b.realloc_size;
        }
        const u128 ncap = up128(nw, b.page);
        if (ncap >= over) {
            r.status[i] = ERR;
            continue;
        }
        const u128 slot = std::min(up128(ncap, b.align), over), off = std::min(base + run, over);
        if (b.end <= b.dev_bytes && off < over && off + slot < over && off + slot <= (u128) b.end) {
            r.offs[i] = (uint64_t) off;
            r.caps[i] = (uint64_t) ncap;
            top = off + slot;
        } else {
            r.status[i] = ERR;
        }
        run = std::min(run + slot, over);
    }
    r.total = run == 0 ? 0 : base == over ? kPlaceOver : (uint64_t) std::min(base - b.top + run, over);
    r.top = (uint64_t) top;
    return r;
}

int check(const Batch &b, const char *what, std::mt19937_64 &rng)
{
    const Result want = sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(kernels(b, order, rng) == want)) {
            fprintf(stderr,
                    "grow_check: %s: n = %zu, align = %llu, page = %llu, realloc = %llu, top = %llu, end = %llu, "
                    "order %d differs\n",
                    what, b.img.size(), (unsigned long long) b.align, (unsigned long long) b.page,
                    (unsigned long long) b.realloc_size, (unsigned long long) b.top, (unsigned long long) b.end,
                    order);
            return 1;
        }
    }
    return 0;
}

// Images laid out one behind another from byte 64, the arena behind them.
// Kinds: need 0, fits, fits exactly, one byte over, many steps over, invalid.
Batch random_batch(size_t n, uint64_t align, uint64_t page, uint64_t realloc_size, std::mt19937_64 &rng)
{
    Batch b;
    b.img.resize(n);
    uint64_t pos = 64;
    for (size_t i = 0; i < n; ++i) {
        Img &m = b.img[i];
        const uint64_t meta = rng() % 5 == 0 ? rng() % 300 : 0;
        m.content = rng() % 6000;
        m.used = kReadHdr + meta + m.content;
        m.cap = m.used + rng() % 9000;
        m.off = pos;
        pos += m.cap + rng() % 40;
        m.valid = rng() % 9 != 0;
        const uint64_t room = m.cap - m.used;
        switch (rng() % 6) {
        case 0: m.need = 0; break;
        case 1: m.need = room ? rng() % room : 0; break;
        case 2: m.need = room; break;
        case 3: m.need = room + 1; break;
        case 4: m.need = room + 1 + rng() % 200000; break;
        default: m.need = rng() % 3 ? room + 1 + rng() % 5000 : 0; break;
        }
    }
    b.top = pos + rng() % 5000;
    b.end = kPlaceOver - 1;
    b.dev_bytes = kPlaceOver - 1;
    b.realloc_size = realloc_size;
    b.page = page;
    b.align = align;
    return b;
}

// ---------------------------------------------------------------- the zero fill

int zero_batch(const std::vector<uint64_t> &lens, uint64_t first_residue, uint32_t W, bool gaps, int iter,
               std::mt19937_64 &rng)
{
    const uint32_t n = (uint32_t) lens.size();
    std::vector<uint64_t> zoff(n), zlen(lens);
    std::vector<ChunkDesc> desc(n);
    uint64_t pos = 0, S = 0;
    for (uint32_t i = 0; i < n; ++i) {
        pos += gaps ? rng() % 40 : 0;
        zoff[i] = pos;
        pos += zlen[i];
    }
    // a buffer of exactly the batch's extent whose first byte has the residue asked for
    uint8_t *block = (uint8_t *) malloc(pos + 16);
    uint8_t *lo = block;
    while (((uintptr_t) lo & 15u) != first_residue) {
        ++lo;
    }
    // the sanitizer guards the block, not lo: the bytes in front of lo and behind lo + pos are compared instead
    memset(block, 0xA5, pos + 16);
    std::vector<uint8_t> want(block, block + pos + 16);
    for (uint32_t i = 0; i < n; ++i) {
        memset(want.data() + (lo - block) + zoff[i], 0, zlen[i]);
        // plan_chunks1's descriptor (devplan_gpu.hip) of the region in its buffer
        const uint64_t off = (uint64_t) (uintptr_t) lo + zoff[i], len = zlen[i];
        const uint64_t amask = len > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
        ChunkDesc d = {};
        d.a = off & ~amask;
        d.h = (uint32_t) (off & amask);
        d.vlen = d.h + len;
        d.nsteps = len >= 4 ? (uint32_t) ((d.vlen + kStep - 1) / kStep) : 0;
        d.g = S;
        S += d.nsteps;
        desc[i] = d;
    }
    for (uint64_t first = 0; first < 5; ++first) {
        fill_tiny(lo, zoff.data(), zlen.data(), n, first, 5);
    }
    for (uint64_t w = 0; w < W; ++w) {
        for (uint32_t lane = 0; lane < (uint32_t) kWave; ++lane) {
            fill_wave(lo, desc.data(), zoff.data(), zlen.data(), n, S, W, w, lane);
        }
    }
    int rc = 0;
    if (memcmp(block, want.data(), pos + 16) != 0) {
        for (uint64_t k = 0; k < pos + 16; ++k) {
            if (block[k] != want[k]) {
                fprintf(stderr, "grow_check: zero batch %d (n = %u, W = %u, residue %llu): byte %lld differs\n", iter,
                        n, W, (unsigned long long) first_residue, (long long) k - (long long) (lo - block));
                break;
            }
        }
        rc = 1;
    }
    free(block);
    return rc;
}

// One region alone in a buffer of exactly its bytes: the sanitizer sees a
// store on either side of it.
int zero_exact(uint64_t len, uint32_t W)
{
    uint8_t *buf = (uint8_t *) malloc(len);   // 16-byte aligned by the allocator
    memset(buf, 0xA5, len);
    const uint64_t zoff = 0;
    ChunkDesc d = {};
    const uint64_t off = (uint64_t) (uintptr_t) buf;
    const uint64_t amask = len > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
    d.a = off & ~amask;
    d.h = (uint32_t) (off & amask);
    d.vlen = d.h + len;
    d.nsteps = len >= 4 ? (uint32_t) ((d.vlen + kStep - 1) / kStep) : 0;
    fill_tiny(buf, &zoff, &len, 1, 0, 1);
    for (uint64_t w = 0; w < W; ++w) {
        for (uint32_t lane = 0; lane < (uint32_t) kWave; ++lane) {
            fill_wave(buf, &d, &zoff, &len, 1, d.nsteps, W, w, lane);
        }
    }
    int rc = 0;
    for (uint64_t k = 0; k < len; ++k) {
        rc |= buf[k] != 0;
    }
    free(buf);
    if (rc) {
        fprintf(stderr, "grow_check: zero region of %llu bytes, W = %u: not zero\n", (unsigned long long) len, W);
    }
    return rc;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(1);
    const size_t B = kGrowBlock;
    const size_t ns[] = {1, 2, 63, B - 1, B, B + 1, 3 * B + 17, B * B - 1, B * B, B * B + 3};
    const uint64_t reallocs[] = {1, 4096, 32768, 1ull << 40};
    int it = 0;
    // every align, page 1 and 4096, every realloc_size, n on both sides of the workgroup size and of its square
    for (uint64_t align = 1; align <= 4096; align <<= 1) {
        for (uint64_t page : {1ull, 4096ull}) {
            for (uint64_t realloc_size : reallocs) {
                for (size_t n : ns) {
                    if (n > 4 * B && (it++ % 41) != 0) {
                        continue;                  // the long batches: a sample of the parameter triples
                    }
                    Batch b = random_batch(n, align, page, realloc_size, rng);
                    const Result full = sequential(b);
                    if (check(b, "unbounded", rng)) {
                        return 1;
                    }
                    b.end = b.top + full.total / 2 + rng() % 3;     // a cut somewhere in the middle
                    b.dev_bytes = b.end + rng() % 2;
                    if (check(b, "cut", rng)) {
                        return 1;
                    }
                    b.dev_bytes = b.end - 1;                        // the arena leaves the buffer: nothing grows
                    if (check(b, "arena outside", rng)) {
                        return 1;
                    }
                }
            }
        }
    }
    // the arena cutting a batch at every position (one byte short of slot k's end, and exactly at it): every
    // entry of a short batch, and every entry around a workgroup boundary of a longer one
    for (uint64_t align : {1ull, 16ull, 4096ull}) {
        for (uint64_t page : {1ull, 4096ull}) {
            for (size_t n : {(size_t) 150, B + 40}) {
                Batch b = random_batch(n, align, page, page == 1 ? 1 : 4096, rng);
                const Result full = sequential(b);
                for (size_t k = n > B ? B - 30 : 0; k < n; ++k) {
                    if (full.offs[k] == b.img[k].off) {
                        continue;                  // not a growing image
                    }
                    const uint64_t end = full.offs[k] + grow_slot(full.caps[k], align);
                    for (uint64_t cut : {end - 1, end}) {
                        b.end = b.dev_bytes = cut;
                        if (check(b, "cut at every position", rng)) {
                            return 1;
                        }
                    }
                }
                b.end = b.dev_bytes = b.top;       // no room at all
                if (check(b, "no room", rng)) {
                    return 1;
                }
                b.end = b.top - 1;                 // top beyond end
                if (check(b, "top beyond end", rng)) {
                    return 1;
                }
            }
        }
    }
    // images inside the arena's free part, and touching it from either side
    for (int rep = 0; rep < 40; ++rep) {
        Batch b = random_batch(rep % 2 ? 300 : B + 7, 16, 4096, 32768, rng);
        const size_t n = b.img.size();
        b.top = b.img[n / 2].off + (rep % 3 == 0 ? b.img[n / 2].cap : rep % 3 == 1 ? b.img[n / 2].cap - 1 : 0);
        b.end = b.img[n - n / 4].off + (rep % 5 == 0 ? 1 : 0);
        b.dev_bytes = kPlaceOver - 1;
        if (check(b, "images inside the arena", rng)) {
            return 1;
        }
    }
    // needs that saturate; content + need on both sides of 2^32 - 1; capacities near 2^64
    for (int rep = 0; rep < 60; ++rep) {
        const size_t n = rep % 3 == 0 ? 50 : rep % 3 == 1 ? 3 * B + 9 : B + 1;
        Batch b = random_batch(n, 1ull << (rep % 13), rep & 1 ? 4096 : 1, reallocs[rep % 4], rng);
        for (int k = 0; k < 6; ++k) {
            Img &m = b.img[rng() % n];
            m.valid = true;
            switch ((rep + k) % 6) {
            case 0: m.need = ~0ull; break;
            case 1: m.need = kGrowMaxContent - m.content; break;                  // exactly 2^32 - 1
            case 2: m.need = kGrowMaxContent - m.content + 1; break;
            case 3: m.need = (1ull << 32) + rng() % 3; break;
            case 4: m.need = (1ull << 63) + rng(); break;
            default:                               // a capacity near 2^64, from byte 0: the arena is then empty
                m.off = 0;
                m.cap = ~0ull - 1 - rng() % 70000;
                b.end = 0;
                m.need = m.cap - m.used + 1 + rng() % 1000;
                if (m.need > kGrowMaxContent) {
                    m.content = 0xfffff000u;
                    m.used = kReadHdr + m.content;
                    m.need = 0xfff;
                }
                break;
            }
        }
        if (rep % 4 == 0) {
            b.top = ~0ull - rng() % 5000;         // the top near 2^64: its alignment leaves 64 bits
        }
        if (check(b, "saturating", rng)) {
            return 1;
        }
    }
    // realloc_size near 2^64 with few steps, and slots whose alignment leaves 64 bits
    for (int rep = 0; rep < 30; ++rep) {
        Batch b = random_batch(200, rep % 2 ? 4096 : 1, rep % 3 ? 1 : 4096, ~0ull - rng() % 9000, rng);
        if (check(b, "realloc near 2^64", rng)) {
            return 1;
        }
        b.realloc_size = (1ull << 62) + rng() % 1000;
        if (check(b, "slots that sum past 2^64", rng)) {
            return 1;
        }
    }

    // the zero walk: the tails of the issue's list at every start residue modulo 16, alone (exact buffers)
    // and among others; one long tail among many short ones; random batches
    const uint64_t tails[] = {1, 2, 3, 4, 15, 16, 17, 31, 33, 4095, 4096, 4097, 8191, 8193, 12289, 70001};
    const uint32_t waves[] = {7, 64, 8192};       // not a power of two, few, the device's grid
    for (uint64_t len : tails) {
        for (uint32_t W : waves) {
            if (zero_exact(len, W)) {
                return 1;
            }
        }
        for (uint64_t res = 0; res < 16; ++res) {
            if (zero_batch({len}, res, waves[res % 3], false, -1, rng) ||
                zero_batch({3, len, 1, len, 17}, res, waves[(res + 1) % 3], true, -2, rng)) {
                return 1;
            }
        }
    }
    for (int iter = 0; iter < 60; ++iter) {
        const uint32_t n = 1 + (uint32_t) (rng() % 300);
        std::vector<uint64_t> lens(n);
        for (uint64_t &l : lens) {
            l = rng() % 5 == 0 ? tails[rng() % 16] : rng() % 5 == 1 ? 0 : rng() % 70;
        }
        if (iter % 3 == 0) {
            lens[rng() % n] = (1 << 20) + rng() % 4097;            // one long tail among many short ones
        }
        if (zero_batch(lens, rng() % 16, waves[iter % 3], iter % 2 == 0, iter, rng)) {
            return 1;
        }
    }
    puts("grow_check: ok");
    return 0;
}
