// place_check.cpp -- the device read path's placement (read_dev_place.h: the
// text the kernels read_headers, read_scan and read_place run), stand-alone on
// the host under ASan + UBSan: no GPU, no HIP.  `make placecheck`.
//
// The three kernels are restated workgroup by workgroup -- the workgroup scan
// as the kernels do it, in log steps with place_add -- and run with the
// workgroups of each kernel in ascending, descending and random order (no
// workgroup may depend on another of its kernel).  Offsets, total and
// acceptance are compared with a sequential running sum in 128-bit arithmetic.
// Lengths only, no data.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "read_dev_place.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;

struct Batch {
    std::vector<uint64_t> len;
    std::vector<uint8_t> ok;
    uint64_t nul, align, out_bytes;
};

struct Result {
    std::vector<uint64_t> offs;
    std::vector<uint8_t> accepted;
    uint64_t total;
    bool operator==(const Result &o) const { return offs == o.offs && accepted == o.accepted && total == o.total; }
};

Result kernels(const Batch &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.len.size();
    const uint32_t nb = (uint32_t) ((n + kReadBlock - 1) / kReadBlock);
    std::vector<uint64_t> dst(n), rtot(nb), sh(kReadBlock), excl(kReadBlock);
    std::vector<uint8_t> status(n);
    // read_headers<PACKED>
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kReadBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kReadBlock + t;
            sh[t] = i < n && b.ok[i] ? place_slot(b.len[i], b.nul, b.align) : 0;
        }
        wg_scan(kReadBlock, sh, excl, rtot[wg]);
        for (uint32_t t = 0; t < kReadBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kReadBlock + t;
            if (i < n) {
                dst[i] = excl[t];
                status[i] = b.ok[i];
            }
        }
    }
    // read_scan: one workgroup, pass by pass
    Result r;
    const uint64_t carry = scan_totals(kReadBlock, rtot.data(), nb);
    r.total = carry;
    // read_place
    r.offs.resize(n);
    r.accepted.resize(n);
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kReadBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kReadBlock + t;
            if (i >= n) {
                break;
            }
            const uint64_t before = place_add(rtot[wg], dst[i]);
            r.offs[i] = before;
            r.accepted[i] = status[i] && place_fits(before, place_slot(b.len[i], b.nul, b.align), b.out_bytes);
        }
    }
    return r;
}

Result sequential(const Batch &b)
{
    const u128 over = (u128) kPlaceOver;
    Result r;
    u128 run = 0;
    for (size_t i = 0; i < b.len.size(); ++i) {
        u128 slot = 0;
        if (b.ok[i]) {
            slot = ((u128) b.len[i] + b.nul + (b.align - 1)) & ~(u128) (b.align - 1);
            slot = std::min(slot, over);
        }
        r.offs.push_back((uint64_t) std::min(run, over));
        r.accepted.push_back(b.ok[i] && run < over && run + slot < over && run + slot <= (u128) b.out_bytes);
        run = std::min(run + slot, over);          // once out of 64 bits, out for good
    }
    r.total = (uint64_t) run;
    return r;
}

int check(const Batch &b, const char *what, std::mt19937_64 &rng)
{
    const Result want = sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(kernels(b, order, rng) == want)) {
            fprintf(stderr, "place_check: %s: n = %zu, align = %llu, nul = %llu, out_bytes = %llu, order %d differs\n",
                    what, b.len.size(), (unsigned long long) b.align, (unsigned long long) b.nul,
                    (unsigned long long) b.out_bytes, order);
            return 1;
        }
    }
    return 0;
}

Batch random_batch(size_t n, uint64_t align, uint64_t nul, uint64_t maxlen, std::mt19937_64 &rng)
{
    Batch b;
    b.len.resize(n);
    b.ok.resize(n);
    for (size_t i = 0; i < n; ++i) {
        b.len[i] = rng() % 8 == 0 ? 0 : rng() % maxlen;
        b.ok[i] = rng() % 7 != 0;                  // failed entries sprinkled in
    }
    b.nul = nul;
    b.align = align;
    b.out_bytes = ~0ull;
    return b;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(1);
    const size_t B = kReadBlock;
    const size_t ns[] = {1, 2, 63, B - 1, B, B + 1, 3 * B + 17, B * B - 1, B * B, B * B + 3};
    int it = 0;
    // every align, NUL on and off, n on both sides of the workgroup size and of its square
    for (uint64_t align = 1; align <= 4096; align <<= 1) {
        for (uint64_t nul = 0; nul < 2; ++nul) {
            for (size_t n : ns) {
                if (n > 4 * B && (it++ % 7) != 0) {
                    continue;                      // the long batches: a sample of the (align, nul) pairs
                }
                Batch b = random_batch(n, align, nul, 70000, rng);
                const Result full = sequential(b);
                if (check(b, "unbounded", rng)) {
                    return 1;
                }
                b.out_bytes = full.total / 2 + rng() % 3;   // a cut somewhere in the middle
                if (check(b, "cut", rng)) {
                    return 1;
                }
            }
        }
    }
    // out_bytes cutting a batch at every position (one byte short of entry k's end, and exactly at it):
    // every entry of a short batch, and every entry around a workgroup boundary of a longer one
    for (uint64_t align : {1ull, 16ull, 4096ull}) {
        for (uint64_t nul = 0; nul < 2; ++nul) {
            for (size_t n : {(size_t) 150, B + 40}) {
                Batch b = random_batch(n, align, nul, 300, rng);
                const Result full = sequential(b);
                for (size_t k = n > B ? B - 30 : 0; k < n; ++k) {
                    const uint64_t end = full.offs[k] + (b.ok[k] ? place_slot(b.len[k], nul, align) : 0);
                    for (uint64_t cut : {end - (end ? 1 : 0), end}) {
                        b.out_bytes = cut;
                        if (check(b, "cut at every position", rng)) {
                            return 1;
                        }
                    }
                }
                b.out_bytes = 0;
                if (check(b, "no room", rng)) {
                    return 1;
                }
            }
        }
    }
    // totals that cross 2^32: inside a workgroup, between workgroups, between passes of the scan
    for (size_t n : {(size_t) 40, B + 5, 5 * B, B * B + 3}) {
        Batch b = random_batch(n, 64, 1, n > 100 * B ? (1ull << 14) : (1ull << 32), rng);
        const Result full = sequential(b);
        if (full.total <= (1ull << 32)) {
            fprintf(stderr, "place_check: the 2^32 batch is too small\n");
            return 1;
        }
        b.out_bytes = (1ull << 32) + 12345;
        if (check(b, "2^32", rng)) {
            return 1;
        }
    }
    // synthetic lengths whose sum leaves 64 bits: at an entry, at a workgroup boundary, in the scan
    for (int rep = 0; rep < 12; ++rep) {
        const size_t n = rep % 3 == 0 ? 50 : rep % 3 == 1 ? 3 * B + 9 : 1100 * B;
        Batch b = random_batch(n, 1ull << (rep % 13), rep & 1, 5000, rng);
        const size_t at = rng() % n, at2 = rng() % n;
        b.len[at] = (1ull << 63) + rng() % 1000;
        b.ok[at] = 1;
        b.len[at2] = rep % 4 == 3 ? ~0ull - rng() % 3 : (1ull << 63) - rng() % 3000;
        b.ok[at2] = 1;
        const Result full = sequential(b);
        if (full.total != kPlaceOver) {
            fprintf(stderr, "place_check: the overflow batch does not overflow\n");
            return 1;
        }
        if (check(b, "2^64", rng)) {
            return 1;
        }
    }
    // the record selection and the caller-placed slot rule
    uint64_t first, len;
    place_select(kReadMeta, 7, 100, first, len);
    bool ok = first == 24 && len == 7;
    place_select(kReadContent, 7, 100, first, len);
    ok = ok && first == 31 && len == 100;
    place_select(kReadImage, 65535, 0xffffffffull, first, len);
    ok = ok && first == 0 && len == 24 + 65535 + 0xffffffffull;
    ok = ok && placed_fits(10, 5, 15, 5, 0) && !placed_fits(10, 5, 15, 5, 1) && !placed_fits(11, 5, 15, 4, 0) &&
         placed_fits(0, 0, 0, 0, 0) && !placed_fits(0, 0, 0, 0, 1) && !placed_fits(~0ull - 1, 4, ~0ull, 1, 0) &&
         placed_fits(3, 1, 4, 0, 1);
    if (!ok) {
        fprintf(stderr, "place_check: record selection / placed slot rule\n");
        return 1;
    }
    puts("place_check: ok");
    return 0;
}
