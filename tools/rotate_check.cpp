// rotate_check.cpp -- rotating full chunk images (rotate_dev.h: the text the
// kernels rotate_sums_wave, rotate_headers, rotate_scan, rotate_place and
// rotate_commit run), stand-alone on the host under ASan + UBSan: no GPU, no
// HIP.  `make rotatecheck`.
//
// Bookkeeping: the header, scan, place and commit kernels are restated
// workgroup by workgroup -- the workgroup scan as the kernels do it, in log
// steps with place_add -- and run with the workgroups of each kernel in
// ascending, descending and random order (no workgroup may depend on another
// of its kernel).  Statuses, offsets, capacities, the list of finished chunks
// (in arrays of EXACTLY the list's capacity, so the sanitizer sees an entry
// beyond it), both totals, the arena's top and the list's count, and the
// number of threads that write each of the two, are compared with a sequential
// loop in 128-bit arithmetic.  The images are given by their fields: no data.
//
// Sums: the wave-level pre-reduction (rot_wave_sums, the kernel's steps over
// an explicit array of 64 lanes) wave by wave against a sequential sum.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "rotate_dev.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int OK = 0, ERR = -1;

struct Img {
    uint64_t off, cap, content, need;
    uint32_t meta;
    bool valid;                               // the write path's image check
};

struct Batch {
    std::vector<Img> img;
    uint64_t top, end, dev_bytes, limit, new_cap, align, have, list_cap;
};

struct Result {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps, lo, lc;  // after the commit; the list's offsets and capacities
    std::vector<uint32_t> li;
    uint64_t total[2], top, count;
    int top_writers, count_writers;
    bool operator==(const Result &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && lo == o.lo && lc == o.lc && li == o.li &&
               total[0] == o.total[0] && total[1] == o.total[1] && top == o.top && count == o.count &&
               top_writers == o.top_writers && count_writers == o.count_writers;
    }
};

const uint64_t kUnwritten = 0x7777777777777777ull;

// The list arrays hold min(list_cap, a bound) entries: exactly the capacity
// where that can be allocated.
size_t list_len(const Batch &b)
{
    return (size_t) std::min<uint64_t>(b.list_cap, b.have + b.img.size() + 1);
}

Result kernels(const Batch &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.img.size();
    const uint32_t nb = (uint32_t) ((n + kRotBlock - 1) / kRotBlock);
    std::vector<uint64_t> hlen(n), ord(n), roff(n), rk(n), rtot(nb), sh(kRotBlock), excl(kRotBlock);
    std::vector<uint32_t> code(n);
    Result r;
    r.status.assign(n, OK);
    r.offs.resize(n);
    r.caps.resize(n);
    r.lo.assign(list_len(b), kUnwritten);
    r.lc.assign(list_len(b), kUnwritten);
    r.li.assign(list_len(b), 0x77777777u);
    uint64_t arena[2] = {b.top, b.end}, out_count[2] = {b.have, b.list_cap};
    const uint64_t slot = grow_round_up(b.new_cap, b.align);
    // rotate_headers
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kRotBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kRotBlock + t;
            uint64_t hl = 0;
            if (i < n) {
                const Img &m = b.img[i];
                r.offs[i] = m.off;
                r.caps[i] = m.cap;
                if (m.need != 0 || b.limit != 0) {
                    if (!m.valid) {
                        r.status[i] = ERR;
                    } else {
                        const int v = rot_decide(m.off, m.cap, m.meta, m.content, m.need, b.limit, b.new_cap,
                                                 arena[0], arena[1]);
                        if (v == kRotReject) {
                            r.status[i] = ERR;
                        } else if (v == kRotFull) {
                            hl = kReadHdr + m.meta;
                        }
                    }
                }
                hlen[i] = hl;
            }
            sh[t] = hl ? 1 : 0;
        }
        wg_scan(kRotBlock, sh, excl, rtot[wg]);
        for (uint32_t t = 0; t < kRotBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kRotBlock + t;
            if (i < n) {
                ord[i] = excl[t];
            }
        }
    }
    // rotate_scan: one workgroup, pass by pass
    const uint64_t carry = scan_totals(kRotBlock, rtot.data(), nb);
    r.total[0] = rot_total(arena[0], b.align, carry, slot);
    r.total[1] = carry;
    // rotate_place
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kRotBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kRotBlock + t;
            if (i >= n) {
                break;
            }
            const uint64_t before = place_add(rtot[wg], ord[i]);
            code[i] = rot_place_code(arena[0], arena[1], b.dev_bytes, b.align, slot, out_count[0], out_count[1],
                                     before, hlen[i] != 0, i + 1 == n, roff[i], rk[i]);
            if (!(code[i] & kRotAccepted) && hlen[i] != 0) {
                r.status[i] = ERR;
            }
        }
    }
    // rotate_commit: every thread may run before or after the one store to the top and to the count, so no
    // thread reads either
    r.top_writers = r.count_writers = 0;
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kRotBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kRotBlock + t;
            if (i >= n) {
                break;
            }
            const uint32_t c = code[i];
            if (c & kRotAccepted) {
                r.lo.at(rk[i]) = r.offs[i];       // at(): an index beyond the capacity throws
                r.lc.at(rk[i]) = r.caps[i];
                r.li.at(rk[i]) = (uint32_t) i;
                r.offs[i] = roff[i];
                r.caps[i] = b.new_cap;
            }
            if (c & (kRotEndAt | kRotEndLast)) {
                rot_end_values(c, roff[i], rk[i], slot, arena[0], out_count[0]);
                const int w = 1 + ((c & kRotEndAt) && (c & kRotEndLast));
                r.top_writers += w;
                r.count_writers += w;
            }
        }
    }
    r.top = arena[0];
    r.count = out_count[0];
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
    r.lo.assign(list_len(b), kUnwritten);
    r.lc.assign(list_len(b), kUnwritten);
    r.li.assign(list_len(b), 0x77777777u);
    const u128 base = up128(b.top, b.align), slot = up128(b.new_cap, b.align);
    u128 reach = 0, accepted = 0;
    bool cut = false;
    for (size_t i = 0; i < n; ++i) {
        const Img &m = b.img[i];
        r.offs.push_back(m.off);
        r.caps.push_back(m.cap);
        if (m.need == 0 && b.limit == 0) {
            continue;
        }
        const bool overlap = b.top < b.end && m.cap != 0 && (u128) m.off < b.end && (u128) b.top < (u128) m.off + m.cap;
        if (!m.valid || overlap) {
            r.status[i] = ERR;
            continue;
        }
        const u128 used = (u128) kReadHdr + m.meta + m.content;
        const bool full = m.content > 0 && (used + m.need > m.cap || (b.limit != 0 && (u128) m.content + m.need > b.limit));
        if (!full) {
            continue;
        }
        if ((u128) kReadHdr + m.meta > b.new_cap) {
            r.status[i] = ERR;
            continue;
        }
        const u128 off = base + reach * slot, k = (u128) b.have + reach;
        ++reach;
        if (!cut && b.end <= b.dev_bytes && off + slot < over && off + slot <= (u128) b.end && k < (u128) b.list_cap) {
            r.lo.at((size_t) k) = m.off;
            r.lc.at((size_t) k) = m.cap;
            r.li.at((size_t) k) = (uint32_t) i;
            r.offs[i] = (uint64_t) off;
            r.caps[i] = b.new_cap;
            ++accepted;
        } else {
            cut = true;
            r.status[i] = ERR;
        }
    }
    const u128 slots = std::min(reach * slot, over);
    r.total[0] = reach == 0 ? 0 : base >= over ? kPlaceOver : (uint64_t) std::min(base - b.top + slots, over);
    r.total[1] = (uint64_t) reach;
    r.top = accepted ? (uint64_t) (base + accepted * slot) : b.top;
    r.count = b.have + (uint64_t) accepted;
    r.top_writers = r.count_writers = accepted ? 1 : 0;     // exactly one writer of each, or none
    return r;
}

int check(const Batch &b, const char *what, std::mt19937_64 &rng)
{
    const Result want = sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(kernels(b, order, rng) == want)) {
            fprintf(stderr,
                    "rotate_check: %s: n = %zu, align = %llu, new_cap = %llu, limit = %llu, top = %llu, end = %llu, "
                    "list %llu of %llu, order %d differs\n",
                    what, b.img.size(), (unsigned long long) b.align, (unsigned long long) b.new_cap,
                    (unsigned long long) b.limit, (unsigned long long) b.top, (unsigned long long) b.end,
                    (unsigned long long) b.have, (unsigned long long) b.list_cap, order);
            return 1;
        }
    }
    return 0;
}

// Images laid out one behind another from byte 64, the arena behind them, a
// list that takes all.  Kinds: not read / need 0, not full, exactly full, one
// byte over, empty and over, far over, invalid; a limit in half the batches.
Batch random_batch(size_t n, uint64_t align, uint64_t new_cap, std::mt19937_64 &rng)
{
    Batch b;
    b.img.resize(n);
    b.limit = rng() % 2 ? 3000 + rng() % 3000 : 0;
    uint64_t pos = 64;
    for (size_t i = 0; i < n; ++i) {
        Img &m = b.img[i];
        m.meta = rng() % 5 == 0 ? (uint32_t) (rng() % 300) : 0;
        m.content = rng() % 4 == 0 ? 0 : rng() % 6000;
        const uint64_t used = kReadHdr + m.meta + m.content;
        m.cap = used + rng() % 9000;
        m.off = pos;
        pos += m.cap + rng() % 40;
        m.valid = rng() % 9 != 0;
        const uint64_t room = m.cap - used;
        switch (rng() % 6) {
        case 0: m.need = 0; break;
        case 1: m.need = room ? rng() % room : 0; break;
        case 2: m.need = room; break;
        case 3: m.need = room + 1; break;
        case 4: m.need = room + 1 + rng() % 200000; break;
        default: m.need = b.limit ? b.limit - std::min(b.limit, m.content) + rng() % 2 : room + 1; break;
        }
    }
    b.top = pos + rng() % 5000;
    b.end = kPlaceOver - 1;
    b.dev_bytes = kPlaceOver - 1;
    b.new_cap = new_cap;
    b.align = align;
    b.have = rng() % 5;
    b.list_cap = b.have + n + 1;
    return b;
}

// ---------------------------------------------------------------- the sums

int sums(const std::vector<uint32_t> &img, const std::vector<uint64_t> &len, uint32_t n_img, const char *what)
{
    const size_t n_rec = img.size();
    std::vector<u128> want(n_img, 0);
    bool bad = false;
    for (size_t r = 0; r < n_rec; ++r) {
        if (img[r] >= n_img) {
            bad = true;
        } else {
            want[img[r]] += std::min<uint64_t>(len[r], kGrowLenClamp);
        }
    }
    std::vector<uint64_t> got(n_img, 0);
    bool flagged = false;
    size_t atomics = 0;
    for (size_t w0 = 0; w0 < n_rec; w0 += kRotLanes) {     // wave by wave, as the kernel's lanes load
        uint32_t key[kRotLanes];
        uint64_t v[kRotLanes], sum[kRotLanes];
        bool issue[kRotLanes];
        for (uint32_t l = 0; l < kRotLanes; ++l) {
            key[l] = kRotNoImage;
            v[l] = 0;
            if (w0 + l < n_rec) {
                if (img[w0 + l] >= n_img) {
                    flagged = true;
                } else {
                    key[l] = img[w0 + l];
                    v[l] = std::min<uint64_t>(len[w0 + l], kGrowLenClamp);
                }
            }
        }
        rot_wave_sums(key, v, n_img, sum, issue);
        for (uint32_t l = 0; l < kRotLanes; ++l) {
            if (issue[l]) {
                got.at(key[l]) += sum[l];
                ++atomics;
            }
        }
    }
    bool same = flagged == bad;
    for (uint32_t i = 0; i < n_img; ++i) {
        same = same && (u128) got[i] == want[i];
    }
    // never more atomics than records, and one per wave when all go to one image
    if (!same || atomics > n_rec) {
        fprintf(stderr, "rotate_check: sums: %s: %zu records, %u images differ\n", what, n_rec, n_img);
        return 1;
    }
    return 0;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(1);
    const size_t B = kRotBlock;
    const size_t ns[] = {1, 2, 63, B - 1, B, B + 1, 3 * B + 17, B * B - 1, B * B, B * B + 3};
    const uint64_t caps[] = {24, 25, 300, 4096, 70001};
    int it = 0;
    // every align, several new_cap, n on both sides of the workgroup size and of its square; the arena and the
    // list cutting somewhere in the middle, alone and together; an arena outside the buffer
    for (uint64_t align = 1; align <= 4096; align <<= 1) {
        for (uint64_t new_cap : caps) {
            for (size_t n : ns) {
                if (n > 4 * B && (it++ % 29) != 0) {
                    continue;                      // the long batches: a sample of the parameter pairs
                }
                Batch b = random_batch(n, align, new_cap, rng);
                const Result full = sequential(b);
                if (check(b, "unbounded", rng)) {
                    return 1;
                }
                const uint64_t end = b.top + full.total[0] / 2 + rng() % 3;
                const uint64_t cap = b.have + full.total[1] / 3;
                b.end = end;
                b.dev_bytes = b.end + rng() % 2;
                if (check(b, "arena cut", rng)) {
                    return 1;
                }
                b.list_cap = cap;
                if (check(b, "both cut", rng)) {
                    return 1;
                }
                b.end = b.dev_bytes = kPlaceOver - 1;
                if (check(b, "list cut", rng)) {
                    return 1;
                }
                b.list_cap = b.have + n + 1;
                b.end = end;
                b.dev_bytes = b.end - 1;           // the arena leaves the buffer: nothing is rotated
                if (check(b, "arena outside", rng)) {
                    return 1;
                }
            }
        }
    }
    // the arena and the list cutting a batch at every position (one byte short of slot k's end, and exactly at
    // it; a list of k and of k + 1 entries), and both at different places
    for (uint64_t align : {1ull, 16ull, 4096ull}) {
        for (size_t n : {(size_t) 150, B + 40}) {
            Batch b = random_batch(n, align, 300, rng);
            const Result full = sequential(b);
            const uint64_t base = grow_round_up(b.top, align), slot = grow_round_up(b.new_cap, align);
            const uint64_t reach = full.total[1], list_all = b.list_cap;
            for (uint64_t k = reach > 80 ? reach - 80 : 0; k <= reach; ++k) {
                for (uint64_t cut : {base + k * slot - 1, base + k * slot}) {
                    b.end = b.dev_bytes = cut;
                    b.list_cap = list_all;
                    if (check(b, "arena cut at every position", rng)) {
                        return 1;
                    }
                    b.list_cap = b.have + (k * 7 + 3) % (reach + 1);
                    if (check(b, "both cuts at once", rng)) {
                        return 1;
                    }
                }
                b.end = b.dev_bytes = kPlaceOver - 1;
                b.list_cap = b.have + k;
                if (check(b, "list cut at every position", rng)) {
                    return 1;
                }
            }
            b.list_cap = list_all;
            b.end = b.dev_bytes = b.top;           // no room at all
            if (check(b, "no room", rng)) {
                return 1;
            }
            b.end = b.top - 1;                     // top beyond end
            if (check(b, "top beyond end", rng)) {
                return 1;
            }
            b.end = b.dev_bytes = kPlaceOver - 1;
            b.list_cap = b.have ? b.have - 1 : 0;  // a count beyond the capacity
            if (check(b, "count beyond capacity", rng)) {
                return 1;
            }
        }
    }
    // images inside the arena's free part, and touching it from either side
    for (int rep = 0; rep < 40; ++rep) {
        Batch b = random_batch(rep % 2 ? 300 : B + 7, 16, 4096, rng);
        const size_t n = b.img.size();
        b.top = b.img[n / 2].off + (rep % 3 == 0 ? b.img[n / 2].cap : rep % 3 == 1 ? b.img[n / 2].cap - 1 : 0);
        b.end = b.img[n - n / 4].off + (rep % 5 == 0 ? 1 : 0);
        b.dev_bytes = kPlaceOver - 1;
        if (check(b, "images inside the arena", rng)) {
            return 1;
        }
    }
    // need and limit near 2^64; the top near 2^64; new_cap near 2^64; new_cap around 24 + meta
    for (int rep = 0; rep < 90; ++rep) {
        const size_t n = rep % 3 == 0 ? 50 : rep % 3 == 1 ? 3 * B + 9 : B + 1;
        Batch b = random_batch(n, 1ull << (rep % 13), rep % 2 ? 24 : 100, rng);
        for (int k = 0; k < 8; ++k) {
            Img &m = b.img[rng() % n];
            m.valid = true;
            switch ((rep + k) % 5) {
            case 0: m.need = ~0ull; break;
            case 1: m.need = ~0ull - (kReadHdr + m.meta + m.content) + rng() % 3; break;   // used + need around 2^64
            case 2: m.need = ~0ull - m.content + rng() % 2; break;                          // content + need around it
            case 3: m.need = (1ull << 63) + rng(); break;
            default: m.content = m.content ? m.content : 1; m.cap = kReadHdr + m.meta + m.content; m.need = 1; break;
            }
        }
        if (rep % 3 == 0) {
            b.limit = ~0ull - rng() % 3;
        }
        if (rep % 4 == 0) {
            b.top = ~0ull - rng() % 5000;          // its alignment leaves 64 bits
        }
        if (rep % 5 == 0) {
            b.new_cap = ~0ull - rng() % 5000;      // the slot's alignment leaves 64 bits
        }
        if (rep % 7 == 0) {
            b.have = ~0ull - rng() % 3;            // the list index leaves 64 bits; the list is full
            b.list_cap = b.have;
        }
        if (check(b, "saturating", rng)) {
            return 1;
        }
    }
    for (uint32_t meta : {0u, 1u, 40u, 65535u}) {
        for (uint64_t new_cap : {(uint64_t) 24, (uint64_t) 24 + meta - 1, (uint64_t) 24 + meta}) {
            if (new_cap < 24) {
                continue;
            }
            Batch b = random_batch(200, 8, new_cap, rng);
            for (Img &m : b.img) {
                m.meta = meta;
                m.cap = kReadHdr + meta + m.content + 5;
            }
            if (check(b, "new_cap around 24 + meta", rng)) {
                return 1;
            }
        }
    }

    // the fresh header and the seed: write_init_header's bytes, and crc_update over the two length bytes
    {
        uint8_t h[24];
        rot_fresh_header(h, 0x1234, true);
        const uint8_t want[24] = {0xc1, 0, 0xff, 0x12, 0xd9, 0x41, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0x12, 0x34};
        rot_fresh_header(h, 0x1234, true);
        if (memcmp(h, want, 24) != 0 || rot_len_seed(0) != 0xBE26ED00u) {
            fprintf(stderr, "rotate_check: the fresh header or the seed differs\n");
            return 1;
        }
        rot_fresh_header(h, 0, false);
        for (int k = 2; k < 24; ++k) {
            if (h[k] != 0) {
                fprintf(stderr, "rotate_check: the fresh header without checksum differs\n");
                return 1;
            }
        }
    }

    // the sums: runs of 1, 2, 63, 64, 65 and 1000 equal indices starting at every lane, alternating indices,
    // all records to one image, random lists, a malformed index
    for (uint32_t run : {1u, 2u, 63u, 64u, 65u, 1000u}) {
        for (uint32_t start = 0; start < kRotLanes; ++start) {
            std::vector<uint32_t> img;
            std::vector<uint64_t> len;
            for (uint32_t k = 0; k < start; ++k) {
                img.push_back(k % 2);              // a prefix that puts the first run's head at lane `start`
            }
            for (uint32_t g = 0; g < 5; ++g) {
                for (uint32_t k = 0; k < run; ++k) {
                    img.push_back(2 + g % 3);      // the same image again two runs later: separate runs
                }
            }
            for (size_t r = 0; r < img.size(); ++r) {
                len.push_back(rng() % 7 == 0 ? ~0ull - rng() % 9 : rng() % 5000);
            }
            if (sums(img, len, 5, "runs")) {
                return 1;
            }
        }
    }
    {
        std::vector<uint32_t> alt(1000), one(102400, 3), rnd(5000);
        std::vector<uint64_t> la(1000), lo(102400), lr(5000);
        for (size_t r = 0; r < alt.size(); ++r) {
            alt[r] = r % 2;
            la[r] = r;
        }
        for (size_t r = 0; r < one.size(); ++r) {
            lo[r] = 4096 + r % 3;
        }
        for (size_t r = 0; r < rnd.size(); ++r) {
            rnd[r] = (uint32_t) (rng() % 37);
            lr[r] = rng() % 100000;
        }
        if (sums(alt, la, 2, "alternating") || sums(one, lo, 4, "one image") || sums(rnd, lr, 37, "random")) {
            return 1;
        }
        for (size_t at : {(size_t) 0, (size_t) 63, (size_t) 64, rnd.size() - 1}) {
            std::vector<uint32_t> bad(rnd);
            bad[at] = at % 2 ? 37 : kRotNoImage;
            if (sums(bad, lr, 37, "malformed")) {
                return 1;
            }
        }
    }
    puts("rotate_check: ok");
    return 0;
}
