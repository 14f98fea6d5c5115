// alloc_check.cpp -- the allocation out of the pool set (alloc_set.h: the text
// the kernels allocset_class, allocset_serve, allocset_place and
// allocset_commit run), stand-alone on the host under ASan + UBSan: no GPU, no
// HIP.  `make alloccheck`.
//
// The chain is restated entry by entry -- the class ranks and the sums of the
// arena-bound slots as plain running sums (the scans themselves are
// poolsetcheck's and placecheck's) -- and everything a call leaves (statuses,
// offsets, capacities, every word of dev_total, every set word, the arena's
// top, and the number of entries that write the top) is compared with a
// sequential loop in 128-bit arithmetic, at every boundary of the rules: need
// 23 / 24, the class edges, align 1 and 4096, sums that leave 64 bits, an
// arena that ends in mid-batch, a class that runs dry, an entry that fails
// S3's check, an unsound set, no set, and an empty batch.  The set's arrays
// have EXACTLY n_cls * stride entries, so the sanitizer sees an index beyond.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "alloc_set.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int OK = 0, ERR = -1;
long g_cases = 0;

struct Case {
    uint32_t n_cls;
    uint64_t stride, align, dev_bytes, top, end;
    std::vector<uint64_t> words, offs, caps;      // exactly 4 n_cls and n_cls * stride entries
    std::vector<uint64_t> need;
    std::vector<int32_t> gate;                    // empty: no gate
};

struct Result {
    std::vector<int32_t> status;
    std::vector<uint64_t> off, cap, total, words;
    uint64_t top;
};

#define CHECK(c)                                                              \
    do {                                                                      \
        if (!(c)) {                                                           \
            fprintf(stderr, "alloc_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            abort();                                                          \
        }                                                                     \
    } while (0)

// The kernels' chain over alloc_set.h.
Result run_chain(const Case &t)
{
    const size_t n = t.need.size();
    const uint64_t *set = t.words.data();
    Result r;
    r.status.assign(n, ERR);
    r.off.assign(n, kPlaceOver);
    r.cap.assign(n, 0);
    r.total.assign(2 + t.n_cls, 0);
    r.words = t.words;
    r.top = t.top;
    const uint32_t usable = set_usable(set, t.n_cls, t.stride, t.align);
    std::vector<uint64_t> seen(kPoolSetMax, 0), before(n, 0), cap(n, 0), off(n, kPlaceOver);
    std::vector<uint32_t> code(n, 0);
    uint64_t run = 0;
    for (size_t i = 0; i < n; ++i) {              // allocset_class + allocset_serve
        const uint64_t ncap = alloc_new_cap(!t.gate.empty(), t.gate.empty() ? 0 : t.gate[i], t.need[i]);
        before[i] = run;
        if (ncap == 0) {
            continue;
        }
        const uint32_t cls = set_grow_class(set, t.n_cls, usable, ncap);
        uint64_t j = 0, F = 0, aslot = 0;
        if (cls != kSetNone) {
            j = seen[cls]++;
            F = set_serves(set, cls, usable);
        }
        code[i] = (cls << kSetClsShift) |
                  alloc_serve(set, t.offs.data(), t.caps.data(), t.stride, cls, j, F, ncap, t.dev_bytes, t.align,
                              off[i], cap[i], aslot);
        run = place_add(run, aslot);
    }
    uint64_t taken = 0;
    for (uint32_t k = 0; k < t.n_cls; ++k) {      // allocset_cscan
        const uint64_t F = set_serves(set, k, usable);
        bool changed;
        const uint64_t e = set_grow_end(set[4 * k + kPoolCount], F, seen[k], changed);
        CHECK(changed == (e != set[4 * k + kPoolCount]));
        r.words[4 * k + kPoolCount] = e;
        r.total[2 + k] = seen[k];
        taken += seen[k] < F ? seen[k] : F;
    }
    r.total[1] = taken;
    r.total[0] = grow_total(t.top, t.align, run); // allocset_ascan
    int writers = 0;
    for (size_t i = 0; i < n; ++i) {              // allocset_place + allocset_commit
        uint64_t etop = 0;
        const uint32_t c = alloc_place(code[i], t.top, t.end, t.dev_bytes, t.align, before[i], cap[i], i + 1 == n,
                                       off[i], etop);
        if (c & kAllocAccepted) {
            r.status[i] = OK;
            r.off[i] = off[i];
            r.cap[i] = cap[i];
        }
        if (c & (kGrowTopAt | kGrowTopEnd)) {
            ++writers;
            r.top = etop;
        }
    }
    CHECK(writers <= 1);
    return r;
}

u128 up(u128 v, uint64_t a)
{
    return (v + (a - 1)) / a * a;
}

uint64_t sat(u128 v)
{
    return v >= (u128) kPlaceOver ? kPlaceOver : (uint64_t) v;
}

// The header's rules, sequentially, in 128-bit arithmetic.
Result run_rules(const Case &t)
{
    const size_t n = t.need.size();
    Result r;
    r.status.assign(n, ERR);
    r.off.assign(n, kPlaceOver);
    r.cap.assign(n, 0);
    r.total.assign(2 + t.n_cls, 0);
    r.words = t.words;
    r.top = t.top;
    bool sound = true;
    for (uint32_t k = 0; k < t.n_cls; ++k) {
        const uint64_t *p = &t.words[4 * k];
        const bool pal = p[3] >= 1 && p[3] <= 4096 && (p[3] & (p[3] - 1)) == 0;
        if (p[0] > p[1] || p[2] < 24 || !pal || p[1] > t.stride || (k && p[2] <= t.words[4 * (k - 1) + 2])) {
            sound = false;
        }
    }
    std::vector<uint64_t> F(t.n_cls, 0), seen(t.n_cls, 0);
    std::vector<bool> usable(t.n_cls, false);
    for (uint32_t k = 0; k < t.n_cls; ++k) {
        usable[k] = sound && t.words[4 * k + 3] % t.align == 0;
        F[k] = usable[k] ? t.words[4 * k] : 0;
    }
    const u128 base = up(t.top, t.align);
    u128 run = 0;
    for (size_t i = 0; i < n; ++i) {
        if ((!t.gate.empty() && t.gate[i] != OK) || t.need[i] < 24) {
            continue;
        }
        int c = -1;
        for (uint32_t k = 0; k < t.n_cls && c < 0; ++k) {
            if (usable[k] && t.words[4 * k + 2] >= t.need[i]) {
                c = (int) k;
            }
        }
        if (c >= 0) {
            const uint64_t j = seen[c]++;
            if (j < F[c]) {
                const size_t e = (size_t) (c * t.stride + F[c] - 1 - j);
                CHECK(e < t.offs.size());
                const uint64_t eo = t.offs[e], ec = t.caps[e];
                if ((u128) eo + ec <= t.dev_bytes && ec >= t.words[4 * c + 2] && eo % t.align == 0) {
                    r.status[i] = OK;
                    r.off[i] = eo;
                    r.cap[i] = ec;
                }
                continue;
            }
        }
        const uint64_t cap = c >= 0 ? t.words[4 * c + 2] : t.need[i];
        const u128 slot = up(cap, t.align), off = base + run;
        // the kernels' sums saturate at 2^64 - 1: a value that reaches it counts as out
        const bool in64 = sat(base) != kPlaceOver && sat(run) != kPlaceOver && sat(slot) != kPlaceOver &&
                          sat(off) != kPlaceOver && sat(off + slot) != kPlaceOver;
        if (t.end <= t.dev_bytes && in64 && off + slot <= t.end) {
            r.status[i] = OK;
            r.off[i] = (uint64_t) off;
            r.cap[i] = cap;
            r.top = (uint64_t) (off + slot);
        }
        run = sat(run) == kPlaceOver || sat(slot) == kPlaceOver ? (u128) kPlaceOver : run + slot;
        run = sat(run);
    }
    r.total[0] = run == 0 ? 0 : sat(base) == kPlaceOver ? kPlaceOver : sat(base - t.top + run);
    for (uint32_t k = 0; k < t.n_cls; ++k) {
        const uint64_t take = seen[k] < F[k] ? seen[k] : F[k];
        r.words[4 * k] -= take;
        r.total[1] += take;
        r.total[2 + k] = seen[k];
    }
    return r;
}

void compare(const Case &t)
{
    CHECK(t.words.size() == 4 * (size_t) t.n_cls && t.offs.size() == t.n_cls * t.stride &&
          t.caps.size() == t.offs.size());
    const Result a = run_chain(t), b = run_rules(t);
    CHECK(a.status == b.status);
    CHECK(a.off == b.off);
    CHECK(a.cap == b.cap);
    CHECK(a.total == b.total);
    CHECK(a.words == b.words);
    CHECK(a.top == b.top);
    ++g_cases;
}

Case make_set(uint32_t n_cls, uint64_t stride, uint64_t align, const uint64_t *cls, uint64_t fill, uint64_t dev_bytes)
{
    Case t;
    t.n_cls = n_cls;
    t.stride = stride;
    t.align = align;
    t.dev_bytes = dev_bytes;
    uint64_t at = 0;
    for (uint32_t k = 0; k < n_cls; ++k) {
        const uint64_t have = fill < stride ? fill : stride;
        const uint64_t w[4] = {have, stride, cls[k], 4096};
        t.words.insert(t.words.end(), w, w + 4);
        for (uint64_t e = 0; e < stride; ++e) {
            t.offs.push_back(at);
            t.caps.push_back(cls[k] + (e & 1));           // some entries larger than the class
            at += (cls[k] + 1 + 4095) / 4096 * 4096;
        }
    }
    t.top = at;
    t.end = dev_bytes;
    return t;
}

void boundaries()
{
    CHECK(alloc_new_cap(false, 0, 23) == 0 && alloc_new_cap(false, 0, 24) == 24 && alloc_new_cap(false, 0, 0) == 0);
    CHECK(alloc_new_cap(true, 0, 24) == 24 && alloc_new_cap(true, -1, 24) == 0 && alloc_new_cap(true, -3, 4096) == 0);
    CHECK(alloc_new_cap(false, -1, 24) == 24);    // the gate's value is not looked at without a gate
    const uint64_t cls[3] = {64, 512, 4096};
    for (uint64_t align : {1ull, 16ull, 4096ull}) {
        for (uint64_t fill : {0ull, 1ull, 2ull, 4ull}) {
            Case t = make_set(3, 4, align, cls, fill, 1ull << 22);
            t.need = {23, 24, 63, 64, 65, 511, 512, 513, 4095, 4096, 4097, 0, 24, 64, 64, 64, 64, 64, 5000};
            compare(t);                           // class edges; a class that runs dry in mid-batch
            t.gate.assign(t.need.size(), OK);
            t.gate[1] = ERR;
            t.gate[4] = -3;
            t.gate[9] = 1;
            compare(t);
            t.end = t.top + 3 * 4096 + 100;       // the arena ends in mid-batch; pool-served entries behind it
            compare(t);
            t.end = t.dev_bytes + 1;              // an arena beyond the buffer takes nothing
            compare(t);
            t.end = t.dev_bytes;
            t.offs[1] = t.dev_bytes - 10;         // entries that fail S3: outside, too small, unaligned
            t.caps[4 + 1] = 511;
            t.offs[8 + 1] += 1;
            compare(t);
            t.offs[0] = ~0ull - 3;                // off + cap wraps
            compare(t);
        }
    }
    {   // an unsound set (cls not rising; a count above the capacity; a capacity above the stride) is the arena alone
        Case t = make_set(3, 4, 16, cls, 4, 1ull << 22);
        t.need = {24, 64, 512, 4096, 100};
        Case u = t;
        u.words[4 + 2] = 64;
        compare(u);
        u = t;
        u.words[0] = 5;
        compare(u);
        u = t;
        u.words[8 + 1] = 5;
        compare(u);
        u = t;
        u.words[3] = 8;                           // pal no multiple of align: that class alone is unusable
        compare(u);
    }
    {   // no set, and an empty batch
        Case t;
        t.n_cls = 0;
        t.stride = 0;
        t.align = 4096;
        t.dev_bytes = 1 << 20;
        t.top = 5;
        t.end = 1 << 20;
        compare(t);
        t.need = {24, 4096, 4097, 23, 1ull << 19, 1ull << 19};
        compare(t);
        t.align = 1;
        compare(t);
    }
    {   // sums that leave 64 bits: the top near 2^64, needs near 2^63
        Case t;
        t.n_cls = 0;
        t.stride = 0;
        t.dev_bytes = ~0ull;
        t.end = ~0ull;
        for (uint64_t align : {1ull, 4096ull}) {
            t.align = align;
            t.top = 0;
            t.need = {1ull << 63, 1ull << 63, 24, ~0ull, ~0ull - 4095, 24};
            compare(t);
            t.top = ~0ull - 100;
            t.need = {24, 24, 200, 24};
            compare(t);
            t.top = ~0ull - 4096;
            compare(t);
            t.top = ~0ull;
            compare(t);
            t.top = 1ull << 63;
            t.need = {(1ull << 63) - 4096, 4095, 1, 24, 4096};
            compare(t);
        }
    }
}

void random_cases()
{
    std::mt19937_64 rng(20261);
    const uint64_t cls[8] = {24, 100, 256, 700, 1024, 4096, 10000, 65536};
    for (int it = 0; it < 4000; ++it) {
        const uint32_t n_cls = (uint32_t) (rng() % 9);
        const uint64_t stride = 1 + rng() % 6, align = 1ull << (rng() % 13);
        Case t = make_set(n_cls, stride, align, cls, rng() % 7, (1ull << 26) + rng() % 4096);
        for (uint32_t k = 0; k < n_cls; ++k) {
            t.words[4 * k + 3] = 1ull << (rng() % 13);
        }
        if (rng() % 16 == 0 && n_cls) {
            t.words[rng() % t.words.size()] = rng() % 5000;
        }
        t.top = t.top + rng() % 5000;
        t.end = rng() % 3 ? t.dev_bytes : t.top + rng() % 200000;
        const size_t n = rng() % 70;
        for (size_t i = 0; i < n; ++i) {
            const uint64_t pick = rng() % 10;
            t.need.push_back(pick == 0 ? rng() % 24 : pick == 1 ? cls[rng() % 8] + (rng() % 3) - 1 : 24 + rng() % 70000);
        }
        if (rng() % 2) {
            for (size_t i = 0; i < n; ++i) {
                t.gate.push_back(rng() % 5 ? OK : -(int32_t) (rng() % 4));
            }
        }
        for (size_t e = 0; e < t.offs.size(); ++e) {
            if (rng() % 23 == 0) {
                t.offs[e] = rng();
            }
            if (rng() % 23 == 0) {
                t.caps[e] = rng() % 3 ? rng() % 5000 : rng();
            }
        }
        compare(t);
    }
}

}  // namespace

int main()
{
    boundaries();
    random_cases();
    printf("alloc_check: %ld cases passed\n", g_cases);
    return 0;
}
