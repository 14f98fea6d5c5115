// pool_check.cpp -- recycling drained chunk slots (pool_dev.h: the text the
// kernels release_headers, release_scan, release_place, release_commit,
// rotpool_place and rotpool_commit run), stand-alone on the host under ASan +
// UBSan: no GPU, no HIP.  `make poolcheck`.
//
// Both chains are restated workgroup by workgroup -- the workgroup scan as the
// kernels do it, in log steps with place_add -- and run with the workgroups of
// each kernel in ascending, descending and random order (no workgroup may
// depend on another of its kernel).  Everything a call leaves -- statuses, the
// list (for a release in arrays of EXACTLY m entries, so the sanitizer sees an
// entry beyond them; for a rotation by index, an index at or beyond the list's
// capacity aborting), the pool's pushes (a push at or beyond the pool's
// capacity aborts), both totals, the pool's count, the arena's top, the list's
// count and dev_count[0], and the number of threads that write each of the
// four -- is compared with a sequential loop in 128-bit arithmetic.  The
// entries are given by their fields: no data.  rotate_headers and rotate_scan, which the pool
// variant runs unchanged, are rotate_check's; here an entry reaches the
// placement or does not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <map>
#include <numeric>
#include <random>
#include <vector>

#include "pool_dev.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int OK = 0, ERR = -1;
const uint64_t kUnwritten = 0x7777777777777777ull;

// The pool's arrays: a push beyond the capacity aborts.
struct PoolArrays {
    uint64_t cap;
    std::map<uint64_t, std::pair<uint64_t, uint64_t>> e;
    void push(uint64_t k, uint64_t off, uint64_t c)
    {
        if (k >= cap || e.count(k)) {
            fprintf(stderr, "pool_check: a push at %llu of %llu\n", (unsigned long long) k, (unsigned long long) cap);
            abort();
        }
        e[k] = {off, c};
    }
};

// ---------------------------------------------------------------- release

struct Ent {
    uint64_t off, cap;
    uint32_t img;
    bool live, gate_ok, valid;                // rules 1, 2, 3
};

struct Rel {
    std::vector<Ent> ent;                     // n entries; the list's arrays hold m of them
    bool has_count, compact;
    uint64_t count0, pool[4];
};

struct RelResult {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps;
    std::vector<uint32_t> img;
    std::map<uint64_t, std::pair<uint64_t, uint64_t>> pushed;
    std::vector<uint64_t> marked;             // offsets of the slots marked free, sorted
    uint64_t total[2], pool_count, count0;
    int pool_writers, count_writers;
    bool operator==(const RelResult &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && img == o.img && pushed == o.pushed &&
               marked == o.marked && total[0] == o.total[0] && total[1] == o.total[1] &&
               pool_count == o.pool_count && count0 == o.count0 && pool_writers == o.pool_writers &&
               count_writers == o.count_writers;
    }
};

void rel_arrays(const Rel &b, uint64_t m, RelResult &r)
{
    for (uint64_t i = 0; i < m; ++i) {
        r.offs.push_back(b.ent[i].off);
        r.caps.push_back(b.ent[i].cap);
        r.img.push_back(b.ent[i].img);
    }
}

RelResult rel_kernels(const Rel &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.ent.size();
    const uint32_t nb = (uint32_t) ((n + kPoolBlock - 1) / kPoolBlock);
    const uint64_t m = pool_m(n, b.has_count, b.count0);
    std::vector<uint64_t> ord(n), slot(n), zoff(n), zlen(n), rtot(nb), sh(kPoolBlock), excl(kPoolBlock);
    std::vector<uint32_t> code(n);
    RelResult r;
    r.status.assign(n, 99);
    rel_arrays(b, m, r);
    std::vector<uint64_t> koff(m, kUnwritten), kcap(m, kUnwritten);
    std::vector<uint32_t> kimg(m, 0x77777777u);
    uint64_t pool[4] = {b.pool[0], b.pool[1], b.pool[2], b.pool[3]}, count0 = b.count0;
    PoolArrays arr = {b.pool[1], {}};
    // release_headers
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            uint32_t c = 0;
            int st = OK;
            if (i < m) {
                c = kRelIn;
                const Ent &e = b.ent[i];
                if (e.live) {
                } else if (!e.gate_ok) {
                    st = ERR;
                } else if (pool_sound(pool[0], pool[1], pool[2], pool[3]) && e.valid &&
                           pool_takes(r.offs.at(i), r.caps.at(i), pool[2], pool[3])) {
                    c |= kRelReach;
                } else {
                    st = ERR;
                }
            }
            sh[t] = (c & kRelReach) ? 1 : 0;
            if (i < n) {
                r.status[i] = st;
                code[i] = c;
            }
        }
        wg_scan(kPoolBlock, sh, excl, rtot[wg]);
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i < n) {
                ord[i] = excl[t];
            }
        }
    }
    // release_scan
    r.total[0] = scan_totals(kPoolBlock, rtot.data(), (uint32_t) rtot.size());
    r.total[1] = pool_kept_total(m, r.total[0], pool_room(pool[0], pool[1], pool[2], pool[3]));
    // release_place
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i >= n) {
                break;
            }
            zoff[i] = zlen[i] = 0;
            if (!(code[i] & kRelIn)) {
                continue;
            }
            const uint64_t room = pool_room(pool[0], pool[1], pool[2], pool[3]);
            const uint64_t before = place_add(rtot[wg], ord[i]);
            code[i] |= pool_release_code(pool[0], room, before, (code[i] & kRelReach) != 0, i + 1 == m, slot[i]);
            if (code[i] & kRelAccepted) {
                zoff[i] = r.offs.at(i);
                zlen[i] = r.caps.at(i);
            } else if (code[i] & kRelReach) {
                r.status[i] = ERR;
            }
            if (b.compact) {
                if (!(code[i] & kRelAccepted)) {
                    const uint64_t p = pool_kept_pos(i, before, room);
                    if (koff.at(p) != kUnwritten) {
                        fprintf(stderr, "pool_check: two entries at position %llu\n", (unsigned long long) p);
                        abort();
                    }
                    koff.at(p) = r.offs.at(i);
                    kcap.at(p) = r.caps.at(i);
                    kimg.at(p) = r.img.at(i);
                }
                if (i >= r.total[1]) {
                    koff.at(i) = 0;
                    kcap.at(i) = 0;
                    kimg.at(i) = kPoolNoImage;
                }
            }
        }
    }
    // release_commit: no thread reads the pool's count or dev_count[0]
    r.pool_writers = r.count_writers = 0;
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i >= n) {
                break;
            }
            const uint32_t c = code[i];
            if (c == 0) {
                continue;
            }
            if (c & kRelAccepted) {
                arr.push(slot[i], zoff[i], zlen[i]);
                r.marked.push_back(zoff[i]);
            }
            if (c & (kRelEndAt | kRelEndLast)) {
                pool[0] = pool_release_end(c, slot[i]);
                r.pool_writers += 1 + ((c & kRelEndAt) && (c & kRelEndLast));
            }
            if (b.compact) {
                r.offs.at(i) = koff.at(i);
                r.caps.at(i) = kcap.at(i);
                r.img.at(i) = kimg.at(i);
                if (i == 0) {
                    count0 = r.total[1];
                    ++r.count_writers;
                }
            }
        }
    }
    std::sort(r.marked.begin(), r.marked.end());
    r.pushed = arr.e;
    r.pool_count = pool[0];
    r.count0 = count0;
    return r;
}

RelResult rel_sequential(const Rel &b)
{
    const uint64_t n = b.ent.size();
    const u128 m = b.has_count ? std::min<u128>(n, b.count0) : n;
    const u128 have = b.pool[0], pcap = b.pool[1];
    const uint64_t cls = b.pool[2], pal = b.pool[3];
    const bool sound = have <= pcap && cls >= 24 && pal >= 1 && pal <= 4096 && (pal & (pal - 1)) == 0;
    RelResult r;
    r.status.assign(n, OK);
    std::vector<size_t> kept;
    u128 reach = 0, accepted = 0;
    for (size_t i = 0; i < (size_t) m; ++i) {
        const Ent &e = b.ent[i];
        if (e.live) {
            kept.push_back(i);
            continue;
        }
        if (!e.gate_ok || !sound || !e.valid || e.cap < cls || e.off % pal != 0) {
            r.status[i] = ERR;
            kept.push_back(i);
            continue;
        }
        if (have + reach < pcap) {
            r.pushed[(uint64_t) (have + reach)] = {e.off, e.cap};
            r.marked.push_back(e.off);
            ++accepted;
        } else {
            r.status[i] = ERR;
            kept.push_back(i);
        }
        ++reach;
    }
    std::sort(r.marked.begin(), r.marked.end());
    rel_arrays(b, (uint64_t) m, r);
    r.count0 = b.count0;
    if (b.compact) {
        for (size_t p = 0; p < (size_t) m; ++p) {
            r.offs[p] = p < kept.size() ? b.ent[kept[p]].off : 0;
            r.caps[p] = p < kept.size() ? b.ent[kept[p]].cap : 0;
            r.img[p] = p < kept.size() ? b.ent[kept[p]].img : kPoolNoImage;
        }
        r.count0 = m != 0 ? kept.size() : b.count0;
    }
    r.total[0] = (uint64_t) reach;
    r.total[1] = kept.size();
    r.pool_count = (uint64_t) (have + accepted);
    r.pool_writers = accepted ? 1 : 0;        // exactly one writer, or none
    r.count_writers = b.compact && m != 0 ? 1 : 0;
    return r;
}

int rel_check(const Rel &b, const char *what, std::mt19937_64 &rng)
{
    const RelResult want = rel_sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(rel_kernels(b, order, rng) == want)) {
            fprintf(stderr, "pool_check: release, %s: n = %zu, count %d %llu, pool %llu of %llu, cls %llu, pal %llu, "
                            "compact %d, order %d differs\n",
                    what, b.ent.size(), (int) b.has_count, (unsigned long long) b.count0,
                    (unsigned long long) b.pool[0], (unsigned long long) b.pool[1], (unsigned long long) b.pool[2],
                    (unsigned long long) b.pool[3], (int) b.compact, order);
            return 1;
        }
    }
    return 0;
}

// pattern: 0 every entry releasable, 1 none (the gate), 2 alternating, 3 random kinds.
Rel rel_batch(size_t n, int pattern, bool compact, std::mt19937_64 &rng)
{
    Rel b;
    b.ent.resize(n);
    for (size_t i = 0; i < n; ++i) {
        Ent &e = b.ent[i];
        e.off = 64 * (uint64_t) i;
        e.cap = 64;
        e.img = (uint32_t) (i * 7 + 1);
        e.live = false;
        e.gate_ok = pattern == 0 || (pattern == 2 && i % 2 == 0) || (pattern == 3 && rng() % 3 != 0);
        e.valid = true;
        if (pattern == 3) {
            switch (rng() % 8) {
            case 0: e.valid = false; break;
            case 1: e.cap = 63; break;
            case 2: e.off += 8; break;
            case 3: e.live = !compact; break;
            default: break;
            }
        }
    }
    b.has_count = compact || rng() % 2;
    b.count0 = n;
    b.compact = compact;
    b.pool[0] = rng() % 5;
    b.pool[1] = b.pool[0] + n + 1;
    b.pool[2] = 64;
    b.pool[3] = 16;
    return b;
}

int release_cases(std::mt19937_64 &rng)
{
    int bad = 0;
    const size_t mega = 1024u * 1024u;
    for (size_t n : {(size_t) 1, (size_t) 2, (size_t) 1023, (size_t) 1024, (size_t) 1025, (size_t) 3000, mega - 1, mega,
                     mega + 1}) {
        for (int pattern = 0; pattern < 4; ++pattern) {
            for (int compact = 0; compact < 2; ++compact) {
                if (n >= mega - 1 && pattern != 3 && !(pattern == 0 && compact)) {
                    continue;
                }
                Rel b = rel_batch(n, pattern, compact != 0, rng);
                bad += rel_check(b, "sizes", rng);
                if (n == 1025 || (n == mega + 1 && pattern == 3)) {   // the pool cuts inside the batch; dev_count below and above n
                    b.pool[1] = b.pool[0] + n / 3;
                    bad += rel_check(b, "pool cut", rng);
                    b.has_count = true;
                    b.count0 = n - n / 4;
                    bad += rel_check(b, "count below n", rng);
                    b.count0 = n + 5;
                    bad += rel_check(b, "count above n", rng);
                    b.count0 = 0;
                    bad += rel_check(b, "count 0", rng);
                }
            }
        }
    }
    // the pool cutting at every position, with and without entries that do not reach the placement
    for (int pattern : {0, 3}) {
        for (int compact = 0; compact < 2; ++compact) {
            for (uint64_t room = 0; room <= 42; ++room) {
                Rel b = rel_batch(40, pattern, compact != 0, rng);
                b.pool[1] = b.pool[0] + room;
                bad += rel_check(b, "every position", rng);
            }
        }
    }
    // unsound pool words, and words near 2^64
    const uint64_t words[][4] = {{5, 4, 64, 16}, {0, 9, 23, 16}, {0, 9, 64, 0}, {0, 9, 64, 24}, {0, 9, 64, 8192},
                                 {kPlaceOver, kPlaceOver - 1, 64, 16}, {kPlaceOver - 3, kPlaceOver, 64, 16},
                                 {kPlaceOver - 3, kPlaceOver - 1, 64, 1}, {kPlaceOver, kPlaceOver, 64, 16},
                                 {0, kPlaceOver, 24, 4096}};
    for (const auto &w : words) {
        for (int compact = 0; compact < 2; ++compact) {
            Rel b = rel_batch(1500, 3, compact != 0, rng);
            std::copy(w, w + 4, b.pool);
            bad += rel_check(b, "pool words", rng);
            b.has_count = true;
            b.count0 = kPlaceOver - (compact ? 0 : 1);
            bad += rel_check(b, "pool words, count near 2^64", rng);
        }
    }
    return bad;
}

// ---------------------------------------------------------------- rotate from the pool

struct Rot {
    std::vector<bool> reach;
    uint64_t top, end, dev_bytes, new_cap, align, have, list_cap, pool[4];
};

struct RotResult {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps;          // the fresh image's place and capacity; kUnwritten: not rotated
    std::map<uint64_t, uint64_t> li;           // the list's images by index (an index may lie near 2^64)
    uint64_t total[2], top, count, pool_count;
    int top_writers, count_writers, pool_writers;
    bool operator==(const RotResult &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && li == o.li && total[0] == o.total[0] &&
               total[1] == o.total[1] && top == o.top && count == o.count && pool_count == o.pool_count &&
               top_writers == o.top_writers && count_writers == o.count_writers && pool_writers == o.pool_writers;
    }
};

// Pool entry k: its offset and capacity (the arrays are release's output; any
// values do).
uint64_t pool_off(uint64_t k)
{
    return 4096 + 1024 * (k % 1000003);
}

uint64_t pool_cap(const Rot &b, uint64_t k)
{
    return b.pool[2] + k % 7;
}

// A list entry beyond the capacity, or written twice, aborts.
void list_put(const Rot &b, std::map<uint64_t, uint64_t> &li, uint64_t k, uint64_t i)
{
    if (k >= b.list_cap || li.count(k)) {
        fprintf(stderr, "pool_check: a list entry at %llu of %llu\n", (unsigned long long) k,
                (unsigned long long) b.list_cap);
        abort();
    }
    li[k] = i;
}

RotResult rot_kernels(const Rot &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.reach.size();
    const uint32_t nb = (uint32_t) ((n + kPoolBlock - 1) / kPoolBlock);
    std::vector<uint64_t> ord(n), roff(n), rk(n), rcap(n), etop(n), epool(n), rtot(nb), sh(kPoolBlock),
        excl(kPoolBlock);
    std::vector<uint32_t> code(n);
    RotResult r;
    r.status.assign(n, OK);
    r.offs.assign(n, kUnwritten);
    r.caps.assign(n, kUnwritten);
    uint64_t arena[2] = {b.top, b.end}, out_count[2] = {b.have, b.list_cap};
    uint64_t pool[4] = {b.pool[0], b.pool[1], b.pool[2], b.pool[3]};
    const uint64_t slot = grow_round_up(b.new_cap, b.align);
    // rotate_headers' scan and rotate_scan (rotate's dev_total[0] is replaced below)
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            sh[t] = i < n && b.reach[i] ? 1 : 0;
        }
        wg_scan(kPoolBlock, sh, excl, rtot[wg]);
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i < n) {
                ord[i] = excl[t];
            }
        }
    }
    r.total[1] = scan_totals(kPoolBlock, rtot.data(), (uint32_t) rtot.size());
    // rotpool_place
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i >= n) {
                break;
            }
            const uint64_t F = pool_usable(pool[0], pool[1], pool[2], pool[3], b.new_cap, b.align);
            if (i == 0) {
                r.total[0] = pool_rot_total(arena[0], b.align, r.total[1], F, slot);
            }
            const uint64_t before = place_add(rtot[wg], ord[i]);
            uint32_t c = pool_rot_place_code(arena[0], arena[1], b.dev_bytes, b.align, slot, out_count[0],
                                             out_count[1], F, before, b.reach[i], i + 1 == n, roff[i], rk[i]);
            rcap[i] = b.new_cap;
            if ((c & kRotAccepted) && before < F) {
                roff[i] = pool_off(pool[0] - 1 - before);
                rcap[i] = pool_cap(b, pool[0] - 1 - before);
            }
            if (c & (kRotEndAt | kRotEndLast)) {
                uint64_t ncount;
                c |= pool_rot_end_values(c, before, F, arena[0], b.align, slot, out_count[0], pool[0], etop[i],
                                         ncount, epool[i]);
                if (ncount != ((c & kRotAccepted) ? rk[i] + 1 : rk[i])) {
                    fprintf(stderr, "pool_check: the new count does not follow from the list index\n");
                    abort();
                }
            }
            code[i] = c;
            if (!(c & kRotAccepted) && b.reach[i]) {
                r.status[i] = ERR;
            }
        }
    }
    // rotpool_commit: no thread reads the top, the count or the pool's count
    r.top_writers = r.count_writers = r.pool_writers = 0;
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kPoolBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kPoolBlock + t;
            if (i >= n) {
                break;
            }
            const uint32_t c = code[i];
            if (c & kRotAccepted) {
                list_put(b, r.li, rk[i], i);
                r.offs[i] = roff[i];
                r.caps[i] = rcap[i];
            }
            if (c & (kRotEndAt | kRotEndLast)) {
                const int w = 1 + ((c & kRotEndAt) && (c & kRotEndLast));
                out_count[0] = (c & kRotAccepted) ? rk[i] + 1 : rk[i];
                r.count_writers += w;
                if (c & kRotPoolTop) {
                    arena[0] = etop[i];
                    r.top_writers += w;
                }
                if (c & kRotPoolPop) {
                    pool[0] = epool[i];
                    r.pool_writers += w;
                }
            }
        }
    }
    r.top = arena[0];
    r.count = out_count[0];
    r.pool_count = pool[0];
    return r;
}

u128 up128(u128 v, uint64_t a)
{
    return (v + (a - 1)) / a * a;
}

RotResult rot_sequential(const Rot &b)
{
    const u128 over = (u128) kPlaceOver;
    const size_t n = b.reach.size();
    const uint64_t pc = b.pool[0], pal = b.pool[3];
    const bool sound = pc <= b.pool[1] && b.pool[2] >= 24 && pal >= 1 && pal <= 4096 && (pal & (pal - 1)) == 0;
    const u128 F = sound && b.new_cap <= b.pool[2] && pal % b.align == 0 ? pc : 0;
    RotResult r;
    r.status.assign(n, OK);
    r.offs.assign(n, kUnwritten);
    r.caps.assign(n, kUnwritten);
    const u128 base = up128(b.top, b.align), slot = up128(b.new_cap, b.align);
    u128 reach = 0, accepted = 0, from_pool = 0;
    bool cut = false;
    for (size_t i = 0; i < n; ++i) {
        if (!b.reach[i]) {
            continue;
        }
        const u128 j = reach++, k = (u128) b.have + j;
        bool ok = !cut && k < (u128) b.list_cap && k < over;
        u128 off = 0, cap = b.new_cap;
        if (j < F) {
            off = pool_off((uint64_t) (pc - 1 - j));
            cap = pool_cap(b, (uint64_t) (pc - 1 - j));
        } else {
            off = base + (j - F) * slot;
            ok = ok && b.end <= b.dev_bytes && off + slot < over && off + slot <= (u128) b.end;
        }
        if (!ok) {
            cut = true;
            r.status[i] = ERR;
            continue;
        }
        list_put(b, r.li, (uint64_t) k, i);
        r.offs[i] = (uint64_t) off;
        r.caps[i] = (uint64_t) cap;
        ++accepted;
        from_pool += j < F;
    }
    const u128 extra = reach > F ? reach - F : 0, slots = std::min(extra * slot, over);
    r.total[0] = extra == 0 ? 0 : base >= over ? kPlaceOver : (uint64_t) std::min(base - b.top + slots, over);
    r.total[1] = (uint64_t) reach;
    r.top = accepted > from_pool ? (uint64_t) (base + (accepted - from_pool) * slot) : b.top;
    r.count = b.have + (uint64_t) accepted;
    r.pool_count = pc - (uint64_t) from_pool;
    r.top_writers = accepted > from_pool ? 1 : 0;          // exactly one writer of each, or none
    r.count_writers = accepted ? 1 : 0;
    r.pool_writers = from_pool ? 1 : 0;
    return r;
}

int rot_check(const Rot &b, const char *what, std::mt19937_64 &rng)
{
    const RotResult want = rot_sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(rot_kernels(b, order, rng) == want)) {
            fprintf(stderr, "pool_check: rotate, %s: n = %zu, align = %llu, new_cap = %llu, top = %llu, end = %llu, "
                            "list %llu of %llu, pool %llu of %llu, cls %llu, pal %llu, order %d differs\n",
                    what, b.reach.size(), (unsigned long long) b.align, (unsigned long long) b.new_cap,
                    (unsigned long long) b.top, (unsigned long long) b.end, (unsigned long long) b.have,
                    (unsigned long long) b.list_cap, (unsigned long long) b.pool[0], (unsigned long long) b.pool[1],
                    (unsigned long long) b.pool[2], (unsigned long long) b.pool[3], order);
            return 1;
        }
    }
    return 0;
}

Rot rot_batch(size_t n, int density, std::mt19937_64 &rng)
{
    Rot b;
    b.reach.resize(n);
    for (size_t i = 0; i < n; ++i) {
        b.reach[i] = density == 0 ? true : rng() % density == 0;
    }
    b.top = 1000 + rng() % 5000;
    b.end = kPlaceOver - 1;
    b.dev_bytes = kPlaceOver - 1;
    b.new_cap = 200;
    b.align = 64;
    b.have = rng() % 5;
    b.list_cap = b.have + n + 1;
    b.pool[0] = 0;
    b.pool[1] = n + 10;
    b.pool[2] = 256;
    b.pool[3] = 128;
    return b;
}

int rotate_cases(std::mt19937_64 &rng)
{
    int bad = 0;
    const size_t mega = 1024u * 1024u;
    for (size_t n : {(size_t) 1, (size_t) 2, (size_t) 1023, (size_t) 1024, (size_t) 1025, (size_t) 3000, mega - 1, mega,
                     mega + 1}) {
        for (int density : {0, 3}) {
            Rot b = rot_batch(n, density, rng);
            const uint64_t reach = (uint64_t) std::count(b.reach.begin(), b.reach.end(), true);
            // F = 0, below reach, equal to reach, above reach
            for (uint64_t F : {(uint64_t) 0, reach / 2, reach, reach + 3}) {
                b.pool[0] = F;
                b.pool[1] = F + 3;
                bad += rot_check(b, "F", rng);
            }
            if (n > 3000) {
                continue;
            }
            const uint64_t slot = grow_round_up(b.new_cap, b.align), base = grow_round_up(b.top, b.align);
            b.pool[0] = reach / 2;
            // the list cutting inside and beyond the pool part; the arena cutting the arena part
            for (uint64_t room : {(uint64_t) 0, reach / 4, reach / 2, reach / 2 + 1, reach - reach / 8, reach}) {
                Rot c = b;
                c.list_cap = c.have + room;
                bad += rot_check(c, "list cut", rng);
                c = b;
                c.end = base + room * slot + slot - 1;
                c.dev_bytes = c.end + 7;
                bad += rot_check(c, "arena cut", rng);
                c.list_cap = c.have + reach / 2 + 2;
                bad += rot_check(c, "both cut", rng);
                c = b;
                c.dev_bytes = c.end - 1;                   // the arena outside dev_bytes: the pool part alone
                bad += rot_check(c, "arena outside", rng);
            }
        }
    }
    // every cut position of a small batch, list and arena
    for (uint64_t F = 0; F <= 12; F += 3) {
        for (uint64_t room = 0; room <= 12; ++room) {
            Rot b = rot_batch(10, 0, rng);
            b.pool[0] = F;
            b.list_cap = b.have + room;
            bad += rot_check(b, "every list position", rng);
            b = rot_batch(10, 0, rng);
            b.pool[0] = F;
            b.end = grow_round_up(b.top, b.align) + room * grow_round_up(b.new_cap, b.align);
            bad += rot_check(b, "every arena position", rng);
        }
    }
    // unusable and unsound pools, and words near 2^64
    const uint64_t words[][4] = {{5, 4, 256, 128}, {5, 9, 23, 128}, {5, 9, 199, 128}, {5, 9, 200, 64}, {5, 9, 256, 32},
                                 {5, 9, 256, 0}, {5, 9, 256, 8192}, {5, 9, 256, 96},
                                 {kPlaceOver, kPlaceOver, 256, 128}, {kPlaceOver - 1, kPlaceOver, 256, 4096}};
    for (const auto &w : words) {
        Rot b = rot_batch(1500, 2, rng);
        std::copy(w, w + 4, b.pool);
        bad += rot_check(b, "pool words", rng);
        b.have = kPlaceOver - 700;                         // the list index leaves 64 bits inside the batch
        b.list_cap = kPlaceOver;
        bad += rot_check(b, "pool words, count near 2^64", rng);
        b.have = 3;
        b.list_cap = 2000;
        b.top = kPlaceOver - 100000;                       // the arena slots leave 64 bits inside the batch
        b.end = b.dev_bytes = kPlaceOver;
        bad += rot_check(b, "pool words, top near 2^64", rng);
        b.top = kPlaceOver - 10;                           // the base itself does
        bad += rot_check(b, "pool words, base beyond 2^64", rng);
    }
    return bad;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20240607);
    const int bad = release_cases(rng) + rotate_cases(rng);
    if (bad) {
        fprintf(stderr, "pool_check: %d case(s) differ\n", bad);
        return 1;
    }
    printf("pool_check: ok\n");
    return 0;
}
