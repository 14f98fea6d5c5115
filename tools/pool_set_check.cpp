// pool_set_check.cpp -- the size-classed pool set (pool_set.h: the text the
// kernels relset_headers, relset_scan, relset_place, relset_kscan,
// relset_kmove, relset_commit, growset_class, growset_cscan, growset_serve,
// growset_ascan, growset_place and growset_commit run), stand-alone on the
// host under ASan + UBSan: no GPU, no HIP.  `make poolsetcheck`.
//
// Both chains are restated workgroup by workgroup -- the K-way counting scan
// wave by wave with the three ballots taken over 64 explicit lanes, the
// workgroup scans as the kernels do them, in log steps with place_add -- and
// run with the workgroups of each kernel in ascending, descending and random
// order (no workgroup may depend on another of its kernel).  Everything a call
// leaves -- statuses, the list (in arrays of EXACTLY m entries, so the
// sanitizer sees an entry beyond them), the pushes into the set's arrays
// (arrays of exactly n_cls * stride entries), the new offsets and capacities,
// every word of dev_total, every set word, the arena's top, dev_count[0], and
// the number of threads that write each of these words -- is compared with a
// sequential loop in 128-bit arithmetic.  Entries and images are given by
// their fields: no data.  grow_headers, which the set variant runs unchanged,
// is grow_check's; here an image reaches rule 4 with a new capacity or does
// not.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "pool_set.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int OK = 0, ERR = -1;
const uint64_t kUnwritten = 0x7777777777777777ull;
long g_cases = 0;

// class_rank of the kernels for workgroup b: cls[i] of its entries (kSetNone
// beyond n).  rank[i] and the workgroup's K counts into tab.
void class_rank_wg(uint32_t b, uint32_t nb, uint64_t n, const std::vector<uint32_t> &cls, std::vector<uint64_t> &rank,
                   uint64_t *tab)
{
    uint32_t wcount[kSetWaves * kPoolSetMax] = {};
    uint32_t c[kSetBlock], lr[kSetBlock];
    uint64_t match[kSetBlock];
    for (uint32_t t = 0; t < kSetBlock; ++t) {
        const uint64_t i = (uint64_t) b * kSetBlock + t;
        c[t] = i < n ? cls[i] : kSetNone;
    }
    for (uint32_t w = 0; w < kSetWaves; ++w) {
        uint64_t all = 0, ballot[kSetBits] = {};
        for (uint32_t l = 0; l < kSetWave; ++l) {             // the ballots: every lane of the wave votes
            const uint32_t v = c[w * kSetWave + l];
            if (v != kSetNone) {
                all |= 1ull << l;
                for (uint32_t bit = 0; bit < kSetBits; ++bit) {
                    ballot[bit] |= (uint64_t) ((v >> bit) & 1u) << l;
                }
            }
        }
        for (uint32_t l = 0; l < kSetWave; ++l) {
            const uint32_t t = w * kSetWave + l;
            match[t] = set_match(all, ballot, c[t]);
            lr[t] = sort_lane_rank(match[t], l);
        }
    }
    for (uint32_t t = 0; t < kSetBlock; ++t) {
        if (c[t] != kSetNone && lr[t] == 0) {
            if (wcount[(t / kSetWave) * kPoolSetMax + c[t]] != 0) {
                fprintf(stderr, "pool_set_check: two first lanes of one class in a wave\n");
                abort();
            }
            wcount[(t / kSetWave) * kPoolSetMax + c[t]] = sort_popcount(match[t]);
        }
    }
    for (uint32_t k = 0; k < kPoolSetMax; ++k) {
        tab[set_tab_at(k, b, nb)] = set_wave_scan(wcount, k);
    }
    for (uint32_t t = 0; t < kSetBlock; ++t) {
        const uint64_t i = (uint64_t) b * kSetBlock + t;
        if (i < n) {
            rank[i] = c[t] != kSetNone ? wcount[(t / kSetWave) * kPoolSetMax + c[t]] + lr[t] : 0;
        }
    }
}

// class_scan of the kernels: per class the exclusive scan of the workgroups'
// counts; reach[k] the class's total.
void class_scan(uint64_t *tab, uint32_t nb, uint32_t n_cls, uint64_t *reach)
{
    const uint32_t words = n_cls * nb;
    const uint64_t all = scan_totals(kSetBlock, tab, words);            // one linear scan of the class-major table
    uint64_t first[kPoolSetMax];
    for (uint32_t k = 0; k < n_cls; ++k) {
        first[k] = tab[set_tab_at(k, 0, nb)];
        reach[k] = set_class_total(first[k], k + 1 < n_cls ? tab[set_tab_at(k + 1, 0, nb)] : all);
    }
    for (uint32_t j = 0; j < words; ++j) {
        tab[j] = set_class_excl(tab[j], first[j / nb]);
    }
}

struct Set {
    uint32_t n_cls;
    uint64_t stride;
    std::vector<uint64_t> words, offs, caps;      // exactly 4 n_cls and n_cls * stride entries
};

// ---------------------------------------------------------------- release

struct Ent {
    uint64_t off, cap;
    uint32_t img;
    bool live, gate_ok, valid;                // rules 1, 2, 3
};

struct RelResult {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps, total, words, set_offs, set_caps;
    std::vector<uint32_t> img;
    std::vector<uint64_t> marked;
    uint64_t count0;
    std::vector<int> word_writers;
    int count_writers;
    bool operator==(const RelResult &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && total == o.total && words == o.words &&
               set_offs == o.set_offs && set_caps == o.set_caps && img == o.img && marked == o.marked &&
               count0 == o.count0 && word_writers == o.word_writers && count_writers == o.count_writers;
    }
};

RelResult rel_start(const std::vector<Ent> &ent, uint64_t m, const Set &s, uint64_t count0)
{
    RelResult r;
    r.status.assign(ent.size(), 99);
    for (uint64_t i = 0; i < m; ++i) {
        r.offs.push_back(ent[i].off);
        r.caps.push_back(ent[i].cap);
        r.img.push_back(ent[i].img);
    }
    r.total.assign(2 + s.n_cls, kUnwritten);
    r.words = s.words;
    r.set_offs = s.offs;
    r.set_caps = s.caps;
    r.count0 = count0;
    r.word_writers.assign(s.n_cls, 0);
    r.count_writers = 0;
    return r;
}

RelResult rel_reference(const std::vector<Ent> &ent, bool has_count, uint64_t count0, bool compact, const Set &s)
{
    const uint64_t n = ent.size(), m = has_count && count0 < n ? count0 : n;
    RelResult r = rel_start(ent, m, s, count0);
    bool sound = true;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        const uint64_t *p = &s.words[4 * k];
        sound = sound && p[0] <= p[1] && p[2] >= 24 && p[3] != 0 && (p[3] & (p[3] - 1)) == 0 && p[3] <= 4096 &&
                p[1] <= s.stride && (k == 0 || p[2] > s.words[4 * k - 2]);
    }
    std::vector<u128> seen(s.n_cls, 0);
    std::vector<bool> acc(n, false);
    u128 reach = 0;
    for (uint64_t i = 0; i < n; ++i) {
        r.status[i] = OK;
        if (i >= m || ent[i].live) {
            continue;
        }
        int cls = -1;
        if (ent[i].gate_ok && sound && ent[i].valid) {
            for (uint32_t k = 0; k < s.n_cls; ++k) {
                if (s.words[4 * k + 2] <= ent[i].cap && ent[i].off % s.words[4 * k + 3] == 0) {
                    cls = (int) k;
                }
            }
        }
        if (cls < 0) {
            r.status[i] = ERR;
            continue;
        }
        reach += 1;
        const u128 j = seen[cls]++;
        if ((u128) s.words[4 * cls] + j < s.words[4 * cls + 1]) {
            acc[i] = true;
            const uint64_t at = (uint64_t) (cls * (u128) s.stride + s.words[4 * cls] + j);
            r.set_offs.at(at) = ent[i].off;
            r.set_caps.at(at) = ent[i].cap;
            r.marked.push_back(ent[i].off);
        } else {
            r.status[i] = ERR;
        }
    }
    u128 kept = m;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        const u128 room = sound ? s.words[4 * k + 1] - s.words[4 * k] : 0;
        const u128 a = seen[k] < room ? seen[k] : room;
        r.total[2 + k] = (uint64_t) seen[k];
        kept -= a;
        if (a != 0) {
            r.words[4 * k] += (uint64_t) a;
            r.word_writers[k] = 1;
        }
    }
    r.total[0] = (uint64_t) reach;
    r.total[1] = (uint64_t) kept;
    if (compact) {
        uint64_t p = 0;
        for (uint64_t i = 0; i < m; ++i) {
            if (!acc[i]) {
                r.offs[p] = ent[i].off;
                r.caps[p] = ent[i].cap;
                r.img[p] = ent[i].img;
                ++p;
            }
        }
        for (; p < m; ++p) {
            r.offs[p] = 0;
            r.caps[p] = 0;
            r.img[p] = kPoolNoImage;
        }
        r.count0 = (uint64_t) kept;
        r.count_writers = m != 0;
    }
    std::sort(r.marked.begin(), r.marked.end());
    return r;
}

RelResult rel_kernels(const std::vector<Ent> &ent, bool has_count, uint64_t count0, bool compact, const Set &s,
                      int order, std::mt19937_64 &rng)
{
    const uint64_t n = ent.size(), m = pool_m(n, has_count, count0);
    const uint32_t nb = (uint32_t) ((n + kSetBlock - 1) / kSetBlock);
    RelResult r = rel_start(ent, m, s, count0);
    const uint64_t *set = s.words.data();
    std::vector<uint64_t> scratch(set_scratch_words(nb), kUnwritten);     // exactly the words the launcher reserves
    uint64_t *tab = scratch.data(), *words = tab + set_words_at(nb);
    std::vector<uint32_t> code(n), cls(n, kSetNone);
    std::vector<uint64_t> ord(n), slot(n, kUnwritten), rtot(nb), koff(n), kcap(n);
    std::vector<uint32_t> kimg(n);
    // relset_headers
    for (uint64_t i = 0; i < n; ++i) {
        int st = OK;
        uint32_t c = 0;
        if (i < m) {
            c = kRelIn;
            if (ent[i].live) {
            } else if (!ent[i].gate_ok) {
                st = ERR;
            } else {
                if (set_sound(set, s.n_cls, s.stride) && ent[i].valid) {
                    cls[i] = set_release_class(set, s.n_cls, ent[i].off, ent[i].cap);
                }
                if (cls[i] != kSetNone) {
                    c |= kRelReach | (cls[i] << kSetClsShift);
                } else {
                    st = ERR;
                }
            }
        }
        r.status[i] = st;
        code[i] = c;
    }
    for (uint32_t b : order_of(nb, order, rng)) {
        class_rank_wg(b, nb, n, cls, ord, tab);
    }
    // relset_scan
    uint64_t reach[kPoolSetMax] = {};
    class_scan(tab, nb, s.n_cls, reach);
    {
        const bool sound = set_sound(set, s.n_cls, s.stride);
        uint64_t all = 0, kept = m, mask = 0;
        for (uint32_t k = 0; k < s.n_cls; ++k) {
            const uint64_t room = set_room(set, k, sound);
            bool changed;
            words[kSetWEnd + k] = set_release_end(set[4 * k + kPoolCount], room, reach[k], changed);
            mask |= changed ? 1ull << k : 0;
            r.total[2 + k] = reach[k];
            all += reach[k];
            kept -= reach[k] < room ? reach[k] : room;
        }
        words[kSetWMask] = mask;
        r.total[0] = all;
        r.total[1] = kept;
    }
    // relset_place
    for (uint32_t b : order_of(nb, order, rng)) {
        std::vector<uint64_t> sh(kSetBlock, 0), excl(kSetBlock);
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i >= n) {
                continue;
            }
            uint32_t c = code[i];
            if (c & kRelReach) {
                const uint32_t k = (c >> kSetClsShift) & 15u;
                const uint64_t before = tab[set_tab_at(k, b, nb)] + ord[i];
                if (before < set_room(set, k, true)) {
                    c |= kRelAccepted;
                    slot[i] = k * s.stride + set[4 * k + kPoolCount] + before;
                    code[i] = c;
                } else {
                    r.status[i] = ERR;
                }
            }
            sh[t] = (c & kRelIn) && !(c & kRelAccepted) ? 1 : 0;
        }
        if (compact) {
            uint64_t total;
            wg_scan(kSetBlock, sh, excl, total);
            rtot[b] = total;
            for (uint32_t t = 0; t < kSetBlock; ++t) {
                const uint64_t i = (uint64_t) b * kSetBlock + t;
                if (i < n) {
                    ord[i] = excl[t];
                }
            }
        }
    }
    if (compact) {
        scan_totals(kSetBlock, rtot.data(), nb);             // relset_kscan
        for (uint32_t b : order_of(nb, order, rng)) {         // relset_kmove
            for (uint32_t t = 0; t < kSetBlock; ++t) {
                const uint64_t i = (uint64_t) b * kSetBlock + t;
                if (i >= n || !(code[i] & kRelIn)) {
                    continue;
                }
                if (!(code[i] & kRelAccepted)) {
                    const uint64_t p = rtot[b] + ord[i];
                    koff.at(p) = ent[i].off;
                    kcap.at(p) = ent[i].cap;
                    kimg.at(p) = ent[i].img;
                }
                if (i >= r.total[1]) {
                    koff[i] = 0;
                    kcap[i] = 0;
                    kimg[i] = kPoolNoImage;
                }
            }
        }
    }
    // relset_commit: the list's arrays hold exactly m entries
    uint64_t *lo = r.offs.data(), *lc = r.caps.data();
    uint32_t *li = r.img.data();
    uint64_t *so = r.set_offs.data(), *sc = r.set_caps.data();
    for (uint32_t b : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i < s.n_cls && ((words[kSetWMask] >> i) & 1u)) {
                r.words[4 * i + kPoolCount] = words[kSetWEnd + i];
                r.word_writers[i] += 1;
            }
            if (i >= n || code[i] == 0) {
                continue;
            }
            if (code[i] & kRelAccepted) {
                so[slot[i]] = ent[i].off;         // beyond n_cls * stride: the sanitizer's
                sc[slot[i]] = ent[i].cap;
                r.marked.push_back(ent[i].off);
            }
            if (compact) {
                lo[i] = koff[i];                  // beyond m: the sanitizer's
                lc[i] = kcap[i];
                li[i] = kimg[i];
                if (i == 0) {
                    r.count0 = r.total[1];
                    r.count_writers += 1;
                }
            }
        }
    }
    std::sort(r.marked.begin(), r.marked.end());
    return r;
}

void rel_case(const std::vector<Ent> &ent, bool has_count, uint64_t count0, bool compact, const Set &s,
              std::mt19937_64 &rng, const char *what)
{
    const RelResult want = rel_reference(ent, has_count, count0, compact, s);
    for (int order = 0; order < 3; ++order) {
        const RelResult got = rel_kernels(ent, has_count, count0, compact, s, order, rng);
        if (!(got == want)) {
            fprintf(stderr, "pool_set_check: release %s: n %zu n_cls %u order %d differs\n", what, ent.size(), s.n_cls,
                    order);
            exit(1);
        }
    }
    ++g_cases;
}

// ---------------------------------------------------------------- grow

struct Img {
    uint64_t off, cap, used, new_cap;         // new_cap 0: the image does not reach rule 4
};

struct GrowResult {
    std::vector<int> status;
    std::vector<uint64_t> offs, caps, total, words;
    uint64_t top;
    std::vector<int> word_writers;
    int top_writers;
    bool operator==(const GrowResult &o) const
    {
        return status == o.status && offs == o.offs && caps == o.caps && total == o.total && words == o.words &&
               top == o.top && word_writers == o.word_writers && top_writers == o.top_writers;
    }
};

GrowResult grow_start(const std::vector<Img> &im, const Set &s, uint64_t top)
{
    GrowResult r;
    r.status.assign(im.size(), OK);           // the front's statuses: every image here passed rules 1..4
    for (const Img &x : im) {
        r.offs.push_back(x.off);
        r.caps.push_back(x.cap);
    }
    r.total.assign(2 + s.n_cls, kUnwritten);
    r.words = s.words;
    r.top = top;
    r.word_writers.assign(s.n_cls, 0);
    r.top_writers = 0;
    return r;
}

u128 up128(u128 v, uint64_t a)
{
    return (v + (a - 1)) / a * a;
}

GrowResult grow_reference(const std::vector<Img> &im, const Set &s, uint64_t top, uint64_t end, uint64_t dev_bytes,
                          uint64_t align)
{
    const u128 over = ~0ull;
    GrowResult r = grow_start(im, s, top);
    bool sound = true;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        const uint64_t *p = &s.words[4 * k];
        sound = sound && p[0] <= p[1] && p[2] >= 24 && p[3] != 0 && (p[3] & (p[3] - 1)) == 0 && p[3] <= 4096 &&
                p[1] <= s.stride && (k == 0 || p[2] > s.words[4 * k - 2]);
    }
    std::vector<bool> usable(s.n_cls);
    std::vector<u128> F(s.n_cls), seen(s.n_cls, 0);
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        usable[k] = sound && s.words[4 * k + 3] % align == 0;
        F[k] = usable[k] ? s.words[4 * k] : 0;
    }
    const u128 base = up128(top, align);
    u128 run = 0, new_top = top;
    bool any = false;
    for (size_t i = 0; i < im.size(); ++i) {
        if (im[i].new_cap == 0) {
            continue;
        }
        int c = -1;
        for (uint32_t k = 0; k < s.n_cls && c < 0; ++k) {
            if (usable[k] && s.words[4 * k + 2] >= im[i].new_cap) {
                c = (int) k;
            }
        }
        if (c >= 0) {
            const u128 j = seen[c]++;
            if (j < F[c]) {
                const uint64_t e = (uint64_t) (c * (u128) s.stride + F[c] - 1 - j);
                const uint64_t eo = s.offs.at(e), ec = s.caps.at(e);
                if ((u128) eo + ec <= dev_bytes && ec >= s.words[4 * c + 2] && eo % align == 0) {
                    r.offs[i] = eo;
                    r.caps[i] = ec;
                } else {
                    r.status[i] = ERR;
                }
                continue;
            }
        }
        const uint64_t cap = c >= 0 ? s.words[4 * c + 2] : im[i].new_cap;
        const u128 slot = up128(cap, align), off = base + run;
        any = true;
        if (end <= dev_bytes && off + slot < over && off + slot <= end) {
            r.offs[i] = (uint64_t) off;
            r.caps[i] = cap;
            new_top = off + slot;
        } else {
            r.status[i] = ERR;
        }
        run += slot;
        if (run > over) {
            run = over;
        }
    }
    const u128 t0 = !any ? 0 : base >= over ? over : base - top + run;
    r.total[0] = (uint64_t) (t0 > over ? over : t0);
    u128 taken = 0;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        const u128 a = seen[k] < F[k] ? seen[k] : F[k];
        r.total[2 + k] = (uint64_t) seen[k];
        taken += a;
        if (a != 0) {
            r.words[4 * k] -= (uint64_t) a;
            r.word_writers[k] = 1;
        }
    }
    r.total[1] = (uint64_t) taken;
    if (new_top != top) {
        r.top = (uint64_t) new_top;
        r.top_writers = 1;
    }
    return r;
}

GrowResult grow_kernels(const std::vector<Img> &im, const Set &s, uint64_t top, uint64_t end, uint64_t dev_bytes,
                        uint64_t align, int order, std::mt19937_64 &rng)
{
    const uint64_t n = im.size();
    const uint32_t nb = (uint32_t) ((n + kSetBlock - 1) / kSetBlock);
    GrowResult r = grow_start(im, s, top);
    const uint64_t *set = s.words.data();
    const uint64_t arena[2] = {top, end};
    std::vector<uint64_t> scratch(set_scratch_words(nb), kUnwritten);
    uint64_t *tab = scratch.data(), *words = tab + set_words_at(nb);
    std::vector<uint32_t> code(n), cls(n, kSetNone);
    std::vector<uint64_t> ord(n), gcap(n), dst(n, kUnwritten), etop(n, kUnwritten), rtot(nb);
    const uint32_t usable = set_usable(set, s.n_cls, s.stride, align);
    // growset_class
    for (uint64_t i = 0; i < n; ++i) {
        gcap[i] = im[i].new_cap;
        if (gcap[i] != 0) {
            cls[i] = set_grow_class(set, s.n_cls, usable, gcap[i]);
        }
        code[i] = cls[i] << kSetClsShift;
    }
    for (uint32_t b : order_of(nb, order, rng)) {
        class_rank_wg(b, nb, n, cls, ord, tab);
    }
    // growset_cscan
    uint64_t images[kPoolSetMax] = {};
    class_scan(tab, nb, s.n_cls, images);
    {
        uint64_t taken = 0, mask = 0;
        for (uint32_t k = 0; k < s.n_cls; ++k) {
            const uint64_t F = set_serves(set, k, usable);
            bool changed;
            words[kSetWEnd + k] = set_grow_end(set[4 * k + kPoolCount], F, images[k], changed);
            mask |= changed ? 1ull << k : 0;
            r.total[2 + k] = images[k];
            taken += images[k] < F ? images[k] : F;
        }
        words[kSetWMask] = mask;
        r.total[1] = taken;
    }
    // growset_serve: the set's arrays hold exactly n_cls * stride entries
    const uint64_t *so = s.offs.data(), *sc = s.caps.data();
    for (uint32_t b : order_of(nb, order, rng)) {
        std::vector<uint64_t> sh(kSetBlock, 0), excl(kSetBlock);
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i >= n || gcap[i] == 0) {
                continue;
            }
            uint32_t c = code[i];
            const uint32_t k = (c >> kSetClsShift) & 15u;
            bool pooled = false;
            if (k != kSetNone) {
                const uint64_t j = tab[set_tab_at(k, b, nb)] + ord[i], F = set_serves(set, k, usable);
                if (j < F) {
                    pooled = true;
                    const uint64_t e = k * s.stride + (F - 1 - j);
                    if (set_entry_ok(so[e], sc[e], dev_bytes, set[4 * k + kPoolCls], align)) {
                        c |= kSetServed;
                        dst[i] = so[e];
                        gcap[i] = sc[e];
                    } else {
                        r.status[i] = ERR;
                        gcap[i] = 0;
                    }
                }
            }
            if (!pooled) {
                const uint64_t cap = set_arena_cap(set, k, gcap[i]);
                c |= kSetArena;
                gcap[i] = cap;
                sh[t] = grow_slot(cap, align);
            }
            code[i] = c;
        }
        uint64_t total;
        wg_scan(kSetBlock, sh, excl, total);
        rtot[b] = total;
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i < n) {
                ord[i] = excl[t];
            }
        }
    }
    // growset_ascan
    r.total[0] = grow_total(arena[0], align, scan_totals(kSetBlock, rtot.data(), nb));
    // growset_place
    for (uint32_t b : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i >= n) {
                continue;
            }
            uint32_t c = code[i];
            const uint64_t slot = (c & kSetArena) ? grow_slot(gcap[i], align) : 0;
            const uint64_t before = place_add(rtot[b], ord[i]);
            uint64_t off;
            const uint32_t g = grow_place_code(arena[0], arena[1], dev_bytes, align, before, slot, i + 1 == n, off);
            if (g & (kGrowTopAt | kGrowTopEnd)) {
                etop[i] = (g & kGrowTopAt) ? off : off + slot;
            }
            c |= g;
            if (c & kSetServed) {
                c |= kGrowMoved;
                off = dst[i];
            } else if (slot != 0 && !(g & kGrowMoved)) {
                r.status[i] = ERR;
            }
            code[i] = c;
            if (c & kGrowMoved) {
                dst[i] = off;
            }
        }
    }
    // growset_commit
    for (uint32_t b : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kSetBlock; ++t) {
            const uint64_t i = (uint64_t) b * kSetBlock + t;
            if (i < s.n_cls && ((words[kSetWMask] >> i) & 1u)) {
                r.words[4 * i + kPoolCount] = words[kSetWEnd + i];
                r.word_writers[i] += 1;
            }
            if (i >= n) {
                continue;
            }
            if (code[i] & kGrowMoved) {
                r.offs[i] = dst[i];
                r.caps[i] = gcap[i];
            }
            if (code[i] & (kGrowTopAt | kGrowTopEnd)) {
                r.top = etop[i];
                r.top_writers += 1;
            }
        }
    }
    return r;
}

void grow_case(const std::vector<Img> &im, const Set &s, uint64_t top, uint64_t end, uint64_t dev_bytes, uint64_t align,
               std::mt19937_64 &rng, const char *what)
{
    const GrowResult want = grow_reference(im, s, top, end, dev_bytes, align);
    for (int order = 0; order < 3; ++order) {
        const GrowResult got = grow_kernels(im, s, top, end, dev_bytes, align, order, rng);
        if (!(got == want)) {
            fprintf(stderr, "pool_set_check: grow %s: n %zu n_cls %u order %d differs\n", what, im.size(), s.n_cls,
                    order);
            exit(1);
        }
    }
    ++g_cases;
}

// ---------------------------------------------------------------- the cases

const uint64_t kCls[kPoolSetMax] = {64, 96, 128, 192, 256, 384, 512, 768};

Set make_set(uint32_t n_cls, uint64_t stride, const std::vector<uint64_t> &have, const std::vector<uint64_t> &cap,
             uint64_t pal = 16)
{
    Set s;
    s.n_cls = n_cls;
    s.stride = stride;
    s.offs.assign(n_cls * stride, kUnwritten);
    s.caps.assign(n_cls * stride, kUnwritten);
    for (uint32_t k = 0; k < n_cls; ++k) {
        s.words.insert(s.words.end(), {have[k], cap[k], kCls[k], pal});
        for (uint64_t e = 0; e < have[k] && e < stride; ++e) {
            s.offs[k * stride + e] = (1ull << 32) + (k * stride + e) * 1024;
            s.caps[k * stride + e] = kCls[k] + 8 * (e % 3);
        }
    }
    return s;
}

std::vector<Ent> make_entries(uint64_t n, uint32_t n_cls, int keep, std::mt19937_64 &rng)
{
    std::vector<Ent> ent(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint32_t k = (uint32_t) (rng() % n_cls);
        Ent &e = ent[i];
        e.off = 4096 + i * 1024;
        e.cap = kCls[k] + rng() % 24;
        e.img = (uint32_t) (1000 + i);
        e.live = rng() % 11 == 0;
        e.valid = rng() % 7 != 0;
        e.gate_ok = keep == 0 ? true : keep == 1 ? false : keep == 2 ? i % 2 == 0 : rng() % 2 == 0;
        if (rng() % 9 == 0) {
            e.cap = 63 - rng() % 40;              // below class 0
        }
        if (rng() % 9 == 0) {
            e.off += 8;                           // off the alignment
        }
    }
    return ent;
}

void release_cases(std::mt19937_64 &rng)
{
    const uint64_t sizes[] = {1, 63, 64, 65, 1023, 1024, 1025, 2055};
    for (uint32_t n_cls = 1; n_cls <= kPoolSetMax; ++n_cls) {
        for (uint64_t n : sizes) {
            for (int keep = 0; keep < 4; ++keep) {            // none, all, alternating, random entries kept by the gate
                const std::vector<Ent> ent = make_entries(n, n_cls, keep, rng);
                std::vector<uint64_t> have(n_cls), cap(n_cls);
                uint64_t stride = 1;
                for (uint32_t k = 0; k < n_cls; ++k) {        // room 0, small, or for all
                    have[k] = rng() % 3;
                    cap[k] = have[k] + (k % 3 == 0 ? 0 : k % 3 == 1 ? rng() % (n / n_cls + 1) : n);
                    stride = std::max(stride, cap[k]);
                }
                const Set s = make_set(n_cls, stride, have, cap);
                rel_case(ent, false, 0, false, s, rng, "mixed");
                rel_case(ent, true, n, true, s, rng, "compact");
                rel_case(ent, true, n / 2, true, s, rng, "compact, half the count");
                rel_case(ent, true, n + 5, false, s, rng, "a count beyond n");
            }
        }
    }
    // every class cutting at every position: 24 releasable entries over three classes, every room 0 .. reach + 1
    for (uint64_t r0 = 0; r0 <= 9; ++r0) {
        for (uint64_t r1 = 0; r1 <= 9; ++r1) {
            for (uint64_t r2 = 0; r2 <= 9; r2 += 3) {
                std::vector<Ent> ent(24);
                for (uint64_t i = 0; i < 24; ++i) {
                    ent[i] = {4096 + i * 1024, kCls[(i * 7) % 3] + i % 5, (uint32_t) i, false, true, true};
                }
                const Set s = make_set(3, 12, {1, 2, 0}, {1 + r0, 2 + r1, r2});
                rel_case(ent, true, 24, true, s, rng, "cut positions");
            }
        }
    }
    // every unsoundness: nothing reaches, nothing is written
    const std::vector<Ent> ent = make_entries(70, 3, 0, rng);
    const uint64_t bad[][3] = {{0, 0, 9}, {1, 2, 23}, {2, 3, 48}, {2, 3, 0}, {2, 3, 8192}, {1, 1, 9}, {1, 2, 64},
                               {2, 2, 90}};
    for (const auto &m : bad) {
        Set s = make_set(3, 8, {1, 2, 3}, {8, 8, 8});
        s.words[4 * m[0] + m[1]] = m[2];
        rel_case(ent, true, 70, true, s, rng, "unsound");
        const RelResult r = rel_reference(ent, true, 70, true, s);
        if (r.total[0] != 0 || r.words != s.words) {
            fprintf(stderr, "pool_set_check: an unsound set took an entry\n");
            exit(1);
        }
    }
    // words and offsets near 2^64: a class of nearly 2^64 bytes takes nothing here, offsets at the end of the space
    {
        std::vector<Ent> e2 = make_entries(130, 2, 0, rng);
        for (uint64_t i = 0; i < e2.size(); i += 3) {
            e2[i].off = ~0ull - 15 - 16 * i;
            e2[i].cap = i % 2 ? ~0ull - 3 : kCls[0] + 1;
        }
        Set s = make_set(2, 1, {0, 0}, {0, 0});
        s.offs.assign(4096, kUnwritten);
        s.caps.assign(4096, kUnwritten);
        s.stride = 2048;
        s.words = {5, 2048, 64, 16, 2040, 2048, ~0ull - 7, 16};
        rel_case(e2, false, 0, false, s, rng, "near 2^64");
    }
    // both sides of 1024 * 1024
    for (uint64_t n : {1024ull * 1024 - 1, 1024ull * 1024, 1024ull * 1024 + 1}) {
        const std::vector<Ent> big = make_entries(n, 8, 3, rng);
        const Set s = make_set(8, n / 4, std::vector<uint64_t>(8, 1), {n / 4, 7, 1, n / 9, n / 4, 1, 2, n / 4});
        rel_case(big, true, n - 1, true, s, rng, "a million entries");
    }
}

void grow_cases(std::mt19937_64 &rng)
{
    const uint64_t sizes[] = {1, 63, 64, 65, 1023, 1024, 1025, 2055};
    const uint64_t dev_bytes = 1ull << 40;
    for (uint32_t n_cls = 1; n_cls <= kPoolSetMax; ++n_cls) {
        for (uint64_t n : sizes) {
            for (int fsel = 0; fsel < 4; ++fsel) {            // F_k 0, below, equal to, above the demand
                std::vector<Img> im(n);
                std::vector<uint64_t> demand(n_cls, 0);
                for (uint64_t i = 0; i < n; ++i) {
                    const uint64_t pick = rng() % (n_cls + 2);
                    const uint64_t nc = pick == n_cls ? 0 : pick == n_cls + 1 ? 1024 + 64 * (rng() % 4)
                                                                              : kCls[pick] - rng() % 16;
                    im[i] = {4096 + i * 128, 100, 60, nc};
                    if (pick < n_cls) {
                        demand[pick] += 1;
                    }
                }
                std::vector<uint64_t> have(n_cls);
                uint64_t stride = 1;
                for (uint32_t k = 0; k < n_cls; ++k) {
                    const int f = (fsel + k) % 4;
                    have[k] = f == 0 ? 0 : f == 1 ? demand[k] / 2 : f == 2 ? demand[k] : demand[k] + 2;
                    stride = std::max(stride, have[k]);
                }
                Set s = make_set(n_cls, stride, have, std::vector<uint64_t>(n_cls, stride));
                for (uint64_t e = 0; e < s.offs.size(); e += 5) {     // S3: outside dev_bytes, below its class, off
                    if (s.offs[e] == kUnwritten) {                    // the alignment
                        continue;
                    }
                    switch (rng() % 4) {
                    case 0: s.offs[e] = dev_bytes - 8; break;
                    case 1: s.offs[e] = ~0ull - 31; break;            // off + cap wraps
                    case 2: s.caps[e] = kCls[e / stride] - 1; break;
                    default: s.offs[e] += 8; break;
                    }
                }
                const uint64_t top = (1ull << 33) + 5, all = 64 + n * 1300;
                // the arena takes all; ends inside the arena-bound part; takes nothing; lies outside dev_bytes
                for (uint64_t end : {top + all, top + all / 3, top + 10, dev_bytes + 1}) {
                    grow_case(im, s, top, end, dev_bytes, 16, rng, "mixed");
                }
                grow_case(im, s, top, top + all, dev_bytes, 32, rng, "no class usable under align 32");
                Set mixed = s;
                for (uint32_t k = 0; k < n_cls; k += 2) {
                    mixed.words[4 * k + 3] = 64;
                }
                grow_case(im, mixed, top, top + all / 2, dev_bytes, 32, rng, "every other class usable");
            }
        }
    }
    // every unsoundness: the plain grow, no set word written
    std::vector<Img> im(90);
    for (uint64_t i = 0; i < 90; ++i) {
        im[i] = {4096 + i * 128, 100, 60, i % 4 == 0 ? 0 : kCls[i % 3]};
    }
    const uint64_t bad[][3] = {{0, 0, 9}, {1, 2, 23}, {2, 3, 48}, {2, 3, 0}, {2, 3, 8192}, {1, 1, 9}, {1, 2, 64},
                               {2, 2, 90}};
    for (const auto &m : bad) {
        Set s = make_set(3, 8, {1, 2, 3}, {8, 8, 8});
        s.words[4 * m[0] + m[1]] = m[2];
        grow_case(im, s, 1 << 20, 1 << 24, 1ull << 30, 16, rng, "unsound");
        const GrowResult r = grow_reference(im, s, 1 << 20, 1 << 24, 1ull << 30, 16);
        if (r.total[1] != 0 || r.words != s.words) {
            fprintf(stderr, "pool_set_check: an unsound set served an image\n");
            exit(1);
        }
    }
    // words and offsets near 2^64: a top whose rounding leaves 64 bits, a class of nearly 2^64 bytes that the arena
    // cannot hold, entries at the end of the space
    {
        Set s = make_set(2, 4, {2, 1}, {4, 4});
        s.words[6] = ~0ull - 15;
        s.offs[1] = ~0ull - 63;
        s.caps[1] = 64;
        for (uint64_t top : {~0ull - 3, ~0ull - 4096, 1ull << 20}) {
            for (uint64_t db : {~0ull, 1ull << 40}) {
                std::vector<Img> v(9);
                for (uint64_t i = 0; i < 9; ++i) {
                    v[i] = {4096 + i * 128, 100, 60, i % 3 == 0 ? 60 : i % 3 == 1 ? ~0ull - 100 : ~0ull - 8};
                }
                grow_case(v, s, top, ~0ull - 1, db, 16, rng, "near 2^64");
            }
        }
    }
    // both sides of 1024 * 1024
    for (uint64_t n : {1024ull * 1024 - 1, 1024ull * 1024, 1024ull * 1024 + 1}) {
        std::vector<Img> big(n);
        for (uint64_t i = 0; i < n; ++i) {
            big[i] = {4096 + i * 128, 100, 60, rng() % 5 == 0 ? 0 : kCls[rng() % 8] - rng() % 8};
        }
        const Set s = make_set(8, 4096, {4096, 0, 100, 4000, 1, 2, 3, 4096}, std::vector<uint64_t>(8, 4096));
        grow_case(big, s, 1ull << 33, (1ull << 33) + n * 200, 1ull << 40, 16, rng, "a million images");
    }
}

}  // namespace

int main()
{
    std::mt19937_64 rng(18);
    release_cases(rng);
    grow_cases(rng);
    printf("pool_set_check: ok (%ld cases, each in three workgroup orders)\n", g_cases);
    return 0;
}
