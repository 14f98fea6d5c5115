// coalesce_check.cpp -- coalesce.h, the text the kernels of coalesce_gpu.hip
// run, on the host under ASan + UBSan (`make coalescecheck`): no GPU, no HIP.
//
// Every kernel of the chain is restated as a function of ONE workgroup that
// calls coalesce.h / pool_set.h / sort_records.h for every decision and keeps
// the workgroup scans as plain loops; the workgroups of a kernel run in
// ascending, descending and random order (no workgroup may depend on another
// of its kernel), the ballots of the K-way counting scan are taken over 64
// explicit lanes, the sort runs as sort_records.h's digit passes, and every
// array has exactly the extent the call may touch, so ASan sees a stray index.
// The result -- both arrays whole, the set words, dev_total -- is compared with
// a sequential loop in 128-bit arithmetic that shares no text with the header.
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <random>
#include <vector>

#include "coalesce.h"

using namespace cioa;
typedef unsigned __int128 u128;

namespace {

struct Set {
    std::vector<uint64_t> offs, caps, words;
    uint32_t n_cls;
    uint64_t stride;
};

struct Call {
    uint64_t dev_bytes, align;
    uint32_t target;
    bool dry;
};

[[noreturn]] void die(const char *what, const char *name)
{
    std::fprintf(stderr, "coalesce_check: %s: %s\n", name, what);
    std::exit(1);
}

// ---------------------------------------------------------------- the reference

bool ref_sound(const Set &s)
{
    u128 below = 0;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        const uint64_t *p = &s.words[4 * k];
        const bool pow2 = p[3] != 0 && (p[3] & (p[3] - 1)) == 0 && p[3] <= 4096;
        if (p[0] > p[1] || p[2] < 24 || !pow2 || p[1] > s.stride || (k != 0 && (u128) p[2] <= below)) {
            return false;
        }
        below = p[2];
    }
    return true;
}

int ref_class(const Set &s, u128 off, u128 cap)
{
    int c = -1;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        if ((u128) s.words[4 * k + 2] <= cap && off % s.words[4 * k + 3] == 0) {
            c = (int) k;
        }
    }
    return c;
}

struct Slot {
    u128 off, cap;
};

// The rules C0..C8, sequentially.  Changes s as the call does; returns dev_total.
std::vector<uint64_t> reference(Set &s, const Call &c)
{
    std::vector<uint64_t> total(5 + s.n_cls, 0);
    if (!ref_sound(s)) {
        total[0] = 1;
        return total;
    }
    const u128 T = s.words[4 * c.target + 2], P = s.words[4 * c.target + 3];
    std::vector<Slot> ent;
    uint64_t ill = 0, hit = 0, groups = 0, absorbed = 0;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        for (uint64_t j = 0; j < s.words[4 * k]; ++j) {
            const u128 off = s.offs[k * s.stride + j], cap = s.caps[k * s.stride + j];
            if (cap >= 1 && off + cap <= (u128) c.dev_bytes && off % c.align == 0) {
                ent.push_back({off, cap});
            } else {
                ill += 1;
            }
        }
    }
    std::stable_sort(ent.begin(), ent.end(), [](const Slot &a, const Slot &b) { return a.off < b.off; });
    std::vector<Slot> surv, outs;
    u128 reach = 0;
    for (const Slot &e : ent) {
        if (e.off < reach) {
            hit += 1;
        } else {
            surv.push_back(e);
        }
        reach = std::max(reach, e.off + e.cap);
    }
    const size_t n = surv.size();
    for (size_t i = 0; i < n;) {
        if (surv[i].cap >= T) {
            outs.push_back(surv[i++]);
            continue;
        }
        size_t e = i + 1;
        while (e < n && surv[e].cap < T &&
               (surv[e - 1].off + surv[e - 1].cap + c.align - 1) / c.align * c.align == surv[e].off) {
            e += 1;
        }
        size_t g = i;
        for (; g < e && surv[g].off % P != 0; ++g) {
            outs.push_back(surv[g]);
        }
        while (g < e) {
            size_t h = g + 1;
            while (h < e && !(surv[h].off >= surv[g].off + T && surv[h].off % P == 0)) {
                h += 1;
            }
            const u128 end = surv[h - 1].off + surv[h - 1].cap;
            if (h == e && end - surv[g].off < T) {
                outs.insert(outs.end(), surv.begin() + g, surv.begin() + e);
            } else {
                outs.push_back({surv[g].off, end - surv[g].off});
                if (h - g >= 2) {
                    groups += 1;
                    absorbed += h - g;
                }
            }
            g = h;
        }
        i = e;
    }
    std::vector<std::vector<Slot>> filed(s.n_cls);
    for (const Slot &o : outs) {
        const int k = ref_class(s, o.off, o.cap);
        if (k < 0) {
            ill += 1;
        } else {
            filed[k].push_back(o);
        }
    }
    bool over = false;
    for (uint32_t k = 0; k < s.n_cls; ++k) {
        total[5 + k] = filed[k].size();
        over = over || filed[k].size() > s.words[4 * k + 1];
    }
    total[0] = over ? 2 : 0;
    total[1] = ill;
    total[2] = hit;
    total[3] = groups;
    total[4] = absorbed;
    if (!over && !c.dry) {
        for (uint32_t k = 0; k < s.n_cls; ++k) {
            for (size_t j = 0; j < filed[k].size(); ++j) {
                s.offs[k * s.stride + j] = (uint64_t) filed[k][j].off;
                s.caps[k * s.stride + j] = (uint64_t) filed[k][j].cap;
            }
            s.words[4 * k] = filed[k].size();
        }
    }
    return total;
}

// ---------------------------------------------------------------- the chain, workgroup by workgroup

struct Chain {
    Set &s;
    Call c;
    uint32_t n, nb, sentinel;
    // the writer's arenas, each of exactly n words, and the table's 64-bit words
    std::vector<uint32_t> key, skey, sidx, code, rank, local;
    std::vector<uint64_t> eoff, ecap, emax, soff, scap, ocap, tab;
    std::vector<uint64_t> total;
    std::vector<uint32_t> writes;             // stores per set word / array word, for the one-writer rule

    Chain(Set &set, const Call &call)
        : s(set), c(call), n((uint32_t) (set.n_cls * set.stride)), nb((n + kCoalBlock - 1) / kCoalBlock),
          sentinel((uint32_t) coal_key_bound(call.dev_bytes, call.align)), key(n), skey(n), sidx(n), code(n), rank(n),
          local(n), eoff(n), ecap(n), emax(n), soff(n), scap(n), ocap(n),
          tab(coal_col_at(kCoalCols, nb)), total(5 + set.n_cls, 0x55), writes(4 * set.n_cls + 2 * n, 0)
    {
    }
    uint64_t *words() { return &tab[set_words_at(nb)]; }
    uint64_t *col(uint32_t which) { return &tab[coal_col_at(which, nb)]; }

    void gather(uint32_t wg)
    {
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t p = (uint64_t) wg * kCoalBlock + t;
            if (p >= n) {
                continue;
            }
            const uint64_t k = p / s.stride, j = p - k * s.stride;
            const bool entry = set_sound(s.words.data(), s.n_cls, s.stride) && j < s.words[4 * k + kPoolCount];
            key[p] = coal_key(entry, entry ? s.offs[p] : 0, entry ? s.caps[p] : 0, c.dev_bytes, c.align, sentinel);
        }
    }

    // sort_records.h's passes: a stable counting sort per digit of min(key, sentinel).
    void sort()
    {
        std::vector<uint32_t> k(n), x(n);
        for (uint32_t r = 0; r < n; ++r) {
            k[r] = sort_key(key[r], sentinel);
            x[r] = r;
        }
        for (uint32_t pass = 0; pass < sort_passes(sentinel); ++pass) {
            std::vector<uint32_t> at(kSortRadix + 1, 0), k2(n), x2(n);
            for (uint32_t r = 0; r < n; ++r) {
                at[sort_digit(k[r], pass) + 1] += 1;
            }
            for (uint32_t d = 0; d < kSortRadix; ++d) {
                at[d + 1] += at[d];
            }
            for (uint32_t r = 0; r < n; ++r) {
                const uint32_t q = at[sort_digit(k[r], pass)]++;
                k2[q] = k[r];
                x2[q] = x[r];
            }
            k.swap(k2);
            x.swap(x2);
        }
        skey = k;
        sidx = x;
        for (uint32_t r = 0; r + 1 < n; ++r) {
            if (skey[r] > skey[r + 1] || (skey[r] == skey[r + 1] && sidx[r] > sidx[r + 1])) {
                die("the passes do not sort the keys stably", "sort");
            }
        }
    }

    void ends(uint32_t wg)
    {
        uint64_t run = 0;
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kCoalBlock + t;
            uint64_t off = 0, cap = 0;
            if (i < n) {
                const uint32_t p = sidx[i];
                const bool valid = skey[i] < sentinel && p < n;
                if (valid) {
                    off = s.offs[p];
                    cap = s.caps[p];
                }
                eoff[i] = off;
                ecap[i] = cap;
                const bool next = i + 1 < n && skey[i + 1] < sentinel;
                if (valid && !next) {
                    words()[kCoalWValid] = i + 1;
                } else if (i == 0 && !valid) {
                    words()[kCoalWValid] = 0;
                }
                emax[i] = run;
            }
            run = std::max(run, off + cap);
        }
        col(kCoalColMax)[wg] = run;
    }

    void mscan()
    {
        uint64_t run = 0;
        for (uint32_t j = 0; j < nb; ++j) {
            const uint64_t v = col(kCoalColMax)[j];
            col(kCoalColMax)[j] = run;
            run = std::max(run, v);
        }
    }

    void survive(uint32_t wg)
    {
        uint64_t cnt = 0;
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kCoalBlock + t;
            if (i >= n) {
                continue;
            }
            const bool surv =
                skey[i] < sentinel && !coal_collides(eoff[i], std::max(col(kCoalColMax)[wg], emax[i]));
            rank[i] = surv ? 2 * (uint32_t) cnt + 1 : 0;
            cnt += surv ? 1 : 0;
        }
        col(kCoalColSurv)[wg] = cnt;
    }

    uint64_t scan_col(uint32_t which)
    {
        uint64_t run = 0;
        for (uint32_t j = 0; j < nb; ++j) {
            const uint64_t v = col(which)[j];
            col(which)[j] = run;
            run = place_add(run, v);
        }
        return run;
    }

    void compact(uint32_t wg)
    {
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kCoalBlock + t;
            if (i >= n || rank[i] == 0) {
                continue;
            }
            const uint64_t q = col(kCoalColSurv)[wg] + (rank[i] >> 1);
            if (q > i) {
                die("a survivor moves up", "compact");
            }
            soff[q] = eoff[i];
            scap[q] = ecap[i];
        }
    }

    void link(uint32_t wg)
    {
        const uint64_t ns = words()[kCoalWSurv];
        uint64_t cnt = 0;
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t q = (uint64_t) wg * kCoalBlock + t;
            if (q >= ns) {
                continue;
            }
            const uint64_t T = s.words[4 * c.target + kPoolCls];
            const bool linked = q != 0 && coal_links(soff[q - 1], scap[q - 1], soff[q], scap[q], T, c.align);
            code[q] = (scap[q] < T ? kCoalCand : 0) | (linked ? 0 : kCoalStart);
            ocap[q] = scap[q];
            cnt += linked ? 0 : 1;
            local[q] = (uint32_t) cnt;
        }
        col(kCoalColRun)[wg] = cnt;
    }

    void groups(uint32_t wg)
    {
        const uint64_t ns = words()[kCoalWSurv];
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t q = (uint64_t) wg * kCoalBlock + t;
            if (q >= ns || (code[q] & (kCoalCand | kCoalStart)) != (kCoalCand | kCoalStart)) {
                continue;
            }
            coal_walk_run(soff.data(), scap.data(), col(kCoalColRun), local.data(), ns, q,
                          s.words[4 * c.target + kPoolCls], s.words[4 * c.target + kPoolAlign], ocap.data(),
                          code.data());
        }
    }

    // class_rank, wave by wave: the ballots over 64 explicit lanes.
    void classes(uint32_t wg)
    {
        const uint64_t ns = words()[kCoalWSurv];
        std::vector<uint32_t> wcount(kSetWaves * kPoolSetMax, 0), cls(kCoalBlock, kSetNone), lrank(kCoalBlock, 0);
        uint64_t packed = 0;
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t q = (uint64_t) wg * kCoalBlock + t;
            if (q >= ns) {
                continue;
            }
            const uint32_t cd = code[q];
            const bool out = !(cd & kCoalAbsorbed);
            if (out) {
                cls[t] = set_release_class(s.words.data(), s.n_cls, soff[q], ocap[q]);
            }
            packed += coal_cnt_pack((cd & kCoalGroup) ? 1 : 0, (cd & (kCoalGroup | kCoalAbsorbed)) ? 1 : 0,
                                    out && cls[t] == kSetNone ? 1 : 0);
        }
        for (uint32_t wave = 0; wave < kSetWaves; ++wave) {
            uint64_t all = 0, ballot[kSetBits] = {0, 0, 0};
            for (uint32_t lane = 0; lane < kSetWave; ++lane) {
                const uint32_t cl = cls[wave * kSetWave + lane];
                if (cl != kSetNone) {
                    all |= 1ull << lane;
                    for (uint32_t bit = 0; bit < kSetBits; ++bit) {
                        ballot[bit] |= (uint64_t) ((cl >> bit) & 1u) << lane;
                    }
                }
            }
            for (uint32_t lane = 0; lane < kSetWave; ++lane) {
                const uint32_t cl = cls[wave * kSetWave + lane];
                if (cl == kSetNone) {
                    continue;
                }
                const uint64_t match = set_match(all, ballot, cl);
                lrank[wave * kSetWave + lane] = sort_lane_rank(match, lane);
                if (lrank[wave * kSetWave + lane] == 0) {
                    wcount[wave * kPoolSetMax + cl] = sort_popcount(match);
                }
            }
        }
        for (uint32_t k = 0; k < kPoolSetMax; ++k) {
            tab[set_tab_at(k, wg, nb)] = set_wave_scan(wcount.data(), k);
        }
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t q = (uint64_t) wg * kCoalBlock + t;
            if (q >= ns) {
                continue;
            }
            rank[q] = cls[t] != kSetNone ? wcount[(t / kSetWave) * kPoolSetMax + cls[t]] + lrank[t] : 0;
            code[q] |= cls[t] << kSetClsShift;
        }
        col(kCoalColCnt)[wg] = packed;
    }

    void final()
    {
        // class_scan: one linear exclusive scan of the class-major table, then every word less its class's first
        const uint32_t wordsn = s.n_cls * nb;
        uint64_t run = 0, count[kPoolSetMax] = {0}, first[kPoolSetMax] = {0};
        for (uint32_t j = 0; j < wordsn; ++j) {
            const uint64_t v = tab[j];
            tab[j] = run;
            run += v;
        }
        for (uint32_t k = 0; k < s.n_cls; ++k) {
            first[k] = tab[set_tab_at(k, 0, nb)];
            count[k] = set_class_total(first[k], k + 1 < s.n_cls ? tab[set_tab_at(k + 1, 0, nb)] : run);
        }
        for (uint32_t j = 0; j < wordsn; ++j) {
            tab[j] = set_class_excl(tab[j], first[j / nb]);
        }
        uint64_t f[3] = {0, 0, 0};
        for (uint32_t j = 0; j < nb; ++j) {
            for (uint32_t i = 0; i < 3; ++i) {
                f[i] += coal_cnt_field(col(kCoalColCnt)[j], i);
            }
        }
        uint64_t mask;
        words()[kCoalWVerdict] =
            coal_totals(s.words.data(), s.n_cls, set_sound(s.words.data(), s.n_cls, s.stride), count,
                        words()[kCoalWValid], words()[kCoalWSurv], f[0], f[1], f[2], total.data(), mask);
        words()[kCoalWMask] = mask;
        for (uint32_t k = 0; k < s.n_cls; ++k) {
            words()[kCoalWCount + k] = count[k];
        }
    }

    void commit(uint32_t wg)
    {
        if (words()[kCoalWVerdict] != kCoalOk) {
            return;
        }
        for (uint32_t t = 0; t < kCoalBlock; ++t) {
            const uint64_t q = (uint64_t) wg * kCoalBlock + t;
            if (q < s.n_cls && ((words()[kCoalWMask] >> q) & 1u)) {
                s.words[4 * q + kPoolCount] = words()[kCoalWCount + q];
                writes[4 * q] += 1;
            }
            if (q >= words()[kCoalWSurv]) {
                continue;
            }
            const uint32_t cd = code[q], cl = (cd >> kSetClsShift) & 15u;
            if ((cd & kCoalAbsorbed) || cl >= s.n_cls) {
                continue;
            }
            const uint64_t at = tab[set_tab_at(cl, wg, nb)] + rank[q];
            if (at >= s.stride) {
                die("an output lands outside its class", "commit");
            }
            s.offs[cl * s.stride + at] = soff[q];
            s.caps[cl * s.stride + at] = ocap[q];
            writes[4 * s.n_cls + cl * s.stride + at] += 1;
            writes[4 * s.n_cls + n + cl * s.stride + at] += 1;
        }
    }

    void run(int order, std::mt19937_64 &rng)
    {
        std::vector<uint32_t> wgs(nb);
        for (uint32_t j = 0; j < nb; ++j) {
            wgs[j] = order == 1 ? nb - 1 - j : j;
        }
        auto each = [&](void (Chain::*kernel)(uint32_t)) {
            if (order == 2) {
                std::shuffle(wgs.begin(), wgs.end(), rng);
            }
            for (uint32_t wg : wgs) {
                (this->*kernel)(wg);
            }
        };
        each(&Chain::gather);
        sort();
        each(&Chain::ends);
        mscan();
        each(&Chain::survive);
        words()[kCoalWSurv] = scan_col(kCoalColSurv);
        each(&Chain::compact);
        each(&Chain::link);
        (void) scan_col(kCoalColRun);
        each(&Chain::groups);
        each(&Chain::classes);
        final();
        if (!c.dry) {
            each(&Chain::commit);
        }
    }
};

// ---------------------------------------------------------------- cases

uint64_t round_up(uint64_t v, uint64_t a)
{
    return (v + a - 1) / a * a;
}

struct Shape {
    const char *name;
    uint32_t n_cls;
    uint64_t stride;
    uint32_t entries;
    uint64_t dev_bytes, align;
    uint32_t target;
    double adjacent, bad;
    uint64_t pal_target;                      // the target class's alignment (the others: align)
    bool dry;
    uint64_t room_target;                     // the target class's capacity word (0: stride)
};

Set make_set(const Shape &sh, std::mt19937_64 &rng)
{
    static const uint64_t cls[8] = {40, 96, 200, 520, 1100, 2304, 5000, 12000};
    Set s;
    s.n_cls = sh.n_cls;
    s.stride = sh.stride;
    s.offs.assign(sh.n_cls * sh.stride, 0x7777777777777777ull);
    s.caps.assign(sh.n_cls * sh.stride, 0x7777777777777777ull);
    for (uint32_t k = 0; k < sh.n_cls; ++k) {
        const uint64_t w[4] = {0, k == sh.target && sh.room_target ? sh.room_target : sh.stride, cls[k],
                               k == sh.target ? sh.pal_target : sh.align};
        s.words.insert(s.words.end(), w, w + 4);
    }
    auto uni = [&](uint64_t lo, uint64_t hi) { return lo + rng() % (hi - lo); };
    const uint64_t sizes[7] = {cls[0], cls[0] + 5, cls[1], cls[sh.target] / 2 + 1, 3 * sh.align, 1, cls[sh.n_cls - 1]};
    std::vector<std::pair<uint64_t, uint64_t>> slots;
    uint64_t cur = sh.align * uni(0, 3);
    while (slots.size() < sh.entries) {
        uint64_t cap = sizes[uni(0, 7)];
        const uint64_t left = sh.entries - slots.size();
        if (left == 1 && (sh.dev_bytes - 1) / sh.align * sh.align >= cur) {
            cur = (sh.dev_bytes - 1) / sh.align * sh.align;   // the highest key there is
            cap = sh.dev_bytes - cur;
        }
        if (cur + cap > sh.dev_bytes) {
            break;
        }
        slots.push_back({cur, cap});
        cur = round_up(cur + cap, sh.align);
        if ((double) (rng() % 1000) / 1000.0 >= sh.adjacent) {
            const uint64_t units = std::max<uint64_t>(2, (sh.dev_bytes - cur) / sh.align / (2 * left));
            cur += sh.align * uni(1, units);
        }
    }
    for (size_t i = 1; i < slots.size(); ++i) {
        if ((double) (rng() % 1000) / 1000.0 >= sh.bad) {
            continue;
        }
        const auto [o, c] = slots[uni(0, i)];
        const uint64_t big = ~0ull;
        const std::pair<uint64_t, uint64_t> kinds[8] = {
            {o, c}, {o, std::max<uint64_t>(1, c / 2)}, {o + sh.align * ((c / 2) / sh.align), c}, {o, 0},
            {sh.align > 1 ? o + 1 : o, sh.align > 1 ? c : 0}, {sh.dev_bytes - std::min(sh.dev_bytes, sh.align), 2 * sh.align + 1},
            {big - 5, 6 + i % 8}, {big / sh.align * sh.align, big}};
        slots[i] = kinds[uni(0, 8)];
    }
    std::shuffle(slots.begin(), slots.end(), rng);
    for (const auto &sl : slots) {
        uint32_t k = set_release_class(s.words.data(), s.n_cls, sl.first, sl.second);
        if (k == kSetNone || s.words[4 * k] >= s.words[4 * k + 1]) {
            std::vector<uint32_t> free;
            for (uint32_t c = 0; c < s.n_cls; ++c) {
                if (s.words[4 * c] < s.words[4 * c + 1]) {
                    free.push_back(c);
                }
            }
            if (free.empty()) {
                break;
            }
            k = free[uni(0, free.size())];
        }
        s.offs[k * s.stride + s.words[4 * k]] = sl.first;
        s.caps[k * s.stride + s.words[4 * k]] = sl.second;
        s.words[4 * k] += 1;
    }
    return s;
}

void compare(const Set &got, const std::vector<uint64_t> &gt, const Set &want, const std::vector<uint64_t> &wt,
             const char *name)
{
    if (gt != wt) {
        std::fprintf(stderr, "coalesce_check: %s: dev_total", name);
        for (size_t i = 0; i < gt.size(); ++i) {
            std::fprintf(stderr, " %llu/%llu", (unsigned long long) gt[i], (unsigned long long) wt[i]);
        }
        std::fprintf(stderr, " (chain/reference)\n");
        std::exit(1);
    }
    if (got.words != want.words) {
        die("the set words differ", name);
    }
    if (got.offs != want.offs || got.caps != want.caps) {
        die("the set arrays differ", name);
    }
}

uint64_t g_done = 0, g_groups = 0, g_hits = 0, g_ill = 0, g_over = 0, g_tail_short = 0;

// One set through the chain in three orders and through the reference; then
// the second call (C9).
void run_case(const Shape &sh, uint64_t seed, const Set *given = nullptr)
{
    std::mt19937_64 rng(seed);
    const Set start = given ? *given : make_set(sh, rng);
    const Call call = {sh.dev_bytes, sh.align, sh.target, sh.dry};
    Set want = start;
    const std::vector<uint64_t> wt = reference(want, call);
    Set after = start;
    for (int order = 0; order < 3; ++order) {
        Set got = start;
        Chain ch(got, call);
        ch.run(order, rng);
        compare(got, ch.total, want, wt, sh.name);
        for (uint32_t wr : ch.writes) {
            if (wr > 1) {
                die("a word has two writers", sh.name);
            }
        }
        if (sh.dry || wt[0] != 0) {
            if (got.words != start.words || got.offs != start.offs || got.caps != start.caps) {
                die("a call that must change nothing did", sh.name);
            }
            for (uint32_t wr : ch.writes) {
                if (wr != 0) {
                    die("a call that must change nothing stored", sh.name);
                }
            }
        } else {
            for (uint32_t k = 0; k < got.n_cls; ++k) {        // no store of a word that keeps its value
                if ((got.words[4 * k] == start.words[4 * k]) != (ch.writes[4 * k] == 0)) {
                    die("the mask of the set words that change is wrong", sh.name);
                }
            }
        }
        after = got;
    }
    g_groups += wt[3];
    g_hits += wt[2];
    g_ill += wt[1];
    g_over += wt[0] == 2;
    g_done += wt[0] == 0 && !sh.dry;
    if (wt[0] == 0 && !sh.dry) {                  // C9
        Set again = after;
        Chain ch(again, call);
        ch.run(2, rng);
        if (again.words != after.words || again.offs != after.offs || again.caps != after.caps) {
            die("a second call changed the set", sh.name);
        }
        if (ch.total[0] != 0 || ch.total[1] || ch.total[2] || ch.total[3] || ch.total[4]) {
            die("a second call reports work", sh.name);
        }
    }
}

}  // namespace

int main()
{
    const uint64_t big = 1ull << 40, big32 = 1ull << 36;      // 2^28 and 2^31 keys: four passes
    uint64_t seed = 1;
    // E on both sides of 64 and 1024, in one and in several workgroups
    for (uint32_t e : {0u, 1u, 2u, 63u, 64u, 65u, 1023u, 1024u, 1025u, 2049u, 3077u, 4096u}) {
        for (double adj : {0.0, 0.7, 1.0}) {
            const Shape sh = {"sizes", 4, 1024, e, big, 4096, 3, adj, 0.08, 4096, false, 0};
            run_case(sh, seed++);
            const Shape sm = {"sizes, align 32", 4, 1024, e, 1ull << 36, 32, 2, adj, 0.08, 128, false, 0};
            run_case(sm, seed++);
        }
    }
    // key widths of 1 .. 4 passes, both sides of each, and the largest accepted
    for (uint64_t units : {255ull, 256ull, 257ull, 65535ull, 65537ull, (1ull << 24) - 1, (1ull << 24) + 1,
                           0xffffffffull}) {
        for (uint64_t align : {1ull, 32ull, 4096ull}) {
            if (coal_key_bound(units * align, align) != units ||
                sort_passes((uint32_t) units) != (units < 256 ? 1u : units < 65536 ? 2u : units < (1u << 24) ? 3u : 4u)) {
                die("the key bound or its passes", "keys");
            }
            const Shape sh = {"keys", 3, 700, 1500, units * align, align, 1, 0.6, 0.1, align, false, 0};
            run_case(sh, seed++);
        }
    }
    // every n_cls and every legal target; the target's alignment above align: groups ended by alignment
    for (uint32_t n_cls = 2; n_cls <= kPoolSetMax; ++n_cls) {
        for (uint32_t target = 1; target < n_cls; ++target) {
            for (uint64_t pal : {32ull, 128ull, 1024ull}) {
                const Shape sh = {"classes", n_cls, 300, 110u * n_cls, 1ull << 30, 32, target, 0.85, 0.05, pal, false, 0};
                run_case(sh, seed++);
            }
        }
    }
    // one run holding every entry; no two adjacent; DRY; the target overflowing; E above 1024^2
    for (uint32_t e : {65u, 1025u, 2500u}) {
        const Shape one = {"one run", 4, 1024, e, big32, 32, 3, 1.0, 0.0, 32, false, 0};
        run_case(one, seed++);
        const Shape none = {"none adjacent", 4, 1024, e, big32, 32, 3, 0.0, 0.0, 32, false, 0};
        run_case(none, seed++);
        const Shape dry = {"dry", 4, 1024, e, big32, 32, 2, 0.9, 0.1, 64, true, 0};
        run_case(dry, seed++);
        const Shape over = {"overflow", 4, 1024, e, big32, 32, 2, 1.0, 0.0, 32, false, 1};
        run_case(over, seed++);
    }
    if (g_over == 0) {
        die("no case overflowed", "overflow");
    }
    {
        const Shape huge = {"above 1024^2", 8, 300000, 1049000, big, 4096, 5, 0.8, 0.02, 4096, false, 0};
        run_case(huge, seed++);
        const Shape below = {"below 1024^2", 8, 300000, 1048000, big, 4096, 5, 0.8, 0.02, 4096, false, 0};
        run_case(below, seed++);
    }
    // every class overflowing: capacities of one entry against singles that stay where they are
    for (uint32_t k = 0; k < 4; ++k) {
        Shape sh = {"class overflow", 4, 64, 0, big32, 32, 3, 0, 0, 32, false, 0};
        std::mt19937_64 rng(seed++);
        Set s = make_set(sh, rng);
        static const uint64_t cap[4] = {40, 96, 200, 520};
        const uint32_t at = (k + 1) % 4;          // three isolated entries of class k, filed under another class
        for (uint32_t j = 0; j < 3; ++j) {
            s.offs[at * 64 + j] = 4096 * (j + 1);
            s.caps[at * 64 + j] = cap[k];
        }
        s.words[4 * at] = 3;
        s.words[4 * k + 1] = 2;                   // room for two
        Set want = s;
        const std::vector<uint64_t> wt = reference(want, {big32, 32, 3, false});
        if (wt[0] != 2 || wt[5 + k] != 3) {
            die("the case does not overflow its class", "class overflow");
        }
        run_case(sh, seed++, &s);
    }
    // every unsoundness
    for (uint32_t why = 0; why < 6; ++why) {
        Shape sh = {"unsound", 4, 256, 300, big32, 32, 2, 0.8, 0.05, 32, false, 0};
        std::mt19937_64 rng(seed++);
        Set s = make_set(sh, rng);
        switch (why) {
        case 0: s.words[4 * 1 + 0] = s.words[4 * 1 + 1] + 1; break;   // entries above the capacity
        case 1: s.words[4 * 0 + 2] = 23; break;                       // cls below a header
        case 2: s.words[4 * 2 + 3] = 48; break;                       // pal no power of two
        case 3: s.words[4 * 3 + 3] = 8192; break;                     // pal above 4096
        case 4: s.words[4 * 1 + 1] = s.stride + 1; break;             // capacity above the stride
        default: s.words[4 * 2 + 2] = s.words[4 * 1 + 2]; break;      // cls not rising
        }
        Set want = s;
        if (reference(want, {big32, 32, 2, false})[0] != 1) {
            die("the case is sound", "unsound");
        }
        run_case(sh, seed++, &s);
    }
    // groups ended by T, by alignment, by the run's end with and without T bytes left -- by hand:
    // T = 520, P = 128, align = 32, slots of 96 (cap 96) from 4096 on
    {
        Shape sh = {"by hand", 4, 64, 0, big32, 32, 3, 0, 0, 128, false, 0};
        std::mt19937_64 rng(seed++);
        Set s = make_set(sh, rng);
        const uint32_t count = 14;                // offsets 4096 + 96 j: multiples of 128 at j = 0, 4, 8, 12
        for (uint32_t j = 0; j < count; ++j) {
            s.offs[1 * 64 + j] = 4096 + 96 * (count - 1 - j);         // in descending order: the sort has work
            s.caps[1 * 64 + j] = 96;
        }
        s.words[4] = count;
        Set want = s;
        const std::vector<uint64_t> wt = reference(want, {big32, 32, 3, false});
        // g_0 = 0; off >= 520 first at j = 6, aligned at j = 8: group 0 = 8 entries (768 bytes), ended by
        // alignment; from j = 8 the run's end leaves 6 * 96 = 576 >= 520: group 1 = 6 entries
        if (wt[0] != 0 || wt[3] != 2 || wt[4] != 14 || want.words[12] != 2 || want.caps[3 * 64] != 768 ||
            want.caps[3 * 64 + 1] != 576 || want.offs[3 * 64 + 1] != 4096 + 768) {
            die("the reference disagrees with the hand computation", "by hand");
        }
        run_case(sh, seed++, &s);
        s.words[4] = count - 1;                   // without the lowest... the array is descending: drop offset 4096
        Set w2 = s;
        const std::vector<uint64_t> t2 = reference(w2, {big32, 32, 3, false});
        // the run starts at j = 1 (unaligned): j = 1..3 stay single, g_0 = j 4; off >= 4480 + 520 needs j >= 10
        // (4096 + 960 = 5056 >= 5000), aligned at j = 12: group 0 = j 4..11; from j = 12 only 2 * 96 are left: single
        if (t2[0] != 0 || t2[3] != 1 || t2[4] != 8 || w2.words[12] != 1 || w2.caps[3 * 64] != 768 || w2.words[4] != 5) {
            die("the reference disagrees with the second hand computation", "by hand");
        }
        g_tail_short += 1;
        run_case(sh, seed++, &s);
    }
    if (g_groups == 0 || g_hits == 0 || g_ill == 0 || g_tail_short == 0) {
        die("the cases do not reach every rule", "coverage");
    }
    std::printf("coalesce_check: ok (%llu sets coalesced, %llu groups, %llu collisions, %llu ill-formed or classless, %llu overflows)\n",
                (unsigned long long) g_done, (unsigned long long) g_groups, (unsigned long long) g_hits, (unsigned long long) g_ill,
                (unsigned long long) g_over);
    return 0;
}
