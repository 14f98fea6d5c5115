// route_check.cpp -- the arithmetic of routing records to chunk images by
// their metadata (route.h: the text route_gpu.hip's kernels run), stand-alone
// on the host under ASan + UBSan: no GPU, no HIP.  `make routecheck`.
//
// The tag rule at every boundary of R2.  Then the lower bound, the candidates'
// walk and the choice of R4 over directories of exactly n entries on the heap
// -- so the sanitizer sees any load outside -- that are sorted, shuffled, hold
// entries >= n, hold one key only, and hold the keys 0 and 0xffffffff, with
// verdicts that pass every image, none, and a pseudo-random half: against a
// linear restatement that knows nothing of a bound.  On a sorted directory the
// result is the lowest passing image of the key (R4); on any directory it is a
// passing image < n of the key or none (R6).  Last the packed counts of the
// totals' scan against three plain counters.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <vector>

#include "route.h"

using namespace cioa;

namespace {

int g_cases = 0, g_failed = 0;

void check(bool ok, const char *what, uint64_t a = 0, uint64_t b = 0)
{
    ++g_cases;
    if (!ok) {
        fprintf(stderr, "route_check: %s (%llu, %llu)\n", what, (unsigned long long) a, (unsigned long long) b);
        ++g_failed;
    }
}

uint64_t g_rng = 0x9e3779b97f4a7c15ull;
uint32_t rnd()
{
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t) (g_rng >> 16);
}

void tag_rule()
{
    const uint64_t top = ~0ull;
    check(route_tag_ok(0, 0, 0), "empty tag in an empty buffer");
    check(route_tag_ok(top, 0, 0), "empty tag at any offset");
    check(route_tag_ok(1000, 0, 10), "empty tag beyond the buffer");
    check(route_tag_ok(0, 65535, 65535), "len 65535");
    check(!route_tag_ok(0, 65536, 1 << 20), "len 65536");
    check(!route_tag_ok(0, top, top), "len 2^64 - 1");
    check(route_tag_ok(10, 5, 15), "ends at tag_bytes");
    check(!route_tag_ok(10, 5, 14), "ends one past tag_bytes");
    check(!route_tag_ok(11, 5, 15), "starts one late");
    check(!route_tag_ok(16, 1, 15), "starts beyond tag_bytes");
    check(!route_tag_ok(top, 1, top), "off + len wraps to 0");
    check(!route_tag_ok(top - 3, 65535, top), "off + len wraps");
    check(!route_tag_ok(0, 1, 0), "a byte of an empty buffer");
}

// The linear restatement of the lower bound over a sorted array: a plain scan.
uint32_t linear_lower_bound(const std::vector<uint32_t> &keys, uint32_t key)
{
    uint32_t j = 0;
    while (j < keys.size() && keys[j] < key) {
        ++j;
    }
    return j;
}

struct Dir {
    uint32_t *keys, *imgs;      // exactly n entries each, on the heap
    uint32_t n;
};

Dir make_dir(const std::vector<uint32_t> &keys, const std::vector<uint32_t> &imgs)
{
    Dir d;
    d.n = (uint32_t) keys.size();
    d.keys = (uint32_t *) malloc(d.n ? d.n * sizeof(uint32_t) : 1);
    d.imgs = (uint32_t *) malloc(d.n ? d.n * sizeof(uint32_t) : 1);
    if (!d.keys || !d.imgs) {
        fprintf(stderr, "route_check: out of memory\n");
        exit(2);
    }
    std::copy(keys.begin(), keys.end(), d.keys);
    std::copy(imgs.begin(), imgs.end(), d.imgs);
    return d;
}

// One directory against every probe key of interest and three verdicts.
void probe_all(const std::vector<uint32_t> &keys, const std::vector<uint32_t> &imgs, bool sorted, const char *what)
{
    const Dir d = make_dir(keys, imgs);
    const uint32_t n = d.n;
    std::vector<uint32_t> probes = {0, 1, 0x7fffffffu, 0x80000000u, 0xfffffffeu, 0xffffffffu};
    for (uint32_t k : keys) {
        probes.push_back(k);
        probes.push_back(k + 1);
        probes.push_back(k - 1);
    }
    for (uint32_t key : probes) {
        const uint32_t lb = route_lower_bound(d.keys, n, key);
        check(lb <= n, "lower bound outside 0 .. n", lb, n);
        if (sorted) {
            check(lb == linear_lower_bound(keys, key), what, key, lb);
        }
        for (int mode = 0; mode < 3; ++mode) {
            const uint32_t salt = rnd();
            uint32_t calls = 0;
            auto pass = [&](uint32_t i) {
                ++calls;
                check(i < n, "a verdict was asked for an image >= n", i, n);
                return mode == 0 ? true : mode == 1 ? false : (((i * 2654435761u) ^ salt) >> 7 & 1u) != 0;
            };
            const uint32_t got = route_match(d.keys, d.imgs, n, key, pass);
            check(calls <= n, "more than n steps", calls, n);
            // R6, any contents: a passing image < n that the directory lists under the key, or none
            if (got != kRouteNone) {
                bool listed = false;
                for (uint32_t j = 0; j < n; ++j) {
                    listed |= keys[j] == key && imgs[j] == got;
                }
                uint32_t before = calls;
                check(got < n && listed && pass(got), "a match the directory does not hold", key, got);
                calls = before;
            }
            if (sorted) {                         // R4: the first passing candidate in ascending position
                uint32_t want = kRouteNone;
                for (uint32_t j = 0; j < n && want == kRouteNone; ++j) {
                    if (keys[j] == key && imgs[j] < n && pass(imgs[j])) {
                        want = imgs[j];
                    }
                }
                check(got == want, what, key, got);
            }
        }
    }
    free(d.keys);
    free(d.imgs);
}

void directories()
{
    const uint32_t sizes[] = {0, 1, 2, 3, 7, 64, 65, 257, 1000};
    for (uint32_t n : sizes) {
        // R1's shape: the stable sort of (key, i), few distinct keys so that runs are long
        for (uint32_t distinct : {1u, 2u, 5u, 1u << 30}) {
            std::vector<std::pair<uint32_t, uint32_t>> e;
            for (uint32_t i = 0; i < n; ++i) {
                uint32_t k = distinct == 1 ? 0x1234u : rnd() % distinct;
                if (distinct == 5) {
                    const uint32_t ends[] = {0, 0xffffffffu, 1, 0xfffffffeu, 0x80000000u};
                    k = ends[k];
                }
                e.push_back({k, i});
            }
            std::stable_sort(e.begin(), e.end(), [](auto &a, auto &b) { return a.first < b.first; });
            std::vector<uint32_t> keys, imgs;
            for (auto &p : e) {
                keys.push_back(p.first);
                imgs.push_back(p.second);
            }
            probe_all(keys, imgs, true, "sorted directory");
            // entries >= n among the indices: skipped, the rest as before
            std::vector<uint32_t> holes = imgs;
            for (uint32_t j = 0; j < n; j += 3) {
                holes[j] = j % 2 ? n : 0xffffffffu;
            }
            probe_all(keys, holes, true, "sorted directory with entries >= n");
            std::vector<uint32_t> all_out(n, 0xffffffffu);
            probe_all(keys, all_out, true, "sorted directory of entries >= n alone");
            // shuffled: keys and indices no longer in any order
            std::vector<uint32_t> sk = keys, si = imgs;
            for (uint32_t j = n; j > 1; --j) {
                const uint32_t a = j - 1, b = rnd() % j;
                std::swap(sk[a], sk[b]);
                std::swap(si[a], si[b]);
            }
            probe_all(sk, si, false, "shuffled directory");
            std::vector<uint32_t> garbage(n);
            for (uint32_t j = 0; j < n; ++j) {
                garbage[j] = rnd();
            }
            probe_all(sk, garbage, false, "shuffled keys over garbage indices");
        }
        probe_all(std::vector<uint32_t>(n, 0), std::vector<uint32_t>(n, 0), true, "all keys 0, all image 0");
        probe_all(std::vector<uint32_t>(n, 0xffffffffu), std::vector<uint32_t>(n, n ? n - 1 : 0), true,
                  "all keys 0xffffffff");
    }
}

void counts()
{
    for (int round = 0; round < 8; ++round) {
        uint64_t sum = 0, matched = 0, missed = 0, bad = 0;
        const uint32_t n = round == 0 ? 0 : 1 + rnd() % 5000;
        for (uint32_t r = 0; r < n; ++r) {
            const bool dir_ok = round != 1, tag_ok = rnd() % 7 != 0, hit = rnd() % 3 != 0;
            const int32_t st = route_status(dir_ok, tag_ok, hit);
            check(st == (!dir_ok || !tag_ok ? -1 : hit ? 0 : -2), "status");
            check(route_count_missed(sum) == missed, "a missed record's rank", r, missed);
            sum += route_count_pack(st);
            matched += st == 0;
            missed += st == -2;
            bad += st == -1;
        }
        check(route_count_matched(sum) == matched && route_count_missed(sum) == missed &&
                  n - matched - missed == bad,
              "totals", matched, missed);
    }
    // the halves at their ends: 2^32 - 1 of either kind do not meet
    const uint64_t full = 0xffffffffull;
    check(route_count_missed(full * route_count_pack(-2)) == full && route_count_matched(full) == 0, "low half full");
    check(route_count_matched(full * route_count_pack(0)) == full && route_count_missed(full << 32) == 0,
          "high half full");
}

}  // namespace

int main()
{
    tag_rule();
    directories();
    counts();
    if (g_failed) {
        fprintf(stderr, "route_check: %d of %d cases failed\n", g_failed, g_cases);
        return 1;
    }
    printf("route_check: ok (%d cases)\n", g_cases);
    return 0;
}
