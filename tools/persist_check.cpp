// persist_check.cpp -- the host arithmetic of moving chunk images between HBM
// and chunk files (persist_plan.h: the round planner and the file-size rule
// that persist_host.hip runs), stand-alone under ASan + UBSan: no GPU, no HIP.
// `make persistcheck`.
//
// The planner is compared with a restatement in 128-bit arithmetic, and its
// result is checked against what a round IS: consecutive files, slots that
// fit the round maximum, and maximal -- the first file of a round would not
// have fitted the round before.  Boundaries: a file exactly at the maximum and
// one byte over, sizes at and around the 128-byte slot, empty files, a stage
// smaller than a slot, stage sizes near 2^64, and an empty batch.  round_of
// has EXACTLY n entries, so the sanitizer sees an index beyond.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <random>
#include <vector>

#include "persist_plan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
long g_cases = 0;

#define CHECK(c)                                                                \
    do {                                                                        \
        if (!(c)) {                                                             \
            fprintf(stderr, "persist_check: %s:%d: %s\n", __FILE__, __LINE__, #c); \
            abort();                                                            \
        }                                                                       \
    } while (0)

void check_rounds(const std::vector<uint64_t> &sizes, uint64_t stage)
{
    const size_t n = sizes.size();
    std::vector<uint32_t> got(n);
    const uint32_t rounds = persist_rounds(sizes.data(), n, stage, got.data());
    const u128 room = (u128) stage / 128 * 128;
    CHECK(persist_round_max(stage) == (uint64_t) room);
    // the restatement
    uint32_t want_rounds = 0;
    u128 used = 0;
    bool open = false;
    for (size_t i = 0; i < n; ++i) {
        uint32_t want;
        if ((u128) sizes[i] > room) {
            want = kPersistNoRound;
            open = false;
        } else {
            const u128 slot = ((u128) sizes[i] + 127) / 128 * 128;
            if (!open || used + slot > room) {
                ++want_rounds;
                used = 0;
                open = true;
            }
            want = want_rounds - 1;
            used += slot;
        }
        CHECK(got[i] == want);
    }
    CHECK(rounds == want_rounds);
    // what a round is
    std::vector<u128> fill(rounds, 0);
    uint32_t last = 0;
    bool any = false, closed = true;
    for (size_t i = 0; i < n; ++i) {
        if (got[i] == kPersistNoRound) {
            CHECK(sizes[i] > persist_round_max(stage));
            closed = true;
            continue;
        }
        CHECK(got[i] < rounds && (!any || got[i] == last || got[i] == last + 1));
        const u128 slot = (u128) persist_slot(sizes[i]);
        CHECK(slot >= sizes[i] && slot % 128 == 0 && slot - sizes[i] < 128);
        if (any && got[i] == last + 1 && !closed) {
            CHECK(fill[last] + slot > room);      // maximal: it did not fit the round before
        }
        CHECK(!any || got[i] != last || !closed);  // a file over the maximum closed the round before it
        fill[got[i]] += slot;
        CHECK(fill[got[i]] <= room);
        last = got[i];
        any = true;
        closed = false;
    }
    ++g_cases;
}

void boundaries()
{
    check_rounds({}, 0);
    check_rounds({}, 4096);
    for (uint64_t stage : {0ull, 1ull, 127ull, 128ull, 129ull, 255ull, 256ull, 4096ull, 4097ull, 4223ull, 4224ull}) {
        const uint64_t mx = persist_round_max(stage);
        CHECK(mx <= stage && stage - mx < 128 && mx % 128 == 0);
        check_rounds({mx}, stage);                // a file exactly at the maximum
        check_rounds({mx + 1}, stage);            // and one byte over
        check_rounds({mx, mx + 1, mx, 0, mx}, stage);
        check_rounds({0, 0, 0}, stage);
        check_rounds({1, 127, 128, 129, 0, 24, mx + 1, 1, mx, 1}, stage);
        check_rounds({mx / 2, mx / 2, 1, mx / 2 + 1, mx / 2}, stage);
    }
    for (uint64_t stage : {~0ull, ~0ull - 127, 1ull << 63}) {
        check_rounds({~0ull, ~0ull - 126, ~0ull - 127, 1ull << 63, 1ull << 63, (1ull << 63) - 128, 128, 1}, stage);
    }
    // the file-size rule
    CHECK(persist_file_size(100, 4096, false, 4096) == 4096 && persist_file_size(100, 100, false, 1) == 100);
    CHECK(persist_file_size(24, 9999, true, 1) == 24 && persist_file_size(4096, 9999, true, 4096) == 4096);
    CHECK(persist_file_size(4097, 9999, true, 4096) == 8192 && persist_file_size(1, 1, true, 4096) == 4096);
    CHECK(persist_file_size(4095, 4095, true, 4096) == 4096);   // the trimmed file may exceed the slot
    CHECK(persist_file_size(100, 200, true, kPersistPageMax) == kPersistPageMax);
    CHECK(persist_file_size(~0ull - 5, ~0ull, true, 4096) == ~0ull - 5);   // a round-up that would wrap: exact
    g_cases += 8;
}

void random_cases()
{
    std::mt19937_64 rng(20262);
    for (int it = 0; it < 20000; ++it) {
        const uint64_t stage = rng() % 3 ? rng() % 20000 : rng() % 600;
        const size_t n = rng() % 40;
        std::vector<uint64_t> sizes(n);
        for (uint64_t &s : sizes) {
            const uint64_t pick = rng() % 8;
            s = pick == 0 ? 0 : pick == 1 ? persist_round_max(stage) + rng() % 3 - 1 : rng() % (stage / 2 + 200);
        }
        check_rounds(sizes, stage);
        const uint64_t used = rng() % 100000, cap = used + rng() % 5000, page = 1ull << (rng() % 31);
        const uint64_t f = persist_file_size(used, cap, true, page);
        CHECK(f >= used && f % page == 0 && f - used < page && persist_file_size(used, cap, false, page) == cap);
    }
}

}  // namespace

int main()
{
    boundaries();
    random_cases();
    printf("persist_check: %ld cases passed\n", g_cases);
    return 0;
}
