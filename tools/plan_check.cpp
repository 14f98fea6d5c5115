// plan_check.cpp -- the host planner (crc_plan.cpp) run stand-alone, for
// `make plancheck` (ASan + UBSan, no GPU, no HIP, no Python): plan_init and
// plan_choose over the geometries of tests/test_plan_choice.py plus an empty
// and an all-tiny batch.  For every geometry the npieces of the chunks sum to
// the number of (wave, chunk) pairs whose step ranges overlap, and the shipped
// grid is the one the tests expect.  Exits 0, or 1 with a message.
#include <math.h>
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <vector>

#include "cio_plan.h"

using namespace cioa;

// The planner's only link to the rest of the library: no A/B switch is
// honoured here, so every plan below is the shipped one.
extern "C" const char *cioa_diag_getenv(const char *)
{
    return nullptr;
}

namespace {

int g_failed = 0;

std::vector<uint64_t> packed(const std::vector<uint64_t> &lens, uint64_t align)
{
    std::vector<uint64_t> offs(lens.size());
    uint64_t o = 0;
    for (size_t i = 0; i < lens.size(); i++) {
        offs[i] = o;
        o += (lens[i] + align - 1) / align * align;
    }
    return offs;
}

// chunkio_amd/workloads.py cfg3_lens: 65,536 lengths, 4 KiB to 4 MiB.
std::vector<uint64_t> cfg3_lens()
{
    std::vector<uint64_t> lens(65536);
    for (uint64_t i = 0; i < lens.size(); i++) {
        uint64_t z = (0xC1000003ull ^ i) + 0x9E3779B97F4A7C15ull;
        z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
        z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
        z ^= z >> 31;
        lens[i] = (uint64_t) floor(4096.0 * pow(1024.0, (double) (z >> 11) * 0x1p-53));
    }
    return lens;
}

// One geometry on a device of `cus` compute units; want_grid 0: any.
void check(const char *name, const std::vector<uint64_t> &lens, uint64_t align, int cus, uint32_t want_grid,
           int want_aligned = -1)
{
    const std::vector<uint64_t> offs = packed(lens, align);
    const size_t n = lens.size();
    DeviceState st;
    st.cus = cus;
    cio_crc32_plan p;
    PlanHost ph;
    plan_init(&p, &st, n);
    if (const char *err = plan_choose(&p, ph, offs.data(), lens.data(), n)) {
        printf("FAIL %s: %s\n", name, err);
        g_failed = 1;
        return;
    }
    // (wave, chunk) pairs: wave w owns steps [w S / W, (w + 1) S / W), chunk k
    // steps [g, g + nsteps).
    uint64_t pairs = 0, pieces = 0;
    size_t c = 0;
    for (uint32_t w = 0; w < p.W && ph.S > 0; w++) {
        const uint64_t g0 = (uint64_t) w * ph.S / p.W, g1 = (uint64_t) (w + 1) * ph.S / p.W;
        while (c < n && ph.desc[c].g + ph.desc[c].nsteps <= g0) {
            c++;
        }
        for (size_t k = c; g0 < g1 && k < n && ph.desc[k].g < g1; k++) {
            pairs += ph.desc[k].nsteps != 0;
        }
    }
    for (size_t k = 0; k < n; k++) {
        pieces += ph.desc[k].nsteps ? ph.desc[k].npieces : 0;
    }
    const bool ok = pairs == pieces && (want_grid == 0 || p.grid == want_grid) && p.W == p.grid * kWavesPerWg &&
                    p.S == ph.S && p.ntiny == ph.tiny.size() && ph.ws.size() == p.W &&
                    (want_aligned < 0 || (int) p.aligned == want_aligned) &&
                    ph.afac.size() == (p.aligned ? (size_t) kWave << p.alg2p : 0) &&
                    (!p.aligned || ((uint64_t) p.aq * p.W == p.S && ((uint64_t) p.aq << p.alg2p) == p.unsteps));
    printf("%s %s: cus %d grid %u small %d ahead %d aligned %d S %llu pieces %llu pairs %llu\n", ok ? "ok  " : "FAIL",
           name, cus, p.grid, (int) p.small, (int) p.ahead, (int) p.aligned, (unsigned long long) p.S,
           (unsigned long long) pieces, (unsigned long long) pairs);
    g_failed |= !ok;
}

}  // namespace

int main()
{
    const int cus = 256;
    check("cfg3 packed", cfg3_lens(), 1, cus, 4 * cus);
    check("cfg2 align 16", std::vector<uint64_t>(1024, 409600), 16, cus, cus, 1);
    // the wave-aligned class and its neighbours (tests/test_plan_aligned.py)
    check("aligned 256 x 16 x 3 steps", std::vector<uint64_t>(256, 48 * 4096), 16, cus, cus, 1);
    check("aligned 2048 x 2 x 1 step", std::vector<uint64_t>(2048, 2 * 4096), 16, cus, cus, 1);
    check("not aligned: one chunk more", std::vector<uint64_t>(2049, 2 * 4096), 16, cus, cus, 0);
    check("not aligned: whole chunks per wave", std::vector<uint64_t>(4096, 5 * 4096), 16, cus, cus, 0);
    check("not aligned: 32 waves per chunk", std::vector<uint64_t>(128, 32 * 3 * 4096), 16, cus, cus, 0);
    check("1024 x 4 MiB", std::vector<uint64_t>(1024, 4 << 20), 1, cus, cus, 0);
    check("8192 x 4 MiB", std::vector<uint64_t>(8192, 4 << 20), 1, cus, 4 * cus);
    check("4096 x 4096 B", std::vector<uint64_t>(4096, 4096), 1, cus, 0);
    check("empty", std::vector<uint64_t>(), 1, cus, cus);
    check("all tiny", std::vector<uint64_t>{0, 3, 1, 2, 0, 3}, 1, cus, cus);
    // test_anticamp_grid's rows: chunk length, steps (or chunks) per wave, reduced grid.
    const struct {
        uint64_t clen, per_wave;
        bool reduced;
    } rows[] = {{4096, 16, true},  {4096, 128, true}, {4096, 25, false},  {4096, 256, false},
                {65536, 16, true}, {65536, 64, true}, {65536, 25, false}, {65536, 128, false}};
    for (const auto &r : rows) {
        for (int c : {256, 304}) {    // 304: not a multiple of 32, never reduced
            const size_t n = (size_t) c * 16 * r.per_wave / (r.clen / 4096);
            char name[64];
            snprintf(name, sizeof(name), "anticamp %llu x %llu", (unsigned long long) r.clen,
                     (unsigned long long) r.per_wave);
            check(name, std::vector<uint64_t>(n, r.clen), 16, c, r.reduced && c % 32 == 0 ? c / 32 * 31 : c);
        }
    }
    return g_failed;
}
