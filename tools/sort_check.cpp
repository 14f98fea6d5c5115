// sort_check.cpp -- the ungrouped append's stable radix sort (sort_records.h:
// the text the kernels sort_hist, sort_scan and sort_scatter run), stand-alone
// on the host under ASan + UBSan: no GPU, no HIP.  `make sortcheck`.
//
// The three kernels of a pass are restated workgroup by workgroup and, inside
// sort_scatter, wave by wave with the ballot emulated over 64 lanes; the
// workgroups of sort_hist and of sort_scatter run in ascending, descending and
// random order (no workgroup may depend on another of its kernel), and so do
// the waves inside a workgroup.  The sorted (key, index) list is compared with
// std::stable_sort over (clamped key, index).  Keys only, no data.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "sort_records.h"
#include "check_scan.h"

using namespace cioa;

namespace {

struct Sorted {
    std::vector<uint32_t> key, idx;
    bool operator==(const Sorted &o) const { return key == o.key && idx == o.idx; }
};

// Record r of the pass: load_key of sort_records_gpu.hip.
uint32_t load_key(const std::vector<uint32_t> &img, const std::vector<uint32_t> &kin, uint32_t pass, uint32_t n_img,
                  uint64_t r)
{
    return pass == 0 ? sort_key(img[r], n_img) : kin[r];
}

// sort_hist, workgroup wg.
void hist_wg(const std::vector<uint32_t> &img, const std::vector<uint32_t> &kin, uint32_t pass, uint32_t n_img,
             uint32_t nb, uint32_t wg, std::vector<uint32_t> &table)
{
    const uint64_t n = img.size();
    uint32_t cnt[kSortRadix] = {0};
    for (uint32_t t = 0; t < kSortBlock; ++t) {
        const uint64_t r = (uint64_t) wg * kSortBlock + t;
        if (r < n) {
            cnt[sort_digit(load_key(img, kin, pass, n_img, r), pass)] += 1;
        }
    }
    for (uint32_t d = 0; d < kSortRadix; ++d) {
        table.at(sort_table_at(d, wg, nb)) = cnt[d];
    }
}

// sort_scan: one workgroup, kSortBlock words at a time, the scan in log steps.
void scan(std::vector<uint32_t> &table)
{
    const uint32_t words = (uint32_t) table.size();
    std::vector<uint32_t> sh(kSortBlock), x(kSortBlock), v(kSortBlock);
    uint32_t carry = 0;
    for (uint32_t base = 0; base < words; base += kSortBlock) {
        for (uint32_t t = 0; t < kSortBlock; ++t) {
            v[t] = base + t < words ? table[base + t] : 0;
            sh[t] = v[t];
        }
        for (uint32_t off = 1; off < kSortBlock; off <<= 1) {
            for (uint32_t t = 0; t < kSortBlock; ++t) {
                x[t] = t >= off ? sh[t - off] : 0;
            }
            for (uint32_t t = 0; t < kSortBlock; ++t) {
                sh[t] += x[t];
            }
        }
        for (uint32_t t = 0; t < kSortBlock && base + t < words; ++t) {
            table[base + t] = carry + sh[t] - v[t];
        }
        carry += sh[kSortBlock - 1];
    }
}

// sort_scatter, workgroup wg; the waves in the order `waves`.
int scatter_wg(const std::vector<uint32_t> &img, const std::vector<uint32_t> &kin, const std::vector<uint32_t> &iin,
               uint32_t pass, uint32_t n_img, uint32_t nb, uint32_t wg, const std::vector<uint32_t> &table,
               const std::vector<uint32_t> &waves, Sorted &out, std::vector<uint8_t> &written)
{
    const uint64_t n = img.size();
    std::vector<uint32_t> wcount(kSortWaves * kSortRadix, 0), gbase(kSortRadix);
    std::vector<uint32_t> key(kSortBlock, 0), idx(kSortBlock, 0), digit(kSortBlock, 0), rank(kSortBlock, 0);
    std::vector<uint8_t> active(kSortBlock, 0);
    for (uint32_t d = 0; d < kSortRadix; ++d) {
        gbase[d] = table.at(sort_table_at(d, wg, nb));
    }
    // up to the first barrier: loads, ballots, the rank inside the wave
    std::vector<uint64_t> match(kSortBlock, 0);
    for (uint32_t wave : waves) {
        for (uint32_t lane = 0; lane < kSortWave; ++lane) {
            const uint32_t t = wave * kSortWave + lane;
            const uint64_t r = (uint64_t) wg * kSortBlock + t;
            active[t] = r < n;
            if (active[t]) {
                key[t] = load_key(img, kin, pass, n_img, r);
                idx[t] = pass == 0 ? (uint32_t) r : iin[r];
                digit[t] = sort_digit(key[t], pass);
            }
        }
        auto ballot = [&](auto pred) {
            uint64_t m = 0;
            for (uint32_t lane = 0; lane < kSortWave; ++lane) {
                if (pred(wave * kSortWave + lane)) {
                    m |= 1ull << lane;
                }
            }
            return m;
        };
        const uint64_t act = ballot([&](uint32_t t) { return active[t] != 0; });
        for (uint32_t lane = 0; lane < kSortWave; ++lane) {
            match[wave * kSortWave + lane] = act;
        }
        for (uint32_t bit = 0; bit < kSortBits; ++bit) {
            const uint64_t b = ballot([&](uint32_t t) { return active[t] && ((digit[t] >> bit) & 1u); });
            for (uint32_t lane = 0; lane < kSortWave; ++lane) {
                const uint32_t t = wave * kSortWave + lane;
                match[t] = sort_match_step(match[t], b, digit[t], bit);
            }
        }
        for (uint32_t lane = 0; lane < kSortWave; ++lane) {
            const uint32_t t = wave * kSortWave + lane;
            rank[t] = sort_lane_rank(match[t], lane);
        }
    }
    // barrier; the first lane of each digit of each wave
    for (uint32_t wave : waves) {
        for (uint32_t lane = 0; lane < kSortWave; ++lane) {
            const uint32_t t = wave * kSortWave + lane;
            if (active[t] && rank[t] == 0) {
                if (wcount[wave * kSortRadix + digit[t]] != 0) {
                    fprintf(stderr, "sort_check: two lanes of a wave claim rank 0 of digit %u\n", digit[t]);
                    return 1;
                }
                wcount[wave * kSortRadix + digit[t]] = sort_popcount(match[t]);
            }
        }
    }
    // barrier; one thread per digit
    for (uint32_t d = 0; d < kSortRadix; ++d) {
        (void) sort_wave_scan(wcount.data(), d);
    }
    // barrier; the stores
    for (uint32_t wave : waves) {
        for (uint32_t lane = 0; lane < kSortWave; ++lane) {
            const uint32_t t = wave * kSortWave + lane;
            if (!active[t]) {
                continue;
            }
            const uint32_t pos = sort_position(gbase[digit[t]], wcount[wave * kSortRadix + digit[t]], rank[t]);
            if (pos >= n || written[pos]) {
                fprintf(stderr, "sort_check: position %u of %zu is outside the list or taken twice\n", pos,
                        (size_t) n);
                return 1;
            }
            written[pos] = 1;
            out.key[pos] = key[t];
            out.idx[pos] = idx[t];
        }
    }
    return 0;
}

int kernels(const std::vector<uint32_t> &img, uint32_t n_img, int order, std::mt19937_64 &rng, Sorted &res)
{
    const uint64_t n = img.size();
    const uint32_t nb = sort_blocks(n), passes = sort_passes(n_img);
    Sorted arena[2];
    for (Sorted &a : arena) {
        a.key.assign(n, 0xdeadbeefu);
        a.idx.assign(n, 0xdeadbeefu);
    }
    std::vector<uint32_t> table((size_t) kSortRadix * nb);
    int in = 1;
    for (uint32_t p = 0; p < passes; ++p) {
        const int out = in ^ 1;
        std::fill(table.begin(), table.end(), 0xdeadbeefu);
        for (uint32_t wg : order_of(nb, order, rng)) {
            hist_wg(img, arena[in].key, p, n_img, nb, wg, table);
        }
        scan(table);
        std::vector<uint8_t> written(n, 0);
        for (uint32_t wg : order_of(nb, order, rng)) {
            if (scatter_wg(img, arena[in].key, arena[in].idx, p, n_img, nb, wg, table,
                           order_of(kSortWaves, order, rng), arena[out], written)) {
                return 1;
            }
        }
        in = out;
    }
    res = arena[in];
    return 0;
}

Sorted reference(const std::vector<uint32_t> &img, uint32_t n_img)
{
    const uint64_t n = img.size();
    std::vector<uint32_t> idx(n);
    std::iota(idx.begin(), idx.end(), 0u);
    std::stable_sort(idx.begin(), idx.end(), [&](uint32_t a, uint32_t b) {
        return std::min(img[a], n_img) < std::min(img[b], n_img);
    });
    Sorted s;
    s.idx = idx;
    s.key.resize(n);
    for (uint64_t j = 0; j < n; ++j) {
        s.key[j] = std::min(img[idx[j]], n_img);
    }
    return s;
}

int check(const std::vector<uint32_t> &img, uint32_t n_img, const char *what, std::mt19937_64 &rng)
{
    const Sorted want = reference(img, n_img);
    for (int order = 0; order < 3; ++order) {
        Sorted got;
        if (kernels(img, n_img, order, rng, got) || !(got == want)) {
            fprintf(stderr, "sort_check: %s: n_rec = %zu, n_img = %u, order %d differs\n", what, img.size(), n_img,
                    order);
            return 1;
        }
    }
    return 0;
}

std::vector<uint32_t> random_keys(uint64_t n, uint32_t n_img, std::mt19937_64 &rng)
{
    std::vector<uint32_t> img(n);
    // half of them from a few images, so that equal keys are frequent at every n_img
    const uint32_t hot[4] = {0, n_img - 1, n_img / 2, (uint32_t) (rng() % n_img)};
    for (uint64_t r = 0; r < n; ++r) {
        img[r] = rng() & 1 ? hot[rng() % 4] : (uint32_t) (rng() % n_img);
    }
    return img;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(1);
    const uint64_t B = kSortBlock;
    const uint32_t n_imgs[] = {1, 2, 255, 256, 257, 65535, 65536, 65537, (1u << 24) - 1, 1u << 24, (1u << 24) + 1};
    const uint32_t want_passes[] = {1, 1, 1, 2, 2, 2, 3, 3, 3, 4, 4};
    for (size_t k = 0; k < sizeof n_imgs / sizeof n_imgs[0]; ++k) {
        if (sort_passes(n_imgs[k]) != want_passes[k]) {
            fprintf(stderr, "sort_check: passes of n_img = %u\n", n_imgs[k]);
            return 1;
        }
    }
    if (sort_passes(0xffffffffu) != 4 || sort_key(5, 5) != 5 || sort_key(0xffffffffu, 5) != 5 || sort_key(4, 5) != 4) {
        fprintf(stderr, "sort_check: passes or key\n");
        return 1;
    }
    // n_rec on both sides of the wave, of the workgroup and of its square; every n_img (one to four passes)
    const uint64_t ns[] = {1, 2, 63, 64, 65, B - 1, B, B + 1, 2 * B + 1, 3 * B + 17};
    for (uint64_t n : ns) {
        for (uint32_t n_img : n_imgs) {
            if (check(random_keys(n, n_img, rng), n_img, "random", rng)) {
                return 1;
            }
        }
    }
    for (uint64_t n : {B * B - 1, B * B, B * B + 1}) {
        for (uint32_t n_img : {1u, 257u, (1u << 24) + 1}) {
            if (n != B * B + 1 && n_img == (1u << 24) + 1) {
                continue;                          // four passes over 2^20 records: once
            }
            if (check(random_keys(n, n_img, rng), n_img, "random, 1024 workgroups", rng)) {
                return 1;
            }
        }
    }
    // all to one image, all distinct, reversed, already sorted
    for (uint64_t n : {(uint64_t) 1, (uint64_t) 65, B, B + 1, 5 * B + 3}) {
        for (uint32_t n_img : {(uint32_t) (5 * B + 3), 65537u, (1u << 24) + 1}) {
            std::vector<uint32_t> img(n, n_img - 1);
            if (check(img, n_img, "all to one image", rng)) {
                return 1;
            }
            std::iota(img.begin(), img.end(), n_img - (uint32_t) n);
            if (check(img, n_img, "already sorted, all distinct", rng)) {
                return 1;
            }
            std::reverse(img.begin(), img.end());
            if (check(img, n_img, "reversed, all distinct", rng)) {
                return 1;
            }
            std::shuffle(img.begin(), img.end(), rng);
            if (check(img, n_img, "all distinct", rng)) {
                return 1;
            }
            std::vector<uint32_t> runs = random_keys(n, n_img, rng);
            std::sort(runs.begin(), runs.end());
            if (check(runs, n_img, "already sorted, with runs", rng)) {
                return 1;
            }
        }
    }
    // equal keys straddling wave and workgroup boundaries: runs of one key across lanes 60 .. 67 of
    // a wave pair and across records B - 3 .. B + 3, between keys that differ in every byte
    for (uint32_t n_img : {300u, 70000u, (1u << 24) + 5}) {
        std::vector<uint32_t> img(3 * B + 5);
        for (uint64_t r = 0; r < img.size(); ++r) {
            img[r] = (uint32_t) ((r * 2654435761u) % n_img);
        }
        for (uint64_t r = 60; r < 68; ++r) {
            img[r] = n_img - 2;
        }
        for (uint64_t r = B - 3; r < B + 4; ++r) {
            img[r] = r & 1 ? 1 : n_img - 2;       // two keys interleaved across the workgroup boundary
        }
        for (uint64_t r = 2 * B - 64; r < 2 * B + 64; ++r) {
            img[r] = 257 % n_img;                  // a run over the last wave of one and the first of the next
        }
        if (check(img, n_img, "equal keys across wave and workgroup boundaries", rng)) {
            return 1;
        }
    }
    // keys >= n_img, 0xFFFFFFFF among them, at the first record, the last and a workgroup boundary
    for (uint32_t n_img : {1u, 255u, 256u, 65536u, 1u << 24}) {
        for (uint64_t n : {(uint64_t) 1, B, 2 * B + 1}) {
            const uint64_t spots[] = {0, n - 1, std::min(B, n - 1), std::min(B, n - 1) - (n > 1 ? 1 : 0), n / 2};
            for (uint64_t at : spots) {
                for (uint32_t bad : {n_img, n_img + 1, 0xffffffffu}) {
                    std::vector<uint32_t> img = random_keys(n, n_img, rng);
                    img[at] = bad;
                    if (reference(img, n_img).key.back() != n_img ||
                        check(img, n_img, "an index outside the batch", rng)) {
                        return 1;
                    }
                }
            }
            std::vector<uint32_t> img = random_keys(n, n_img, rng);
            img[0] = 0xffffffffu;                  // several, equal after the clamp: they keep list order
            img[n - 1] = n_img;
            img[n / 2] = 0x80000000u;
            if (check(img, n_img, "several indices outside the batch", rng)) {
                return 1;
            }
        }
    }
    puts("sort_check: ok");
    return 0;
}
