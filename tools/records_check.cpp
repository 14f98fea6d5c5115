// records_check.cpp -- the grouped append's bookkeeping (write_dev_records.h:
// the text the kernels rec_scan_local, rec_scan_groups and rec_place run),
// stand-alone on the host under ASan + UBSan: no GPU, no HIP.
// `make recordscheck`.
//
// The three kernels are restated workgroup by workgroup -- the segmented
// workgroup scan as the kernels do it, in log steps with rec_combine -- and run
// with the workgroups of each kernel in ascending, descending and random order
// (no workgroup may depend on another of its kernel).  Record status,
// destinations, each image's appended total and the malformed flag are
// compared with a sequential loop per image in 128-bit arithmetic.  Lengths
// only, no data.
#include <stdint.h>
#include <stdio.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "write_dev_records.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;

struct Batch {
    std::vector<uint32_t> img;                 // per record
    std::vector<uint64_t> off, len;
    std::vector<uint8_t> img_ok;               // per image: the image check's result
    std::vector<uint64_t> room, base;
    uint64_t src_bytes;
};

struct Result {
    bool malformed;
    std::vector<uint8_t> accepted;
    std::vector<uint64_t> dst, slen, total;    // total: per image, the accepted bytes
    bool operator==(const Result &o) const
    {
        return malformed == o.malformed && accepted == o.accepted && dst == o.dst && slen == o.slen &&
               total == o.total;
    }
};

// block_seg_scan_excl of write_records_gpu.hip, every "thread".
void wg_scan(std::vector<RecSeg> &sh, std::vector<RecSeg> &excl, RecSeg &total)
{
    std::vector<RecSeg> x(kRecBlock);
    for (uint32_t off = 1; off < kRecBlock; off <<= 1) {
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            x[t] = t >= off ? sh[t - off] : rec_none();
        }
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            sh[t] = rec_combine(x[t], sh[t]);
        }
    }
    for (uint32_t t = 0; t < kRecBlock; ++t) {
        excl[t] = t ? sh[t - 1] : rec_none();
    }
    total = sh[kRecBlock - 1];
}

Result kernels(const Batch &b, int order, std::mt19937_64 &rng)
{
    const uint64_t n = b.img.size(), n_img = b.img_ok.size();
    const uint32_t nb = (uint32_t) ((n + kRecBlock - 1) / kRecBlock);
    std::vector<RecSeg> local(n), agg(nb), sh(kRecBlock), excl(kRecBlock);
    std::vector<uint8_t> aggbad(nb);
    // rec_scan_local
    for (uint32_t wg : order_of(nb, order, rng)) {
        bool bad = false;
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            const uint64_t r = (uint64_t) wg * kRecBlock + t;
            sh[t] = rec_none();
            if (r < n) {
                const uint32_t img = b.img[r], prev = r ? b.img[r - 1] : 0;
                bad = bad || rec_malformed(r, img, prev, n_img);
                sh[t].flag = rec_head(r, img, prev);
                sh[t].sum = rec_value(b.off[r], b.len[r], b.src_bytes);
            }
        }
        wg_scan(sh, excl, agg[wg]);
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            const uint64_t r = (uint64_t) wg * kRecBlock + t;
            if (r < n) {
                local[r] = excl[t];
            }
        }
        aggbad[wg] = bad;
    }
    // rec_scan_groups: one workgroup, pass by pass
    Result res;
    res.malformed = false;
    RecSeg carry = rec_none();
    for (uint32_t base = 0; base < nb; base += kRecBlock) {
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            sh[t] = base + t < nb ? agg[base + t] : rec_none();
            res.malformed = res.malformed || (base + t < nb && aggbad[base + t]);
        }
        RecSeg pass;
        wg_scan(sh, excl, pass);
        for (uint32_t t = 0; t < kRecBlock && base + t < nb; ++t) {
            agg[base + t] = rec_combine(carry, excl[t]);
        }
        carry = rec_combine(carry, pass);
    }
    // rec_place
    res.accepted.assign(n, 0);
    res.dst.assign(n, 0);
    res.slen.assign(n, 0);
    res.total.assign(n_img, 0);
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kRecBlock; ++t) {
            const uint64_t r = (uint64_t) wg * kRecBlock + t;
            if (r >= n) {
                break;
            }
            if (res.malformed) {
                continue;
            }
            const uint32_t img = b.img[r];
            const uint64_t before = rec_before(rec_head(r, img, r ? b.img[r - 1] : 0), agg[wg], local[r]);
            const uint64_t v = rec_value(b.off[r], b.len[r], b.src_bytes), rm = b.room[img];
            const bool ok = b.img_ok[img];
            if (!rec_accept(ok, before, v, rm)) {
                continue;
            }
            res.accepted[r] = 1;
            res.slen[r] = v;
            res.dst[r] = b.base[img] + before;
            const uint64_t end = before + v;
            bool last = r + 1 == n || b.img[r + 1] != img;
            if (!last) {
                last = !rec_accept(ok, end, rec_value(b.off[r + 1], b.len[r + 1], b.src_bytes), rm);
            }
            if (last && end != 0) {
                if (res.total[img] != 0) {
                    fprintf(stderr, "records_check: two records claim to be the last of image %u\n", img);
                    res.malformed = !res.malformed;    // makes the comparison fail
                }
                res.total[img] = end;
            }
        }
    }
    return res;
}

Result sequential(const Batch &b)
{
    const uint64_t n = b.img.size(), n_img = b.img_ok.size();
    Result res;
    res.malformed = false;
    res.accepted.assign(n, 0);
    res.dst.assign(n, 0);
    res.slen.assign(n, 0);
    res.total.assign(n_img, 0);
    for (uint64_t r = 0; r < n; ++r) {
        if (b.img[r] >= n_img || (r && b.img[r] < b.img[r - 1])) {
            res.malformed = true;
        }
    }
    if (res.malformed) {
        return res;
    }
    uint64_t r = 0;
    for (uint32_t i = 0; i < n_img; ++i) {
        u128 sum = 0;                              // every length of the run so far, rejected ones too
        bool open = b.img_ok[i];                   // no record of the run was rejected yet
        for (; r < n && b.img[r] == i; ++r) {
            const bool src_ok = b.len[r] == 0 || (b.len[r] <= 0xffffffffull &&
                                                  (u128) b.off[r] + b.len[r] <= (u128) b.src_bytes);
            if (open && src_ok && sum + b.len[r] <= (u128) b.room[i]) {
                res.accepted[r] = 1;
                res.slen[r] = b.len[r];
                res.dst[r] = b.base[i] + (uint64_t) sum;
                res.total[i] = (uint64_t) sum + b.len[r];
            } else {
                open = false;
            }
            sum += b.len[r];
        }
    }
    return res;
}

int check(const Batch &b, const char *what, std::mt19937_64 &rng)
{
    const Result want = sequential(b);
    for (int order = 0; order < 3; ++order) {
        if (!(kernels(b, order, rng) == want)) {
            fprintf(stderr, "records_check: %s: n_rec = %zu, n_img = %zu, order %d differs\n", what, b.img.size(),
                    b.img_ok.size(), order);
            return 1;
        }
    }
    return 0;
}

// runs[i] records for image i, lengths below maxlen (one in eight empty), every
// image good with room for all of it.
Batch make_batch(const std::vector<uint64_t> &runs, uint64_t maxlen, std::mt19937_64 &rng)
{
    Batch b;
    b.src_bytes = 1ull << 40;
    uint64_t base = 1000;
    for (uint32_t i = 0; i < runs.size(); ++i) {
        u128 sum = 0;
        for (uint64_t k = 0; k < runs[i]; ++k) {
            b.img.push_back(i);
            b.len.push_back(rng() % 8 == 0 ? 0 : rng() % maxlen);
            b.off.push_back(rng() % (1ull << 30));
            sum += b.len.back();
        }
        b.img_ok.push_back(1);
        b.room.push_back((uint64_t) std::min(sum, (u128) kRecMaxContent));
        b.base.push_back(base);
        base += b.room.back() + 24 + rng() % 100;
    }
    return b;
}

// n records dealt to n_img images in random run lengths, some images empty.
std::vector<uint64_t> random_runs(uint64_t n, uint32_t n_img, std::mt19937_64 &rng)
{
    std::vector<uint64_t> runs(n_img, 0);
    for (uint64_t r = 0; r < n; ++r) {
        runs[rng() % n_img] += 1;
    }
    for (uint32_t i = 0; n_img > 1 && i < n_img; i += 3) {   // empty images, the first among them
        runs[(i + 1) % n_img] += runs[i];
        runs[i] = 0;
    }
    return runs;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(1);
    const uint64_t B = kRecBlock;
    // n_rec on both sides of the workgroup size and of its square; few and many images; failed images,
    // bad sources and rooms that cut sprinkled in
    const uint64_t ns[] = {1, 2, 63, B - 1, B, B + 1, 2 * B + 1, 3 * B + 17, B * B - 1, B * B, B * B + 1, B * B + B + 1};
    for (uint64_t n : ns) {
        for (uint32_t n_img : {1u, 5u, 700u}) {
            if (n > 4 * B && n_img == 700u) {
                continue;
            }
            Batch b = make_batch(random_runs(n, n_img, rng), n > 4 * B ? 9 : 5000, rng);
            if (check(b, "all fit", rng)) {
                return 1;
            }
            for (uint32_t i = 0; i < n_img; ++i) {
                if (rng() % 5 == 0) {
                    b.img_ok[i] = 0;
                } else if (rng() % 2) {
                    b.room[i] = b.room[i] ? rng() % (b.room[i] + 1) : 0;
                }
            }
            for (int k = 0; k < 3; ++k) {
                const uint64_t r = rng() % n;
                b.off[r] = k == 0 ? ~0ull - 3 : b.src_bytes - 1;   // overflows; leaves src_bytes
                b.len[r] = 7;
            }
            if (check(b, "cuts, failed images, bad sources", rng)) {
                return 1;
            }
        }
    }
    // runs that start exactly at a workgroup boundary; a run spanning three and more workgroups; empty
    // images first, last and in between
    {
        Batch b = make_batch({0, B, 0, 0, 3 * B, 5, B - 5, 2 * B + 1, 0}, 300, rng);
        if (check(b, "runs at workgroup boundaries", rng)) {
            return 1;
        }
        // room cutting the long run at every position around its workgroup boundaries and at its ends
        const Result full = sequential(b);
        const uint64_t first = B;                  // the 3 B run starts at record B
        for (uint64_t k = 0; k < 3 * B; ++k) {
            if (k > 20 && k + 20 < 3 * B && (k % B) > 20 && (k % B) + 20 < B) {
                continue;
            }
            const uint64_t end = full.dst[first + k] - b.base[4] + b.len[first + k];
            for (uint64_t cut : {end - (end ? 1 : 0), end}) {
                b.room[4] = cut;
                if (check(b, "cut at every position", rng)) {
                    return 1;
                }
            }
        }
    }
    // room cutting a short run at every position: one byte short of record k's end, exactly at it
    {
        Batch b = make_batch({0, 150, 40}, 300, rng);
        const Result full = sequential(b);
        for (uint64_t k = 0; k < 150; ++k) {
            const uint64_t end = full.dst[k] - b.base[1] + b.len[k];
            for (uint64_t cut : {end - (end ? 1 : 0), end}) {
                b.room[1] = cut;
                if (check(b, "cut at every position (short)", rng)) {
                    return 1;
                }
            }
        }
    }
    // a run spanning more than 1024 workgroups (the scan workgroup's second pass carries it), after a
    // short one and before one that starts in the second pass
    {
        Batch b = make_batch({7, 0, B * B + 2 * B + 3, 3 * B, 0}, 9, rng);
        if (check(b, "a run over more than 1024 workgroups", rng)) {
            return 1;
        }
        b.room[2] = b.room[2] / 2 + 1;             // cut behind the first pass or before it
        if (check(b, "a run over more than 1024 workgroups, cut", rng)) {
            return 1;
        }
        b.len[B * B + 40] = 0x100000000ull;        // a length no content can hold, in the second pass
        if (check(b, "a run over more than 1024 workgroups, saturated", rng)) {
            return 1;
        }
    }
    // lengths that saturate the sum (near 2^64, and 2^32: one more than a content can hold) among valid
    // records whose sums cross 2^32 - 1, where the 32-bit bound is the room
    for (int rep = 0; rep < 6; ++rep) {
        const uint64_t n = rep % 3 == 0 ? 50 : rep % 3 == 1 ? 3 * B + 9 : 40 * B;
        Batch b = make_batch(random_runs(n, 3, rng), 1ull << 31, rng);
        for (uint32_t i = 0; i < 3; ++i) {
            b.room[i] = rep & 1 ? kRecMaxContent : kRecMaxContent - 12345;   // the 32-bit bound binds
        }
        const uint64_t at = rng() % n;
        b.len[at] = rep < 3 ? ~0ull - rng() % 3 : kRecMaxContent + 1;
        if (check(b, "saturating sums", rng)) {
            return 1;
        }
    }
    // malformed grouping: at the first record, the last record, at a workgroup boundary
    for (uint64_t n : {(uint64_t) 1, B, 2 * B + 1, 5 * B + 3}) {
        const Batch good = make_batch(random_runs(n, 6, rng), 100, rng);
        const uint64_t spots[] = {0, n - 1, std::min(B, n - 1), std::min(B, n - 1) - (n > 1 ? 1 : 0), n / 2};
        for (uint64_t at : spots) {
            Batch b = good;
            b.img[at] = 6;                         // == n_img
            if (!sequential(b).malformed || check(b, "index == n_img", rng)) {
                fprintf(stderr, "records_check: index == n_img at %llu of %llu\n", (unsigned long long) at,
                        (unsigned long long) n);
                return 1;
            }
            b = good;
            if (at > 0 && b.img[at - 1] > 0) {
                b.img[at] = b.img[at - 1] - 1;     // a descending pair
                if (!sequential(b).malformed || check(b, "descending pair", rng)) {
                    fprintf(stderr, "records_check: descending pair at %llu of %llu\n", (unsigned long long) at,
                            (unsigned long long) n);
                    return 1;
                }
            }
        }
    }
    // the operator: associative over a sample, the identity on both sides
    for (int k = 0; k < 100000; ++k) {
        auto seg = [&]() {
            const RecSeg s = {(uint32_t) (rng() & 1), rng() % 4 == 0 ? kPlaceOver - rng() % 3 : rng() >> (rng() % 64)};
            return s;
        };
        const RecSeg a = seg(), b = seg(), c = seg();
        const RecSeg l = rec_combine(rec_combine(a, b), c), r = rec_combine(a, rec_combine(b, c));
        const RecSeg i1 = rec_combine(rec_none(), a), i2 = rec_combine(a, rec_none());
        if (l.flag != r.flag || l.sum != r.sum || i1.flag != a.flag || i1.sum != a.sum || i2.flag != a.flag ||
            i2.sum != a.sum) {
            fprintf(stderr, "records_check: the operator is not associative, or has no identity\n");
            return 1;
        }
    }
    // room
    if (rec_room(1000, 10, 100) != 866 || rec_room(24, 0, 0) != 0 ||
        rec_room((1ull << 32) + 1000, 0, kRecMaxContent - 10) != 10 || rec_room(~0ull, 65535, 0) != kRecMaxContent) {
        fprintf(stderr, "records_check: room\n");
        return 1;
    }
    puts("records_check: ok");
    return 0;
}
