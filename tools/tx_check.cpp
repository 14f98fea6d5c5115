// tx_check.cpp -- transactions on chunk images (tx_dev.h: the text the kernels
// tx_begin, tx_rollback, tx_rollback_headers, tx_rollback_commit, tx_commit and
// the four tx_cond_* kernels run), stand-alone on the host under ASan + UBSan:
// no GPU, no HIP.  `make txcheck`.
//
// Images: the per-thread functions of tx_dev.h run over REAL image bytes,
// workgroup by workgroup, with the workgroups of each kernel in ascending,
// descending and random order (no workgroup may depend on another of its
// kernel), and the buffer, crc_cur, the state entries and the statuses are
// compared with a sequential loop written here from the public header's rules.
// The buffer has EXACTLY the batch's extent and the arrays exactly n entries,
// so the sanitizer sees a byte or an entry beyond them; an entry the rules say
// is "not read" has an offset far outside the buffer.  Between the chain's two
// steps the check plays the zero fill and the CRC launch over the regions the
// header step published, after asserting that each lies inside its image.
//
// Lengths at 2^32 - 1 cannot be allocated: those images exist as 24 header
// bytes under a claimed dev_bytes of 2^40, and the regions are compared with
// 128-bit arithmetic instead of being touched.
//
// The condition: tx_cond_records wave by wave over explicit 64-lane arrays
// (tx_cond_wave), the waves in three orders, with a count of the atomics
// issued per run.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "tx_dev.h"
#include "check_scan.h"

using namespace cioa;

namespace {

typedef unsigned __int128 u128;
const int32_t OK = 0, ERR = -1;
const int CK = 4, REC = 256, ZERO = 512;
const uint64_t kFar = 1ull << 50;             // an offset no buffer here reaches

#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            fprintf(stderr, "tx_check: ");    \
            fprintf(stderr, __VA_ARGS__);     \
            fprintf(stderr, "\n");            \
            exit(1);                          \
        }                                     \
    } while (0)

uint32_t crc_bytes(uint32_t crc, const uint8_t *p, uint64_t len)
{
    for (uint64_t k = 0; k < len; ++k) {
        crc ^= p[k];
        for (int b = 0; b < 8; ++b) {
            crc = (crc >> 1) ^ (0xEDB88320u & (0u - (crc & 1u)));
        }
    }
    return crc;
}

// Everything a call may touch.
struct World {
    std::vector<uint8_t> buf;
    uint64_t dev_bytes;
    std::vector<uint64_t> offs, caps;
    std::vector<TxState> tx;
    std::vector<uint32_t> crc_cur;
    std::vector<int32_t> cond, status;
    bool same(const World &o) const
    {
        if (buf != o.buf || crc_cur != o.crc_cur || status != o.status || tx.size() != o.tx.size()) {
            return false;
        }
        for (size_t i = 0; i < tx.size(); ++i) {
            if (memcmp(&tx[i], &o.tx[i], sizeof(TxState)) != 0) {
                return false;
            }
        }
        return true;
    }
};

void put_header(uint8_t *p, uint32_t meta, uint32_t content)
{
    memset(p, 0, 24);
    p[0] = 0xc1;
    p[2] = 0x11;                              // stale CRC bytes: a rollback must replace all eight
    p[9] = 0x99;
    p[10] = (uint8_t) (content >> 24);
    p[11] = (uint8_t) (content >> 16);
    p[12] = (uint8_t) (content >> 8);
    p[13] = (uint8_t) content;
    p[22] = (uint8_t) (meta >> 8);
    p[23] = (uint8_t) meta;
}

// Image i of kind i % kKinds; every branch of the rollback's order, and the
// lengths and capacities at their edges.
enum {
    kSkipped = 0,     // cond says CIO_OK: not read (its offset lies far outside)
    kInactive,        // active == 0
    kMagic,           // active, bad magic
    kTiny,            // active, cap < 24
    kOutside,         // active, off + cap beyond dev_bytes: not read
    kShrunk,          // cur < tx.content_len
    kMeta,            // meta != tx.meta_len: CIO_ERROR, or rolled back with RECOMPUTE
    kSame,            // tx.content_len == cur: nothing dropped
    kOne,             // tx.content_len == cur - 1
    kAll,             // tx.content_len == 0
    kCap24,           // cap == 24: no metadata, no content
    kCapMeta,         // cap == 24 + meta: no content
    kKinds
};

World make_world(uint64_t n, bool with_cond, uint64_t seed)
{
    std::mt19937_64 rng(seed);
    World w;
    w.offs.resize(n);
    w.caps.resize(n);
    w.tx.resize(n);
    w.crc_cur.resize(n);
    w.status.assign(n, 99);
    if (with_cond) {
        w.cond.resize(n);
    }
    struct Plan {
        uint32_t meta, cur;
        uint64_t cap;
    };
    std::vector<Plan> plan(n);
    uint64_t pos = 1;                          // odd offsets, one guard byte between images
    for (uint64_t i = 0; i < n; ++i) {
        const int kind = (int) (i % kKinds);
        Plan p;
        p.meta = (uint32_t) (rng() % 3 == 0 ? 0 : rng() % 34);
        p.cur = (uint32_t) (1 + rng() % 40);
        p.cap = 24 + p.meta + p.cur + rng() % 5;
        if (kind == kCap24) {
            p.meta = p.cur = 0;
            p.cap = 24;
        } else if (kind == kCapMeta) {
            p.cur = 0;
            p.cap = 24 + p.meta;
        } else if (kind == kTiny) {
            p.cap = 23;
        }
        plan[i] = p;
        w.offs[i] = pos;
        w.caps[i] = p.cap;
        pos += p.cap + 1 + (i % 2);
    }
    // the buffer ends with the last image that lies inside it
    uint64_t extent = 1;
    for (uint64_t i = 0; i < n; ++i) {
        extent = std::max(extent, w.offs[i] + w.caps[i]);
    }
    w.buf.resize(extent);
    w.dev_bytes = extent;
    for (uint64_t k = 0; k < extent; ++k) {
        w.buf[k] = (uint8_t) (1 + (k * 37 + (k >> 8) * 11) % 253);
    }
    for (uint64_t i = 0; i < n; ++i) {
        const int kind = (int) (i % kKinds);
        const Plan &p = plan[i];
        uint8_t *img = w.buf.data() + w.offs[i];
        if (kind != kTiny) {
            put_header(img, p.meta, p.cur);
        }
        TxState s = {1, p.cur, (uint32_t) (0x9e3779b9u * (i + 1)), p.meta};
        switch (kind) {
        case kSkipped:
            if (with_cond) {
                w.offs[i] = kFar + i;
            }
            s.content_len = p.cur / 2;
            break;
        case kInactive:
            s.active = 0;
            break;
        case kMagic:
            img[1] = 0x01;
            break;
        case kOutside:
            w.offs[i] = extent - 5;
            w.caps[i] = 100;
            break;
        case kShrunk:
            s.content_len = p.cur + 1;
            break;
        case kMeta:
            s.meta_len = p.meta + 1;
            s.content_len = p.cur / 2;
            break;
        case kOne:
            s.content_len = p.cur - 1;
            break;
        case kAll:
            s.content_len = 0;
            break;
        default:
            break;
        }
        w.tx[i] = s;
        w.crc_cur[i] = (uint32_t) (0x1000 + i);
        if (with_cond) {
            w.cond[i] = kind == kSkipped ? OK : (i % 5 == 0 ? -3 : ERR);      // any value but CIO_OK selects
        }
    }
    return w;
}

bool seq_image(const World &w, uint64_t i, uint32_t &meta, uint64_t &content)
{
    const uint64_t off = w.offs[i], cap = w.caps[i];
    if ((u128) off + cap > w.dev_bytes || cap < 24) {
        return false;
    }
    const uint8_t *p = w.buf.data() + off;
    if (p[0] != 0xc1 || p[1] != 0) {
        return false;
    }
    meta = (uint32_t) p[22] << 8 | p[23];
    content = (uint64_t) p[10] << 24 | (uint64_t) p[11] << 16 | (uint64_t) p[12] << 8 | p[13];
    return (u128) 24 + meta + content <= cap;
}

// The public header's rules, one image after another.
void seq_rollback(World &w, int flags)
{
    for (uint64_t i = 0; i < w.offs.size(); ++i) {
        w.status[i] = OK;
        if (!w.cond.empty() && w.cond[i] == OK) {
            continue;
        }
        TxState &s = w.tx[i];
        uint32_t meta = 0;
        uint64_t cur = 0;
        if (s.active == 0 || !seq_image(w, i, meta, cur) || cur < s.content_len ||
            (!(flags & REC) && meta != s.meta_len)) {
            w.status[i] = ERR;
            continue;
        }
        uint8_t *p = w.buf.data() + w.offs[i];
        p[10] = (uint8_t) (s.content_len >> 24);
        p[11] = (uint8_t) (s.content_len >> 16);
        p[12] = (uint8_t) (s.content_len >> 8);
        p[13] = (uint8_t) s.content_len;
        if (flags & CK) {
            const uint32_t c = (flags & REC) ? crc_bytes(0xffffffffu, p + 22, 2ull + meta + s.content_len) : s.crc;
            w.crc_cur[i] = c;
            for (int k = 0; k < 8; ++k) {
                p[2 + k] = k < 4 ? (uint8_t) (c >> (8 * k)) : 0;
            }
        }
        if (flags & ZERO) {
            memset(p + 24 + meta + s.content_len, 0, cur - s.content_len);
        }
        s.active = 0;
    }
}

void seq_begin(World &w, int flags)
{
    for (uint64_t i = 0; i < w.offs.size(); ++i) {
        w.status[i] = OK;
        if (w.tx[i].active != 0) {
            continue;
        }
        uint32_t meta = 0;
        uint64_t content = 0;
        if (!seq_image(w, i, meta, content)) {
            w.status[i] = ERR;
            continue;
        }
        w.tx[i] = TxState{1, (uint32_t) content, (flags & CK) ? w.crc_cur[i] : 0, meta};
    }
}

void seq_commit(World &w, int flags)
{
    for (uint64_t i = 0; i < w.offs.size(); ++i) {
        w.status[i] = OK;
        if (!w.cond.empty() && w.cond[i] != OK) {
            continue;
        }
        uint32_t meta = 0;
        uint64_t content = 0;
        if (!seq_image(w, i, meta, content)) {
            w.status[i] = ERR;
            continue;
        }
        if (flags & CK) {
            uint8_t *p = w.buf.data() + w.offs[i];
            const uint32_t fin = w.crc_cur[i] ^ 0xffffffffu;
            p[2] = (uint8_t) (fin >> 24);
            p[3] = (uint8_t) (fin >> 16);
            p[4] = (uint8_t) (fin >> 8);
            p[5] = (uint8_t) fin;
            p[6] = p[7] = p[8] = p[9] = 0;
        }
        w.tx[i].active = 0;
    }
}

template <typename F>
void by_workgroup(uint64_t n, int order, std::mt19937_64 &rng, F f)
{
    const uint32_t nb = (uint32_t) ((n + kTxBlock - 1) / kTxBlock);
    for (uint32_t wg : order_of(nb, order, rng)) {
        for (uint32_t t = 0; t < kTxBlock; ++t) {
            const uint64_t i = (uint64_t) wg * kTxBlock + t;
            if (i < n) {
                f(i);
            }
        }
    }
}

// The launcher's choice: one kernel, or the chain with the fill and the CRC
// played here.  bad: the last planner rejected its batch.
void kern_rollback(World &w, int flags, int order, std::mt19937_64 &rng, bool bad)
{
    const uint64_t n = w.offs.size();
    const int32_t *cond = w.cond.empty() ? nullptr : w.cond.data();
    uint32_t *crc_cur = (flags & CK) ? w.crc_cur.data() : nullptr;
    if (!(flags & (ZERO | REC))) {
        by_workgroup(n, order, rng, [&](uint64_t i) {
            w.status[i] = tx_rollback_one(w.buf.data(), w.dev_bytes, w.offs.data(), w.caps.data(), i, cond, flags,
                                          crc_cur, w.tx.data());
        });
        return;
    }
    std::vector<uint32_t> code(n), crc(n, 0xdeadbeefu);
    std::vector<uint64_t> zoff(n), zlen(n), coff(n), clen(n);
    by_workgroup(n, order, rng, [&](uint64_t i) {
        w.status[i] = tx_rollback_regions(w.buf.data(), w.dev_bytes, w.offs.data(), w.caps.data(), i, cond, flags,
                                          w.tx.data(), code.data(), zoff.data(), zlen.data(), coff.data(),
                                          clen.data());
    });
    for (uint64_t i = 0; i < n; ++i) {
        if (code[i] != kTxRoll) {
            CHECK(zlen[i] == 0 && clen[i] == 0 && zoff[i] == 0 && coff[i] == 0, "a region for entry %llu, not rolled",
                  (unsigned long long) i);
            continue;
        }
        const uint64_t off = w.offs[i], end = off + w.caps[i];
        CHECK(zlen[i] == 0 || (zoff[i] >= off + 24 && zoff[i] + zlen[i] <= end && end <= w.buf.size()),
              "dropped range of %llu outside its image", (unsigned long long) i);
        CHECK(((flags & REC) != 0) == (clen[i] != 0), "CRC region of %llu", (unsigned long long) i);
        CHECK(clen[i] == 0 || (coff[i] == off + 22 && clen[i] >= 2 && coff[i] + clen[i] <= end &&
                               (zlen[i] == 0 || coff[i] + clen[i] == zoff[i])),
              "CRC region of %llu outside its image", (unsigned long long) i);
        if (!(flags & ZERO)) {
            CHECK(zlen[i] == 0, "a dropped range without CIOA_TX_ZERO");
        }
        if (!bad) {
            memset(w.buf.data() + zoff[i], 0, zlen[i]);                          // the fill
            if (clen[i]) {
                crc[i] = crc_bytes(0xffffffffu, w.buf.data() + coff[i], clen[i]);  // the CRC launch
            }
        }
    }
    by_workgroup(n, order, rng, [&](uint64_t i) {
        if (code[i] != kTxRoll) {
            return;
        }
        const bool b = bad && ((flags & REC) || zlen[i] != 0);
        w.status[i] = tx_rollback_finish(w.buf.data(), w.offs.data(), i, flags, b, (flags & REC) ? crc.data() : nullptr,
                                         crc_cur, w.tx.data());
    });
}

const uint64_t kSizes[] = {1, 2, kKinds, kTxBlock - 1, kTxBlock, kTxBlock + 1, (uint64_t) kTxBlock * kTxBlock - 1,
                           (uint64_t) kTxBlock * kTxBlock, (uint64_t) kTxBlock * kTxBlock + 1};

uint64_t check_rollback(std::mt19937_64 &rng)
{
    uint64_t cases = 0;
    const int all_flags[] = {0, CK, CK | REC, ZERO, CK | ZERO, CK | REC | ZERO};
    for (uint64_t n : kSizes) {
        for (int flags : all_flags) {
            for (int with_cond = 0; with_cond < 2; ++with_cond) {
                const World start = make_world(n, with_cond != 0, n * 31 + flags);
                World want = start;
                seq_rollback(want, flags);
                uint64_t rolled = 0, failed = 0;
                for (uint64_t i = 0; i < n; ++i) {
                    rolled += start.tx[i].active && !want.tx[i].active;
                    failed += want.status[i] == ERR;
                }
                if (n >= kKinds) {
                    CHECK(rolled >= n / kKinds * 5 && failed >= n / kKinds * 5, "the batch misses a branch");
                }
                for (int order = 0; order < 3; ++order) {
                    World got = start;
                    kern_rollback(got, flags, order, rng, false);
                    CHECK(got.same(want), "rollback n=%llu flags=%d cond=%d order=%d", (unsigned long long) n, flags,
                          with_cond, order);
                    ++cases;
                }
                if (flags & (ZERO | REC)) {
                    // a planner that rejected its batch: whatever depended on it stays, with CIO_ERROR
                    World got = start;
                    kern_rollback(got, flags, 2, rng, true);
                    for (uint64_t i = 0; i < n; ++i) {
                        const bool was_rolled = start.tx[i].active && !want.tx[i].active;
                        if (!was_rolled) {
                            CHECK(got.status[i] == want.status[i], "bad planner: status of %llu",
                                  (unsigned long long) i);
                        } else if (got.status[i] == ERR) {
                            CHECK(got.tx[i].active == 1 && got.crc_cur[i] == start.crc_cur[i], "bad planner: state");
                        } else {
                            // only an entry that drops nothing, under CIOA_TX_ZERO alone, may still go through
                            CHECK(!(flags & REC) && got.tx[i].active == 0, "bad planner: entry %llu went through",
                                  (unsigned long long) i);
                        }
                    }
                    std::vector<uint8_t> a = got.buf, b = start.buf;
                    for (uint64_t i = 0; i < n; ++i) {          // images that went through may differ; the rest not
                        if (got.status[i] == OK && start.tx[i].active && !got.tx[i].active && start.offs[i] < kFar) {
                            memset(a.data() + start.offs[i], 0, 24);
                            memset(b.data() + start.offs[i], 0, 24);
                        }
                    }
                    CHECK(a == b, "bad planner: bytes changed");
                    ++cases;
                }
            }
        }
    }
    return cases;
}

uint64_t check_begin_commit(std::mt19937_64 &rng)
{
    uint64_t cases = 0;
    for (uint64_t n : kSizes) {
        for (int flags : {0, CK}) {
            // begin: the skipped kind's entries are active and their images far outside -- not read
            World start = make_world(n, true, n * 17 + flags);
            for (uint64_t i = 0; i < n; ++i) {
                start.tx[i].active = i % kKinds == kSkipped ? 7 : (i % 2 ? 0 : start.tx[i].active);
            }
            start.cond.clear();
            World want = start;
            seq_begin(want, flags);
            for (int order = 0; order < 3; ++order) {
                World got = start;
                by_workgroup(n, order, rng, [&](uint64_t i) {
                    got.status[i] = tx_begin_one(got.buf.data(), got.dev_bytes, got.offs.data(), got.caps.data(), i,
                                                 (flags & CK) ? got.crc_cur.data() : nullptr, got.tx.data());
                });
                CHECK(got.same(want) && got.buf == start.buf, "begin n=%llu flags=%d order=%d", (unsigned long long) n,
                      flags, order);
                ++cases;
            }
            // commit: with and without a condition; inactive entries are sealed too
            for (int with_cond = 0; with_cond < 2; ++with_cond) {
                World cstart = make_world(n, with_cond != 0, n * 13 + flags);
                for (uint64_t i = 0; i < n; ++i) {
                    if (with_cond) {
                        // the condition the other way round: the far images are the ones NOT selected
                        cstart.cond[i] = i % kKinds == kSkipped ? ERR : OK;
                    }
                }
                World cwant = cstart;
                seq_commit(cwant, flags);
                for (int order = 0; order < 3; ++order) {
                    World got = cstart;
                    by_workgroup(n, order, rng, [&](uint64_t i) {
                        got.status[i] = tx_commit_one(got.buf.data(), got.dev_bytes, got.offs.data(), got.caps.data(),
                                                      i, got.cond.empty() ? nullptr : got.cond.data(), flags,
                                                      (flags & CK) ? got.crc_cur.data() : nullptr, got.tx.data());
                    });
                    CHECK(got.same(cwant), "commit n=%llu flags=%d cond=%d order=%d", (unsigned long long) n, flags,
                          with_cond, order);
                    ++cases;
                }
            }
        }
    }
    return cases;
}

// One image of 24 real bytes under a claimed dev_bytes of 2^40.
uint64_t check_huge()
{
    uint64_t cases = 0;
    const uint32_t top = 0xffffffffu;
    const uint32_t metas[] = {0, 1, 65535};
    const uint32_t curs[] = {top, top - 1};
    for (uint32_t meta : metas) {
        for (uint32_t cur : curs) {
            for (uint32_t kept : {cur, cur - 1, 0u, top}) {
                for (uint64_t slack : {0ull, 1ull}) {
                    const uint64_t off = 3, cap = 24ull + meta + cur + slack, dev_bytes = 1ull << 40;
                    std::vector<uint8_t> buf(off + 24, 0xa5);
                    put_header(buf.data() + off, meta, cur);
                    std::vector<TxState> tx(1);
                    tx[0] = TxState{1, kept, 0x12345678u, meta};
                    uint32_t code = 9, crc_cur = 5;
                    uint64_t zoff = 9, zlen = 9, coff = 9, clen = 9;
                    const int32_t st = tx_rollback_regions(buf.data(), dev_bytes, &off, &cap, 0, nullptr, CK | REC | ZERO,
                                                           tx.data(), &code, &zoff, &zlen, &coff, &clen);
                    if (kept > cur) {
                        CHECK(st == ERR && code == kTxReject && zlen == 0 && clen == 0, "huge: shrunk");
                    } else {
                        CHECK(st == OK && code == kTxRoll, "huge: verdict");
                        CHECK(zlen == (uint64_t) cur - kept &&
                                  (u128) zoff == (zlen ? (u128) off + 24 + meta + kept : (u128) 0),
                              "huge: drop");
                        CHECK(coff == off + 22 && (u128) clen == (u128) 2 + meta + kept, "huge: CRC region");
                        CHECK((u128) zoff + zlen <= (u128) off + cap && (u128) coff + clen <= (u128) off + cap,
                              "huge: a region leaves the image");
                        const int32_t st1 = tx_rollback_one(buf.data(), dev_bytes, &off, &cap, 0, nullptr, CK, &crc_cur,
                                                            tx.data());
                        uint32_t m2 = 0;
                        uint64_t c2 = 0;
                        CHECK(st1 == OK && tx[0].active == 0 && crc_cur == 0x12345678u &&
                                  image_ok(buf.data(), dev_bytes, off, cap, m2, c2) && c2 == kept && m2 == meta,
                              "huge: rollback");
                        CHECK(tx_begin_one(buf.data(), dev_bytes, &off, &cap, 0, &crc_cur, tx.data()) == OK &&
                                  tx[0].active == 1 && tx[0].content_len == kept && tx[0].meta_len == meta,
                              "huge: begin");
                    }
                    // one byte of capacity less than the header's lengths need: the image check fails
                    const uint64_t small = 24ull + meta + cur - 1;
                    tx[0] = TxState{1, 0, 0, meta};
                    put_header(buf.data() + off, meta, cur);
                    CHECK(tx_rollback_one(buf.data(), dev_bytes, &off, &small, 0, nullptr, 0, nullptr, tx.data()) == ERR &&
                              tx[0].active == 1,
                          "huge: capacity one short");
                    // and an offset at which off + cap wraps
                    const uint64_t wrap = ~0ull - 10;
                    CHECK(tx_commit_one(buf.data(), dev_bytes, &wrap, &cap, 0, nullptr, 0, nullptr, tx.data()) == ERR,
                          "huge: wrap");
                    ++cases;
                }
            }
        }
    }
    return cases;
}

// ---------------------------------------------------------------- the condition

struct CondRun {
    std::vector<int32_t> cond;
    std::vector<uint64_t> atomics;            // per image
    uint64_t markers;
};

CondRun kern_cond(const std::vector<uint32_t> &img, const std::vector<int32_t> &st, uint32_t n_img,
                  const std::vector<int32_t> *img_status, int order, std::mt19937_64 &rng)
{
    CondRun r;
    r.cond.assign(n_img, 77);                  // exactly n_img entries
    r.atomics.assign(n_img, 0);
    r.markers = 0;
    by_workgroup(n_img, order, rng, [&](uint64_t i) {
        r.cond[i] = tx_cond_clear_one(img_status ? img_status->data() : nullptr, i);
    });
    const uint64_t n_rec = img.size();
    if (n_rec == 0) {
        return r;
    }
    const uint32_t nwaves = (uint32_t) ((n_rec + kTxBlock - 1) / kTxBlock) * (kTxBlock / kTxLanes);
    for (uint32_t wv : order_of(nwaves, order, rng)) {
        uint32_t key[kTxLanes];
        bool issue[kTxLanes], mal[kTxLanes];
        tx_cond_wave(img.data(), st.data(), (uint64_t) wv * kTxLanes, n_rec, n_img, key, issue, mal);
        for (uint32_t l = 0; l < kTxLanes; ++l) {
            if (issue[l]) {
                CHECK(key[l] < n_img, "an atomic outside dev_cond");
                r.cond[key[l]] = std::min(r.cond[key[l]], kTxError);
                ++r.atomics[key[l]];
            }
            if (mal[l]) {
                r.cond[0] = std::min(r.cond[0], kTxMalformed);
                ++r.markers;
            }
        }
    }
    if (n_img > 1) {
        // tx_cond_apply: entries 1 .., every workgroup reads entry 0 and none writes it
        const std::vector<int32_t> seen = r.cond;
        by_workgroup(n_img - 1, order, rng, [&](uint64_t j) {
            r.cond[j + 1] = tx_cond_apply_one(seen[j + 1], r.cond[0]);
        });
    }
    r.cond[0] = tx_cond_apply_one(r.cond[0], r.cond[0]);       // tx_cond_last
    return r;
}

std::vector<int32_t> seq_cond(const std::vector<uint32_t> &img, const std::vector<int32_t> &st, uint32_t n_img,
                              const std::vector<int32_t> *img_status)
{
    std::vector<int32_t> c(n_img, OK);
    for (uint32_t i = 0; i < n_img; ++i) {
        if (img_status && (*img_status)[i] != OK) {
            c[i] = ERR;
        }
    }
    for (size_t r = 0; r < img.size(); ++r) {
        if (img[r] >= n_img) {
            return std::vector<int32_t>(n_img, ERR);
        }
    }
    for (size_t r = 0; r < img.size(); ++r) {
        if (st[r] != OK) {
            c[img[r]] = ERR;
        }
    }
    return c;
}

uint64_t check_cond(std::mt19937_64 &rng)
{
    uint64_t cases = 0;
    const uint32_t n_img = 300;
    auto run_all = [&](const std::vector<uint32_t> &img, const std::vector<int32_t> &st, uint32_t ni,
                       const std::vector<int32_t> *is, const char *what) {
        const std::vector<int32_t> want = seq_cond(img, st, ni, is);
        CondRun last;
        for (int order = 0; order < 3; ++order) {
            last = kern_cond(img, st, ni, is, order, rng);
            CHECK(last.cond == want, "cond: %s, order %d", what, order);
            ++cases;
        }
        return last;
    };
    // runs of failing records to image 7 starting at every lane, behind accepted records and followed by them
    for (uint32_t run : {1u, 2u, 63u, 64u, 65u, 1000u}) {
        for (uint32_t start = 0; start < kTxLanes; ++start) {
            std::vector<uint32_t> img(start + run + 70);
            std::vector<int32_t> st(img.size(), OK);
            for (size_t r = 0; r < img.size(); ++r) {
                img[r] = (uint32_t) (r % 5);               // accepted records of other images, and of image 7's none
            }
            for (uint32_t r = start; r < start + run; ++r) {
                img[r] = 7;
                st[r] = r % 3 ? ERR : -3;                  // any status but CIO_OK fails
            }
            const CondRun got = run_all(img, st, n_img, nullptr, "run");
            const uint64_t waves = (start + run - 1) / kTxLanes - start / kTxLanes + 1;
            CHECK(got.atomics[7] == waves, "run %u at lane %u: %llu atomics for %llu waves", run, start,
                  (unsigned long long) got.atomics[7], (unsigned long long) waves);
            CHECK(std::accumulate(got.atomics.begin(), got.atomics.end(), 0ull) == waves && got.markers == 0,
                  "an atomic for an accepted record");
        }
    }
    {
        // alternating images: no two neighbours share an image, every failing record issues
        std::vector<uint32_t> img(1000);
        std::vector<int32_t> st(1000, ERR);
        for (size_t r = 0; r < img.size(); ++r) {
            img[r] = r % 2 ? 11 : 12;
        }
        const CondRun got = run_all(img, st, n_img, nullptr, "alternating");
        CHECK(got.atomics[11] == 500 && got.atomics[12] == 500, "alternating: atomics");
        // failing and accepted records of one image alternate: the accepted one breaks the run
        for (size_t r = 0; r < img.size(); ++r) {
            img[r] = 11;
            st[r] = r % 2 ? ERR : OK;
        }
        const CondRun got2 = run_all(img, st, n_img, nullptr, "every other record");
        CHECK(got2.atomics[11] == 500, "every other record: atomics");
    }
    for (uint32_t at : {0u, 63u, 64u, 127u, 255u, 256u, 999u}) {
        // one failure, at a wave's first or last lane, among accepted records of the same image
        std::vector<uint32_t> img(1000, 5);
        std::vector<int32_t> st(1000, OK);
        st[at] = ERR;
        const CondRun got = run_all(img, st, n_img, nullptr, "edge lane");
        CHECK(got.atomics[5] == 1 && got.cond[5] == ERR, "edge lane %u", at);
    }
    for (uint32_t at : {0u, 63u, 64u, 999u}) {
        for (uint32_t ni : {1u, 2u, kTxBlock, kTxBlock + 1, n_img}) {
            // a malformed index: every entry fails, whatever else the list holds
            std::vector<uint32_t> img(1000);
            std::vector<int32_t> st(1000, OK);
            for (size_t r = 0; r < img.size(); ++r) {
                img[r] = (uint32_t) (r % ni);
                st[r] = r % 7 ? OK : ERR;
            }
            img[at] = at % 2 ? 0xffffffffu : ni;
            const CondRun got = run_all(img, st, ni, nullptr, "malformed");
            CHECK(got.markers == 1, "malformed: markers");
        }
    }
    {
        // the images' own statuses folded in; no records at all; a shuffled list
        std::vector<int32_t> is(n_img, OK);
        is[0] = ERR;
        is[299] = -3;
        is[150] = ERR;
        run_all({}, {}, n_img, &is, "no records, image statuses");
        run_all({}, {}, n_img, nullptr, "no records");
        std::vector<uint32_t> img(5000);
        std::vector<int32_t> st(5000);
        for (size_t r = 0; r < img.size(); ++r) {
            img[r] = (uint32_t) (rng() % n_img);
            st[r] = rng() % 50 ? OK : ERR;
        }
        run_all(img, st, n_img, &is, "shuffled, image statuses");
        run_all(img, st, n_img, nullptr, "shuffled");
        std::sort(img.begin(), img.end());
        run_all(img, st, n_img, nullptr, "grouped");
    }
    return cases;
}

}  // namespace

int main()
{
    std::mt19937_64 rng(20);
    const uint64_t a = check_rollback(rng);
    const uint64_t b = check_begin_commit(rng);
    const uint64_t c = check_huge();
    const uint64_t d = check_cond(rng);
    printf("tx_check: ok (%llu rollback, %llu begin / commit, %llu huge, %llu condition cases)\n",
           (unsigned long long) a, (unsigned long long) b, (unsigned long long) c, (unsigned long long) d);
    return 0;
}
