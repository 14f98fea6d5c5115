// move_check.cpp -- the batched in-place move's arithmetic (write_dev_move.h:
// the text the device kernels move_save and move_shift run), stand-alone on the
// host under ASan + UBSan: no GPU, no HIP.  `make movecheck`.
//
// Random batches of images (content lengths around the 16-byte, 4 KiB and 64
// KiB boundaries and a few large ones, any alignment, both signs of the shift,
// |shift| from 1 to 65535, so pieces both shorter and longer than the shift)
// are partitioned as plan_chunks1 partitions them and moved segment by
// segment, lane by lane -- within a phase of eight tiles every lane's loads
// before any lane's stores, which is all the workgroup's barrier promises --
// in a buffer of
// EXACTLY the bytes the batch spans and an arena of exactly G segments, so the
// sanitizer sees any access outside.  Each kernel's segments run in ascending,
// in descending and in a random order: a segment that depended on another
// one's timing would differ in one of them.  Every byte of the buffer is then
// compared with a memmove per image (and the memcpy of its new metadata, which
// the device does with an append copy after the move).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <algorithm>
#include <numeric>
#include <random>
#include <vector>

#include "write_dev_move.h"

using namespace cioa;

namespace {

// A workgroup: kMoveWaves tiles to a phase, and within a phase every lane's
// loads before any lane's stores.
struct HostTile {
    struct Job {
        uint8_t *d;
        const uint8_t *s;
        uint64_t len;
    };
    std::vector<Job> phase;
    std::vector<MoveRegs> regs = std::vector<MoveRegs>(kMoveThreads);
    uint64_t tiles = 0;
    void tile(uint8_t *d, const uint8_t *s, uint64_t len)
    {
        phase.push_back({d, s, len});
        if (phase.size() == kMoveWaves) {
            end();
        }
    }
    void end()
    {
        for (size_t w = 0; w < phase.size(); ++w) {
            for (uint32_t lane = 0; lane < (uint32_t) kWave; ++lane) {
                tile_load(regs[w * kWave + lane], phase[w].d, phase[w].s, phase[w].len, lane);
            }
        }
        for (size_t w = 0; w < phase.size(); ++w) {
            for (uint32_t lane = 0; lane < (uint32_t) kWave; ++lane) {
                tile_store(regs[w * kWave + lane], phase[w].d, phase[w].len, lane);
            }
        }
        tiles += phase.size();
        phase.clear();
    }
};

uint64_t pick(std::mt19937_64 &rng, const uint64_t *pool, size_t n)
{
    return pool[rng() % n];
}

}  // namespace

int main()
{
    std::mt19937_64 rng(9);
    const uint64_t lens[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 33, 1000, 4095, 4096, 4097, 8191, 8193, 32767,
                             32768, 32769, 65534, 65535, 65536, 65537, 131077, 300000, (1 << 20) + 5};
    const uint64_t mags[] = {1, 2, 15, 16, 17, 127, 4095, 4096, 4097, 32768, 65534, 65535};
    // 5 segments: pieces of megabytes, longer than any shift; 1024 (the device's
    // grid): pieces of one or two 4 KiB steps, shorter than most; 61 in between
    const uint32_t grids[] = {5, 61, 1024};
    uint8_t *arena = (uint8_t *) malloc((size_t) 1024 * kMoveSegBytes);
    uint64_t tiles = 0;
    for (int iter = 0; iter < 36; ++iter) {
        const uint32_t n = 1 + (uint32_t) (rng() % 120), G = grids[iter % 3];
        std::vector<uint64_t> img(n), msrc(n), mlen(n), oldm(n), newm(n);
        std::vector<int64_t> mdelta(n);
        std::vector<ChunkDesc> desc(n);
        uint64_t pos = rng() % 16, S = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint64_t len = pick(rng, lens, sizeof(lens) / sizeof(lens[0]));
            if (len > 100000 && rng() % 3) {
                len = rng() % 9000;
            }
            uint64_t mag = rng() % 4 ? pick(rng, mags, sizeof(mags) / sizeof(mags[0])) : 1 + rng() % 65535;
            if (rng() % 12 == 0) {
                mag = 0;                          // m == old: nothing moves
            }
            const bool grow = rng() & 1;
            const uint64_t lo = rng() % 3 ? 0 : rng() % (65536 - mag);   // the shorter of old and new
            oldm[i] = grow ? lo : lo + mag;
            newm[i] = grow ? lo + mag : lo;
            pos += rng() % 40;                    // guard bytes between the images
            img[i] = pos;
            msrc[i] = pos + 24 + oldm[i];
            mdelta[i] = (int64_t) newm[i] - (int64_t) oldm[i];
            mlen[i] = mag ? len : 0;
            pos += 24 + std::max(oldm[i], newm[i]) + len;
            // plan_chunks1's descriptor of the source region (devplan_gpu.hip)
            const uint64_t amask = mlen[i] > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
            ChunkDesc d = {};
            d.a = msrc[i] & ~amask;
            d.h = (uint32_t) (msrc[i] & amask);
            d.vlen = d.h + mlen[i];
            d.nsteps = mlen[i] >= 4 ? (uint32_t) ((d.vlen + kStep - 1) / kStep) : 0;
            d.g = S;
            S += d.nsteps;
            desc[i] = d;
        }
        std::vector<uint8_t> before(pos), want, meta(65535);
        for (uint64_t k = 0; k < pos; ++k) {
            before[k] = (uint8_t) rng();
        }
        for (auto &b : meta) {
            b = (uint8_t) rng();
        }
        want = before;
        for (uint32_t i = 0; i < n; ++i) {
            if (mlen[i]) {
                memmove(want.data() + msrc[i] + mdelta[i], want.data() + msrc[i], mlen[i]);
            }
            memcpy(want.data() + img[i] + 24, meta.data(), newm[i]);
        }
        for (int order = 0; order < 3; ++order) {
            uint8_t *buf = (uint8_t *) malloc(pos ? pos : 1);
            memcpy(buf, before.data(), pos);
            std::vector<uint32_t> seg(G);
            HostTile ex;
            for (int kernel = 0; kernel < 2; ++kernel) {
                std::iota(seg.begin(), seg.end(), 0u);
                if (order == 1) {
                    std::reverse(seg.begin(), seg.end());
                } else if (order == 2) {
                    std::shuffle(seg.begin(), seg.end(), rng);
                }
                for (uint32_t k : seg) {
                    // the kernels' segment loop; windows of 3 records as well as of kMoveWindow
                    uint8_t *slots = arena + (uint64_t) k * kMoveSegBytes;
                    const uint32_t wsize = (iter + order) % 2 ? 3 : kMoveWindow;
                    uint64_t t = ((uint64_t) k * S) / G;
                    const uint64_t t1 = (((uint64_t) k + 1) * S) / G;
                    if (t >= t1) {
                        continue;
                    }
                    uint32_t c = record_of(desc.data(), n, t);
                    while (t < t1 && c < n) {
                        const uint32_t nw = std::min(wsize, n - c);
                        std::vector<MoveRec> win(nw);     // exactly the window: a read past it is seen
                        for (uint32_t j = 0; j < nw; ++j) {
                            win[j] = move_rec(desc.data(), msrc.data(), mlen.data(), mdelta.data(), c + j);
                        }
                        if (kernel == 0) {
                            move_window<true>(buf, slots, win.data(), c, nw, t, t1, c, ex);
                        } else {
                            move_window<false>(buf, slots, win.data(), c, nw, t, t1, c, ex);
                        }
                    }
                    ex.end();
                }
                if (kernel == 1) {
                    for (uint64_t first = 0; first < 3; ++first) {
                        move_tiny(buf, msrc.data(), mlen.data(), mdelta.data(), n, first, 3);
                    }
                }
            }
            for (uint32_t i = 0; i < n; ++i) {
                memcpy(buf + img[i] + 24, meta.data(), newm[i]);
            }
            tiles += ex.tiles;
            if (memcmp(buf, want.data(), pos) != 0) {
                for (uint64_t k = 0; k < pos; ++k) {
                    if (buf[k] != want[k]) {
                        const uint32_t i = (uint32_t) (std::upper_bound(img.begin(), img.end(), k) - img.begin()) - 1;
                        fprintf(stderr, "move_check: batch %d (n = %u, G = %u, order %d): byte %llu differs "
                                "(image %u at %llu, content %llu, shift %lld)\n", iter, n, G, order,
                                (unsigned long long) k, i, (unsigned long long) img[i],
                                (unsigned long long) mlen[i], (long long) mdelta[i]);
                        break;
                    }
                }
                return 1;
            }
            free(buf);
        }
    }
    free(arena);
    printf("move_check: ok (%llu tiles)\n", (unsigned long long) tiles);
    return 0;
}
