// copy_check.cpp -- the batched append copy's arithmetic (write_dev_copy.h: the
// text the device kernel append_copy runs), stand-alone on the host under ASan
// + UBSan: no GPU, no HIP.  `make copycheck`.
//
// Random batches of records (every length class around the 16-byte, 1 KiB and
// 4 KiB boundaries, a few large ones, any source / destination alignment) are
// partitioned as plan_chunks1 partitions them and copied wave by wave, lane by
// lane, from a source buffer and into a destination buffer of EXACTLY the
// bytes the batch spans, so the sanitizer sees any access outside; the
// destination is then compared, guard bytes included, with a memcpy per record.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <random>
#include <vector>

#include "write_dev_copy.h"

using namespace cioa;

int main()
{
    std::mt19937_64 rng(1);
    const uint64_t pool[] = {0, 1, 2, 3, 4, 5, 15, 16, 17, 31, 32, 33, 63, 64, 65, 1000, 1023, 1024, 1025,
                             4079, 4080, 4081, 4095, 4096, 4097, 8191, 8192, 8193, 12289, 70001, 300000,
                             (1 << 20) + 5};
    const uint32_t waves[] = {7, 64, 8192};       // not a power of two, few, the device's grid
    for (int iter = 0; iter < 90; ++iter) {
        const uint32_t n = 1 + (uint32_t) (rng() % 300), W = waves[iter % 3];
        std::vector<uint64_t> soff(n), slen(n), dst(n);
        std::vector<ChunkDesc> desc(n);
        uint64_t sp = rng() % 16, dp = rng() % 16, S = 0;
        for (uint32_t i = 0; i < n; ++i) {
            uint64_t len = pool[rng() % (sizeof(pool) / sizeof(pool[0]))];
            if (len > 100000 && rng() % 4) {
                len = rng() % 5000;
            }
            sp += rng() % 40;
            dp += rng() % 40;
            soff[i] = sp;
            slen[i] = len;
            dst[i] = dp;
            sp += len;
            dp += len;
            // plan_chunks1's descriptor (devplan_gpu.hip)
            const uint64_t amask = len > (uint64_t) kStep ? (uint64_t) CIO_HEAD_ALIGN - 1 : 15ull;
            ChunkDesc d = {};
            d.a = soff[i] & ~amask;
            d.h = (uint32_t) (soff[i] & amask);
            d.vlen = d.h + len;
            d.nsteps = len >= 4 ? (uint32_t) ((d.vlen + kStep - 1) / kStep) : 0;
            d.g = S;
            S += d.nsteps;
            desc[i] = d;
        }
        uint8_t *src = (uint8_t *) malloc(sp ? sp : 1), *out = (uint8_t *) malloc(dp ? dp : 1);
        std::vector<uint8_t> want(dp, 0xA5);
        for (uint64_t k = 0; k < sp; ++k) {
            src[k] = (uint8_t) rng();
        }
        memset(out, 0xA5, dp);
        for (uint32_t i = 0; i < n; ++i) {
            memcpy(want.data() + dst[i], src + soff[i], slen[i]);
        }
        for (uint64_t first = 0; first < 5; ++first) {
            copy_tiny(out, src, soff.data(), slen.data(), dst.data(), n, first, 5);
        }
        for (uint64_t w = 0; w < W; ++w) {
            for (uint32_t lane = 0; lane < (uint32_t) kWave; ++lane) {
                copy_wave(out, src, desc.data(), soff.data(), slen.data(), dst.data(), n, S, W, w, lane);
            }
        }
        if (memcmp(out, want.data(), dp) != 0) {
            for (uint64_t k = 0; k < dp; ++k) {
                if (out[k] != want[k]) {
                    fprintf(stderr, "copy_check: batch %d (n = %u, W = %u): byte %llu differs\n", iter, n, W,
                            (unsigned long long) k);
                    break;
                }
            }
            return 1;
        }
        free(src);
        free(out);
    }
    puts("copy_check: ok");
    return 0;
}
