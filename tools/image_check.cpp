// image_check.cpp -- the image check of chunk images in HBM (image_dev.h: the
// text every device unit runs before it trusts a byte of an image), stand-alone
// on the host under ASan + UBSan: no GPU, no HIP.  `make imagecheck`.
//
// Every case is one image at a boundary of one rule: the range inside
// dev_bytes (off + cap wrapping 2^64, ending at dev_bytes, one byte short of
// it and one byte past it), the least capacity (23 / 24), each magic byte, and
// 24 + meta + content against the capacity (equal, and one more) with the
// least and the largest value of both length fields.  The image lies in a heap
// buffer that ends with it -- with its header where it is larger than kMaxAlloc
// -- so the sanitizer sees any read outside; a case the range or the capacity
// rule refuses gets a NULL base: no byte may be read there.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include "image_dev.h"

using namespace cioa;

namespace {

const uint64_t kMaxAlloc = 1 << 20;
int g_cases = 0, g_failed = 0;

// An image of capacity cap at off with the two length fields and the bytes
// m0, m1 for a magic, every other header byte 0xff; base: what to hand to the
// check, so that base + off is the image.
struct Image {
    uint8_t *buf;
    const uint8_t *base;
};

Image make_image(uint64_t off, uint64_t cap, uint8_t m0, uint8_t m1, uint32_t meta, uint32_t content)
{
    const uint64_t held = cap > kMaxAlloc ? kReadHdr : cap;
    Image im;
    im.buf = (uint8_t *) malloc(off + held);
    if (!im.buf) {
        fprintf(stderr, "image_check: out of memory\n");
        exit(2);
    }
    memset(im.buf, 0xff, off + held);
    uint8_t *p = im.buf + off;
    p[0] = m0;
    p[1] = m1;
    put_be32(p + 10, content);
    p[22] = (uint8_t) (meta >> 8);
    p[23] = (uint8_t) meta;
    im.base = im.buf;
    return im;
}

void expect(const char *what, const uint8_t *base, uint64_t dev_bytes, uint64_t off, uint64_t cap, bool want,
            uint32_t want_meta = 0, uint64_t want_content = 0)
{
    uint32_t meta = 0x55555555u;
    uint64_t content = 0x5555555555555555ull;
    const bool got = image_ok(base, dev_bytes, off, cap, meta, content);
    ++g_cases;
    if (got != want || (want && (meta != want_meta || content != want_content))) {
        fprintf(stderr, "image_check: %s: got %d (meta %u, content %llu), want %d (meta %u, content %llu)\n", what,
                (int) got, meta, (unsigned long long) content, (int) want, want_meta,
                (unsigned long long) want_content);
        ++g_failed;
    }
}

}  // namespace

int main()
{
    // the range: refused before a byte is read
    expect("off + cap wraps (large off)", nullptr, ~0ull, ~0ull - 7, 24, false);
    expect("off + cap wraps (large cap)", nullptr, ~0ull, 16, ~0ull - 7, false);
    expect("off + cap wraps to 0", nullptr, ~0ull, ~0ull - 23, 24, false);
    expect("off + cap == dev_bytes + 1", nullptr, 40 + 24 - 1, 40, 24, false);
    expect("off beyond dev_bytes", nullptr, 8, 40, 24, false);
    // the capacity: refused before a byte is read
    expect("cap 23", nullptr, 1000, 40, 23, false);
    expect("cap 0", nullptr, 1000, 40, 0, false);
    {
        Image im = make_image(40, 24, 0xc1, 0x00, 0, 0);
        expect("off + cap == dev_bytes", im.base, 40 + 24, 40, 24, true, 0, 0);
        expect("off + cap == dev_bytes - 1", im.base, 40 + 24 + 1, 40, 24, true, 0, 0);
        expect("cap 24 at off 0", im.base + 40, 24, 0, 24, true, 0, 0);
        free(im.buf);
    }
    // the magic, each byte
    const uint8_t wrong0[] = {0x00, 0xc0, 0xc2, 0x41, 0xff}, wrong1[] = {0x01, 0x80, 0xc1, 0xff};
    for (uint8_t b : wrong0) {
        Image im = make_image(7, 24, b, 0x00, 0, 0);
        expect("magic byte 0 wrong", im.base, 7 + 24, 7, 24, false);
        free(im.buf);
    }
    for (uint8_t b : wrong1) {
        Image im = make_image(7, 24, 0xc1, b, 0, 0);
        expect("magic byte 1 wrong", im.base, 7 + 24, 7, 24, false);
        free(im.buf);
    }
    {
        Image im = make_image(7, 24, 0x00, 0xc1, 0, 0);
        expect("magic bytes swapped", im.base, 7 + 24, 7, 24, false);
        free(im.buf);
    }
    // 24 + meta + content against the capacity
    const uint32_t metas[] = {0, 1, 65535}, contents[] = {0, 1, 0xffffffffu};
    for (uint32_t meta : metas) {
        for (uint32_t content : contents) {
            const uint64_t used = kReadHdr + meta + content, off = 9;
            char what[96];
            {
                Image im = make_image(off, used, 0xc1, 0x00, meta, content);
                snprintf(what, sizeof(what), "24 + %u + %u == cap", meta, content);
                expect(what, im.base, off + used, off, used, true, meta, content);
                snprintf(what, sizeof(what), "24 + %u + %u == cap - 1", meta, content);
                expect(what, im.base, off + used + 1, off, used + 1, true, meta, content);
                free(im.buf);
            }
            snprintf(what, sizeof(what), "24 + %u + %u == cap + 1", meta, content);
            if (used - 1 < kReadHdr) {             // cap 23: the capacity rule, no byte read
                expect(what, nullptr, off + used, off, used - 1, false);
            } else {
                Image im = make_image(off, used - 1, 0xc1, 0x00, meta, content);
                expect(what, im.base, off + used, off, used - 1, false);
                free(im.buf);
            }
        }
    }
    // the words the check is made of
    {
        uint8_t w[4];
        const uint32_t vals[] = {0, 1, 0x01020304u, 0x80000000u, 0xffffffffu};
        for (uint32_t v : vals) {
            put_be32(w, v);
            ++g_cases;
            if (be32(w) != v || w[0] != (uint8_t) (v >> 24) || w[3] != (uint8_t) v) {
                fprintf(stderr, "image_check: be32 / put_be32 of %u\n", v);
                ++g_failed;
            }
        }
        ++g_cases;
        if (!range_ok(0, 0, 0) || !range_ok(~0ull, 0, ~0ull) || range_ok(~0ull, 1, ~0ull) || range_ok(1, 0, 0)) {
            fprintf(stderr, "image_check: range_ok at its ends\n");
            ++g_failed;
        }
    }
    if (g_failed) {
        fprintf(stderr, "image_check: %d of %d cases failed\n", g_failed, g_cases);
        return 1;
    }
    printf("image_check: ok (%d cases)\n", g_cases);
    return 0;
}
