// image_dev.h -- the image check of chunk images in HBM: the one text every
// device unit that reads an image's header runs before it trusts a byte of it
// (write_dev_gpu.hip, read_dev_gpu.hip, write_records_gpu.hip,
// grow_dev_gpu.hip, rotate_dev_gpu.hip, pool_dev_gpu.hip, pool_set_gpu.hip,
// and tx_dev.h for tx_dev_gpu.hip), with the range check and the big-endian
// words it is made of.  No HIP type, so that the same text compiles for the
// device and, stand-alone on the host, under ASan + UBSan
// (tools/image_check.cpp, `make imagecheck`).  Not installed.
//
// The layout (cio_layout.h holds it for the host) restated for the device:
//   0..1 magic C1 00 | 2..9 CRC (8-byte crc_t) | 10..13 content length BE
//   22..23 metadata length BE | 24.. metadata, then content.
#ifndef CIOA_IMAGE_DEV_H
#define CIOA_IMAGE_DEV_H

#include <stdint.h>

#ifdef __HIPCC__
#define CIOA_PLACE_FN __device__ __forceinline__
#else
#define CIOA_PLACE_FN inline
#endif

namespace cioa {

constexpr uint64_t kReadHdr = 24;           // the header's bytes: the least capacity of an image

// [off, off + len) lies inside `bytes`, and off + len does not wrap.
CIOA_PLACE_FN bool range_ok(uint64_t off, uint64_t len, uint64_t bytes)
{
    return off + len >= off && off + len <= bytes;
}

CIOA_PLACE_FN uint32_t be32(const uint8_t *p)
{
    return ((uint32_t) p[0] << 24) | ((uint32_t) p[1] << 16) | ((uint32_t) p[2] << 8) | p[3];
}

CIOA_PLACE_FN void put_be32(uint8_t *p, uint32_t v)
{
    p[0] = (uint8_t) (v >> 24);
    p[1] = (uint8_t) (v >> 16);
    p[2] = (uint8_t) (v >> 8);
    p[3] = (uint8_t) v;
}

// The image check: [off, off + cap) inside dev_bytes, room for a header, the
// magic, and metadata + content inside the capacity.  No legacy length
// inference, no CRC.  Reads no byte unless the range and the capacity hold,
// and then only bytes 0..1, 10..13 and 22..23 of the image; meta and content
// are set once the magic holds.
CIOA_PLACE_FN bool image_ok(const uint8_t *base, uint64_t dev_bytes, uint64_t off, uint64_t cap, uint32_t &meta,
                            uint64_t &content)
{
    if (!range_ok(off, cap, dev_bytes) || cap < kReadHdr) {
        return false;
    }
    const uint8_t *p = base + off;
    if (p[0] != 0xc1 || p[1] != 0x00) {
        return false;
    }
    meta = ((uint32_t) p[22] << 8) | p[23];
    content = be32(p + 10);
    return kReadHdr + meta + content <= cap;
}

}  // namespace cioa

#endif
