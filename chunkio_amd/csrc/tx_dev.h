// tx_dev.h -- the arithmetic of transactions on chunk images in HBM
// (tx_dev_gpu.hip: tx_begin, tx_rollback, tx_rollback_headers,
// tx_rollback_commit, tx_commit, tx_cond_clear, tx_cond_records, tx_cond_apply,
// tx_cond_last): what one thread of each kernel does for its image or its
// record, given plain pointers -- the 16-byte state entry, the image check
// (image_dev.h), the order of the rollback's rules, the regions the chain
// hands to the zero fill and to the CRC launch, the header bytes of a rollback
// and of a commit, and which lane of a wave publishes a failing record.  No HIP
// type, so that the same text compiles for the device and, stand-alone on the
// host, under ASan + UBSan (tools/tx_check.cpp, `make txcheck`).  Not installed.
#ifndef CIOA_TX_DEV_H
#define CIOA_TX_DEV_H

#include <stdint.h>

#include "grow_dev.h"

namespace cioa {

constexpr uint32_t kTxBlock = 256;                     // images (records) per workgroup of every kernel: 4 waves
constexpr uint32_t kTxLanes = 64;                      // a wave
constexpr uint32_t kTxNoImage = 0xffffffffu;           // the key of a lane without a failing record
constexpr int32_t kTxOk = 0, kTxError = -1;            // CIO_OK, CIO_ERROR
constexpr int32_t kTxMalformed = -2;                   // dev_cond[0] between tx_cond_records and tx_cond_last
constexpr int kTxChecksum = 4, kTxRecompute = 256, kTxZero = 512;   // CIO_CHECKSUM, CIOA_TX_RECOMPUTE, CIOA_TX_ZERO
// tx_rollback_decide's verdicts; what tx_rollback_headers leaves per image for tx_rollback_commit.
constexpr uint32_t kTxSkip = 0, kTxReject = 1, kTxRoll = 2;

// cio_dev_tx_state, read and written with one 16-byte access.
struct alignas(16) TxState {
    uint32_t active, content_len, crc, meta_len;
};

CIOA_PLACE_FN TxState tx_load(const TxState *p)
{
    const u32x4 v = *reinterpret_cast<const u32x4 *>(p);
    TxState s;
    s.active = v[0];
    s.content_len = v[1];
    s.crc = v[2];
    s.meta_len = v[3];
    return s;
}

CIOA_PLACE_FN void tx_store(TxState *p, uint32_t active, uint32_t content_len, uint32_t crc, uint32_t meta_len)
{
    const u32x4 v = {active, content_len, crc, meta_len};
    *reinterpret_cast<u32x4 *>(p) = v;
}

// Is entry i acted on by a call whose condition selects `want_ok` entries?
// Commit acts where cond is NULL or CIO_OK, rollback where it is NULL or not
// CIO_OK: with the same array every entry is acted on by exactly one of them.
CIOA_PLACE_FN bool tx_selected(const int32_t *cond, uint64_t i, bool want_ok)
{
    return cond == nullptr || (cond[i] == kTxOk) == want_ok;
}

// ---------------------------------------------------------------- begin
// One image: an active entry is left alone and its image not read; otherwise
// the image check, and the entry takes the lengths and (with checksum) the CRC
// state.  No image byte is written.
CIOA_PLACE_FN int32_t tx_begin_one(const uint8_t *base, uint64_t dev_bytes, const uint64_t *offs, const uint64_t *caps,
                                   uint64_t i, const uint32_t *crc_cur, TxState *tx)
{
    const TxState s = tx_load(tx + i);
    if (s.active != 0) {
        return kTxOk;
    }
    uint32_t meta = 0;
    uint64_t content = 0;
    if (!image_ok(base, dev_bytes, offs[i], caps[i], meta, content)) {
        return kTxError;
    }
    tx_store(tx + i, 1, (uint32_t) content, crc_cur ? crc_cur[i] : 0, meta);
    return kTxOk;
}

// ---------------------------------------------------------------- rollback
// The order of the rules for an entry the call acts on: not active; the image
// check; the content shorter than at begin (rotated, or cut by write_at);
// without CIOA_TX_RECOMPUTE another metadata length.  meta, cur: the header's
// lengths, set with kTxRoll.
CIOA_PLACE_FN uint32_t tx_rollback_decide(const uint8_t *base, uint64_t dev_bytes, uint64_t off, uint64_t cap,
                                          const TxState &s, int flags, uint32_t &meta, uint64_t &cur)
{
    if (s.active == 0) {
        return kTxReject;
    }
    if (!image_ok(base, dev_bytes, off, cap, meta, cur)) {
        return kTxReject;
    }
    if (cur < s.content_len) {
        return kTxReject;
    }
    if (!(flags & kTxRecompute) && meta != s.meta_len) {
        return kTxReject;
    }
    return kTxRoll;
}

// The effect on the header, crc_cur and the entry: bytes 10..13 the length at
// begin; with checksum crc_cur and bytes 2..9 the state `crc`, raw, 8 bytes,
// little-endian (write_finish's store); active = 0.
CIOA_PLACE_FN void tx_rollback_apply(uint8_t *p, const TxState &s, bool checksum, uint32_t crc, uint32_t *crc_cur,
                                     TxState *tx, uint64_t i)
{
    put_be32(p + 10, s.content_len);
    if (checksum) {
        crc_cur[i] = crc;
        p[2] = (uint8_t) crc;
        p[3] = (uint8_t) (crc >> 8);
        p[4] = (uint8_t) (crc >> 16);
        p[5] = (uint8_t) (crc >> 24);
        p[6] = p[7] = p[8] = p[9] = 0;
    }
    tx_store(tx + i, 0, s.content_len, s.crc, s.meta_len);
}

// The rollback without CIOA_TX_ZERO / CIOA_TX_RECOMPUTE, whole: one thread
// decides and writes.  Returns the status.
CIOA_PLACE_FN int32_t tx_rollback_one(uint8_t *base, uint64_t dev_bytes, const uint64_t *offs, const uint64_t *caps,
                                      uint64_t i, const int32_t *cond, int flags, uint32_t *crc_cur, TxState *tx)
{
    if (!tx_selected(cond, i, false)) {
        return kTxOk;
    }
    const TxState s = tx_load(tx + i);
    const uint64_t off = offs[i];
    uint32_t meta = 0;
    uint64_t cur = 0;
    if (tx_rollback_decide(base, dev_bytes, off, caps[i], s, flags, meta, cur) != kTxRoll) {
        return kTxError;
    }
    tx_rollback_apply(base + off, s, (flags & kTxChecksum) != 0, s.crc, crc_cur, tx, i);
    return kTxOk;
}

// The chain's first step: the verdict (kTxSkip / kTxReject / kTxRoll) and the
// two regions, zero-length for every entry that is not rolled back: the
// dropped range [24 + meta + tx.content_len, 24 + meta + cur) for the zero
// fill (with CIOA_TX_ZERO) and [22, 24 + meta + tx.content_len) for the CRC
// (with CIOA_TX_RECOMPUTE).  Both lie inside the image: tx.content_len <= cur
// and 24 + meta + cur <= cap.  Returns the status so far.
CIOA_PLACE_FN int32_t tx_rollback_regions(const uint8_t *base, uint64_t dev_bytes, const uint64_t *offs,
                                          const uint64_t *caps, uint64_t i, const int32_t *cond, int flags,
                                          const TxState *tx, uint32_t *code, uint64_t *zoff, uint64_t *zlen,
                                          uint64_t *coff, uint64_t *clen)
{
    uint32_t c = kTxSkip;
    uint64_t zo = 0, zl = 0, co = 0, cl = 0;
    if (tx_selected(cond, i, false)) {
        const TxState s = tx_load(tx + i);
        const uint64_t off = offs[i];
        uint32_t meta = 0;
        uint64_t cur = 0;
        c = tx_rollback_decide(base, dev_bytes, off, caps[i], s, flags, meta, cur);
        if (c == kTxRoll) {
            if ((flags & kTxZero) && cur != s.content_len) {
                zo = off + kReadHdr + meta + s.content_len;
                zl = cur - s.content_len;
            }
            if (flags & kTxRecompute) {
                co = off + 22;
                cl = 2ull + meta + s.content_len;
            }
        }
    }
    code[i] = c;
    zoff[i] = zo;
    zlen[i] = zl;
    coff[i] = co;
    clen[i] = cl;
    return c == kTxReject ? kTxError : kTxOk;
}

// The chain's last step, for an entry with the verdict kTxRoll.  bad: the
// planner the entry depends on rejected its batch (write_finish's check) --
// nothing was filled, no CRC computed: the image stays where it was.  crc: the
// CRC launch's output, or NULL without CIOA_TX_RECOMPUTE.
CIOA_PLACE_FN int32_t tx_rollback_finish(uint8_t *base, const uint64_t *offs, uint64_t i, int flags, bool bad,
                                         const uint32_t *crc, uint32_t *crc_cur, TxState *tx)
{
    if (bad) {
        return kTxError;
    }
    const TxState s = tx_load(tx + i);
    tx_rollback_apply(base + offs[i], s, (flags & kTxChecksum) != 0, crc ? crc[i] : s.crc, crc_cur, tx, i);
    return kTxOk;
}

// ---------------------------------------------------------------- commit
// One image: the image check; with checksum the seal's bytes 2..9
// (seal_finish without recompute: htonl(crc_finalize(crc_cur)) in an 8-byte
// crc_t); active = 0 whether or not it was.
CIOA_PLACE_FN int32_t tx_commit_one(uint8_t *base, uint64_t dev_bytes, const uint64_t *offs, const uint64_t *caps,
                                    uint64_t i, const int32_t *cond, int flags, const uint32_t *crc_cur, TxState *tx)
{
    if (!tx_selected(cond, i, true)) {
        return kTxOk;
    }
    const uint64_t off = offs[i];
    uint32_t meta = 0;
    uint64_t content = 0;
    if (!image_ok(base, dev_bytes, off, caps[i], meta, content)) {
        return kTxError;
    }
    if (flags & kTxChecksum) {
        uint8_t *p = base + off;
        put_be32(p + 2, crc_cur[i] ^ 0xffffffffu);
        p[6] = p[7] = p[8] = p[9] = 0;
    }
    const TxState s = tx_load(tx + i);
    tx_store(tx + i, 0, s.content_len, s.crc, s.meta_len);
    return kTxOk;
}

// ---------------------------------------------------------------- the condition
// dev_cond[i] after the clear: the image's own status folded in.
CIOA_PLACE_FN int32_t tx_cond_clear_one(const int32_t *img_status, uint64_t i)
{
    return img_status != nullptr && img_status[i] != kTxOk ? kTxError : kTxOk;
}

// The key of record r's lane: its image where the record failed, kTxNoImage
// for a lane without a record, with an accepted record, or with an index
// outside the batch (malformed: that lane publishes the marker instead).
CIOA_PLACE_FN uint32_t tx_cond_key(const uint32_t *rec_img, const int32_t *rec_status, uint64_t r, uint64_t n_rec,
                                   uint32_t n_img, bool &malformed)
{
    malformed = false;
    if (r >= n_rec) {
        return kTxNoImage;
    }
    const uint32_t img = rec_img[r];
    if (img >= n_img) {
        malformed = true;
        return kTxNoImage;
    }
    return rec_status[r] != kTxOk ? img : kTxNoImage;
}

// Does the lane issue the atomic?  Not when the previous lane holds a failing
// record of the same image: of a run of failures to one image only the first
// lane of the wave's part of it publishes (rotate_sums_wave's head test).
CIOA_PLACE_FN bool tx_cond_issues(uint32_t lane, uint32_t key, uint32_t prev_key)
{
    return key != kTxNoImage && (lane == 0 || key != prev_key);
}

// After the records: a marker in dev_cond[0] makes every other entry
// CIO_ERROR (tx_cond_apply, entries 1 ..) and then itself (tx_cond_last).
CIOA_PLACE_FN int32_t tx_cond_apply_one(int32_t own, int32_t first)
{
    return first == kTxMalformed ? kTxError : own;
}

#ifndef __HIPCC__
// One wave of tx_cond_records over explicit arrays, as the kernel does it with
// a lane shuffle (host only: tools/tx_check.cpp): issue[l] whether lane l
// publishes its key, mal[l] whether it publishes the marker.
inline void tx_cond_wave(const uint32_t *rec_img, const int32_t *rec_status, uint64_t r0, uint64_t n_rec,
                         uint32_t n_img, uint32_t *key, bool *issue, bool *mal)
{
    for (uint32_t l = 0; l < kTxLanes; ++l) {
        key[l] = tx_cond_key(rec_img, rec_status, r0 + l, n_rec, n_img, mal[l]);
    }
    for (uint32_t l = 0; l < kTxLanes; ++l) {          // the shuffle: every lane reads before any lane writes
        issue[l] = tx_cond_issues(l, key[l], l ? key[l - 1] : 0);
    }
}
#endif

}  // namespace cioa

#endif
