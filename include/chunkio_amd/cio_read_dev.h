/*
 * cio_read_dev.h -- the consumer half of chunkio's chunk API for chunk images
 * that live in device memory (HBM): read a record of every image of a batch
 * into an output buffer, and compare metadata.  Extends cio_write_dev.h (the
 * images are what its calls produce, or chunk files copied into HBM).
 *
 *   cio_file_read_batch_dev         record i to a place the caller gives
 *   cio_file_read_packed_batch_dev  the records packed one after the other, at
 *                                   places a device-side scan computes: the
 *                                   host never learns a length
 *   cio_meta_cmp_batch_dev          cio_meta_cmp (src/cio_meta.c:163-179)
 *
 * with `what` selecting the record:
 *   CIOA_READ_META     cio_meta_read / cio_meta_size (src/cio_meta.c:75-128)
 *   CIOA_READ_CONTENT  cio_chunk_get_content / cio_file_content_copy
 *                      (src/cio_file.c:510-558), cio_chunk_get_content_size
 *   CIOA_READ_IMAGE    the image trimmed to its used bytes: copied to a file,
 *                      that is the chunk file; copied into a larger slot, it
 *                      is the same chunk with room to grow (the layout holds
 *                      no capacity)
 *
 * Everything in cio_write_dev.h's contract holds: dev_* arguments are DEVICE
 * arrays; every call is queued on `stream`, allocates nothing, never
 * synchronises the host and can be captured in a graph (lengths are read from
 * the headers at run time: a replay after an append reads the longer content);
 * the argument checks (unknown what / flags, align, null writer, null
 * pointers, n > max_chunks) run before any device call; n == 0 is a no-op
 * that returns CIO_OK; CIO_OK / CIO_ERROR and cio_gpu_last_error().
 *
 * `w` is any cio_dev_writer, with or without CIOA_WRITER_MOVE: the per-batch
 * workspace.  "One call in flight per writer" covers reads too.
 *
 * Validation runs on the device.  Entry i is accepted when
 *   - dev_gate is NULL or dev_gate[i] == CIO_OK (queue cio_file_verify_batch_dev
 *     ahead on the same stream and pass its dev_status: a verified drain with
 *     no host synchronisation);
 *   - the image passes the write path's image check: off + cap inside
 *     dev_bytes, cap >= 24, magic C1 00, 24 + meta_len + content_len <= cap.
 *     No legacy length inference and no CRC: reading is cio_chunk_get_content
 *     on a chunk that is up;
 *   - its destination has room (below, per call).
 * An accepted entry gets dev_status[i] = CIO_OK and dev_out_lens[i] = the
 * record's length WITHOUT the terminator, so a call also answers cio_meta_size
 * and cio_chunk_get_content_size.  Empty metadata is CIO_OK with length 0: a
 * batch has no use for the -1 cio_meta_read returns there.  Any other entry
 * gets dev_status[i] = CIO_ERROR and dev_out_lens[i] = 0, and no byte of
 * dev_out is written for it.  The images are never written.
 *
 * dev_out == NULL is a size query: the header work (and, packed, the
 * placement) runs with the destination taken as unbounded; nothing is copied.
 *
 * Preconditions, NOT checked:
 *   - placed mode: the output slots of one batch are distinct;
 *   - dev_out overlaps no image of the batch;
 *   - out_bytes is not more than the bytes at dev_out.
 */
#ifndef CIO_READ_DEV_H
#define CIO_READ_DEV_H

#include <stddef.h>
#include <stdint.h>

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* which bytes of image i are "record i" */
#define CIOA_READ_META    0   /* [24, 24 + meta_len) */
#define CIOA_READ_CONTENT 1   /* [24 + meta_len, + content_len) */
#define CIOA_READ_IMAGE   2   /* [0, 24 + meta_len + content_len) */
/* flags: one zero byte after each record, as cio_file_content_copy's
 * buf[size] = 0 */
#define CIOA_READ_NUL     1

/* Caller-placed: record i goes to dev_out + dev_out_offs[i], a slot of
 * dev_out_caps[i] bytes.  Entry i is also rejected when [dev_out_offs[i], +
 * dev_out_caps[i]) lies outside out_bytes or when len + nul > dev_out_caps[i].
 * Bytes of the slot past len + nul keep their values.  With dev_out == NULL
 * dev_out_offs and dev_out_caps are not looked at.  flags: 0 or
 * CIOA_READ_NUL. */
int cio_file_read_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            int what, const int32_t *dev_gate,
                            void *dev_out, uint64_t out_bytes,
                            const uint64_t *dev_out_offs, const uint64_t *dev_out_caps,
                            int flags, uint64_t *dev_out_lens, int32_t *dev_status, void *stream);

/* Packed: align is a power of two in 1 .. 4096.  slot_i = len_i + nul rounded
 * up to align for an entry that passes the gate and the image check, 0 for
 * one that does not; dev_out_offs[i] = the sum of the slots before i, written
 * for EVERY i; dev_total[0] = the sum of all slots, whether or not it fits
 * out_bytes (size the retry with it).  An entry with dev_out_offs[i] + slot_i
 * > out_bytes is rejected, each entry by this rule alone; an entry cut off so
 * keeps its slot in the sums (the offsets and the total do not depend on
 * out_bytes), so the accepted entries are those before the first one that
 * does not fit.  Padding bytes are not written.  A
 * running sum that leaves 64 bits (or reaches 2^64 - 1) rejects every entry
 * from that point, whose dev_out_offs[i] is then UINT64_MAX, and sets
 * dev_total[0] = UINT64_MAX. */
int cio_file_read_packed_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                   const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                   int what, const int32_t *dev_gate,
                                   void *dev_out, uint64_t out_bytes, uint64_t align,
                                   int flags, uint64_t *dev_out_offs, uint64_t *dev_out_lens,
                                   uint64_t *dev_total, int32_t *dev_status, void *stream);

/* cio_meta_cmp for n images against n candidate records (candidate i: the
 * dev_cand_lens[i] bytes at dev_cand + dev_cand_offs[i]); needs no writer.
 * dev_result[i] = 0 when the lengths are equal and the bytes are (two empty
 * ones are equal), -1 otherwise.  A failed image check, a candidate outside
 * cand_bytes or one longer than 65535 bytes gives dev_result[i] = -1 and
 * dev_status[i] = CIO_ERROR; otherwise dev_status[i] = CIO_OK.  dev_cand may
 * be NULL when cand_bytes is 0.  n < 2^32 - 1. */
int cio_meta_cmp_batch_dev(const void *dev_base, uint64_t dev_bytes,
                           const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                           const void *dev_cand, uint64_t cand_bytes,
                           const uint64_t *dev_cand_offs, const uint64_t *dev_cand_lens,
                           int32_t *dev_result, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_READ_DEV_H */
