/*
 * cio_write_dev_records.h -- the grouped append: many records per chunk image
 * in one call.  Extends cio_write_dev.h, whose calls append at most one record
 * to an image (the images of a batch are distinct); chunkio's producers call
 * cio_chunk_write once per record batch, and a chunk takes tens to thousands
 * of records before it is sealed.
 *
 * Record r is the dev_rec_lens[r] bytes at dev_src + dev_rec_offs[r] and goes
 * to image dev_rec_img[r] of the n_img images (dev_img_offs, dev_img_caps as in
 * cio_write_dev.h).
 *
 * Grouping, checked on the device: dev_rec_img must be non-decreasing, so all
 * records of one image form one run; their order inside the run is the order
 * in which they are appended.  Images without a run are allowed anywhere,
 * first and last included.
 *
 * The contract of cio_file_write_batch_dev holds: every dev_* array is a
 * DEVICE array; the call is queued on `stream`, allocates nothing, never
 * synchronises the host and can be captured in a graph, and a captured call
 * replayed twice appends twice.  flags: 0 or CIO_CHECKSUM.  The argument
 * checks run before any device call: unknown flags, null writer, null
 * pointers (dev_crc_cur only with CIO_CHECKSUM), n_img or n_rec greater than
 * the writer's max_chunks.  n_img == 0 or n_rec == 0 is a no-op that returns
 * CIO_OK.  Any writer of cio_dev_writer_create / cio_dev_writer_create_ex
 * serves.
 *
 * Everything else is decided on the device:
 *
 *  1. Malformed grouping.  If any dev_rec_img[r] < dev_rec_img[r - 1], or any
 *     dev_rec_img[r] >= n_img, the whole batch is rejected: every
 *     dev_rec_status and every dev_img_status becomes CIO_ERROR, and no byte of
 *     any image and no dev_crc_cur changes.
 *  2. Image check.  An image with a run is checked as cio_file_write_batch_dev
 *     checks it: inside dev_bytes, cap >= 24, the magic, 24 + meta_len +
 *     content_len <= cap.  If it fails, dev_img_status[i] = CIO_ERROR, all
 *     records of its run are rejected and nothing of it changes.  An image
 *     without a run is not read and gets CIO_OK.
 *  3. Room.  room_i = min(cap - 24 - meta_len - content_len,
 *     2^32 - 1 - content_len).
 *  4. Accounting.  Within a run, before_r is the exclusive running sum of the
 *     run's record lengths, saturating.  A record whose source range [off,
 *     off + len) overflows or lies outside src_bytes, or whose len exceeds
 *     2^32 - 1, contributes the saturated value (a record of length 0 has no
 *     source range).
 *  5. Acceptance.  Record r is accepted (dev_rec_status[r] = CIO_OK) iff its
 *     image passed, before_r is not saturated and before_r + len_r <= room_i;
 *     otherwise dev_rec_status[r] = CIO_ERROR.  A rejected record keeps its
 *     length in the sum.  So THE ACCEPTED RECORDS OF A RUN ARE EXACTLY THOSE
 *     BEFORE THE FIRST REJECTED ONE: a later, shorter record is never appended
 *     after a rejected one (record order is the point of a log chunk).  A
 *     record of length 0 follows the same rule and writes nothing.
 *  6. Effect.  The accepted records of image i land back to back from img +
 *     24 + meta_len + content_len.  If that is at least one byte, bytes 10..13
 *     take the new content length, and with CIO_CHECKSUM dev_crc_cur[i] =
 *     crc_update(dev_crc_cur[i], appended bytes) and bytes 2..9 take the new
 *     state as cio_file_write_batch_dev writes them.  Without CIO_CHECKSUM
 *     there is no CRC launch and bytes 2..9 and dev_crc_cur stay untouched.
 *     dev_img_status[i] = CIO_OK for every image that passed its check (or had
 *     no run), whether or not anything was appended.  No byte outside the
 *     appended range and those header fields is written.
 *  7. Equivalence.  The result is that of cio_file_write_batch_dev called once
 *     per round, round k carrying the k-th record of every image, the caller
 *     feeding an image no further after its first CIO_ERROR.  One difference:
 *     a record of length 0 to an image that fails its check is CIO_ERROR here
 *     (there it is a no-op that never looks at the image).
 *
 * Preconditions, NOT checked: the images are distinct; source and images do
 * not overlap; one call in flight per writer.
 *
 * Records in any order: cio_write_dev_ungrouped.h, which sorts the list by
 * image on the device and then does what this call does.
 *
 * Not here: a CRC per record.  Growing the images for a record list is
 * cio_file_grow_records_batch_dev (cio_write_dev_grow.h), queued ahead.
 */
#ifndef CIO_WRITE_DEV_RECORDS_H
#define CIO_WRITE_DEV_RECORDS_H

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_write_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                     const void *dev_src, uint64_t src_bytes,
                                     const uint32_t *dev_rec_img, const uint64_t *dev_rec_offs,
                                     const uint64_t *dev_rec_lens, size_t n_rec,
                                     int flags, uint32_t *dev_crc_cur, int32_t *dev_img_status,
                                     int32_t *dev_rec_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_RECORDS_H */
