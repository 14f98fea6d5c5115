/*
 * cio_write_dev_move.h -- the two write operations on a chunk image in device
 * memory that touch what is already there: replacing the metadata after
 * content was written, which moves the content inside the image, and
 * write_at, which cuts the content and appends at the cut.  Additions to
 * cio_write_dev.h (the writer, the image layout, the queued / no allocation /
 * capturable contract, return codes, argument checks before any device call,
 * on-device validation into dev_status, preconditions: all as stated there).
 *
 *   cio_file_write_metadata_batch_dev   cio_file_write_metadata (src/cio_file.c:
 *                                       1075-1145) with adjust_layout (:130-146)
 *   cio_file_write_at_batch_dev         cio_chunk_write_at (src/cio_chunk.c:
 *                                       184-209): the crc_reset recompute over
 *                                       the kept prefix, then cio_file_write
 *
 * These calls never grow an image: an entry that does not fit its capacity is
 * rejected (cio_write_dev_grow.h grows images ahead of a call; for a longer
 * metadata the caller passes the difference of the lengths as the need).  A rejected entry changes no byte of its image and not its
 * dev_crc_cur[i].
 */
#ifndef CIO_WRITE_DEV_MOVE_H
#define CIO_WRITE_DEV_MOVE_H

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* cio_dev_writer_create_ex: the writer also owns the scratch arena of the
 * in-place move, which cio_file_write_metadata_batch_dev needs. */
#define CIOA_WRITER_MOVE 1

/* As cio_dev_writer_create; flags: 0 or CIOA_WRITER_MOVE.
 * cio_dev_writer_create(w, n) is cio_dev_writer_create_ex(w, n, 0).  The
 * arena's size depends on the device (128 KiB per segment of the move grid),
 * never on a batch. */
int cio_dev_writer_create_ex(cio_dev_writer **w, size_t max_chunks, int flags);

/* The number of segments (workgroups) the move partitions a batch's bytes
 * into; 0 for a writer without CIOA_WRITER_MOVE (and for NULL). */
uint32_t cio_dev_writer_move_segments(const cio_dev_writer *w);

/* Replace the metadata of image i by record i of dev_meta_src (the
 * dev_meta_lens[i] = m bytes at dev_meta_src + dev_meta_offs[i]).  With `old`
 * and `content` the lengths in the image's header: bytes [24, 24 + m) take the
 * record, bytes [24 + m, 24 + m + content) the content that was at [24 + old,
 * 24 + old + content) -- an overlapping move by m - old -- and bytes 22..23
 * take m.  NO other byte changes: bytes 2..9 and 10..13 stay (adjust_layout
 * does not store the CRC in the map), and after a shrink the bytes between the
 * new and the old end of the content keep their old values, as the
 * reference's memmove leaves them.  m == 0 removes the metadata; m == old
 * rewrites it in place without a move (so a captured call replayed a second
 * time changes nothing).  With CIO_CHECKSUM dev_crc_cur[i] becomes
 * crc_update(crc_init(), image bytes [22, 24 + m + content)); without it there
 * is no CRC launch and dev_crc_cur is not touched.
 *
 * Entry i is rejected (dev_status[i] = CIO_ERROR) when the image fails the
 * checks of cio_file_write_batch_dev (bounds, cap < 24, magic, 24 + old +
 * content > cap), m > 65535, 24 + m + content > cap (the reference would grow
 * the file), or the record lies outside meta_src_bytes.
 *
 * The writer must have been created with CIOA_WRITER_MOVE; otherwise the call
 * returns CIO_ERROR from its argument checks.  dev_meta_src, dev_meta_offs and
 * dev_meta_lens must not be NULL.  The metadata source overlaps no image.
 * flags: 0 or CIO_CHECKSUM. */
int cio_file_write_metadata_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                      const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                      const void *dev_meta_src, uint64_t meta_src_bytes,
                                      const uint64_t *dev_meta_offs, const uint64_t *dev_meta_lens,
                                      int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream);

/* Cut the content of image i to at = dev_at_offs[i] bytes and append record i
 * (the dev_src_lens[i] = count bytes at dev_src + dev_src_offs[i]) there: the
 * record lands at 24 + meta_len + at and bytes 10..13 take at + count.  Bytes
 * past the new end of the content keep their old values.  With CIO_CHECKSUM
 * dev_crc_cur[i] becomes crc_update(crc_update(crc_init(), image bytes [22, 24
 * + meta_len + at)), record) and bytes 2..9 take it as
 * cio_file_write_batch_dev stores it; without it there is no CRC launch.
 * count == 0 is a no-op with CIO_OK: nothing of the image is read or written,
 * the content length included (the reference leaves its header and its
 * in-memory size disagreeing there; that is not reproduced).
 *
 * Entry i is rejected when the image fails the checks of
 * cio_file_write_batch_dev, at > content_len (the reference does not check
 * this and would checksum bytes nobody wrote), 24 + meta_len + at + count >
 * cap, at + count > 2^32 - 1, or the record lies outside src_bytes.
 *
 * Needs no CIOA_WRITER_MOVE.  The record overlaps no image.  flags: 0 or
 * CIO_CHECKSUM. */
int cio_file_write_at_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                const uint64_t *dev_at_offs,
                                const void *dev_src, uint64_t src_bytes,
                                const uint64_t *dev_src_offs, const uint64_t *dev_src_lens,
                                int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_MOVE_H */
