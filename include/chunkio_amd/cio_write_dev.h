/*
 * cio_write_dev.h -- chunkio's write lifecycle for chunk images that live in
 * device memory (HBM): initialise, append, seal.  The device-side counterpart
 * of cio_file_verify_batch_dev (cio_verify.h): what these calls produce, that
 * call accepts, and a sealed image copied byte for byte into a file is a
 * chunk file the reference loads.
 *
 *   cio_file_init_batch_dev    write_init_header (src/cio_file.c:149-162) and,
 *                              with metadata, what cio_file_write_metadata /
 *                              adjust_layout (:130-146) leave in an empty chunk
 *   cio_file_write_batch_dev   cio_file_write + update_checksum (:994-1073,
 *                              :97-113) for an image of a fixed capacity
 *                              (cio_write_dev_grow.h grows it first)
 *   cio_file_seal_batch_dev    finalize_checksum (:116-124); with
 *                              CIOA_SEAL_RECOMPUTE the crc_reset path first
 *                              (cio_file_calculate_checksum over the image)
 *
 * An image is a fixed range of a device buffer: image i occupies
 * dev_img_caps[i] bytes at dev_base + dev_img_offs[i] and none of these calls
 * grows it: an append that does not fit is rejected (the reference's resize
 * is a call of its own, queued ahead of the append: cio_write_dev_grow.h).  Its layout is the chunk file's: magic C1 00, CRC bytes 2..9,
 * content length big-endian at 10..13, metadata length big-endian at 22..23,
 * metadata from byte 24, content after it.
 *
 * Every array argument named dev_* is a DEVICE array.  Every call is queued on
 * `stream` and returns at once: it allocates nothing, never synchronises the
 * host and can be captured in a graph (cio_dev_writer_create is the one call
 * that allocates).  Lengths are read from the image headers on the device at
 * run time, so a captured cio_file_write_batch_dev replayed twice appends
 * twice.
 *
 * Return codes and cio_gpu_last_error() as in cio_crc32_gpu.h.  The argument
 * checks (null pointers, null writer, n > max_chunks, unknown flags) run
 * before any device call; n == 0 is a no-op that returns CIO_OK.
 *
 * Validation of the images and records runs on the device.  Entry i gets
 * dev_status[i] = CIO_ERROR, and NO byte of its image and not its
 * dev_crc_cur[i] changes, when
 *   - off + cap overflows or exceeds dev_bytes, or cap < 24;
 *   - (write, seal) the magic is wrong;
 *   - 24 + meta_len + content_len + count > cap;
 *   - content_len + count > 2^32 - 1 (the length field is 32 bits);
 *   - the source range [src_off, src_off + count) lies outside src_bytes;
 *   - (init) the metadata is longer than 65535 bytes.
 * Otherwise dev_status[i] = CIO_OK.  No byte outside the appended range
 * [img + 24 + meta_len + content_len, + count) and the header fields named
 * below is ever written.
 *
 * Preconditions, NOT checked:
 *   - the images of one batch are distinct (do not overlap);
 *   - source and destination do not overlap;
 *   - one call in flight per writer (the writer's arenas hold the batch's
 *     plan between its kernels); not thread-safe.
 *
 * Metadata written or replaced AFTER content moves the content inside the
 * image (cio_file_write_metadata, src/cio_file.c:1075-1145), and write_at cuts
 * it: both are in cio_write_dev_move.h, which extends this header.  Appending
 * MANY records to an image in one call (these calls take at most one per
 * image) is in cio_write_dev_records.h, which extends it too.  Growing an
 * image out of an arena ahead of an append is in cio_write_dev_grow.h; moving
 * one into a slot the host chose, and reading metadata and content back out,
 * are in cio_read_dev.h.
 */
#ifndef CIO_WRITE_DEV_H
#define CIO_WRITE_DEV_H

#include <stddef.h>
#include <stdint.h>

#include "cio_crc32_gpu.h"

#ifdef __cplusplus
extern "C" {
#endif

#ifndef CIO_CHECKSUM
#define CIO_CHECKSUM 4                 /* chunkio.h:44 */
#endif
/* cio_file_seal_batch_dev: recompute crc_cur from the image before sealing. */
#define CIOA_SEAL_RECOMPUTE 256

typedef struct cio_dev_writer cio_dev_writer;

/* A writer for batches of up to max_chunks (1 .. 2^32 - 2) images: it owns a
 * device plan (cio_crc32_devplan) and its own arenas on the current device. */
int cio_dev_writer_create(cio_dev_writer **w, size_t max_chunks);
void cio_dev_writer_destroy(cio_dev_writer *w);   /* NULL is a no-op */

/* Initialise n images.  Bytes 0..23 become write_init_header's (C1 00, ff 12 d9
 * 41, zeros; without CIO_CHECKSUM bytes 2..5 are zero too).  With metadata
 * (dev_meta_src != NULL; record i is the dev_meta_lens[i] bytes at
 * dev_meta_src + dev_meta_offs[i], 24 + len <= cap) it is copied to byte 24
 * and bytes 22..23 hold its length; bytes 2..9 stay the init bytes, as
 * adjust_layout leaves the map.  With CIO_CHECKSUM dev_crc_cur[i] becomes
 * crc_update(crc_init(), image bytes [22, 24 + meta_len)): 0xBE26ED00 without
 * metadata.  Without CIO_CHECKSUM there is no CRC launch and dev_crc_cur is
 * not written.  flags: 0 or CIO_CHECKSUM. */
int cio_file_init_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            const void *dev_meta_src, uint64_t meta_src_bytes,
                            const uint64_t *dev_meta_offs, const uint64_t *dev_meta_lens,
                            int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream);

/* Append record i (the dev_src_lens[i] bytes at dev_src + dev_src_offs[i]) to
 * image i.  A record of length 0 is a no-op with CIO_OK (nothing of the image
 * is read or written).  Otherwise the record is copied to img + 24 + meta_len
 * + content_len, both read from the header in device memory, and bytes 10..13
 * take the new content length.  With CIO_CHECKSUM dev_crc_cur[i] becomes
 * crc_update(dev_crc_cur[i], record) and bytes 2..9 take it as update_checksum
 * leaves it in the map: the raw state in an 8-byte crc_t, little-endian.
 * Without CIO_CHECKSUM there is no CRC launch and bytes 2..9 and dev_crc_cur
 * stay untouched.  flags: 0 or CIO_CHECKSUM. */
int cio_file_write_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                             const void *dev_src, uint64_t src_bytes,
                             const uint64_t *dev_src_offs, const uint64_t *dev_src_lens,
                             int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream);

/* Seal n images: bytes 2..5 become htonl(crc_finalize(dev_crc_cur[i])) and
 * bytes 6..9 zero.  With CIOA_SEAL_RECOMPUTE dev_crc_cur[i] is first
 * recomputed from the image: crc_update(crc_init(), bytes [22, 24 + meta_len +
 * content_len)).  Without CIO_CHECKSUM nothing is written (the images are
 * still validated into dev_status).  flags: 0, CIO_CHECKSUM, and with it
 * CIOA_SEAL_RECOMPUTE. */
int cio_file_seal_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                            int flags, uint32_t *dev_crc_cur, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_H */
