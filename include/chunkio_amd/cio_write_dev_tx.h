/*
 * cio_write_dev_tx.h -- transactions on chunk images in device memory: begin,
 * roll back, commit.  Extends cio_write_dev.h.  The reference has
 * cio_chunk_tx_begin / _commit / _rollback (src/cio_chunk.c:423-502) and
 * Fluent Bit wraps every append in them: begin, write, then roll back when the
 * batch turns out not to fit, else commit.  These calls do the same for a
 * batch of images without a host round trip, so that
 *
 *   begin -> append -> cond -> rollback(cond) -> commit(cond)
 *
 * is an all-or-nothing append of many records to many images that can be
 * captured in a graph: an image one of whose records was rejected ends as it
 * was before the batch, every other image holds its whole batch and is sealed.
 *
 * Everything in cio_write_dev.h's contract holds: every dev_* argument is a
 * device array, the calls are queued on `stream`, allocate nothing (every
 * writer of cio_dev_writer_create has what they need), never synchronise the
 * host, can be captured, n == 0 is a no-op that returns CIO_OK, results are
 * CIO_OK / CIO_ERROR with cio_gpu_last_error().  The argument checks run
 * before any device call and refuse: unknown flags; CIOA_TX_RECOMPUTE without
 * CIO_CHECKSUM; a null writer; a null required pointer (dev_cond may be NULL:
 * the call acts on every entry; dev_crc_cur only with CIO_CHECKSUM); a dev_tx
 * that is not 16-byte aligned; n above the writer's max_chunks.  Validation is
 * on the device into dev_status, and a rejected entry changes no byte of its
 * image, not its dev_crc_cur[i] and not its transaction state.
 *
 * The transaction state is caller-owned, one 16-byte entry per image, like
 * dev_crc_cur; an all-zero array is the valid initial state (no transaction
 * active).  The kernels read and write an entry with one 16-byte access.  The
 * state is by index: growing or rotating the images (cio_write_dev_grow.h,
 * cio_write_dev_rotate.h) rewrites dev_img_offs / dev_img_caps in place and
 * the entries follow.
 *
 * "The image check" below is the write path's: [off, off + cap) inside
 * dev_bytes, cap >= 24, the magic, 24 + meta_len + content_len <= cap.
 *
 * Preconditions, NOT checked: the images of a batch are distinct, and one call
 * is in flight per writer.
 *
 * Two differences from the reference, both on purpose:
 *
 *  - The reference's rollback touches only data_size and crc_cur.  It leaves
 *    the map's length and CRC bytes stale until the next write
 *    (src/cio_file.c:1052-1068), and a sync straight after a rollback writes
 *    an inconsistent file.  On the device the header IS the state, so the
 *    rollback brings bytes 10..13 and, with CIO_CHECKSUM, bytes 2..9 up to
 *    date at once.
 *  - The reference restores blindly after a write_at or a metadata change
 *    inside the transaction.  Here a content shorter than at begin, or --
 *    without CIOA_TX_RECOMPUTE -- another metadata length, is CIO_ERROR.  A
 *    transaction that contains cio_file_write_at_batch_dev or an equal-length
 *    metadata rewrite MUST be rolled back with CIOA_TX_RECOMPUTE: the saved
 *    CRC state no longer describes the kept bytes, and only the recompute
 *    notices.
 *
 * Not here: nesting (begin on an active entry is a no-op, as in the
 * reference), and restoring bytes that write_at or a metadata replacement
 * overwrote below the length at begin.
 */
#ifndef CIO_WRITE_DEV_TX_H
#define CIO_WRITE_DEV_TX_H

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct { uint32_t active, content_len, crc, meta_len; } cio_dev_tx_state;
#define CIOA_TX_RECOMPUTE 256   /* rollback: recompute crc_cur from the image */
#define CIOA_TX_ZERO      512   /* rollback: zero the dropped content bytes   */

/* Begin a transaction on n images.  Per image: an entry with active != 0 gets
 * CIO_OK, its image is not read and nothing changes
 * (src/cio_chunk.c:435).  Otherwise the image check runs; on failure
 * CIO_ERROR and the state stays.  Otherwise dev_tx[i] = {1, content_len,
 * CIO_CHECKSUM ? dev_crc_cur[i] : 0, meta_len}.  No image byte is written.
 * flags: 0 or CIO_CHECKSUM; dev_crc_cur is needed only with CIO_CHECKSUM.  One
 * kernel. */
int cio_file_tx_begin_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n, int flags,
                                const uint32_t *dev_crc_cur, cio_dev_tx_state *dev_tx, int32_t *dev_status,
                                void *stream);

/* Roll n images back to where they were at begin.  Per image, in this order:
 *  1. dev_cond != NULL and dev_cond[i] == CIO_OK: skipped -- CIO_OK, the image
 *     is not read, the state stays as it is.
 *  2. active == 0: CIO_ERROR (the reference returns -1).
 *  3. The image check fails: CIO_ERROR, the state stays active.
 *  4. With cur and meta the header's lengths: cur < tx.content_len (the image
 *     was rotated, or cut by write_at, inside the transaction) is CIO_ERROR,
 *     and so is, without CIOA_TX_RECOMPUTE, meta != tx.meta_len; the state
 *     stays active.
 *  5. Otherwise bytes 10..13 take tx.content_len.  With CIO_CHECKSUM
 *     dev_crc_cur[i] becomes tx.crc -- with CIOA_TX_RECOMPUTE instead
 *     crc_update(crc_init(), image bytes [22, 24 + meta + tx.content_len)) --
 *     and bytes 2..9 take that state as cio_file_write_batch_dev stores it:
 *     raw, 8 bytes, little-endian.  With CIOA_TX_ZERO the dropped bytes [24 +
 *     meta + tx.content_len, 24 + meta + cur) become zero.  active = 0.  No
 *     other byte changes.
 * flags: 0, CIO_CHECKSUM, with it CIOA_TX_RECOMPUTE, and independently
 * CIOA_TX_ZERO.  Without CIOA_TX_ZERO / CIOA_TX_RECOMPUTE this is one kernel;
 * with either, a chain with the device planner in it (and should that planner
 * reject its batch, the images that depend on it stay where they were with
 * CIO_ERROR). */
int cio_file_tx_rollback_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                   const int32_t *dev_cond, int flags, uint32_t *dev_crc_cur,
                                   cio_dev_tx_state *dev_tx, int32_t *dev_status, void *stream);

/* Commit n images.  The call acts on the entries with dev_cond == NULL or
 * dev_cond[i] == CIO_OK; the others are skipped -- CIO_OK, the image is not
 * read, the state stays -- so that a rollback and a commit given the same
 * dev_cond act on every entry exactly once between them.  For an entry it
 * acts on: the image check runs, on failure CIO_ERROR and nothing changes;
 * with CIO_CHECKSUM the image takes what cio_file_seal_batch_dev without
 * CIOA_SEAL_RECOMPUTE writes (cio_chunk_sync's finalize_checksum); active =
 * 0, whether or not it was active (src/cio_chunk.c:459-472).  flags: 0 or
 * CIO_CHECKSUM.  One kernel. */
int cio_file_tx_commit_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                 const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                                 const int32_t *dev_cond, int flags, uint32_t *dev_crc_cur,
                                 cio_dev_tx_state *dev_tx, int32_t *dev_status, void *stream);

/* The per-image condition of an all-or-nothing append, from the statuses of
 * cio_file_write_records_batch_dev or its ungrouped form; takes no writer.
 * dev_cond[i] = CIO_ERROR iff some record r with dev_rec_img[r] == i has
 * dev_rec_status[r] != CIO_OK, or dev_img_status[i] != CIO_OK (dev_img_status
 * may be NULL); otherwise CIO_OK.  Any dev_rec_img[r] >= n_img makes every
 * dev_cond CIO_ERROR, as the grouped append rejects such a batch whole.  The
 * records may come in any order.  n_rec == 0 gives dev_cond from
 * dev_img_status alone, or all CIO_OK; n_img == 0 is a no-op.  While the call
 * runs dev_cond is its only scratch: it must not be read by anything else
 * before the call's last kernel. */
int cio_file_tx_cond_records_batch_dev(const uint32_t *dev_rec_img, const int32_t *dev_rec_status, size_t n_rec,
                                       const int32_t *dev_img_status, size_t n_img, int32_t *dev_cond, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_TX_H */
