/*
 * cio_write_dev_ungrouped.h -- the ungrouped append: many records per chunk
 * image in one call, the records in ANY order.  Extends
 * cio_write_dev_records.h, whose call wants the records grouped by image
 * (dev_rec_img non-decreasing).  A device-side producer that routes records
 * to chunks as they arrive has them in arrival order; this call sorts them by
 * image on the device, stably, and appends them as the grouped call does.
 *
 * The contract is that of cio_file_write_records_batch_dev in every respect
 * -- the arrays, the flags, the argument checks that run before any device
 * call (unknown flags, null writer, null pointers with dev_crc_cur only under
 * CIO_CHECKSUM, n_img or n_rec greater than the writer's max_chunks; n_img ==
 * 0 or n_rec == 0 is a no-op that returns CIO_OK), no allocation, no host
 * synchronisation, capturable in a graph, a captured call replayed twice
 * appends twice, any writer of cio_dev_writer_create /
 * cio_dev_writer_create_ex serves, the rules 2 to 6 of that header, the
 * unchecked preconditions -- with three differences:
 *
 *  1. Order.  dev_rec_img may be in any order.  Let `order` be the stable
 *     sort of 0 .. n_rec - 1 by dev_rec_img: ties keep list order.  The
 *     records of an image are appended in the order in which they appear in
 *     the list.
 *  2. Statuses and the optional order.  dev_rec_status[r] is reported in the
 *     CALLER's order: entry r belongs to record r of the list as given.
 *     dev_rec_order may be NULL; if given (n_rec words), dev_rec_order[j] is
 *     the caller's index of the j-th record of the grouped list.
 *  3. Malformed batch.  Only an index dev_rec_img[r] >= n_img is malformed.
 *     It rejects the whole batch exactly as rule 1 of the grouped header does:
 *     every dev_rec_status and every dev_img_status becomes CIO_ERROR, and no
 *     byte of any image and no dev_crc_cur changes.  dev_rec_order is still a
 *     valid stable order, of the keys min(dev_rec_img[r], n_img).
 *
 * Equivalence.  The result is that of cio_file_write_records_batch_dev over
 * the stably sorted list (dev_rec_img[order[j]], dev_rec_offs[order[j]],
 * dev_rec_lens[order[j]]), its record statuses scattered back through order.
 * Hence it is also that of cio_file_write_batch_dev called once per round,
 * where round k carries the k-th record, in list order, of every image (rule
 * 7 of the grouped header, with its one difference).
 *
 * Cost: a radix sort of 1 to 4 passes (one per 8 bits of n_img) ahead of the
 * grouped chain; a caller whose list is already grouped calls
 * cio_file_write_records_batch_dev.
 *
 * Not here: a CRC per record, per-record destinations.  Growing the images for
 * a record list is cio_file_grow_records_batch_dev (cio_write_dev_grow.h),
 * queued ahead; it takes the list in any order too.  Producing dev_rec_img
 * from records that carry a tag is cio_file_route_records_batch_dev
 * (cio_route_dev.h), queued ahead of both.
 */
#ifndef CIO_WRITE_DEV_UNGROUPED_H
#define CIO_WRITE_DEV_UNGROUPED_H

#include "cio_write_dev_records.h"

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_write_records_ungrouped_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                               const uint64_t *dev_img_offs, const uint64_t *dev_img_caps,
                                               size_t n_img, const void *dev_src, uint64_t src_bytes,
                                               const uint32_t *dev_rec_img, const uint64_t *dev_rec_offs,
                                               const uint64_t *dev_rec_lens, size_t n_rec, int flags,
                                               uint32_t *dev_crc_cur, int32_t *dev_img_status,
                                               int32_t *dev_rec_status, uint32_t *dev_rec_order, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_UNGROUPED_H */
