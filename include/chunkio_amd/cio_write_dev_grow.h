/*
 * cio_write_dev_grow.h -- growing chunk images in device memory before an
 * append.  Extends cio_write_dev.h, whose images have a fixed capacity: an
 * append that does not fit is rejected.  chunkio's cio_file_write never
 * refuses a record for room; it resizes the file (src/cio_file.c:1021-1048).
 * One call of this header, queued ahead of any of the append calls
 * (cio_file_write_batch_dev, cio_file_write_records_batch_dev,
 * cio_file_write_records_ungrouped_batch_dev), decides on the device which
 * images lack room for what is about to be appended, gives those a new, larger
 * slot out of a caller-provided arena by the reference's growth rule, moves
 * their used bytes there and rewrites dev_img_offs[i] / dev_img_caps[i] IN
 * PLACE.  After it the append accepts every record while the arena lasts, and
 * a captured grow -> append pair can be replayed indefinitely.
 *
 * Everything in cio_write_dev.h's contract holds: the calls are queued on
 * `stream`, allocate nothing (every writer of cio_dev_writer_create /
 * cio_dev_writer_create_ex has the arenas; there is no create flag), never
 * synchronise the host, can be captured in a graph, one call in flight per
 * writer, n == 0 (and, in the records variant, n_rec == 0) is a no-op that
 * returns CIO_OK, results are CIO_OK / CIO_ERROR with cio_gpu_last_error().
 * The argument checks run before any device call and refuse: unknown flags;
 * realloc_size == 0; page not a power of two; align not a power of two in
 * 1 .. 4096; exactly one of dev_prev_offs / dev_prev_caps; a null writer; a
 * null required pointer; n or n_rec above the writer's max_chunks.
 *
 * The arena is the range [dev_arena[0], dev_arena[1]) of the image buffer,
 * offsets from dev_base: [0] is its top, read and advanced by the call, [1]
 * its end.  Both words live in device memory.
 *
 * The rule, per image i with need_i = dev_need[i] content bytes about to be
 * appended (all arithmetic 64-bit, saturating):
 *
 *  1. need_i == 0: the image is not read; CIO_OK, nothing changes.
 *  2. Otherwise the write path's image check applies (inside dev_bytes, cap >=
 *     24, the magic, used = 24 + meta_len + content_len <= cap); in addition
 *     content_len + need_i <= 2^32 - 1, and the image must not share a byte
 *     with [top, end).  A failure gives CIO_ERROR and nothing changes.
 *  3. used + need_i <= cap: there is room; CIO_OK, nothing changes.
 *  4. Otherwise the new capacity is the reference's: new = cap + realloc_size;
 *     while new < used + need_i, new += realloc_size; new_cap = new rounded up
 *     to page.  A value that leaves 64 bits (or reaches 2^64 - 1) is rejected.
 *  5. Placement: base = top rounded up to align; slot_i = new_cap_i rounded up
 *     to align for an image that reaches rule 4, and 0 otherwise; new_off_i =
 *     base + the sum of the slots before i.  The image is accepted iff
 *     new_off_i + slot_i <= end and end <= dev_bytes.  A cut image keeps its
 *     slot in the sums, so the grown images are exactly those before the first
 *     that does not fit.  dev_total[0] = (base - top) + the sum of ALL slots
 *     (0 when no image reaches rule 4): it does not depend on end, so a caller
 *     sizes the retry from it.  The new top is the end of the last accepted
 *     slot, and unchanged when none is accepted.
 *  6. An accepted image has its bytes [0, used) copied from the old slot to
 *     new_off_i; with CIOA_GROW_ZERO the bytes [used, new_cap_i) of the new
 *     slot are zeroed (without it they keep their values); last of all
 *     dev_img_offs[i] = new_off_i and dev_img_caps[i] = new_cap_i.  The old
 *     slot is not touched.  A cut image gets CIO_ERROR and stays valid where
 *     it was; the append behind it applies its own rules as before.
 *  7. dev_prev_offs / dev_prev_caps, when given (both or neither), receive the
 *     values on entry for every i: the caller's free list is built from the
 *     entries where they differ from the new values.
 *  8. dev_crc_cur is not an argument: it belongs to the image index and stays
 *     valid.
 *
 * The records variant takes the record list of the grouped / ungrouped append
 * instead of dev_need: need_i is the sum of min(dev_rec_lens[r], 2^32) over
 * the records r with dev_rec_img[r] == i, in any order (the clamp keeps every
 * impossible length impossible to satisfy; with n_rec < 2^32 the sum cannot
 * wrap).  As in cio_write_dev_ungrouped.h an index >= n is the only malformed
 * input and rejects the whole call: every status is CIO_ERROR, dev_total[0]
 * is 0, and no byte, offset, capacity or top changes (dev_prev_*, if given,
 * still receive the entry values).
 *
 * What is guaranteed: after an accepted grow no record of that image is
 * rejected FOR ROOM.  A bad source range still rejects its record and the rest
 * of its run; the grow has then merely reserved too much.
 *
 * Preconditions, NOT checked: those of cio_write_dev.h (distinct images, one
 * call in flight per writer), and the arena's free part shares no byte with
 * anything the caller still needs.
 *
 * Not here: reusing freed slots -- cio_write_dev_pool.h releases the previous
 * slots (dev_prev_offs / dev_prev_caps with dev_live_offs = dev_img_offs) to a
 * device-side pool that the next rotation takes from, and
 * cio_write_dev_pool_set.h has the grow that takes its larger slots from a
 * size-classed set of such pools before the arena
 * (cio_file_grow_set_batch_dev); the two calls here keep taking from the arena
 * (and a packed CIOA_READ_IMAGE read into a fresh buffer still compacts);
 * extending in place an image that ends at top; growth for
 * cio_file_write_metadata_batch_dev (the caller passes the metadata delta as
 * the need and grows first); fusing the grow into the append kernels.
 */
#ifndef CIO_WRITE_DEV_GROW_H
#define CIO_WRITE_DEV_GROW_H

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

/* zero the new slot's bytes [used, new_cap): the tail ftruncate gives a grown file */
#define CIOA_GROW_ZERO 1

int cio_file_grow_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                            const uint64_t *dev_need, uint64_t *dev_arena,
                            uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                            uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                            uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_grow_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                    uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                    const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                    uint64_t *dev_arena,
                                    uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                    uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                    uint64_t *dev_total, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_GROW_H */
