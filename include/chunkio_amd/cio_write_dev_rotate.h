/*
 * cio_write_dev_rotate.h -- finishing full chunk images in device memory and
 * opening the next ones, before an append.  Extends cio_write_dev.h and sits
 * beside cio_write_dev_grow.h: with grow alone an image only gets larger; a
 * consumer of chunks wants bounded, sealed chunks handed over and a fresh
 * chunk with the same metadata opened in the same index, so that the producer
 * keeps appending to "image i".  One call of this header, queued ahead of a
 * grow and an append, decides on the device which images are full, seals each
 * of them where it lies, appends its (offset, capacity, index) to a
 * device-side list of finished chunks -- the input of
 * cio_file_verify_batch_dev and cio_file_read_packed_batch_dev -- builds a
 * fresh image with the same metadata in a slot of the arena, and rewrites
 * dev_img_offs[i], dev_img_caps[i] and dev_crc_cur[i] IN PLACE.  A captured
 * rotate -> grow -> append chain replays while the arena and the list last.
 *
 * Everything in cio_write_dev.h's contract holds: the calls are queued on
 * `stream`, allocate nothing (every writer of cio_dev_writer_create /
 * cio_dev_writer_create_ex has what they need; there is no create flag), never
 * synchronise the host, can be captured in a graph, one call in flight per
 * writer, n == 0 (and, in the records variant, n_rec == 0) is a no-op that
 * returns CIO_OK, results are CIO_OK / CIO_ERROR with cio_gpu_last_error().
 * The argument checks run before any device call and refuse: unknown flags;
 * new_cap < 24; align not a power of two in 1 .. 4096; a null writer; a null
 * required pointer (dev_need may be NULL: every need is 0; dev_crc_cur only
 * with CIO_CHECKSUM); n or n_rec above the writer's max_chunks.
 *
 * The arena is the range [dev_arena[0], dev_arena[1]) of the image buffer, as
 * in cio_write_dev_grow.h: [0] its top, read and advanced by the call, [1] its
 * end.  The list of finished chunks is the three arrays dev_out_offs,
 * dev_out_caps, dev_out_img: dev_out_count[0] is the number of entries in it,
 * read and advanced by the call, dev_out_count[1] its capacity.  All these
 * words live in device memory.
 *
 * The rule, per image i with need_i = dev_need[i] content bytes about to be
 * appended (all arithmetic 64-bit, saturating):
 *
 *  1. need_i == 0 and limit == 0: the image is not read; CIO_OK, nothing
 *     changes.
 *  2. Otherwise the write path's image check applies (inside dev_bytes, cap >=
 *     24, the magic, used = 24 + meta_len + content_len <= cap), and the image
 *     must share no byte with [top, end).  A failure gives CIO_ERROR and
 *     nothing changes.
 *  3. The image is FULL iff content_len > 0 and (used + need_i > cap, or limit
 *     != 0 and content_len + need_i > limit).  An empty image is never
 *     rotated: a fresh one would be no better, and this is what makes a
 *     replayed chain terminate.  An image that is not full gets CIO_OK and
 *     nothing changes.  It follows that, when every need_i <= limit, no sealed
 *     chunk holds more than limit content bytes.
 *  4. A full image needs 24 + meta_len <= new_cap; otherwise CIO_ERROR,
 *     nothing changes, and it has no slot.
 *  5. Placement, as in cio_write_dev_grow.h: base = top rounded up to align;
 *     slot_i = new_cap rounded up to align for an image that reaches this
 *     point, and 0 otherwise; new_off_i = base + the sum of the slots before
 *     i; the list index is k_i = dev_out_count[0] + the number of such images
 *     before i.  The image is accepted iff new_off_i + slot_i <= end <=
 *     dev_bytes and k_i < dev_out_count[1].  Both tests are monotone in i, so
 *     the rotated images are exactly those before the first that is cut.  A
 *     cut image gets CIO_ERROR and stays byte for byte where it was, unsealed
 *     and valid.  dev_total[0] = (base - top) + the sum of ALL slots (0 when
 *     no image reaches this point) and dev_total[1] = the number of images
 *     that reach this point: neither depends on end or on the list's
 *     capacity, so a caller sizes a retry from them.
 *  6. An accepted image is sealed first, where it lies: with CIO_CHECKSUM its
 *     bytes 2..5 become htonl(crc_finalize(dev_crc_cur[i])) and its bytes 6..9
 *     zero -- what cio_file_seal_batch_dev without CIOA_SEAL_RECOMPUTE writes;
 *     no other byte of it changes.  The list takes dev_out_offs[k_i] = the old
 *     offset, dev_out_caps[k_i] = the old capacity, dev_out_img[k_i] = i.
 *  7. The fresh image at new_off_i is what cio_file_init_batch_dev with that
 *     metadata and the same flags leaves: write_init_header's bytes 0..23 with
 *     the metadata length at 22..23, and the metadata copied from the old
 *     image's [24, 24 + meta_len) to byte 24.  With CIO_CHECKSUM dev_crc_cur[i]
 *     becomes the CRC state over the fresh image's bytes [22, 24 + meta_len).
 *     The bytes of the slot past 24 + meta_len keep their values.
 *  8. Last of all dev_img_offs[i] = new_off_i and dev_img_caps[i] = new_cap;
 *     top becomes the end of the last accepted slot and dev_out_count[0]
 *     advances by the number accepted (neither is written when nothing is
 *     accepted).  List entries at or beyond the new count are not written.
 *     Without CIO_CHECKSUM nothing is checksummed: the old image's bytes 2..9
 *     and dev_crc_cur are not written, and the fresh header is init's for
 *     that flag (bytes 2..5 zero).
 *  9. The records variant takes the record list of the grouped / ungrouped
 *     append instead of dev_need: need_i is the sum of min(dev_rec_lens[r],
 *     2^32) over the records r with dev_rec_img[r] == i, in any order.  An
 *     index >= n is the only malformed input and rejects the whole call:
 *     every status is CIO_ERROR, dev_total[0] and [1] are 0, and no byte,
 *     offset, capacity, top, count or crc_cur changes.
 *
 * Preconditions, NOT checked: those of cio_write_dev_grow.h (distinct images,
 * one call in flight per writer, the arena's free part shares no byte with
 * anything the caller still needs), and the three list arrays hold
 * dev_out_count[1] entries each.
 *
 * Not here: zeroing the fresh slot's tail, and freeing or reusing the slots of
 * the sealed chunks (the caller owns them once they are in the list) -- both
 * are cio_write_dev_pool.h: cio_file_release_batch_dev gives a drained chunk's
 * slot back to a pool, zeroed if asked, and cio_file_rotate_pool_batch_dev
 * takes the fresh slots from that pool before the arena;
 * per-image new capacities -- a caller queues cio_file_grow_batch_dev behind
 * this call, and grow extends a fresh image whose need does not fit new_cap.
 */
#ifndef CIO_WRITE_DEV_ROTATE_H
#define CIO_WRITE_DEV_ROTATE_H

#include "cio_write_dev.h"

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_rotate_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                              uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                              const uint64_t *dev_need, uint64_t limit,
                              uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                              uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                              uint64_t *dev_out_count, int flags,
                              uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_rotate_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                      uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                      const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                      uint64_t limit,
                                      uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                      uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                      uint64_t *dev_out_count, int flags,
                                      uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_ROTATE_H */
