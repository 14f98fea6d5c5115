/*
 * cio_write_dev_pool.h -- recycling the slots of drained chunk images in
 * device memory.  Extends cio_write_dev.h and closes the loop that
 * cio_write_dev_rotate.h and cio_write_dev_grow.h leave open: the arena is a
 * bump allocator and the list of finished chunks only fills, so a captured
 * rotate -> grow -> append chain replays only while both last.  With this
 * header a drained chunk's slot goes back to a device-side pool
 * (cio_file_release_batch_dev, which also compacts the list in place), and
 * the next rotation takes its fresh slots from the pool before it touches the
 * arena (cio_file_rotate_pool_batch_dev and its records variant).  In the
 * steady state the chain
 *
 *     rotate_pool -> grow -> append -> verify -> read_packed -> release
 *
 * replays indefinitely in a bounded buffer, without a host round trip.
 *
 * Everything in cio_write_dev.h's contract holds for the three calls: they are
 * queued on `stream`, allocate nothing (every writer has what they need),
 * never synchronise the host, can be captured in a graph, one call in flight
 * per writer, n == 0 (and, in the records variant, n_rec == 0) is a no-op that
 * returns CIO_OK, results are CIO_OK / CIO_ERROR with cio_gpu_last_error().
 * The argument checks run before any device call.
 *
 * THE POOL is three device arrays the caller owns.  dev_pool_offs[] and
 * dev_pool_caps[] hold one entry per free slot; dev_pool[4] holds four words:
 *
 *   [0] the entries in the pool, used as a stack; the calls read and write it;
 *   [1] the capacity of the two arrays;
 *   [2] cls, the pool's size class: every entry has at least this capacity;
 *   [3] pal, the pool's alignment: every entry's offset is a multiple of it.
 *
 * The words live in device memory, so soundness is decided on the device.  The
 * pool is SOUND iff [0] <= [1], cls >= 24, and pal is a power of two in
 * 1 .. 4096.
 *
 * RELEASE.  dev_offs / dev_caps are either rotate's list of finished chunks,
 * with dev_img the list's third array, or grow's dev_prev_offs /
 * dev_prev_caps.  dev_img, dev_count, dev_gate and dev_live_offs may each be
 * NULL.  The host refuses: unknown flags; CIOA_RELEASE_COMPACT without
 * dev_count; CIOA_RELEASE_COMPACT together with dev_live_offs; a null writer;
 * a null required pointer; n above the writer's max_chunks.
 *
 * The rule, per entry i (all arithmetic 64-bit, saturating).  Let m = n when
 * dev_count is NULL, else min(n, dev_count[0]).
 *
 *  0. i >= m: the entry is not looked at, gets CIO_OK, and nothing changes.
 *     A captured call can so pass the list's whole capacity as n.
 *  1. dev_live_offs != NULL and dev_live_offs[i] == dev_offs[i]: an image still
 *     lives there, as after a grow that did not move it.  CIO_OK, kept.
 *  2. dev_gate != NULL and dev_gate[i] != CIO_OK: CIO_ERROR, kept, and the slot
 *     is not read.  Pass the packed read's dev_status so that only drained
 *     chunks are released.
 *  3. The write path's image check must pass (inside dev_bytes, cap >= 24, the
 *     magic, 24 + meta_len + content_len <= cap).  A slot that was already
 *     released has no magic and fails here, so a second release of the same
 *     entry is caught.
 *  4. dev_caps[i] >= cls must hold, and dev_offs[i] must be a multiple of pal.
 *  5. A failure of rule 3, of rule 4, or an unsound pool gives CIO_ERROR, and
 *     the entry is kept.
 *  6. Placement: let j be the number of entries before i that reach this
 *     point.  The entry is accepted iff dev_pool[0] + j < dev_pool[1]; the test
 *     is monotone.  A cut entry gets CIO_ERROR and is kept.  dev_total[0] is
 *     the number of entries that reach this point; it does not depend on the
 *     pool's capacity, so a caller sizes a retry from it.  dev_total[1] is the
 *     number of kept entries among the first m.
 *  7. An accepted entry is pushed and its slot is marked free:
 *     dev_pool_offs[dev_pool[0] + j] = the offset and dev_pool_caps[..] = the
 *     capacity; bytes 0..1 of the slot become zero, so that a stale reference
 *     fails every image check instead of aliasing a live chunk; with
 *     CIOA_RELEASE_ZERO the bytes [0, cap) become zero (the byte-balanced fill
 *     of cio_write_dev_grow.h), so that a fresh image that rotate later builds
 *     there has the file's zero tail; its status is CIO_OK.  dev_pool[0]
 *     advances by the number accepted; it has one writer and no atomic, and is
 *     not written when nothing is accepted.
 *  8. With CIOA_RELEASE_COMPACT the kept entries among the first m move to the
 *     front of dev_offs, dev_caps and, if given, dev_img, in their order;
 *     positions [kept, m) become (0, 0, 0xffffffff), which a later verify or
 *     read over the whole capacity rejects by cap < 24; dev_count[0] becomes
 *     kept.  Statuses stay at the entries' original positions.  Without the
 *     flag the arrays and dev_count are not written.
 *  9. If the fill's planner reports a failure, no entry is accepted, nothing
 *     is marked, and neither the pool nor the list is written.
 *
 * Preconditions, NOT checked: the entries of one batch are distinct; a
 * released slot shares no byte with a live image, with the arena's free part,
 * or with queued work that still reads it; the pool arrays hold dev_pool[1]
 * entries each.
 *
 * ROTATE FROM THE POOL.  The two calls are cio_file_rotate_batch_dev and
 * cio_file_rotate_records_batch_dev with the pool inserted after dev_arena.
 * Rules 1..4 and 6..9 of cio_write_dev_rotate.h hold unchanged; only the
 * placement (rule 5) and the capacity of rule 8 differ:
 *
 *  P1. Usable pool entries: F = dev_pool[0] when the pool is sound, new_cap <=
 *      cls, and pal is a multiple of align.  Otherwise F = 0, and the call
 *      behaves as cio_file_rotate_batch_dev.
 *  P2. Ordinal j counts the images that reach the placement.  j < F takes pool
 *      entry dev_pool[0] - 1 - j: new_off is that entry's offset, and the fresh
 *      image's dev_img_caps[i] is that entry's WHOLE capacity, so that nothing
 *      leaks when it is released again.  It is accepted iff its list index
 *      dev_out_count[0] + j is below the list's capacity.
 *  P3. j >= F takes arena slot base + (j - F) * round_up(new_cap, align) with
 *      capacity new_cap; the arena and list tests are rotate's.
 *  P4. Both parts are monotone, so the rotated images are exactly those before
 *      the first cut one.
 *  P5. dev_pool[0] becomes dev_pool[0] - min(accepted, F); top advances by the
 *      arena part alone.  Each of dev_pool[0], top and the list's count has
 *      one writer, or none.
 *  P6. dev_total[0] = (base - top) + max(0, reach - F) * slot, and 0 when no
 *      arena slot is needed; dev_total[1] = reach.
 *
 * NOT checked: the pool's entries are trusted -- they are release's output.
 * An entry that does not lie inside dev_bytes, or whose capacity is below cls,
 * makes the call write outside the buffer.
 *
 * GROW keeps taking from the arena in this header: a single-class pool cannot
 * serve its per-image capacities without a second scan.  Its leftovers can be
 * released: pass cio_file_grow_batch_dev's dev_prev_offs / dev_prev_caps as
 * dev_offs / dev_caps with dev_live_offs = dev_img_offs; exactly the old slots
 * of the moved images enter the pool.
 *
 * Not here: grow taking from the pool, and more than one size class per pool
 * -- both are cio_write_dev_pool_set.h's, whose set of K classes is K pools of
 * this header side by side, so the calls here work on one class of it
 * unchanged; coalescing adjacent free slots and checking for duplicate entries
 * within one release -- both are cio_write_dev_coalesce.h's, over a pool set;
 * compaction of live images; a fused verify + copy drain.
 */
#ifndef CIO_WRITE_DEV_POOL_H
#define CIO_WRITE_DEV_POOL_H

#include "cio_write_dev.h"

#define CIOA_RELEASE_ZERO    1
#define CIOA_RELEASE_COMPACT 2

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_release_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                               uint64_t *dev_offs, uint64_t *dev_caps, uint32_t *dev_img, size_t n,
                               uint64_t *dev_count, const int32_t *dev_gate, const uint64_t *dev_live_offs, int flags,
                               uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                               uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_rotate_pool_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                   const uint64_t *dev_need, uint64_t limit,
                                   uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                   uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                                   uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                   uint64_t *dev_out_count, int flags,
                                   uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_rotate_pool_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                           uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                           const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                           uint64_t limit,
                                           uint64_t new_cap, uint64_t align, uint64_t *dev_arena,
                                           uint64_t *dev_pool_offs, uint64_t *dev_pool_caps, uint64_t *dev_pool,
                                           uint64_t *dev_out_offs, uint64_t *dev_out_caps, uint32_t *dev_out_img,
                                           uint64_t *dev_out_count, int flags,
                                           uint32_t *dev_crc_cur, uint64_t *dev_total, int32_t *dev_status,
                                           void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_POOL_H */
