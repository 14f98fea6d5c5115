/*
 * cio_write_dev_pool_set.h -- a size-classed set of pools of free slots in
 * device memory.  Extends cio_write_dev_pool.h and cio_write_dev_grow.h and
 * closes the gap both name first: grow taking from the pool, and more than one
 * size class per pool.  The steady-state chain
 *
 *     rotate_pool -> grow -> append -> verify -> read_packed -> release
 *
 * of cio_write_dev_pool.h is bounded only while no image ever grows: grow takes
 * every larger slot from the bump arena, the old small slot goes to the pool,
 * and the large one is never asked for again.  A producer that starts a chunk
 * small and lets it grow by realloc_size -- what chunkio's cio_file_write does
 * -- so leaks arena on every rotation cycle.  With this header a POOL SET of K
 * size classes stands in front of the arena: grow takes from the set before it
 * touches the arena (cio_file_grow_set_batch_dev and its records variant), and
 * one release files every slot into the class that fits it
 * (cio_file_release_set_batch_dev).
 *
 * Everything in cio_write_dev.h's contract holds for the three calls: they are
 * queued on `stream`, allocate nothing (every writer has what they need; no
 * array was added to the writer), never synchronise the host, add no atomic,
 * can be captured in a graph, one call in flight per writer, n == 0 (and, in
 * the records variant, n_rec == 0) is a no-op that returns CIO_OK, results are
 * CIO_OK / CIO_ERROR with cio_gpu_last_error().  The argument checks run
 * before any device call.
 *
 * THE SET has n_cls classes, 1 <= n_cls <= CIOA_POOL_SET_MAX.  It lives in
 * three device arrays the caller owns, plus the two host arguments n_cls and
 * stride:
 *
 *   dev_set[4 * n_cls]            class k's four words at [4k, 4k + 3], with
 *                                 the meaning of dev_pool[4]: entries,
 *                                 capacity, cls, pal;
 *   dev_set_offs[n_cls * stride]  class k's entries start at k * stride and
 *   dev_set_caps[n_cls * stride]  are used as a stack.
 *
 * So (dev_set_offs + k * stride, dev_set_caps + k * stride, dev_set + 4 * k) is
 * a pool of cio_write_dev_pool.h, and cio_file_release_batch_dev and
 * cio_file_rotate_pool_batch_dev work on one class unchanged.  A rotation has
 * ONE new_cap for all its images, so it needs no set variant: it names the
 * class it rotates into.
 *
 * The set is SOUND iff every class is sound by cio_write_dev_pool.h (entries
 * <= capacity, cls >= 24, pal a power of two in 1 .. 4096), every capacity
 * word is <= stride, and cls is strictly increasing with k.  The words live in
 * device memory, so this is decided on the device, per call.
 *
 * RELEASE INTO THE SET.  The arguments are cio_file_release_batch_dev's with
 * (dev_set_offs, dev_set_caps, dev_set, n_cls, stride) in place of the pool
 * and dev_total of 2 + n_cls words.  The host refuses what that call refuses,
 * n_cls outside 1 .. CIOA_POOL_SET_MAX, stride == 0, and a null set pointer.
 * Rules 0..3, 8 and 9 of cio_write_dev_pool.h hold unchanged; these replace
 * the others:
 *
 *  4'. The entry's class is the largest k with cls_k <= dev_caps[i] and
 *      dev_offs[i] a multiple of pal_k.  An entry with no such class, or an
 *      unsound set, gets CIO_ERROR and is kept.
 *  6'. Let j be the number of entries before i that reach the placement with
 *      the same class.  The entry is accepted iff set[4k] + j < set[4k + 1];
 *      the test is monotone per class.  A cut entry gets CIO_ERROR and is
 *      kept; it is NOT offered to a lower class.  dev_total[0] = the entries
 *      that reach the placement; dev_total[1] = the entries kept among the
 *      first m; dev_total[2 + k] = the entries that reach the placement in
 *      class k, whatever its room: a caller sizes each class from it.
 *  7'. An accepted entry is pushed at index k * stride + set[4k] + j of the two
 *      arrays, and its slot is marked free as in rule 7: bytes 0..1 become
 *      zero, with CIOA_RELEASE_ZERO the whole slot.  set[4k] advances by the
 *      number accepted in class k; each such word has one writer, or none.
 *  8.  CIOA_RELEASE_COMPACT keeps its meaning.  (The accepted entries are no
 *      longer a prefix of those that reach the placement, so a kept entry's
 *      position comes from a second scan, over the kept flags.)
 *
 * With n_cls == 1 the call is cio_file_release_batch_dev output for output.
 *
 * GROW OUT OF THE SET.  The arguments are those of cio_file_grow_batch_dev and
 * cio_file_grow_records_batch_dev with the set inserted after dev_arena and
 * dev_total of 2 + n_cls words; the host refuses what those calls refuse and
 * what the release refuses of the set.  Rules 1..4, 7 and 8 of
 * cio_write_dev_grow.h hold unchanged, so new_cap_i is the reference's.  The
 * placement:
 *
 *  S1. Class k is usable iff the set is sound and pal_k is a multiple of
 *      align.  F_k = set[4k] for a usable class, else 0.
 *  S2. c_i is the smallest usable k with cls_k >= new_cap_i.  There may be
 *      none.
 *  S3. Let j_i be the number of images before i that reach rule 4 with the
 *      same class.  If j_i < F_c, the image takes entry F_c - 1 - j_i of class
 *      c WITH ITS WHOLE CAPACITY, so that nothing leaks when the slot is
 *      released again.  The entry is checked on the device before any byte of
 *      it is touched: off + cap <= dev_bytes without a wrap, cap >= cls_c, and
 *      off a multiple of align.  A failing entry is consumed; the image gets
 *      CIO_ERROR and stays valid where it was.  Every other pool-served image
 *      is accepted.
 *  S4. Otherwise the image is arena-bound.  Its capacity is cls_c when it has
 *      a class, so that its slot comes back to exactly that class when it is
 *      released, and new_cap_i without one; its slot is that capacity rounded
 *      up to align.  It is placed by grow's rule 5 over the arena-bound images
 *      alone: a cut image keeps its slot in the sums, the test is monotone
 *      within this part, and pool-served images behind an arena cut are still
 *      accepted.
 *  S5. As grow's rule 6: bytes [0, used) are copied; CIOA_GROW_ZERO zeroes
 *      [used, capacity) of the slot actually taken; last of all dev_img_offs
 *      and dev_img_caps are rewritten in place.
 *  S6. set[4k] decreases by min(images of class k, F_k), and the top advances
 *      by the arena part.  Each of these words has one writer or none, and no
 *      kernel that writes a word reads it.  A planner failure changes nothing.
 *  S7. dev_total[0] = the alignment gap plus ALL arena-bound slots (0 when
 *      there is none; it does not depend on the arena's end); dev_total[1] =
 *      the pool entries consumed; dev_total[2 + k] = the images whose class is
 *      k, served or not.
 *  S8. With no usable class the call is cio_file_grow_batch_dev output for
 *      output.
 *
 * The records variant sums the needs on the device as
 * cio_file_grow_records_batch_dev does; a malformed index rejects the whole
 * call, and no set word changes.
 *
 * Preconditions, NOT checked: those of the two headers; the set's arrays hold
 * n_cls * stride entries each; an entry that passes S3's check shares no byte
 * with a live image or with the arena's free part (the entries are release's
 * output).
 *
 * Not here: spilling to the next class when one runs out (a cut entry of a
 * release is kept, an image whose class is empty goes to the arena).
 * Coalescing adjacent free slots of the set, and with it checking for
 * duplicate entries within one release (the same sorted pass finds both), is
 * cio_write_dev_coalesce.h's cio_file_coalesce_set_dev.
 */
#ifndef CIO_WRITE_DEV_POOL_SET_H
#define CIO_WRITE_DEV_POOL_SET_H

#include "cio_write_dev_grow.h"
#include "cio_write_dev_pool.h"

#define CIOA_POOL_SET_MAX 8

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_release_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                   uint64_t *dev_offs, uint64_t *dev_caps, uint32_t *dev_img, size_t n,
                                   uint64_t *dev_count, const int32_t *dev_gate, const uint64_t *dev_live_offs,
                                   int flags,
                                   uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set, size_t n_cls,
                                   uint64_t stride,
                                   uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_grow_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                const uint64_t *dev_need, uint64_t *dev_arena,
                                uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set, size_t n_cls,
                                uint64_t stride,
                                uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                uint64_t *dev_total, int32_t *dev_status, void *stream);

int cio_file_grow_set_records_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                        uint64_t *dev_img_offs, uint64_t *dev_img_caps, size_t n,
                                        const uint32_t *dev_rec_img, const uint64_t *dev_rec_lens, size_t n_rec,
                                        uint64_t *dev_arena,
                                        uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                                        size_t n_cls, uint64_t stride,
                                        uint64_t realloc_size, uint64_t page, uint64_t align, int flags,
                                        uint64_t *dev_prev_offs, uint64_t *dev_prev_caps,
                                        uint64_t *dev_total, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_POOL_SET_H */
