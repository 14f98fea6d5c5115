/*
 * cio_write_dev_coalesce.h -- coalescing the adjacent free slots of a pool set
 * in device memory.  Extends cio_write_dev_pool_set.h and closes two of the
 * three gaps it names last: coalescing adjacent free slots, and checking for
 * duplicate entries within one release.
 *
 * The steady-state chain of cio_write_dev_pool_set.h is bounded only while the
 * producer's size mix stays the same.  When the workload drifts towards larger
 * chunks the small classes fill with slots nobody asks for again, the large
 * classes stay empty, every large slot comes from the bump arena, and the
 * arena runs out while the buffer is full of free bytes.  Those idle slots are
 * mostly neighbours in memory: one grow or rotate call lays its arena slots
 * side by side.  cio_file_coalesce_set_dev merges such neighbours into slots
 * of one TARGET class, on the device, without a copy of the set to the host.
 * It needs the free entries in address order, and that order also exposes
 * duplicates and overlaps, so the same pass drops those.
 *
 * Everything in cio_write_dev.h's contract holds: the call is queued on
 * `stream`, allocates nothing (it uses the writer's existing scratch; no array
 * was added to the writer), adds no atomic, never synchronises the host, can
 * be captured in a graph, one call in flight per writer, the result is CIO_OK
 * / CIO_ERROR with cio_gpu_last_error().  The argument checks run before any
 * device call.  The call reads and writes no byte of any slot: it takes no
 * dev_base.
 *
 * The set is (dev_set_offs, dev_set_caps, dev_set, n_cls, stride) of
 * cio_write_dev_pool_set.h; `target` is the index of the class to coalesce
 * into, `align` the alignment every slot of the buffer starts on, dev_total
 * has 5 + n_cls words.  The host refuses: unknown flags; a null writer or a
 * null pointer; n_cls outside 2 .. CIOA_POOL_SET_MAX; target outside 1 ..
 * n_cls - 1; stride == 0; n_cls * stride > the writer's max_chunks (the scratch
 * is sized by it); align that is not a power of two in 1 .. 4096; dev_bytes ==
 * 0; (dev_bytes - 1) / align >= 2^32 - 1 (the sort key off / align and its
 * sentinel must fit 32 bits).
 *
 * The rules, decided on the device.  T = cls_target and P = pal_target, both
 * read from dev_set.
 *
 *  C0. UNSOUND SET.  Soundness is cio_write_dev_pool_set.h's.  If the set is
 *      unsound, dev_total[0] = 1, every other dev_total word is 0, and nothing
 *      else changes.
 *  C1. ENTRIES.  The entries are (k, j) with j < set[4k], enumerated
 *      class-major and position-minor.  An entry is well-formed iff cap >= 1,
 *      off + cap <= dev_bytes without a wrap, and off is a multiple of align.
 *      Ill-formed entries are dropped.
 *  C2. DUPLICATES AND OVERLAPS.  Sort the well-formed entries by off, stably
 *      in enumeration order.  Let M_i be the largest off + cap of the entries
 *      before i in that order (dropped ones included).  Entry i collides iff
 *      off_i < M_i; it is dropped.  Of two identical entries the first in
 *      enumeration order survives.
 *  C3. RUNS.  Take the survivors in sorted order.  A survivor is a CANDIDATE
 *      iff cap < T.  Survivor i + 1 continues survivor i's run iff both are
 *      candidates and round_up(off_i + cap_i, align) == off_{i+1}; the padding
 *      up to align belongs to nobody, because every slot starts on align.
 *      Every other candidate starts a run.  A non-candidate is never part of a
 *      run.
 *  C4. GROUPS.  Inside one run, g_0 is the first entry whose off is a multiple
 *      of P, and g_{m+1} is the first entry with off >= off(g_m) + T whose off
 *      is a multiple of P.  Group m is the entries from g_m up to, but not
 *      including, g_{m+1}; if g_{m+1} does not exist, group m is the entries
 *      from g_m to the run's end provided that covers at least T bytes (end of
 *      the last entry - off(g_m) >= T), otherwise those entries stay single.
 *      Entries before g_0 stay single.  A group becomes ONE slot: off is that
 *      of its first entry, cap is the end of its last entry minus that off.
 *      It keeps its whole capacity, so nothing leaks.  A group of one entry is
 *      that entry, unchanged: it counts as an entry outside a group
 *      everywhere below (C9 needs this: an interior group may end up to
 *      align - 1 bytes short of T, stay a candidate, and be met again).
 *  C5. FILING.  The outputs are the groups and every survivor outside a group,
 *      in ascending off.  Each is filed by release's rule 4': the largest k
 *      with cls_k <= cap and off a multiple of pal_k.  An output with no class
 *      is dropped and counted, once, with the ill-formed entries.
 *  C6. COMMIT.  Let c_k be the number of outputs filed in class k.  If any c_k
 *      > set[4k + 1]: dev_total[0] = 2 and no word of the set or its arrays
 *      changes -- the call is all or nothing; the counts below are still
 *      reported, so that a caller can size the classes.  Otherwise class k's
 *      entries become its outputs in ascending off at k * stride + 0 .. c_k -
 *      1, set[4k] = c_k, array words at positions >= c_k keep their values,
 *      and dev_total[0] = 0.  Each set word has one writer or none, and no
 *      kernel that writes a word reads it.
 *  C7. TOTALS.  dev_total[1] = the entries dropped as ill-formed plus the
 *      classless outputs; dev_total[2] = the entries dropped by C2;
 *      dev_total[3] = the groups (of two or more entries); dev_total[4] = the
 *      entries those groups are made of; dev_total[5 + k] = c_k.
 *  C8. DRY RUN.  CIOA_COALESCE_DRY computes dev_total exactly as above and
 *      changes nothing else.
 *  C9. IDEMPOTENCE.  A second call on the result changes nothing and reports
 *      dev_total[1] = dev_total[2] = dev_total[3] = dev_total[4] = 0.
 *
 * Preconditions, NOT checked: the arrays hold n_cls * stride entries each;
 * every live image and every arena slot of the buffer begins at a multiple of
 * align; the set's entries are the output of release.
 *
 * Where it goes: after the releases of a round, and before the grow when a
 * class's demand (cio_file_grow_set_batch_dev's dev_total[2 + k]) exceeded its
 * entries.
 *
 * Not here: spilling to another class in release or grow; splitting large
 * slots into smaller ones; more than one target per call; moving live images
 * to create adjacency.
 */
#ifndef CIO_WRITE_DEV_COALESCE_H
#define CIO_WRITE_DEV_COALESCE_H

#include "cio_write_dev_pool_set.h"

#define CIOA_COALESCE_DRY 1   /* compute dev_total, change nothing */

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_coalesce_set_dev(cio_dev_writer *w, uint64_t dev_bytes,
                              uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                              size_t n_cls, uint64_t stride, size_t target, uint64_t align, int flags,
                              uint64_t *dev_total /* 5 + n_cls words */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_WRITE_DEV_COALESCE_H */
