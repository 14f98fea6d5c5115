/*
 * cio_persist_dev.h -- chunk images in device memory (HBM) down to chunk files
 * and up again.  Extends cio_write_dev_pool_set.h and cio_read_dev.h and closes
 * the gap both leave: cio_read_dev.h says of CIOA_READ_IMAGE "copied to a file,
 * that is the chunk file" and leaves the copying to the caller, and nothing
 * hands out fresh slots of given sizes from the pool set -- a loader has n
 * sizes and no images yet.
 *
 *   cio_file_alloc_set_batch_dev  n slots of given sizes from the set, then
 *                                 the arena: device-side, queued, capturable
 *   cio_file_load_paths_dev       chunk files into HBM: cio_chunk_up
 *                                 (src/cio_chunk.c:556-590, _cio_file_up ->
 *                                 mmap_file, src/cio_file.c:345-493) for a batch
 *   cio_file_store_paths_dev      images in HBM into chunk files: cio_file_sync
 *                                 (src/cio_file.c:1147-1250) + cio_chunk_down
 *                                 for a batch
 *
 * ALLOCATION.  The contract is cio_write_dev_pool_set.h's: queued on `stream`,
 * no allocation, no host synchronisation, no atomic, capturable, one call in
 * flight per writer, n == 0 is a no-op that returns CIO_OK, CIO_OK / CIO_ERROR
 * with cio_gpu_last_error().  The argument checks (unknown flags, align not a
 * power of two in 1 .. 4096, n_cls > CIOA_POOL_SET_MAX, stride == 0 with
 * classes, null writer, null pointers, n > max_chunks) run before any device
 * call.  n_cls == 0 with null set pointers means arena only.
 *
 *  A1. Entry i reaches the placement iff dev_gate is NULL or dev_gate[i] ==
 *      CIO_OK, and dev_need[i] >= 24.
 *  A2. The placement is rules S1..S4 and S6..S7 of cio_write_dev_pool_set.h
 *      with new_cap_i := dev_need[i]: the smallest usable class that holds the
 *      need; that class's top entry, taken with its whole capacity and checked
 *      on the device before it is handed out (a failing entry is consumed, and
 *      entry i gets CIO_ERROR); otherwise an arena slot of the class's size, or
 *      of the need when no class holds it, rounded up to align and placed by
 *      grow's rule 5 over the arena-bound entries alone -- a cut entry keeps
 *      its slot in the sums, and pool-served entries behind an arena cut are
 *      still accepted.
 *  A3. An accepted entry gets dev_out_offs[i], dev_out_caps[i] (the pool
 *      entry's whole capacity, or the arena-bound capacity: the class's size or
 *      the need) and dev_status[i] = CIO_OK.  Any other entry gets UINT64_MAX,
 *      0 and CIO_ERROR.
 *  A4. CIOA_ALLOC_ZERO zeroes [dev_out_offs[i], + dev_out_caps[i]) of every
 *      accepted entry with grow's byte-balanced fill.  Without it no byte of
 *      the buffer is touched: what a slot holds is whatever was there.
 *  A5. dev_total has 2 + n_cls words with grow_set's meaning: [0] the alignment
 *      gap plus ALL arena-bound slots, [1] the pool entries consumed, [2 + k]
 *      the entries whose class is k, served or not.
 *
 * Preconditions, NOT checked: those of cio_write_dev_pool_set.h.
 *
 * ROUNDS.  The two file calls stage their bytes through dev_stage, a device
 * buffer of stage_bytes the caller owns, in rounds.  A round is a maximal run
 * of consecutive files whose sizes, each rounded up to 128 bytes, fit what one
 * round may use of the stage.  This implementation uses the stage WHOLE: a
 * round's reads do not overlap the previous round's device chain.  The two
 * HIP-free functions say so:
 *
 *   cio_file_persist_round_max(stage_bytes)  the largest file a stage of that
 *       size takes: stage_bytes rounded down to 128;
 *   cio_file_persist_rounds(sizes, n, stage_bytes, round_of)  the partition:
 *       round_of[i] is file i's round, UINT32_MAX for a file larger than the
 *       maximum, which closes the round before it; returns the number of
 *       rounds, or CIO_ERROR for a null pointer with n != 0.
 *
 * LOAD.  Host-synchronous, as cio_verify_paths is: it returns when every
 * output, host and device, is final.  flags: 0, CIO_CHECKSUM (4) and / or
 * CIOA_LOAD_ZERO.  Per round: pread on at most 16 host threads into pinned
 * staging; one H2D into the stage; cio_file_verify_batch_dev over the staged
 * bytes with sizes = the file sizes, whose verdicts are the call's;
 * cio_file_alloc_set_batch_dev gated by those verdicts with need = the file
 * size (the reference maps a chunk at fs_size), so a file that does not verify
 * never takes a slot; the write path's copy from the stage into the slots; and
 * the adopt step, which writes an inferred legacy content length to bytes
 * 10..13 of the HBM copy (the reference's read-write load does: the slot's
 * capacity no longer says where the content ends) and sets the outputs.
 *
 *   status[i], error[i]  host: verify's verdict (CIO_OK, CIO_CORRUPTED with a
 *       CIO_ERR_* code); CIO_ERROR for a file that cannot be opened or read in
 *       full, for one larger than the round maximum, and for one that verified
 *       and found no slot.  fs_sizes[i] (may be NULL): the file size, 0 when
 *       unknown.
 *   dev_img_offs[i], dev_img_caps[i], dev_crc_cur[i], dev_status[i]  device:
 *       the slot and the verified raw CRC state of a loaded image, else
 *       UINT64_MAX, 0, 0 and the status.
 *
 * CIOA_LOAD_ZERO zeroes [fs_size, cap) of each slot taken.  After the call the
 * loaded images are ordinary images of the write path: appends continue their
 * CRC and seal closes them.  The writer must hold n images (n <= max_chunks).
 *
 * STORE.  Host-synchronous.  The gate and the image check are the read path's
 * (cio_read_dev.h); the call computes no CRC -- to store only verified chunks,
 * queue seal and cio_file_verify_batch_dev ahead and pass verify's status as
 * dev_gate.  One size query (cio_file_read_packed_batch_dev, CIOA_READ_IMAGE,
 * dev_out = NULL) and a D2H of lengths, capacities and statuses is the call's
 * one early synchronisation; the host splits the batch into rounds by the
 * same planner over the used bytes; each round packs its images' used bytes
 * into the stage (128-byte slots), makes one D2H into pinned staging and
 * writes the files on at most 16 host threads.
 *
 *   File i holds the image's used bytes [0, 24 + meta + content) followed by
 *   zeros up to the file size: dev_img_caps[i] without CIOA_STORE_TRIM (the
 *   reference's untrimmed file), with it the used bytes rounded up to `page`,
 *   a power of two, 1 meaning exact (cio_file_sync under CIO_TRIM_FILES).  Slot
 *   bytes past the used ones never cross PCIe: the tail comes from ftruncate.
 *   CIOA_STORE_SYNC calls fdatasync before close.
 *
 * A rejected entry creates no file and leaves an existing file untouched.  A
 * failed write unlinks its partial file and reports CIO_ERROR.  An image whose
 * used bytes exceed cio_file_persist_round_max(stage_bytes) is CIO_ERROR.
 * status[i] (host), file_sizes[i] (host, may be NULL; 0 when no file was
 * written); dev_status is uploaded at the end, so that
 * cio_file_release_set_batch_dev can be queued behind the call gated by it:
 * "stored, therefore releasable" is one device-side condition.
 *
 * Not here: a fused verify + copy kernel for the drain; mmap or peer-to-peer
 * file I/O into HBM; multi-GPU variants; keeping down chunks' names in a
 * device-side directory; a max_chunks_up budget enforced by the library (the
 * caller composes store -> release_set and load); the new calls in the
 * lifecycle walk of the existing tests (a later walk of its own may add them).
 *
 * The pinned staging of the two file calls is one buffer per process, sized to
 * the largest round a call planned and kept between calls, with the rounds'
 * small device arrays; cio_file_persist_trim() frees both (they come back with
 * the next call).  The two file calls do not overlap one another in a process.
 */
#ifndef CIO_PERSIST_DEV_H
#define CIO_PERSIST_DEV_H

#include "cio_read_dev.h"
#include "cio_write_dev_pool_set.h"

#define CIOA_ALLOC_ZERO  1
#define CIOA_LOAD_ZERO   512    /* beside CIO_CHECKSUM (4); clear of chunkio.h's flag bits, as CIOA_TX_ZERO is */
#define CIOA_STORE_TRIM  1
#define CIOA_STORE_SYNC  2

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_alloc_set_batch_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                                 const uint64_t *dev_need, const int32_t *dev_gate, size_t n,
                                 uint64_t *dev_arena,
                                 uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set, size_t n_cls,
                                 uint64_t stride,
                                 uint64_t align, int flags,
                                 uint64_t *dev_out_offs, uint64_t *dev_out_caps,
                                 uint64_t *dev_total, int32_t *dev_status, void *stream);

uint64_t cio_file_persist_round_max(uint64_t stage_bytes);

void cio_file_persist_trim(void);

int cio_file_persist_rounds(const uint64_t *sizes, size_t n, uint64_t stage_bytes, uint32_t *round_of);

int cio_file_load_paths_dev(cio_dev_writer *w, void *dev_base, uint64_t dev_bytes,
                            const char *const *paths, size_t n, int flags,
                            void *dev_stage, uint64_t stage_bytes,
                            uint64_t *dev_arena, uint64_t *dev_set_offs, uint64_t *dev_set_caps, uint64_t *dev_set,
                            size_t n_cls, uint64_t stride, uint64_t align,
                            uint64_t *dev_img_offs, uint64_t *dev_img_caps, uint32_t *dev_crc_cur,
                            int32_t *dev_status,
                            int *status, int *error, uint64_t *fs_sizes, void *stream);

int cio_file_store_paths_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n,
                             const int32_t *dev_gate, const char *const *paths, int flags, uint64_t page,
                             void *dev_stage, uint64_t stage_bytes,
                             int *status, uint64_t *file_sizes, int32_t *dev_status, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_PERSIST_DEV_H */
