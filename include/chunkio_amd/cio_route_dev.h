/*
 * cio_route_dev.h -- routing records to chunk images in device memory by their
 * metadata.  Every append call of cio_write_dev_records.h and
 * cio_write_dev_ungrouped.h takes dev_rec_img[r], the index of the image that
 * record r goes to; the rotate and grow calls ahead of them take it too.  This
 * header produces that array on the device, for a producer whose records carry
 * a TAG: in chunkio's main user the tag is the chunk's metadata, and the one
 * primitive for it is cio_meta_cmp.  cio_meta_cmp_batch_dev (cio_read_dev.h)
 * is that primitive one-to-one; the two calls here are one-to-many:
 *
 *   cio_file_route_build_dev          a DIRECTORY of the images that are up,
 *                                     keyed by a hash of their metadata
 *   cio_file_route_records_batch_dev  for every record the image whose metadata
 *                                     equals the record's tag, through the
 *                                     directory
 *
 * so that route -> rotate_records -> grow_records -> ungrouped append is one
 * chain on one stream, with no tag and no index crossing to the host.
 *
 * Everything in cio_write_dev.h's contract holds: dev_* arguments are device
 * arrays, the calls are queued on `stream`, allocate nothing (they use the
 * writer's existing scratch; no array was added to the writer), add no atomic,
 * never synchronise the host, can be captured in a graph, one call in flight
 * per writer, the result is CIO_OK / CIO_ERROR with cio_gpu_last_error().  The
 * argument checks run before any device call.  The host refuses: unknown flags
 * (only 0 is known); a null writer; a null required pointer (dev_base,
 * dev_img_offs and dev_img_caps only when n_img > 0, the directory arrays
 * likewise, dev_tags only when tag_bytes > 0, dev_miss_list never); n_img or
 * n_rec greater than the writer's max_chunks (the scratch is sized by it);
 * n_img >= 2^32 - 1.  Neither call writes a byte of the image buffer.
 *
 * The directory is caller-owned: dev_dir_keys and dev_dir_imgs of n_img words
 * each and dev_dir_hdr of four words.
 *
 * The rules, decided on the device.
 *
 *  R0. KEY.  The key of a byte string is its raw CRC-32 state: what
 *      cio_crc32_devplan_exec writes with dev_seeds == NULL, un-finalized, as
 *      chunkio keeps crc_cur -- ~crc32(bytes) of zlib.  The key of the empty
 *      string is the raw init state, 0xffffffff.
 *  R1. BUILD.  key_i is the key of the metadata bytes [24, 24 + meta_i) of
 *      image i when the image check of the write path (magic, lengths inside
 *      the capacity, the slot inside dev_bytes) passes, and the key of the
 *      empty string when it fails.  (dev_dir_keys, dev_dir_imgs) is the stable
 *      sort of (key_i, i) by key: ties keep ascending i.  dev_dir_hdr[0] =
 *      n_img, dev_dir_hdr[1] = the number of images that passed the check,
 *      dev_dir_hdr[2] = dev_dir_hdr[3] = 0.  n_img == 0 writes only the header.
 *  R2. A WELL-FORMED TAG.  Tag r is dev_tags[dev_tag_offs[r] : +
 *      dev_tag_lens[r]].  It is well-formed when its length is <= 65535 and
 *      [off, off + len) lies inside tag_bytes without overflow.  A tag of
 *      length 0 has no source range and is well-formed whatever its offset, as
 *      a zero-length record of cio_write_dev.h.  dev_tags may be NULL when
 *      tag_bytes == 0.
 *  R3. CANDIDATES.  The candidates of a well-formed record r are the positions
 *      j with dev_dir_keys[j] == key(tag_r) and dev_dir_imgs[j] < n_img, in
 *      ascending j, found by a lower bound over dev_dir_keys.
 *  R4. MATCH.  The match of r is the first candidate i = dev_dir_imgs[j] for
 *      which dev_img_gate is NULL or dev_img_gate[i] == CIO_OK, the image
 *      check of image i passes NOW, at the offsets given to this call, meta_i
 *      == len_r, and the bytes are equal -- the last three are cio_meta_cmp ==
 *      0.  With a directory that R1 built over the same images, the match is
 *      the lowest i that satisfies all of them.
 *  R5. OUTPUTS.  Matched: dev_rec_img[r] = i, dev_rec_status[r] = CIO_OK.
 *      Well-formed without a match: dev_rec_img[r] = miss_img, status
 *      CIO_RETRY -- open a chunk for that tag and route again.  Malformed:
 *      dev_rec_img[r] = miss_img, status CIO_ERROR.  miss_img is any value: a
 *      catch-all image's index, or n_img to make a following append refuse the
 *      batch.  dev_total[0..2] are the numbers of matched, missed and malformed
 *      records.  dev_miss_list may be NULL; if given (n_rec words), its first
 *      dev_total[1] entries are the missed record indices in ascending order
 *      and the rest keep their values.
 *  R6. A STALE OR DAMAGED DIRECTORY CAN ONLY LOSE MATCHES.  Take any contents
 *      of the two directory arrays with dev_dir_hdr[0] == n_img.  Every
 *      dev_rec_img[r] with status CIO_OK is an i < n_img whose current metadata
 *      equals the tag, and no load leaves the arrays: an entry >= n_img is
 *      skipped.  So a directory stays usable across rotate, grow and append,
 *      which keep the metadata; after write_metadata, init or load it needs a
 *      rebuild only to FIND the changed images.
 *  R7. A DIRECTORY OF ANOTHER SIZE.  With dev_dir_hdr[0] != n_img every status
 *      is CIO_ERROR, every dev_rec_img[r] is miss_img, and dev_total is {0, 0,
 *      n_rec}.
 *  R8. EMPTY BATCHES.  n_rec == 0 is a no-op that returns CIO_OK.  n_img == 0
 *      with n_rec > 0 looks at no image array and no directory array (the
 *      header alone): every well-formed record misses.
 *
 * Preconditions, NOT checked: the arrays hold the entries the counts say; two
 * tags of one batch may overlap; the images do not change while a call runs.
 *
 * Cost: the build is one CRC launch over the metadata and a four-pass sort;
 * the route is one CRC launch over the tags and one wave per record that walks
 * the images of its key -- one image unless metadata is duplicated or keys
 * collide.  Images that fail the check and images with empty metadata share
 * the key of the empty string: an empty tag walks all of them.
 *
 * Not here: opening chunks for the missed tags, which needs the missed tags
 * de-duplicated first; a per-image count of the routed records, which
 * rotate_records and grow_records sum themselves; prefix or wildcard matching;
 * incremental updates of a directory; multi-GPU.
 */
#ifndef CIO_ROUTE_DEV_H
#define CIO_ROUTE_DEV_H

#include "cio_write_dev_ungrouped.h"

#ifndef CIO_RETRY
#define CIO_RETRY   -2   /* as in cioa_chunk.h */
#endif

#ifdef __cplusplus
extern "C" {
#endif

int cio_file_route_build_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                             const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                             uint32_t *dev_dir_keys, uint32_t *dev_dir_imgs, uint32_t *dev_dir_hdr /* 4 words */,
                             void *stream);

int cio_file_route_records_batch_dev(cio_dev_writer *w, const void *dev_base, uint64_t dev_bytes,
                                     const uint64_t *dev_img_offs, const uint64_t *dev_img_caps, size_t n_img,
                                     const int32_t *dev_img_gate,
                                     const uint32_t *dev_dir_keys, const uint32_t *dev_dir_imgs,
                                     const uint32_t *dev_dir_hdr,
                                     const void *dev_tags, uint64_t tag_bytes,
                                     const uint64_t *dev_tag_offs, const uint64_t *dev_tag_lens, size_t n_rec,
                                     uint32_t miss_img, int flags,
                                     uint32_t *dev_rec_img, int32_t *dev_rec_status,
                                     uint32_t *dev_miss_list, uint64_t *dev_total /* 3 words */, void *stream);

#ifdef __cplusplus
}
#endif

#endif /* CIO_ROUTE_DEV_H */
