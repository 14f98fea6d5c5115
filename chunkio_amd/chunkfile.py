"""Python binding of the C chunk layer (include/chunkio_amd/cioa_chunk.h).

The chunk layer itself is C (chunkio_amd/csrc/cioa_chunk.c): chunkio's
filesystem backend with the reference's on-disk format and CRC lifecycle,
its verifies and deferred CRCs on the batched GPU path.  Names follow the
reference (file:line citations into /root/reference):

  Context(root, flags)            cio_create (src/chunkio.c:84-207)
  Context.stream(name)            cio_stream_create (src/cio_stream.c:113-178)
  Context.scan(stream, ext)       cio_scan_stream_files (src/cio_scan.c:39-125), one
                                  GPU verify batch, CIO_DELETE_IRRECOVERABLE
  Stream.open(name, flags)        cio_chunk_open (src/cio_chunk.c:30-109)
  Chunk.write / write_at          cio_chunk_write / _write_at (src/cio_chunk.c:184-227)
  Chunk.meta_write / meta_len     cio_meta_write / _size (src/cio_meta.c:46-88)
  Chunk.sync / sync_batch(chunks) cio_chunk_sync (src/cio_file.c:1147-1250); batched
  Chunk.up / up_force / down      src/cio_chunk.c:556-605
  Chunk.tx_begin/commit/rollback  src/cio_chunk.c:423-502
  Chunk.hash()                    cio_chunk_hash: the 4 bytes at map+2

ChunkFile.open(path, ...) is the one-chunk convenience form used by the
tests and benches: a private context rooted at dirname(dirname(path)) with
the stream dirname(path).

verify_paths(paths) is the batched verify-on-load of a list of chunk files
(cio_verify_paths_multi).

DevWriter with init_batch_dev / write_batch_dev / seal_batch_dev is the write
lifecycle of chunk images that live in device memory
(include/chunkio_amd/cio_write_dev.h): write_init_header, cio_file_write +
update_checksum and finalize_checksum (src/cio_file.c:149-162, 994-1073,
97-124) in batches, on cuda tensors, without waiting.  DevWriter(n, move=True)
with write_metadata_batch_dev replaces the metadata of images that already
hold content (cio_file_write_metadata, src/cio_file.c:1075-1145: the content
moves inside the image), and write_at_batch_dev is cio_chunk_write_at
(src/cio_chunk.c:184-209); include/chunkio_amd/cio_write_dev_move.h.

write_records_batch_dev is the grouped append: many records per image in one
call, the records grouped by image
(include/chunkio_amd/cio_write_dev_records.h).

read_batch_dev / read_packed_batch_dev gather the metadata, the content or the
trimmed image of every image of a batch into an output tensor
(cio_meta_read, cio_file_content_copy; include/chunkio_amd/cio_read_dev.h),
and meta_cmp_batch_dev is cio_meta_cmp.

tx_state with tx_begin_batch_dev / tx_rollback_batch_dev / tx_commit_batch_dev
are cio_chunk_tx_begin / _rollback / _commit (src/cio_chunk.c:423-502) on
images in device memory, and tx_cond_records_batch_dev turns the statuses of a
records append into the per-image condition of an all-or-nothing append
(include/chunkio_amd/cio_write_dev_tx.h).

alloc_set_batch_dev hands out fresh slots of given sizes from a pool set and
the arena, and load_paths_dev / store_paths_dev move batches of chunks between
chunk files and images in device memory: cio_chunk_up, and cio_file_sync +
cio_chunk_down (src/cio_chunk.c:556-605), for device images
(include/chunkio_amd/cio_persist_dev.h).
"""
import ctypes
import os
import struct

import numpy as np

from . import _lib

CIO_OK, CIO_ERROR, CIO_RETRY, CIO_CORRUPTED = 0, -1, -2, -3
CIO_OPEN, CIO_OPEN_RD, CIO_CHECKSUM, CIO_FULL_SYNC = 1, 2, 4, 8
CIO_DELETE_IRRECOVERABLE, CIO_TRIM_FILES = 16, 32
CIOA_DEFERRED_CRC = 128
CIOA_BENCH_PIPELINED_SYNC = 0x10000      # cioa_bench_perf_write only
CIO_ERR_BAD_CHECKSUM, CIO_ERR_BAD_LAYOUT, CIO_ERR_PERMISSION, CIO_ERR_BAD_FILE_SIZE = -10, -11, -12, -13
CIOA_VERIFY_DELETE_IRRECOVERABLE = 16
CIOA_VERIFY_WRITEBACK = 64
CIOA_SYNC_FINALIZE, CIOA_SYNC_MSYNC, CIOA_SYNC_FULL = 1, 2, 8
CIOA_SEAL_RECOMPUTE = 256
CIOA_WRITER_MOVE = 1
CIOA_READ_META, CIOA_READ_CONTENT, CIOA_READ_IMAGE = 0, 1, 2
CIOA_READ_NUL = 1
CIOA_GROW_ZERO = 1              # cio_write_dev_grow.h
CIOA_TX_RECOMPUTE, CIOA_TX_ZERO = 256, 512      # cio_write_dev_tx.h
CIOA_RELEASE_ZERO, CIOA_RELEASE_COMPACT = 1, 2  # cio_write_dev_pool.h
CIOA_POOL_SET_MAX = 8           # cio_write_dev_pool_set.h
COALESCE_DRY = 1                # cio_write_dev_coalesce.h: CIOA_COALESCE_DRY
CIOA_ALLOC_ZERO, CIOA_LOAD_ZERO = 1, 512        # cio_persist_dev.h
CIOA_STORE_TRIM, CIOA_STORE_SYNC = 1, 2

HDR_MIN = 24
CONTENT_OFFSET = 22
CRC_INIT = 0xFFFFFFFF


class VerifyItem(ctypes.Structure):
    _fields_ = [("map", ctypes.c_void_p), ("fs_size", ctypes.c_size_t), ("taint", ctypes.c_int),
                ("status", ctypes.c_int), ("error", ctypes.c_int), ("crc_raw", ctypes.c_uint32),
                ("meta_len", ctypes.c_uint16), ("content_len", ctypes.c_uint64)]


class SyncItem(ctypes.Structure):
    _fields_ = [("map", ctypes.c_void_p), ("fs_size", ctypes.c_size_t), ("crc_end", ctypes.c_uint64),
                ("crc_cur", ctypes.c_uint32), ("status", ctypes.c_int), ("data_end", ctypes.c_uint64)]


def _bind():
    lib = _lib.lib()
    if getattr(lib, "_chunk_bound", False):
        return lib
    V, I, S = ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t
    IP, U32 = ctypes.POINTER(ctypes.c_int), ctypes.c_uint32
    sig = {
        "cio_file_verify_batch": (I, [ctypes.POINTER(VerifyItem), S, I]),
        "cio_file_verify_batch_multi": (I, [ctypes.POINTER(VerifyItem), S, I, IP, I]),
        "cio_verify_paths": (I, [ctypes.POINTER(ctypes.c_char_p), S, I, IP, IP, ctypes.POINTER(U32)]),
        "cio_verify_paths_multi": (I, [ctypes.POINTER(ctypes.c_char_p), S, I, IP, I, IP, IP,
                                       ctypes.POINTER(U32)]),
        "cio_file_sync_batch": (I, [ctypes.POINTER(SyncItem), S, I]),
        "cio_file_sync_batch_multi": (I, [ctypes.POINTER(SyncItem), S, I, IP, I]),
        "cioa_create": (V, [ctypes.c_char_p, I]),
        "cioa_destroy": (None, [V]),
        "cioa_set_max_chunks_up": (I, [V, I]),
        "cioa_set_realloc_size_hint": (I, [V, S]),
        "cioa_set_devices": (I, [V, IP, I]),
        "cioa_last_chunk_error": (I, [V]),
        "cioa_total_chunks_up": (S, [V]),
        "cioa_stream_create": (V, [V, ctypes.c_char_p]),
        "cioa_stream_get": (V, [V, ctypes.c_char_p]),
        "cioa_stream_chunks": (S, [V, ctypes.POINTER(V), S]),
        "cioa_stream_size_chunks_up": (S, [V]),
        "cioa_scan_stream": (V, [V, ctypes.c_char_p, ctypes.c_char_p]),
        "cioa_scan_streams": (I, [V, ctypes.c_char_p]),
        "cioa_scan_dump": (I, [V, V]),
        "cioa_chunk_open": (V, [V, V, ctypes.c_char_p, I, S, IP]),
        "cioa_chunk_close": (None, [V, I]),
        "cioa_chunk_write": (I, [V, V, S]),
        "cioa_chunk_write_at": (I, [V, ctypes.c_long, V, S]),
        "cioa_chunk_sync": (I, [V]),
        "cioa_chunk_sync_batch": (I, [ctypes.POINTER(V), S]),
        "cioa_chunk_sync_batch_begin": (I, [ctypes.POINTER(V), S, ctypes.POINTER(V)]),
        "cioa_chunk_sync_batch_end": (I, [V]),
        "cio_file_sync_batch_begin": (I, [ctypes.POINTER(SyncItem), S, I, IP, I, ctypes.POINTER(V)]),
        "cio_file_sync_batch_end": (I, [V]),
        "cioa_chunk_get_content_size": (ctypes.c_ssize_t, [V]),
        "cioa_chunk_get_content_end_pos": (S, [V]),
        "cioa_chunk_is_file": (I, [V]),
        "cioa_chunk_close_stream": (None, [V]),
        "cioa_chunk_get_real_size": (ctypes.c_ssize_t, [V]),
        "cioa_chunk_hash": (V, [V]),
        "cioa_chunk_map": (V, [V, ctypes.POINTER(S)]),
        "cioa_chunk_name": (ctypes.c_char_p, [V]),
        "cioa_chunk_lock": (I, [V]),
        "cioa_chunk_unlock": (I, [V]),
        "cioa_chunk_tx_begin": (I, [V]),
        "cioa_chunk_tx_commit": (I, [V]),
        "cioa_chunk_tx_rollback": (I, [V]),
        "cioa_chunk_is_up": (I, [V]),
        "cioa_chunk_up": (I, [V]),
        "cioa_chunk_up_force": (I, [V]),
        "cioa_chunk_up_batch": (I, [ctypes.POINTER(V), S, IP]),
        "cioa_chunk_up_force_batch": (I, [ctypes.POINTER(V), S, IP]),
        "cioa_chunk_down": (I, [V]),
        "cioa_error_get": (I, [V]),
        "cioa_chunk_crc_cur": (U32, [V]),
        "cioa_chunk_set_crc_cur": (None, [V, U32]),
        "cioa_meta_write": (I, [V, ctypes.c_char_p, S]),
        "cioa_meta_size": (I, [V]),
        "cioa_bench_perf_write": (I, [ctypes.c_char_p, V, S, I, I, I, I, ctypes.POINTER(ctypes.c_double),
                                      ctypes.POINTER(ctypes.c_uint64)]),
    }
    for name, (res, args) in sig.items():
        fn = getattr(lib, name)
        fn.restype = res
        fn.argtypes = args
    lib._chunk_bound = True
    return lib


def _devs(devices):
    if not devices:
        return None, 0
    arr = (ctypes.c_int * len(devices))(*devices)
    return arr, len(devices)


def verify_paths(paths, flags=CIO_CHECKSUM, devices=None):
    """Batched verify-on-load: (status, error, crc_raw) numpy arrays per path."""
    lib = _bind()
    n = len(paths)
    arr = (ctypes.c_char_p * max(n, 1))(*[os.fsencode(p) for p in paths])
    st = np.zeros(max(n, 1), np.int32)
    er = np.zeros(max(n, 1), np.int32)
    cr = np.zeros(max(n, 1), np.uint32)
    dv, nd = _devs(devices)
    rc = lib.cio_verify_paths_multi(arr, n, flags, dv, nd, st.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                    er.ctypes.data_as(ctypes.POINTER(ctypes.c_int)),
                                    cr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint32)))
    _lib.check(rc, "cio_verify_paths_multi")
    return st[:n], er[:n], cr[:n]


def verify_batch_dev(plan, base, img_offs, img_sizes, flags=CIO_CHECKSUM, stream=None):
    """Verify-on-load of chunk images that are in device memory
    (cio_file_verify_batch_dev): image i is base[img_offs[i]:img_offs[i] +
    img_sizes[i]].  plan: a crc32.Crc32DevPlan with max_chunks >= n; base: uint8
    cuda tensor; img_offs, img_sizes: 64-bit cuda tensors.  Queues the work on
    `stream` and returns cuda tensors (status int32, error int32, crc_raw
    int32 holding the uint32 bits, meta_len int32, content_len int64) without
    waiting for them."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    dev = base.device
    st = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    er = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    cr = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    ml = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    cl = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    rc = _lib.lib().cio_file_verify_batch_dev(plan._handle, _ptr(base), base.numel() * base.element_size(),
                                              _ptr(img_offs), _ptr(img_sizes), n, int(flags), _ptr(st), _ptr(er),
                                              _ptr(cr), _ptr(ml), _ptr(cl), _stream_ptr(stream))
    _lib.check(rc, "cio_file_verify_batch_dev")
    return st[:n], er[:n], cr[:n], ml[:n], cl[:n]


class DevWriter:
    """A writer of chunk images in device memory (cio_dev_writer_*): a device
    plan and arenas for batches of up to max_chunks images.  move=True
    (CIOA_WRITER_MOVE) adds the scratch arena of the in-place move, which
    write_metadata_batch_dev needs.  Not thread-safe; one call in flight at a
    time."""

    def __init__(self, max_chunks, move=False):
        self.max_chunks = int(max_chunks)
        handle = ctypes.c_void_p()
        _lib.check(_lib.lib().cio_dev_writer_create_ex(ctypes.byref(handle), self.max_chunks,
                                                       CIOA_WRITER_MOVE if move else 0),
                   "cio_dev_writer_create_ex")
        self._handle = handle

    @property
    def move_segments(self):
        """Segments the move partitions a batch into; 0 without move=True."""
        return int(_lib.lib().cio_dev_writer_move_segments(self._handle)) if self._handle else 0

    def close(self):
        if getattr(self, "_handle", None):
            _lib.lib().cio_dev_writer_destroy(self._handle)
            self._handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def _status_out(status, n, dev):
    import torch
    if status is None:
        status = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    return status


def init_batch_dev(writer, base, img_offs, img_caps, meta_src=None, meta_offs=None, meta_lens=None,
                   flags=CIO_CHECKSUM, crc_cur=None, status=None, stream=None):
    """Initialise chunk images in device memory (cio_file_init_batch_dev):
    image i is base[img_offs[i]:img_offs[i] + img_caps[i]].  With meta_src (uint8
    cuda tensor) record i of it, meta_src[meta_offs[i]:+meta_lens[i]], becomes
    the image's metadata.  base: uint8 cuda tensor; offsets, capacities and
    lengths: 64-bit cuda tensors.  Queues the work on `stream` and returns
    (status int32, crc_cur int32 holding the uint32 bits) cuda tensors without
    waiting; crc_cur / status may be passed in to be reused."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    if crc_cur is None:
        crc_cur = torch.zeros(max(n, 1), dtype=torch.int32, device=base.device)
    rc = _lib.lib().cio_file_init_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n,
        _ptr(meta_src), 0 if meta_src is None else meta_src.numel() * meta_src.element_size(),
        _ptr(meta_offs), _ptr(meta_lens), int(flags), _ptr(crc_cur), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_init_batch_dev")
    return status[:n], crc_cur[:n]


def write_batch_dev(writer, base, img_offs, img_caps, src, src_offs, src_lens, crc_cur, flags=CIO_CHECKSUM,
                    status=None, stream=None):
    """Append record i, src[src_offs[i]:+src_lens[i]], to image i
    (cio_file_write_batch_dev); crc_cur (int32 cuda tensor of n, from
    init_batch_dev) is updated in place when flags has CIO_CHECKSUM.  The
    content lengths are read from the images on the device, so a captured call
    appends again on every replay.  Returns the status cuda tensor (int32)
    without waiting; pass `status` to reuse one (under graph capture)."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_write_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n,
        _ptr(src), src.numel() * src.element_size(), _ptr(src_offs), _ptr(src_lens), int(flags), _ptr(crc_cur),
        _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_write_batch_dev")
    return status[:n]


def write_metadata_batch_dev(writer, base, img_offs, img_caps, meta_src, meta_offs, meta_lens, crc_cur,
                             flags=CIO_CHECKSUM, status=None, stream=None):
    """Replace the metadata of image i by meta_src[meta_offs[i]:+meta_lens[i]]
    (cio_file_write_metadata_batch_dev): the content moves inside the image by
    the difference of the lengths, bytes 22..23 take the new length, and with
    CIO_CHECKSUM crc_cur is recomputed in place over the new layout.  writer: a
    DevWriter(..., move=True).  An entry whose new layout does not fit its
    capacity is refused (status CIO_ERROR, nothing changed).  Returns the
    status cuda tensor (int32) without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_write_metadata_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n,
        _ptr(meta_src), meta_src.numel() * meta_src.element_size(), _ptr(meta_offs), _ptr(meta_lens), int(flags),
        _ptr(crc_cur), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_write_metadata_batch_dev")
    return status[:n]


def write_at_batch_dev(writer, base, img_offs, img_caps, at_offs, src, src_offs, src_lens, crc_cur,
                       flags=CIO_CHECKSUM, status=None, stream=None):
    """Cut the content of image i to at_offs[i] bytes and append record i,
    src[src_offs[i]:+src_lens[i]], there (cio_file_write_at_batch_dev); with
    CIO_CHECKSUM crc_cur is recomputed over the kept prefix and chained over
    the record.  at_offs[i] beyond the content is refused; a record of length
    0 is a no-op.  Returns the status cuda tensor (int32) without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_write_at_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n,
        _ptr(at_offs), _ptr(src), src.numel() * src.element_size(), _ptr(src_offs), _ptr(src_lens), int(flags),
        _ptr(crc_cur), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_write_at_batch_dev")
    return status[:n]


def write_records_batch_dev(writer, base, img_offs, img_caps, src, rec_img, rec_offs, rec_lens, crc_cur,
                            flags=CIO_CHECKSUM, img_status=None, rec_status=None, stream=None):
    """Append record r, src[rec_offs[r]:+rec_lens[r]], to image rec_img[r]
    (cio_file_write_records_batch_dev): many records per image in one call.
    rec_img (int32 cuda tensor holding uint32 indices) must be non-decreasing:
    the records of an image form one run and are appended in that order; a
    malformed grouping rejects the whole batch.  The accepted records of a run
    are exactly those before the first rejected one.  crc_cur (int32 cuda
    tensor of n_img) is updated in place when flags has CIO_CHECKSUM.  Returns
    (img_status, rec_status) int32 cuda tensors without waiting; pass them in
    to reuse them (under graph capture)."""
    from .crc32 import _ptr, _stream_ptr
    n_img, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    img_status = _status_out(img_status, n_img, base.device)
    rec_status = _status_out(rec_status, n_rec, base.device)
    rc = _lib.lib().cio_file_write_records_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n_img,
        _ptr(src), src.numel() * src.element_size(), _ptr(rec_img), _ptr(rec_offs), _ptr(rec_lens), n_rec,
        int(flags), _ptr(crc_cur), _ptr(img_status), _ptr(rec_status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_write_records_batch_dev")
    return img_status[:n_img], rec_status[:n_rec]


def write_records_ungrouped_batch_dev(writer, base, img_offs, img_caps, src, rec_img, rec_offs, rec_lens, crc_cur,
                                      flags=CIO_CHECKSUM, img_status=None, rec_status=None, order=None,
                                      stream=None):
    """Append record r, src[rec_offs[r]:+rec_lens[r]], to image rec_img[r]
    (cio_file_write_records_ungrouped_batch_dev): write_records_batch_dev for
    rec_img in ANY order.  The list is sorted by image on the device, stably:
    the records of an image are appended in the order in which they appear in
    the list, and rec_status[r] belongs to record r of the list as given.  Only
    an index >= n_img is malformed and rejects the whole batch.  order: an
    optional int32 cuda tensor of n_rec; order[j] becomes the caller's index of
    the j-th record of the grouped list (the stable argsort of rec_img).
    Returns (img_status, rec_status) int32 cuda tensors without waiting; pass
    them in to reuse them (under graph capture)."""
    from .crc32 import _ptr, _stream_ptr
    n_img, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    if order is not None and (order.element_size() != 4 or order.numel() < n_rec):
        raise ValueError("order must be a 32-bit tensor of n_rec elements")
    img_status = _status_out(img_status, n_img, base.device)
    rec_status = _status_out(rec_status, n_rec, base.device)
    rc = _lib.lib().cio_file_write_records_ungrouped_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n_img,
        _ptr(src), src.numel() * src.element_size(), _ptr(rec_img), _ptr(rec_offs), _ptr(rec_lens), n_rec,
        int(flags), _ptr(crc_cur), _ptr(img_status), _ptr(rec_status), _ptr(order), _stream_ptr(stream))
    _lib.check(rc, "cio_file_write_records_ungrouped_batch_dev")
    return img_status[:n_img], rec_status[:n_rec]


def _grow_outs(n, dev, total, status):
    import torch
    if total is None:
        total = torch.zeros(1, dtype=torch.int64, device=dev)
    return total, _status_out(status, n, dev)


def grow_batch_dev(writer, base, img_offs, img_caps, need, arena, realloc=32768, page=4096, align=16, flags=0,
                   prev_offs=None, prev_caps=None, total=None, status=None, stream=None):
    """Grow the images that lack room for need[i] more content bytes
    (cio_file_grow_batch_dev), queued ahead of an append: such an image gets a
    slot of the reference's new capacity (cap + k * realloc, rounded up to
    page) out of the arena, its used bytes are copied there, and img_offs[i] /
    img_caps[i] are rewritten IN PLACE.  arena: int64 cuda tensor, [0] the top
    (advanced by the call), [1] the end, offsets into base; align: the slots'
    alignment, a power of two in 1..4096; flags: 0 or CIOA_GROW_ZERO (zero the
    new slot behind the used bytes); prev_offs / prev_caps: optional int64
    cuda tensors of n that receive the entry values.  Returns (status int32,
    total int64[1]) cuda tensors without waiting: total[0] is what the arena
    would have to hold for all of them, whether or not it does."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    total, status = _grow_outs(n, base.device, total, status)
    rc = _lib.lib().cio_file_grow_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(need), _ptr(arena),
        int(realloc), int(page), int(align), int(flags), _ptr(prev_offs), _ptr(prev_caps), _ptr(total),
        _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_grow_batch_dev")
    return status[:n], total


def grow_records_batch_dev(writer, base, img_offs, img_caps, rec_img, rec_lens, arena, realloc=32768, page=4096,
                           align=16, flags=0, prev_offs=None, prev_caps=None, total=None, status=None, stream=None):
    """grow_batch_dev ahead of write_records_batch_dev or its ungrouped form
    (cio_file_grow_records_batch_dev): the need of image i is the sum of the
    lengths rec_lens[r] of the records with rec_img[r] == i, in any order,
    summed on the device.  An index >= n rejects the whole call."""
    from .crc32 import _ptr, _stream_ptr
    n, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    total, status = _grow_outs(n, base.device, total, status)
    rc = _lib.lib().cio_file_grow_records_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(rec_img),
        _ptr(rec_lens), n_rec, _ptr(arena), int(realloc), int(page), int(align), int(flags), _ptr(prev_offs),
        _ptr(prev_caps), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_grow_records_batch_dev")
    return status[:n], total


def _rotate_outs(n, dev, out_offs, out_caps, out_img, out_count, total, status):
    import torch
    if out_count is None:
        out_count = torch.tensor([0, max(n, 1)], dtype=torch.int64, device=dev)
    if out_offs is None:
        out_offs = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    if out_caps is None:
        out_caps = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    if out_img is None:
        out_img = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    if total is None:
        total = torch.zeros(2, dtype=torch.int64, device=dev)
    return out_offs, out_caps, out_img, out_count, total, _status_out(status, n, dev)


def rotate_batch_dev(writer, base, img_offs, img_caps, need, limit=0, new_cap=None, align=16, arena=None,
                     out_offs=None, out_caps=None, out_img=None, out_count=None, flags=CIO_CHECKSUM, crc_cur=None,
                     total=None, status=None, stream=None):
    """Finish the images that are full and open the next ones
    (cio_file_rotate_batch_dev), queued ahead of a grow and an append: an
    image with content that lacks room for need[i] more bytes, or would hold
    more than `limit` content bytes with them (limit 0: no limit), is sealed
    where it lies and entered into the list of finished chunks (out_offs,
    out_caps, out_img; out_count: int64 cuda tensor, [0] the entries in it,
    advanced by the call, [1] its capacity); a fresh image of new_cap bytes
    with the same metadata is built in a slot of the arena (int64 cuda tensor,
    [0] the top, advanced, [1] the end), and img_offs[i], img_caps[i] and
    crc_cur[i] are rewritten IN PLACE.  need: int64 cuda tensor or None (every
    need 0); flags: 0 or CIO_CHECKSUM.  The list tensors are made, for n
    entries and empty, when not given.  Returns (status int32, total int64[2],
    out_offs, out_caps, out_img, out_count) cuda tensors without waiting:
    total[0] is what the arena would have to hold for all full images and
    total[1] their number, whether or not arena and list take them."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    out_offs, out_caps, out_img, out_count, total, status = _rotate_outs(
        n, base.device, out_offs, out_caps, out_img, out_count, total, status)
    rc = _lib.lib().cio_file_rotate_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(need), int(limit),
        int(new_cap), int(align), _ptr(arena), _ptr(out_offs), _ptr(out_caps), _ptr(out_img), _ptr(out_count),
        int(flags), _ptr(crc_cur), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_rotate_batch_dev")
    return status[:n], total, out_offs, out_caps, out_img, out_count


def rotate_records_batch_dev(writer, base, img_offs, img_caps, rec_img, rec_lens, limit=0, new_cap=None, align=16,
                             arena=None, out_offs=None, out_caps=None, out_img=None, out_count=None,
                             flags=CIO_CHECKSUM, crc_cur=None, total=None, status=None, stream=None):
    """rotate_batch_dev ahead of write_records_batch_dev or its ungrouped form
    (cio_file_rotate_records_batch_dev): the need of image i is the sum of the
    lengths rec_lens[r] of the records with rec_img[r] == i, in any order,
    summed on the device.  An index >= n rejects the whole call."""
    from .crc32 import _ptr, _stream_ptr
    n, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    out_offs, out_caps, out_img, out_count, total, status = _rotate_outs(
        n, base.device, out_offs, out_caps, out_img, out_count, total, status)
    rc = _lib.lib().cio_file_rotate_records_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(rec_img),
        _ptr(rec_lens), n_rec, int(limit), int(new_cap), int(align), _ptr(arena), _ptr(out_offs), _ptr(out_caps),
        _ptr(out_img), _ptr(out_count), int(flags), _ptr(crc_cur), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_rotate_records_batch_dev")
    return status[:n], total, out_offs, out_caps, out_img, out_count


def pool_state(capacity, cls, align, device):
    """An empty pool of free slots (cio_write_dev_pool.h): (pool_offs,
    pool_caps, pool) int64 cuda tensors -- the two arrays of `capacity`
    entries and the four words [entries, capacity, cls, align]: every slot
    released into the pool has at least cls bytes at a multiple of align."""
    import torch
    offs = torch.zeros(max(int(capacity), 1), dtype=torch.int64, device=device)
    caps = torch.zeros(max(int(capacity), 1), dtype=torch.int64, device=device)
    pool = torch.tensor([0, int(capacity), int(cls), int(align)], dtype=torch.int64, device=device)
    return offs, caps, pool


def release_batch_dev(writer, base, offs, caps, pool_offs, pool_caps, pool, img=None, count=None, gate=None,
                      live_offs=None, flags=0, total=None, status=None, stream=None):
    """Give the slots of drained chunks back to a pool
    (cio_file_release_batch_dev).  offs / caps (/ img): rotate's list of
    finished chunks, or grow's prev_offs / prev_caps; count: the list's
    out_count (only the first min(n, count[0]) entries are looked at); gate:
    int32 statuses, an entry whose gate is not CIO_OK is kept (pass the packed
    read's status); live_offs: an entry whose offset equals live_offs[i] is
    kept (pass img_offs behind a grow).  A slot that passes the image check and
    fits the pool's class and alignment is pushed while the pool has room, and
    its bytes 0..1 are zeroed; flags: CIOA_RELEASE_ZERO zeroes the whole slot,
    CIOA_RELEASE_COMPACT moves the kept entries to the front of the list IN
    PLACE and sets count[0].  Returns (status int32, total int64[2]) cuda
    tensors without waiting: total[0] the entries that were releasable,
    whatever the pool's room, total[1] the entries kept."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(offs.numel())
    if img is not None and img.element_size() != 4:
        raise ValueError("img must be a 32-bit tensor")
    if total is None:
        total = torch.zeros(2, dtype=torch.int64, device=base.device)
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_release_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(offs), _ptr(caps), _ptr(img), n, _ptr(count), _ptr(gate),
        _ptr(live_offs), int(flags), _ptr(pool_offs), _ptr(pool_caps), _ptr(pool), _ptr(total), _ptr(status),
        _stream_ptr(stream))
    _lib.check(rc, "cio_file_release_batch_dev")
    return status[:n], total


def rotate_pool_batch_dev(writer, base, img_offs, img_caps, need, limit=0, new_cap=None, align=16, arena=None,
                          pool_offs=None, pool_caps=None, pool=None, out_offs=None, out_caps=None, out_img=None,
                          out_count=None, flags=CIO_CHECKSUM, crc_cur=None, total=None, status=None, stream=None):
    """rotate_batch_dev that takes the fresh slots from a pool of released
    slots before it touches the arena (cio_file_rotate_pool_batch_dev): the
    first pool[0] full images -- when the pool is sound, new_cap <= its class
    and its alignment a multiple of align -- get the pool's top entries, with
    the entry's whole capacity in img_caps[i]; the others arena slots as in
    rotate_batch_dev.  pool_offs, pool_caps, pool: from pool_state, filled by
    release_batch_dev; pool[0] is lowered by the call.  Returns what
    rotate_batch_dev returns; total[0] counts the arena bytes only."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    out_offs, out_caps, out_img, out_count, total, status = _rotate_outs(
        n, base.device, out_offs, out_caps, out_img, out_count, total, status)
    rc = _lib.lib().cio_file_rotate_pool_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(need), int(limit),
        int(new_cap), int(align), _ptr(arena), _ptr(pool_offs), _ptr(pool_caps), _ptr(pool), _ptr(out_offs),
        _ptr(out_caps), _ptr(out_img), _ptr(out_count), int(flags), _ptr(crc_cur), _ptr(total), _ptr(status),
        _stream_ptr(stream))
    _lib.check(rc, "cio_file_rotate_pool_batch_dev")
    return status[:n], total, out_offs, out_caps, out_img, out_count


def rotate_pool_records_batch_dev(writer, base, img_offs, img_caps, rec_img, rec_lens, limit=0, new_cap=None,
                                  align=16, arena=None, pool_offs=None, pool_caps=None, pool=None, out_offs=None,
                                  out_caps=None, out_img=None, out_count=None, flags=CIO_CHECKSUM, crc_cur=None,
                                  total=None, status=None, stream=None):
    """rotate_pool_batch_dev ahead of write_records_batch_dev or its ungrouped
    form (cio_file_rotate_pool_records_batch_dev): the needs are summed on the
    device from the record list, as in rotate_records_batch_dev."""
    from .crc32 import _ptr, _stream_ptr
    n, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    out_offs, out_caps, out_img, out_count, total, status = _rotate_outs(
        n, base.device, out_offs, out_caps, out_img, out_count, total, status)
    rc = _lib.lib().cio_file_rotate_pool_records_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(rec_img),
        _ptr(rec_lens), n_rec, int(limit), int(new_cap), int(align), _ptr(arena), _ptr(pool_offs), _ptr(pool_caps),
        _ptr(pool), _ptr(out_offs), _ptr(out_caps), _ptr(out_img), _ptr(out_count), int(flags), _ptr(crc_cur),
        _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_rotate_pool_records_batch_dev")
    return status[:n], total, out_offs, out_caps, out_img, out_count


def pool_set_state(classes, stride, device):
    """An empty pool set (cio_write_dev_pool_set.h).  classes: a list of 1 ..
    CIOA_POOL_SET_MAX (cls, pal) pairs, cls strictly increasing; stride: the
    entries each class's arrays hold, which is also its capacity.  Returns
    (set_offs, set_caps, set, n_cls, stride): int64 cuda tensors of n_cls *
    stride entries and of 4 * n_cls words [entries, capacity, cls, pal], and
    the two host arguments."""
    import torch
    classes = [(int(c), int(p)) for c, p in classes]
    n_cls, stride = len(classes), int(stride)
    if not 1 <= n_cls <= CIOA_POOL_SET_MAX or stride < 1:
        raise ValueError("a pool set has 1 .. 8 classes and a stride of at least 1")
    offs = torch.zeros(n_cls * stride, dtype=torch.int64, device=device)
    caps = torch.zeros(n_cls * stride, dtype=torch.int64, device=device)
    words = torch.tensor([w for c, p in classes for w in (0, stride, c, p)], dtype=torch.int64, device=device)
    return offs, caps, words, n_cls, stride


def pool_set_class(set, k):
    """Class k of a pool set as a pool of cio_write_dev_pool.h: the views
    (pool_offs, pool_caps, pool) for release_batch_dev and the
    rotate_pool_*_batch_dev calls.  set: what pool_set_state returns."""
    offs, caps, words, n_cls, stride = set
    if not 0 <= k < n_cls:
        raise IndexError("no such class")
    return offs[k * stride:(k + 1) * stride], caps[k * stride:(k + 1) * stride], words[4 * k:4 * k + 4]


def _set_args(set):
    from .crc32 import _ptr
    offs, caps, words, n_cls, stride = set
    return _ptr(offs), _ptr(caps), _ptr(words), int(n_cls), int(stride)


def release_set_batch_dev(writer, base, offs, caps, set, img=None, count=None, gate=None, live_offs=None, flags=0,
                          total=None, status=None, stream=None):
    """release_batch_dev into a pool set (cio_file_release_set_batch_dev): every
    releasable slot is filed into the largest class whose cls it reaches and
    whose alignment its offset has, while that class has room; a cut entry is
    kept and not offered to a lower class.  set: (set_offs, set_caps, set,
    n_cls, stride) as from pool_set_state.  Returns (status int32, total
    int64[2 + n_cls]) cuda tensors without waiting: total[0] the releasable
    entries, total[1] the entries kept, total[2 + k] the releasable entries of
    class k, whatever its room."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(offs.numel())
    if img is not None and img.element_size() != 4:
        raise ValueError("img must be a 32-bit tensor")
    if total is None:
        total = torch.zeros(2 + int(set[3]), dtype=torch.int64, device=base.device)
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_release_set_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(offs), _ptr(caps), _ptr(img), n, _ptr(count), _ptr(gate),
        _ptr(live_offs), int(flags), *_set_args(set), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_release_set_batch_dev")
    return status[:n], total


def grow_set_batch_dev(writer, base, img_offs, img_caps, need, arena, set, realloc=32768, page=4096, align=16,
                       flags=0, prev_offs=None, prev_caps=None, total=None, status=None, stream=None):
    """grow_batch_dev that takes the larger slots from a pool set before it
    touches the arena (cio_file_grow_set_batch_dev): an image that is to grow
    asks the smallest usable class whose cls holds its new capacity, and gets
    that class's top entry with the entry's whole capacity in img_caps[i];
    when the class is empty it gets an arena slot of the class's size, and
    without a class one of its new capacity.  set: (set_offs, set_caps, set,
    n_cls, stride) as from pool_set_state, filled by release_set_batch_dev; the
    classes' counts are lowered by the call.  Returns (status int32, total
    int64[2 + n_cls]): total[0] the arena bytes all arena-bound images would
    need, total[1] the pool entries consumed, total[2 + k] the images of class
    k."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    if total is None:
        total = torch.zeros(2 + int(set[3]), dtype=torch.int64, device=base.device)
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_grow_set_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(need), _ptr(arena),
        *_set_args(set), int(realloc), int(page), int(align), int(flags), _ptr(prev_offs), _ptr(prev_caps),
        _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_grow_set_batch_dev")
    return status[:n], total


def grow_set_records_batch_dev(writer, base, img_offs, img_caps, rec_img, rec_lens, arena, set, realloc=32768,
                               page=4096, align=16, flags=0, prev_offs=None, prev_caps=None, total=None, status=None,
                               stream=None):
    """grow_set_batch_dev ahead of write_records_batch_dev or its ungrouped form
    (cio_file_grow_set_records_batch_dev): the needs are summed on the device
    from the record list, as in grow_records_batch_dev.  An index >= n rejects
    the whole call, and no set word changes."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n, n_rec = int(img_offs.numel()), int(rec_img.numel())
    if rec_img.element_size() != 4:
        raise ValueError("rec_img must be a 32-bit tensor")
    if total is None:
        total = torch.zeros(2 + int(set[3]), dtype=torch.int64, device=base.device)
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_grow_set_records_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(rec_img),
        _ptr(rec_lens), n_rec, _ptr(arena), *_set_args(set), int(realloc), int(page), int(align), int(flags),
        _ptr(prev_offs), _ptr(prev_caps), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_grow_set_records_batch_dev")
    return status[:n], total


def coalesce_set_dev(writer, dev_bytes, set, target, align=16, flags=0, total=None, stream=None):
    """Coalesce the adjacent free slots of a pool set into slots of class
    `target` on the device (cio_file_coalesce_set_dev), and drop its
    ill-formed, duplicate and overlapping entries: the entries are sorted by
    offset, runs of neighbouring slots below the target class become slots of
    at least that class, and every class is rewritten in ascending offset --
    all or nothing.  dev_bytes: the size of the buffer the slots lie in (no
    byte of it is touched); set: (set_offs, set_caps, set, n_cls, stride) as
    from pool_set_state; align: the alignment every slot of the buffer starts
    on.  COALESCE_DRY computes the totals and changes nothing.  Returns total
    int64[5 + n_cls] without waiting: total[0] 0 done, 1 the set is unsound, 2
    a class would overflow (nothing changed); total[1] entries dropped as
    ill-formed or classless, total[2] as duplicates or overlaps; total[3] the
    groups formed, total[4] the entries they are made of; total[5 + k] the
    entries of class k afterwards."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    if total is None:
        total = torch.zeros(5 + int(set[3]), dtype=torch.int64, device=set[2].device)
    rc = _lib.lib().cio_file_coalesce_set_dev(writer._handle, int(dev_bytes), *_set_args(set), int(target),
                                              int(align), int(flags), _ptr(total), _stream_ptr(stream))
    _lib.check(rc, "cio_file_coalesce_set_dev")
    return total


def route_dir(n_img, device):
    """An unbuilt directory for n_img images (cio_route_dev.h): (dir_keys,
    dir_imgs, dir_hdr) int32 cuda tensors holding uint32 bits -- the two arrays
    of n_img words and the four header words [n_img, images that passed the
    check, 0, 0].  route_build_dev fills it."""
    import torch
    keys = torch.zeros(max(int(n_img), 1), dtype=torch.int32, device=device)
    imgs = torch.zeros(max(int(n_img), 1), dtype=torch.int32, device=device)
    hdr = torch.zeros(4, dtype=torch.int32, device=device)
    return keys, imgs, hdr


def route_build_dev(writer, base, offs, caps, dir, stream=None):
    """Build the directory of the images base[offs[i]:offs[i] + caps[i]]
    (cio_file_route_build_dev): dir = (dir_keys, dir_imgs, dir_hdr) as from
    route_dir(n, device) becomes the stable sort of (key_i, i) by key, key_i
    the raw CRC-32 state of image i's metadata -- of the empty string for an
    image that fails the image check -- and the header.  No byte of base is
    written.  Returns dir without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(offs.numel())
    keys, imgs, hdr = dir
    if min(int(keys.numel()), int(imgs.numel())) < n or keys.element_size() != 4 or imgs.element_size() != 4:
        raise ValueError("dir must hold 32-bit tensors of n_img elements")
    rc = _lib.lib().cio_file_route_build_dev(writer._handle, _ptr(base), _nbytes(base), _ptr(offs), _ptr(caps), n,
                                             _ptr(keys), _ptr(imgs), _ptr(hdr), _stream_ptr(stream))
    _lib.check(rc, "cio_file_route_build_dev")
    return dir


def route_records_batch_dev(writer, base, offs, caps, dir, tags, tag_offs, tag_lens, miss_img, gate=None,
                            miss_list=False, flags=0, stream=None):
    """Route record r to the image whose metadata equals its tag,
    tags[tag_offs[r]:+tag_lens[r]] (cio_file_route_records_batch_dev), through
    the directory dir of route_build_dev: the lowest such image i that passes
    the image check now and whose gate (int32 statuses, optional) is CIO_OK.
    rec_img[r] = i with status CIO_OK; a well-formed tag without a match gets
    miss_img and CIO_RETRY, a malformed one (longer than 65535 bytes, or
    outside tags) miss_img and CIO_ERROR.  A stale directory can only lose
    matches; one of another size makes every record CIO_ERROR.  tags: uint8
    cuda tensor, or None when every tag is empty.  miss_list: True, or an
    int32 cuda tensor of n_rec to reuse -- its first total[1] entries become
    the missed record indices in ascending order.  Returns (rec_img int32
    holding uint32 indices, rec_status int32, total int64[3]: matched, missed,
    malformed[, miss_list]) cuda tensors without waiting; rec_img is what the
    rotate, grow and append calls take."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n_img, n_rec = int(offs.numel()), int(tag_offs.numel())
    keys, imgs, hdr = dir
    dev = hdr.device
    rec_img = torch.zeros(max(n_rec, 1), dtype=torch.int32, device=dev)
    rec_status = torch.zeros(max(n_rec, 1), dtype=torch.int32, device=dev)
    total = torch.zeros(3, dtype=torch.int64, device=dev)
    want_list = miss_list is not None and miss_list is not False
    if want_list and miss_list is True:
        miss_list = torch.zeros(max(n_rec, 1), dtype=torch.int32, device=dev)
    if want_list and (miss_list.element_size() != 4 or miss_list.numel() < n_rec):
        raise ValueError("miss_list must be a 32-bit tensor of n_rec elements")
    rc = _lib.lib().cio_file_route_records_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(offs), _ptr(caps), n_img, _ptr(gate), _ptr(keys), _ptr(imgs),
        _ptr(hdr), _ptr(tags), 0 if tags is None else _nbytes(tags), _ptr(tag_offs), _ptr(tag_lens), n_rec,
        int(miss_img) & 0xffffffff, int(flags), _ptr(rec_img), _ptr(rec_status),
        _ptr(miss_list) if want_list else None, _ptr(total), _stream_ptr(stream))
    _lib.check(rc, "cio_file_route_records_batch_dev")
    out = (rec_img[:n_rec], rec_status[:n_rec], total)
    return out + (miss_list[:n_rec],) if want_list else out


def _set_or_none(set):
    return _set_args(set) if set is not None else (None, None, None, 0, 0)


def alloc_set_batch_dev(writer, base, need, arena, set=None, gate=None, align=16, flags=0, out_offs=None,
                        out_caps=None, total=None, status=None, stream=None):
    """n fresh slots of need[i] bytes each out of a pool set, then the arena
    (cio_file_alloc_set_batch_dev): entry i, when gate is None or gate[i] ==
    CIO_OK and need[i] >= 24, takes the top entry of the smallest usable class
    that holds its need, with the entry's whole capacity; when the class is
    empty an arena slot of the class's size, and without a class one of its
    need.  set: (set_offs, set_caps, set, n_cls, stride) as from
    pool_set_state, or None for the arena alone; flags: 0 or CIOA_ALLOC_ZERO
    (zero every slot taken; without it no byte of base is touched).  Returns
    (status int32, total int64[2 + n_cls], out_offs int64, out_caps int64)
    cuda tensors without waiting: an entry without a slot has out_offs -1
    (UINT64_MAX), out_caps 0 and CIO_ERROR; total as grow_set_batch_dev's."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(need.numel())
    dev = base.device
    if total is None:
        total = torch.zeros(2 + (int(set[3]) if set is not None else 0), dtype=torch.int64, device=dev)
    status = _status_out(status, n, dev)
    out_offs, out_caps = _u64_out(out_offs, n, dev), _u64_out(out_caps, n, dev)
    rc = _lib.lib().cio_file_alloc_set_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(need), _ptr(gate), n, _ptr(arena), *_set_or_none(set),
        int(align), int(flags), _ptr(out_offs), _ptr(out_caps), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_alloc_set_batch_dev")
    return status[:n], total, out_offs[:n], out_caps[:n]


def persist_round_max(stage_bytes):
    """The largest file (load) or image (store) a stage of stage_bytes takes
    (cio_file_persist_round_max)."""
    return int(_lib.lib().cio_file_persist_round_max(int(stage_bytes)))


def persist_rounds(sizes, stage_bytes):
    """How load_paths_dev and store_paths_dev cut files of these sizes into
    rounds of the stage (cio_file_persist_rounds).  Returns (rounds, round_of
    uint32 array): round_of[i] is 0xffffffff for a file larger than
    persist_round_max(stage_bytes)."""
    sizes = np.ascontiguousarray(sizes, dtype=np.uint64)
    round_of = np.zeros(max(len(sizes), 1), np.uint32)
    rc = _lib.lib().cio_file_persist_rounds(sizes.ctypes.data, len(sizes), int(stage_bytes), round_of.ctypes.data)
    if rc < 0:
        _lib.check(rc, "cio_file_persist_rounds")
    return rc, round_of[:len(sizes)]


def persist_trim():
    """Free the pinned staging and the device scratch that load_paths_dev and
    store_paths_dev keep between calls (cio_file_persist_trim)."""
    _lib.lib().cio_file_persist_trim()


def _paths(paths):
    return (ctypes.c_char_p * max(len(paths), 1))(*[os.fsencode(p) for p in paths])


def load_paths_dev(writer, base, paths, stage, arena, set=None, flags=CIO_CHECKSUM, align=16, img_offs=None,
                   img_caps=None, crc_cur=None, dev_status=None, stream=None):
    """Chunk files into device memory, cio_chunk_up for a batch
    (cio_file_load_paths_dev): the files are read in rounds of the stage (a
    uint8 cuda tensor), verified there, given slots of their file sizes out of
    the set and the arena, and copied into them.  flags: 0 or CIO_CHECKSUM,
    with CIOA_LOAD_ZERO the slots' tails are zeroed.  WAITS for the work.
    Returns (status int32, error int32, fs_sizes uint64) numpy arrays and
    (img_offs int64, img_caps int64, crc_cur int32, dev_status int32) cuda
    tensors: a file that was not loaded has img_offs -1 and img_caps 0."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = len(paths)
    dev = base.device
    img_offs, img_caps = _u64_out(img_offs, n, dev), _u64_out(img_caps, n, dev)
    if crc_cur is None:
        crc_cur = torch.zeros(max(n, 1), dtype=torch.int32, device=dev)
    dev_status = _status_out(dev_status, n, dev)
    st, er = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    fs = np.zeros(max(n, 1), np.uint64)
    rc = _lib.lib().cio_file_load_paths_dev(
        writer._handle, _ptr(base), _nbytes(base), ctypes.cast(_paths(paths), ctypes.c_void_p), n, int(flags),
        _ptr(stage), _nbytes(stage), _ptr(arena), *_set_or_none(set), int(align), _ptr(img_offs), _ptr(img_caps),
        _ptr(crc_cur), _ptr(dev_status), st.ctypes.data, er.ctypes.data, fs.ctypes.data, _stream_ptr(stream))
    _lib.check(rc, "cio_file_load_paths_dev")
    return st[:n], er[:n], fs[:n], img_offs[:n], img_caps[:n], crc_cur[:n], dev_status[:n]


def store_paths_dev(writer, base, img_offs, img_caps, paths, stage, gate=None, flags=0, page=4096, dev_status=None,
                    stream=None):
    """Chunk images in device memory into chunk files, cio_file_sync +
    cio_chunk_down for a batch (cio_file_store_paths_dev): file i holds image
    i's used bytes followed by zeros up to img_caps[i], or with
    CIOA_STORE_TRIM up to the used bytes rounded up to page (1: exact).  No CRC
    is computed: seal and verify_batch_dev ahead, and pass verify's status as
    gate.  A rejected image creates no file.  CIOA_STORE_SYNC: fdatasync.
    WAITS for the work.  Returns (status int32, file_sizes uint64) numpy arrays
    and dev_status, the int32 cuda tensor release_set_batch_dev takes as its
    gate."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    if len(paths) != n:
        raise ValueError("one path per image")
    dev_status = _status_out(dev_status, n, base.device)
    st, fs = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.uint64)
    rc = _lib.lib().cio_file_store_paths_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(gate),
        ctypes.cast(_paths(paths), ctypes.c_void_p), int(flags), int(page), _ptr(stage), _nbytes(stage),
        st.ctypes.data, fs.ctypes.data, _ptr(dev_status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_store_paths_dev")
    return st[:n], fs[:n], dev_status[:n]


def tx_state(n, device):
    """The transaction state of n images (cio_dev_tx_state, 16 bytes each): an
    int32 cuda tensor of shape (n, 4) -- active, content_len, crc, meta_len --
    zeroed: no transaction active."""
    import torch
    return torch.zeros((max(int(n), 1), 4), dtype=torch.int32, device=device)[:int(n)]


def tx_begin_batch_dev(writer, base, img_offs, img_caps, tx, crc_cur=None, flags=CIO_CHECKSUM, status=None,
                       stream=None):
    """Begin a transaction on every image (cio_file_tx_begin_batch_dev): entry
    i of tx (from tx_state) takes the image's content and metadata lengths and,
    with CIO_CHECKSUM, crc_cur[i]; an entry that is already active is left
    alone.  No image byte is written.  Returns the status cuda tensor (int32)
    without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_tx_begin_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, int(flags), _ptr(crc_cur),
        _ptr(tx), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_tx_begin_batch_dev")
    return status[:n]


def tx_rollback_batch_dev(writer, base, img_offs, img_caps, tx, crc_cur=None, cond=None, flags=CIO_CHECKSUM,
                          status=None, stream=None):
    """Roll the images back to where they were at tx_begin_batch_dev
    (cio_file_tx_rollback_batch_dev): the content length and, with
    CIO_CHECKSUM, crc_cur and the header's CRC bytes.  cond: optional int32
    cuda tensor of n; entries with cond[i] == CIO_OK are skipped.  flags: 0,
    CIO_CHECKSUM, with it CIOA_TX_RECOMPUTE (crc_cur is recomputed from the
    image: needed after write_at or a metadata rewrite inside the
    transaction), and CIOA_TX_ZERO (the dropped bytes become zero).  An entry
    that is not active, or whose image shrank inside the transaction, gets
    CIO_ERROR.  Returns the status cuda tensor (int32) without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_tx_rollback_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(cond), int(flags),
        _ptr(crc_cur), _ptr(tx), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_tx_rollback_batch_dev")
    return status[:n]


def tx_commit_batch_dev(writer, base, img_offs, img_caps, tx, crc_cur=None, cond=None, flags=CIO_CHECKSUM,
                        status=None, stream=None):
    """Commit the images (cio_file_tx_commit_batch_dev): with CIO_CHECKSUM
    they are sealed as seal_batch_dev does it, and their entries of tx become
    inactive.  cond: optional int32 cuda tensor of n; only entries with cond[i]
    == CIO_OK are acted on, so the same cond given to tx_rollback_batch_dev and
    to this call handles every image exactly once.  Returns the status cuda
    tensor (int32) without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_tx_commit_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(cond), int(flags),
        _ptr(crc_cur), _ptr(tx), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_tx_commit_batch_dev")
    return status[:n]


def tx_cond_records_batch_dev(rec_img, rec_status, n_img, img_status=None, cond=None, stream=None):
    """The per-image condition of an all-or-nothing append
    (cio_file_tx_cond_records_batch_dev): cond[i] is CIO_ERROR iff a record of
    image i has rec_status != CIO_OK or img_status[i] != CIO_OK, for records in
    any order; an index >= n_img makes every entry CIO_ERROR.  rec_img,
    rec_status: 32-bit cuda tensors (or None: no records).  Returns the cond
    cuda tensor (int32 of n_img) without waiting; pass `cond` to reuse one."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n_img = int(n_img)
    n_rec = 0 if rec_img is None else int(rec_img.numel())
    if n_rec and (rec_img.element_size() != 4 or rec_status.element_size() != 4 or rec_status.numel() < n_rec):
        raise ValueError("rec_img and rec_status must be 32-bit tensors of n_rec elements")
    if cond is None:
        dev = rec_img.device if rec_img is not None else img_status.device
        cond = torch.zeros(max(n_img, 1), dtype=torch.int32, device=dev)
    rc = _lib.lib().cio_file_tx_cond_records_batch_dev(_ptr(rec_img), _ptr(rec_status), n_rec, _ptr(img_status),
                                                       n_img, _ptr(cond), _stream_ptr(stream))
    _lib.check(rc, "cio_file_tx_cond_records_batch_dev")
    return cond[:n_img]


def seal_batch_dev(writer, base, img_offs, img_caps, crc_cur, flags=CIO_CHECKSUM, status=None, stream=None):
    """Seal the images (cio_file_seal_batch_dev): the finalized CRC goes into
    bytes 2..9; with CIOA_SEAL_RECOMPUTE crc_cur is first recomputed from the
    image.  Returns the status cuda tensor (int32) without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    rc = _lib.lib().cio_file_seal_batch_dev(
        writer._handle, _ptr(base), base.numel() * base.element_size(), _ptr(img_offs), _ptr(img_caps), n,
        int(flags), _ptr(crc_cur), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_seal_batch_dev")
    return status[:n]


def _u64_out(t, n, dev):
    import torch
    if t is None:
        t = torch.zeros(max(n, 1), dtype=torch.int64, device=dev)
    return t


def _nbytes(t):
    return 0 if t is None else t.numel() * t.element_size()


def read_batch_dev(writer, base, img_offs, img_caps, what, out, out_offs=None, out_caps=None, gate=None, flags=0,
                   out_lens=None, status=None, stream=None, out_bytes=None):
    """Read record `what` (CIOA_READ_META / _CONTENT / _IMAGE) of image i into
    out[out_offs[i]:+out_caps[i]] (cio_file_read_batch_dev).  out: uint8 cuda
    tensor, or None for a size query (out_offs / out_caps are then not needed);
    gate: int32 cuda tensor, entry i is read only when gate[i] == CIO_OK (the
    status of a verify_batch_dev queued ahead); flags: 0 or CIOA_READ_NUL;
    out_bytes: defaults to out's size.  The lengths are read from the images on
    the device.  Returns (status int32, out_lens int64) cuda tensors without
    waiting; pass `status` / `out_lens` to reuse them (under graph capture)."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    out_lens = _u64_out(out_lens, n, base.device)
    rc = _lib.lib().cio_file_read_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, int(what), _ptr(gate),
        _ptr(out), _nbytes(out) if out_bytes is None else int(out_bytes), _ptr(out_offs), _ptr(out_caps),
        int(flags), _ptr(out_lens), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_read_batch_dev")
    return status[:n], out_lens[:n]


def read_packed_batch_dev(writer, base, img_offs, img_caps, what, out, align=1, gate=None, flags=0, out_offs=None,
                          out_lens=None, total=None, status=None, stream=None, out_bytes=None):
    """Read record `what` of every image into `out`, packed in index order at
    places computed on the device (cio_file_read_packed_batch_dev): slot i is
    the record (and its terminator with CIOA_READ_NUL) rounded up to `align`, a
    power of two in 1..4096; a rejected entry has no slot.  out = None is a
    size query: the placement as if `out` were unbounded.  Returns (status
    int32, out_offs int64, out_lens int64, total int64[1]) cuda tensors without
    waiting; total[0] is the sum of all slots whether or not it fits."""
    import torch
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    out_offs = _u64_out(out_offs, n, base.device)
    out_lens = _u64_out(out_lens, n, base.device)
    if total is None:
        total = torch.zeros(1, dtype=torch.int64, device=base.device)
    rc = _lib.lib().cio_file_read_packed_batch_dev(
        writer._handle, _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, int(what), _ptr(gate),
        _ptr(out), _nbytes(out) if out_bytes is None else int(out_bytes), int(align), int(flags), _ptr(out_offs),
        _ptr(out_lens), _ptr(total), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_file_read_packed_batch_dev")
    return status[:n], out_offs[:n], out_lens[:n], total


def meta_cmp_batch_dev(base, img_offs, img_caps, cand, cand_offs, cand_lens, result=None, status=None, stream=None):
    """cio_meta_cmp of image i's metadata against cand[cand_offs[i]:
    +cand_lens[i]] (cio_meta_cmp_batch_dev).  Returns (result int32: 0 equal,
    -1 not; status int32) cuda tensors without waiting."""
    from .crc32 import _ptr, _stream_ptr
    n = int(img_offs.numel())
    status = _status_out(status, n, base.device)
    result = _status_out(result, n, base.device)
    rc = _lib.lib().cio_meta_cmp_batch_dev(
        _ptr(base), _nbytes(base), _ptr(img_offs), _ptr(img_caps), n, _ptr(cand), _nbytes(cand), _ptr(cand_offs),
        _ptr(cand_lens), _ptr(result), _ptr(status), _stream_ptr(stream))
    _lib.check(rc, "cio_meta_cmp_batch_dev")
    return result[:n], status[:n]


class Context:
    """cio_ctx: a root directory of streams of chunk files."""

    def __init__(self, root, flags=CIO_CHECKSUM, devices=None, max_chunks_up=None):
        self._lib = _bind()
        self.root = root
        self._h = self._lib.cioa_create(os.fsencode(root), flags)
        if not self._h:
            raise OSError(f"cioa_create({root!r}) failed")
        if devices:
            dv, nd = _devs(devices)
            self._lib.cioa_set_devices(self._h, dv, nd)
        if max_chunks_up is not None:
            self._lib.cioa_set_max_chunks_up(self._h, int(max_chunks_up))
        self._chunks = []

    def stream(self, name):
        h = self._lib.cioa_stream_get(self._h, name.encode()) or self._lib.cioa_stream_create(self._h, name.encode())
        if not h:
            raise OSError(f"cannot create stream {name!r}")
        return Stream(self, h, name)

    def scan(self, stream, ext=None):
        """Load a stream directory (one batched GPU verify): (Stream, [Chunk])."""
        h = self._lib.cioa_scan_stream(self._h, stream.encode(), ext.encode() if ext else None)
        if not h:
            raise OSError(f"cannot scan stream {stream!r}")
        st = Stream(self, h, stream)
        return st, st.chunks()

    def scan_all(self, ext=None):
        """cioa_scan_streams: load every stream directory of the root (the
        verifies of all streams batched together): {stream name: [Chunk]}."""
        if self._lib.cioa_scan_streams(self._h, ext.encode() if ext else None) != 0:
            raise OSError("cannot scan the root")
        out = {}
        for name in sorted(os.listdir(self.root)):
            h = self._lib.cioa_stream_get(self._h, name.encode())
            if h:
                out[name] = Stream(self, h, name).chunks()
        return out

    def dump(self):
        """The `tools/cio -l` listing of every stream (cioa_scan_dump), as text."""
        import tempfile
        libc = ctypes.CDLL(None)
        libc.fopen.restype = ctypes.c_void_p
        libc.fopen.argtypes = [ctypes.c_char_p, ctypes.c_char_p]
        libc.fclose.argtypes = [ctypes.c_void_p]
        with tempfile.NamedTemporaryFile(prefix="cioa-dump-") as tf:
            fp = libc.fopen(tf.name.encode(), b"w")
            if not fp:
                raise OSError("fopen failed")
            try:
                rc = self._lib.cioa_scan_dump(self._h, fp)
            finally:
                libc.fclose(fp)
            if rc != 0:
                raise OSError("cioa_scan_dump failed")
            with open(tf.name, "r") as f:
                return f.read()

    @property
    def last_chunk_error(self):
        return int(self._lib.cioa_last_chunk_error(self._h))

    @property
    def total_chunks_up(self):
        return int(self._lib.cioa_total_chunks_up(self._h))

    def close(self):
        if self._h:
            for c in self._chunks:
                c._h = None
            self._lib.cioa_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


class Stream:
    def __init__(self, ctx, h, name):
        self.ctx, self._h, self.name = ctx, h, name

    def open(self, name, flags=CIO_OPEN, size=0):
        """(Chunk or None, err)."""
        err = ctypes.c_int(0)
        h = self.ctx._lib.cioa_chunk_open(self.ctx._h, self._h, name.encode(), flags, size, ctypes.byref(err))
        if not h:
            return None, int(err.value)
        c = Chunk(self.ctx, h)
        self.ctx._chunks.append(c)
        return c, CIO_OK

    def chunks(self):
        lib = self.ctx._lib
        n = int(lib.cioa_stream_chunks(self._h, None, 0))
        arr = (ctypes.c_void_p * max(n, 1))()
        lib.cioa_stream_chunks(self._h, arr, n)
        known = {c._h: c for c in self.ctx._chunks if c._h}
        out = []
        for i in range(n):
            c = known.get(arr[i])
            if c is None:
                c = Chunk(self.ctx, arr[i])
                self.ctx._chunks.append(c)
            out.append(c)
        return out

    def size_chunks_up(self):
        return int(self.ctx._lib.cioa_stream_size_chunks_up(self._h))

    def close_chunks(self):
        """cioa_chunk_close_stream: close every chunk of the stream (files kept)."""
        chunks = self.chunks()
        self.ctx._lib.cioa_chunk_close_stream(self._h)
        for c in chunks:
            c._h = None


class Chunk:
    """cio_chunk over the C layer."""

    def __init__(self, ctx, h):
        self.ctx, self._h, self._lib = ctx, h, ctx._lib

    def _c(self):
        if not self._h:
            raise ValueError("chunk is closed")
        return self._h

    @property
    def name(self):
        return self._lib.cioa_chunk_name(self._c()).decode()

    def write(self, data):
        b = bytes(data)
        return int(self._lib.cioa_chunk_write(self._c(), b, len(b)))

    def write_at(self, data, offset):
        b = bytes(data)
        return int(self._lib.cioa_chunk_write_at(self._c(), int(offset), b, len(b)))

    def meta_write(self, meta):
        b = bytes(meta)
        return int(self._lib.cioa_meta_write(self._c(), b, len(b)))

    write_metadata = meta_write

    def meta_len(self):
        return int(self._lib.cioa_meta_size(self._c()))

    def sync(self):
        return int(self._lib.cioa_chunk_sync(self._c()))

    def up(self):
        return int(self._lib.cioa_chunk_up(self._c()))

    def up_force(self):
        return int(self._lib.cioa_chunk_up_force(self._c()))

    def down(self):
        return int(self._lib.cioa_chunk_down(self._c()))

    def is_up(self):
        return bool(self._lib.cioa_chunk_is_up(self._c()))

    def lock(self):
        return int(self._lib.cioa_chunk_lock(self._c()))

    def unlock(self):
        return int(self._lib.cioa_chunk_unlock(self._c()))

    def tx_begin(self):
        return int(self._lib.cioa_chunk_tx_begin(self._c()))

    def tx_commit(self):
        return int(self._lib.cioa_chunk_tx_commit(self._c()))

    def tx_rollback(self):
        return int(self._lib.cioa_chunk_tx_rollback(self._c()))

    @property
    def error(self):
        return int(self._lib.cioa_error_get(self._c()))

    @property
    def data_size(self):
        return int(self._lib.cioa_chunk_get_content_size(self._c()))

    @property
    def content_end_pos(self):
        return int(self._lib.cioa_chunk_get_content_end_pos(self._c()))

    def is_file(self):
        return bool(self._lib.cioa_chunk_is_file(self._c()))

    @property
    def real_size(self):
        return int(self._lib.cioa_chunk_get_real_size(self._c()))

    @property
    def crc_cur(self):
        return int(self._lib.cioa_chunk_crc_cur(self._c()))

    @crc_cur.setter
    def crc_cur(self, v):
        self._lib.cioa_chunk_set_crc_cur(self._c(), v & 0xFFFFFFFF)

    @property
    def map(self):
        """The chunk's mapping as a ctypes byte array (None when down)."""
        size = ctypes.c_size_t(0)
        p = self._lib.cioa_chunk_map(self._c(), ctypes.byref(size))
        if not p:
            return None
        return (ctypes.c_char * size.value).from_address(p)

    @property
    def alloc_size(self):
        m = self.map
        return 0 if m is None else len(m)

    def hash(self):
        m = self.map
        return None if m is None else bytes(m[2:6])

    def content(self):
        m = self.map
        off = HDR_MIN + self.meta_len()
        return bytes(m[off:off + self.data_size])

    def close(self, delete=False):
        if self._h:
            self._lib.cioa_chunk_close(self._h, 1 if delete else 0)
            self._h = None


def up_batch(chunks, force=False):
    """cioa_chunk_up_batch / _up_force_batch: bring the chunks up with the
    outcome of chunk.up() / up_force() called on each in order, the verifies
    batched.  Returns the per-chunk statuses (list of int)."""
    if not chunks:
        return []
    lib = chunks[0]._lib
    n = len(chunks)
    arr = (ctypes.c_void_p * n)(*[c._c() for c in chunks])
    st = (ctypes.c_int * n)()
    fn = lib.cioa_chunk_up_force_batch if force else lib.cioa_chunk_up_batch
    fn(arr, n, st)
    return list(st)


def sync_batch(chunks):
    """cioa_chunk_sync_batch: every chunk's deferred CRC in ONE GPU pass."""
    chunks = [c for c in chunks if c is not None]
    if not chunks:
        return CIO_OK
    lib = _bind()
    arr = (ctypes.c_void_p * len(chunks))(*[c._c() for c in chunks])
    return int(lib.cioa_chunk_sync_batch(arr, len(chunks)))


class SyncJob:
    """A begun batch sync (cioa_chunk_sync_batch_begin); end() returns what
    sync_batch would have.  Ended on garbage collection if never ended."""

    def __init__(self, lib, handle):
        self._lib, self._h = lib, handle

    def end(self):
        if not self._h:
            raise ValueError("SyncJob already ended")
        h, self._h = self._h, None
        return int(self._lib.cioa_chunk_sync_batch_end(h))

    def __del__(self):
        if getattr(self, "_h", None):
            self.end()


def sync_batch_begin(chunks):
    """cioa_chunk_sync_batch_begin: the batch's CRC pass starts on a thread of
    its own; SyncJob.end() waits for it and writes the headers.  Writing,
    syncing, a transaction, down or close of one of the chunks ends the batch
    first."""
    chunks = [c for c in chunks if c is not None]
    lib = _bind()
    arr = (ctypes.c_void_p * max(1, len(chunks)))(*[c._c() for c in chunks])
    job = ctypes.c_void_p()
    if lib.cioa_chunk_sync_batch_begin(arr, len(chunks), ctypes.byref(job)) != CIO_OK:
        raise MemoryError("cioa_chunk_sync_batch_begin")
    return SyncJob(lib, job.value)


class ChunkFile(Chunk):
    """One chunk addressed by its path (root/stream/name), in a private context."""

    @classmethod
    def open(cls, path, flags=CIO_OPEN | CIO_CHECKSUM, deferred_crc=False, ctx_flags=0):
        path = os.path.abspath(path)
        stream_dir = os.path.dirname(path)
        root, stream, name = os.path.dirname(stream_dir), os.path.basename(stream_dir), os.path.basename(path)
        cflags = (flags & (CIO_CHECKSUM | CIO_FULL_SYNC | CIO_TRIM_FILES)) | ctx_flags
        if deferred_crc:
            cflags |= CIOA_DEFERRED_CRC
        ctx = Context(root, cflags | (flags & (CIO_OPEN | CIO_OPEN_RD)))
        st = ctx.stream(stream)
        c, err = st.open(name, (flags & (CIO_OPEN | CIO_OPEN_RD)) or CIO_OPEN)
        if c is None:
            cf = cls.__new__(cls)
            cf.ctx, cf._h, cf._lib, cf.path = ctx, None, ctx._lib, path
            cf._open_error = ctx.last_chunk_error
            return cf, err
        cf = cls(ctx, c._h)
        ctx._chunks[-1] = cf
        cf.path = path
        return cf, CIO_OK

    @property
    def error(self):
        if not self._h:
            return getattr(self, "_open_error", 0)
        return super().error

    def close(self, delete=False):
        super().close(delete)
        self.ctx.close()


def perf_write(root, data, files=1000, writes=5, batch=100, flags=CIO_CHECKSUM | CIOA_DEFERRED_CRC):
    """BASELINE config 1's loop through the C layer (cioa_bench_perf_write):
    (seconds, bytes)."""
    lib = _bind()
    buf = np.frombuffer(bytes(data), np.uint8)
    secs, nb = ctypes.c_double(0), ctypes.c_uint64(0)
    rc = lib.cioa_bench_perf_write(os.fsencode(root), buf.ctypes.data, buf.size, files, writes, batch, flags,
                                   ctypes.byref(secs), ctypes.byref(nb))
    if rc != CIO_OK:
        raise _lib.CioGpuError(f"cioa_bench_perf_write failed: {_lib.lib().cio_gpu_last_error().decode()}")
    return secs.value, int(nb.value)


def header_crc_be(path):
    with open(path, "rb") as f:
        return struct.unpack(">I", f.read(6)[2:6])[0]
