"""A model of the grouped append (include/chunkio_amd/cio_write_dev_records.h)
in plain Python over a bytearray, with zlib for the CRC: the semantics of the
header, rule by rule -- malformed grouping, the image check, room, the
per-record accounting, the prefix rule of acceptance, the effect on the image.
Per image the accounting is vectorised with numpy, so that a batch of a
million records stays a matter of seconds.  Shared by
test_write_dev_records_abi.py (which pins it to the reference-written fixtures
and to the host chunk layer) and test_gpu_write_dev_records.py (which pins the
device to it).  Not a test."""
import struct

import numpy as np

from write_dev_move_model import M32, m_init, m_seal, pattern, raw_update  # noqa: F401

OK, ERROR = 0, -1
MAX_CONTENT = 0xFFFFFFFF


def image_check(buf, off, cap):
    """(meta, content) of the image at off, or None: inside the buffer, room
    for a header, the magic, 24 + meta + content <= cap."""
    if off + cap > len(buf) or cap < 24 or buf[off] != 0xC1 or buf[off + 1] != 0x00:
        return None
    meta = struct.unpack(">H", bytes(buf[off + 22:off + 24]))[0]
    content = struct.unpack(">I", bytes(buf[off + 10:off + 14]))[0]
    return (meta, content) if 24 + meta + content <= cap else None


def m_write_records(buf, img_offs, img_caps, src, rec_img, rec_offs, rec_lens, crc_cur, checksum=True):
    """The grouped append on buf (bytearray) and crc_cur (list of raw states),
    both changed in place.  src: bytes-like; the other arguments: sequences of
    non-negative integers below 2^64.  Returns (img_status, rec_status) as
    numpy int32 arrays."""
    n_img, n_rec = len(img_offs), len(rec_img)
    img_status = np.zeros(n_img, np.int32)
    rec_status = np.full(n_rec, ERROR, np.int32)
    if n_img == 0 or n_rec == 0:
        return img_status, np.zeros(n_rec, np.int32)
    img = np.asarray(rec_img, dtype=np.uint64)
    offs = np.asarray(rec_offs, dtype=np.uint64)
    lens = np.asarray(rec_lens, dtype=np.uint64)
    # 1. malformed grouping: the whole batch
    if (img >= n_img).any() or (img[1:] < img[:-1]).any():
        img_status[:] = ERROR
        return img_status, rec_status
    # 4. what a record adds to its run's sum; `bad` stands for the saturated value
    src_len = np.uint64(len(src))
    end = offs + lens                                    # wraps like the device's
    bad = (lens != 0) & ((lens > MAX_CONTENT) | (end < offs) | (end > src_len))
    value = np.where(bad, 0, lens).astype(np.uint64)
    view = np.frombuffer(buf, np.uint8)
    source = np.frombuffer(src, np.uint8)
    starts = np.searchsorted(img, np.arange(n_img + 1, dtype=np.uint64), side="left")
    for i in range(n_img):
        a, b = int(starts[i]), int(starts[i + 1])
        if a == b:
            continue                                     # 2. no run: not read, CIO_OK
        off, cap = int(img_offs[i]), int(img_caps[i])
        geo = image_check(buf, off, cap)
        if geo is None:
            img_status[i] = ERROR
            continue
        meta, content = geo
        room = min(cap - 24 - meta - content, MAX_CONTENT - content)     # 3.
        # 5. accepted: before the first saturated record and while the inclusive sum fits; the sum is
        # monotone, so these are exactly the records before the first rejected one
        incl = np.cumsum(value[a:b], dtype=np.uint64)    # <= 2^20 values below 2^32 each in the tests
        first_bad = int(np.argmax(bad[a:b])) if bad[a:b].any() else b - a
        fits = incl <= np.uint64(room)
        n_acc = min(first_bad, int(np.argmin(fits)) if not fits.all() else b - a)
        rec_status[a:a + n_acc] = OK
        total = int(incl[n_acc - 1]) if n_acc else 0
        if total == 0:
            continue
        # 6. the accepted records back to back from the old end of the content
        ln = value[a:a + n_acc].astype(np.int64)
        excl = np.cumsum(ln) - ln
        idx = np.repeat(offs[a:a + n_acc].astype(np.int64) - excl, ln) + np.arange(total, dtype=np.int64)
        pos = off + 24 + meta + content
        appended = source[idx]
        view[pos:pos + total] = appended
        view[off + 10:off + 14] = np.frombuffer(struct.pack(">I", content + total), np.uint8)
        if checksum:
            crc_cur[i] = raw_update(crc_cur[i], appended.tobytes())
            view[off + 2:off + 10] = np.frombuffer(struct.pack("<Q", crc_cur[i]), np.uint8)
    return img_status, rec_status


def rounds(rec_img, n_img):
    """Equivalence rule 7: the record indices of round k (the k-th record of
    every image), as a list of {image: record} per round."""
    nxt = [0] * n_img
    out = []
    for r, i in enumerate(rec_img):
        k = nxt[i]
        nxt[i] += 1
        if k == len(out):
            out.append({})
        out[k][i] = r
    return out
