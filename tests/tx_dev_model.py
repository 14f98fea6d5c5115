"""The numpy model of transactions on chunk images
(include/chunkio_amd/cio_write_dev_tx.h): the header's rules, sequentially, in
Python integers, over the whole buffer, crc_cur and the state entries (lists of
[active, content_len, crc, meta_len]).  The seal is m_seal's, the CRC the move
model's raw_update (write_dev_move_model.py), the image check the grow model's.
Shared by test_tx_dev_abi.py (which asserts it by hand) and test_gpu_tx_dev.py
(which pins the device to it).  Not a test."""
import struct

import numpy as np

from grow_dev_model import ERR, HDR, OK, image_check
from write_dev_move_model import M32, m_seal, raw_update

CK, RECOMPUTE, ZERO = 4, 256, 512             # CIO_CHECKSUM, CIOA_TX_RECOMPUTE, CIOA_TX_ZERO


def new_state(n):
    return [[0, 0, 0, 0] for _ in range(n)]


def m_tx_begin(buf, offs, caps, tx, crc_cur=None, flags=CK, dev_bytes=None):
    """cio_file_tx_begin_batch_dev: tx is changed in place; the status."""
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    status = np.zeros(len(offs), np.int32)
    for i in range(len(offs)):
        if tx[i][0] != 0:
            continue
        img = image_check(buf, dev_bytes, int(offs[i]), int(caps[i]))
        if img is None:
            status[i] = ERR
            continue
        meta, content = img
        tx[i] = [1, content, int(crc_cur[i]) if flags & CK else 0, meta]
    return status


def m_tx_rollback(buf, offs, caps, tx, crc_cur=None, cond=None, flags=CK, dev_bytes=None):
    """cio_file_tx_rollback_batch_dev: buf, crc_cur and tx are changed in
    place; (status, indices rolled back)."""
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    status = np.zeros(len(offs), np.int32)
    rolled = []
    for i in range(len(offs)):
        if cond is not None and int(cond[i]) == OK:
            continue                                         # 1. skipped
        active, t_content, t_crc, t_meta = tx[i]
        off = int(offs[i])
        img = image_check(buf, dev_bytes, off, int(caps[i])) if active else None
        if img is None:                                      # 2., 3.
            status[i] = ERR
            continue
        meta, cur = img
        if cur < t_content or (not flags & RECOMPUTE and meta != t_meta):    # 4.
            status[i] = ERR
            continue
        buf[off + 10:off + 14] = np.frombuffer(struct.pack(">I", t_content), np.uint8)
        if flags & CK:
            raw = t_crc
            if flags & RECOMPUTE:
                raw = raw_update(M32, buf[off + 22:off + HDR + meta + t_content].tobytes())
            crc_cur[i] = raw
            buf[off + 2:off + 10] = np.frombuffer(struct.pack("<Q", raw), np.uint8)
        if flags & ZERO:
            buf[off + HDR + meta + t_content:off + HDR + meta + cur] = 0
        tx[i] = [0, t_content, t_crc, t_meta]
        rolled.append(i)
    return status, rolled


def m_tx_commit(buf, offs, caps, tx, crc_cur=None, cond=None, flags=CK, dev_bytes=None):
    """cio_file_tx_commit_batch_dev: buf and tx are changed in place; (status,
    indices committed)."""
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    status = np.zeros(len(offs), np.int32)
    done = []
    for i in range(len(offs)):
        if cond is not None and int(cond[i]) != OK:
            continue
        off = int(offs[i])
        if image_check(buf, dev_bytes, off, int(caps[i])) is None:
            status[i] = ERR
            continue
        if flags & CK:
            m_seal(buf, off, int(crc_cur[i]))
        tx[i] = [0] + list(tx[i][1:])
        done.append(i)
    return status, done


def m_tx_cond(rec_img, rec_status, n_img, img_status=None):
    """cio_file_tx_cond_records_batch_dev: the condition, int32 of n_img."""
    cond = np.zeros(n_img, np.int32)
    if img_status is not None:
        cond[np.asarray(img_status)[:n_img] != OK] = ERR
    img = np.asarray(rec_img, dtype=np.uint64)
    if len(img) == 0 or n_img == 0:
        return cond
    if (img >= n_img).any():
        cond[:] = ERR
        return cond
    cond[img[np.asarray(rec_status) != OK].astype(np.int64)] = ERR
    return cond
