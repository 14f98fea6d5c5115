"""A model of the ungrouped append
(include/chunkio_amd/cio_write_dev_ungrouped.h) in plain Python: a stable
argsort of the keys min(rec_img, n_img), the grouped model
(write_dev_records_model.m_write_records) over the sorted list, and the record
statuses scattered back to the caller's order.  Shared by
test_write_dev_ungrouped_abi.py (which pins it on a hand-written batch) and
test_gpu_write_dev_ungrouped.py (which pins the device to it).  Not a test."""
import numpy as np

from write_dev_records_model import m_write_records


def stable_order(rec_img, n_img):
    """The stable sort of 0 .. n_rec - 1 by min(rec_img, n_img), as uint32."""
    key = np.minimum(np.asarray(rec_img, dtype=np.uint64), np.uint64(n_img))
    return np.argsort(key, kind="stable").astype(np.uint32), key


def m_write_records_ungrouped(buf, img_offs, img_caps, src, rec_img, rec_offs, rec_lens, crc_cur, checksum=True):
    """The ungrouped append on buf (bytearray or uint8 array) and crc_cur (list
    of raw states), both changed in place.  Returns (img_status, rec_status,
    order): rec_status in the caller's order, order[j] the caller's index of the
    j-th record of the grouped list."""
    n_img, n_rec = len(img_offs), len(rec_img)
    order, key = stable_order(rec_img, n_img)
    if n_img == 0 or n_rec == 0:
        return np.zeros(n_img, np.int32), np.zeros(n_rec, np.int32), order
    offs = np.asarray(rec_offs, dtype=np.uint64)
    lens = np.asarray(rec_lens, dtype=np.uint64)
    img_status, grouped = m_write_records(buf, img_offs, img_caps, src, key[order], offs[order], lens[order],
                                          crc_cur, checksum=checksum)
    rec_status = np.empty(n_rec, np.int32)
    rec_status[order] = grouped
    return img_status, rec_status, order
