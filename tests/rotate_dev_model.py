"""The numpy model of rotating full chunk images
(include/chunkio_amd/cio_write_dev_rotate.h): the header's rule, sequentially,
in Python integers, over the whole buffer, the two arrays, crc_cur, the arena
words and the list of finished chunks.  The fresh image is m_init's and the
seal m_seal's (write_dev_move_model.py); round_up, image_check and needs_of are
the grow model's.  The GPU tests compare every output of the device calls with
it."""
import numpy as np

from grow_dev_model import ERR, HDR, OK, OVER, image_check, needs_of, round_up  # noqa: F401
from write_dev_move_model import m_init, m_seal

CK = 4                                        # CIO_CHECKSUM


def m_rotate(buf, offs, caps, need, limit, new_cap, align, arena, out_offs, out_caps, out_img, out_count,
             flags=CK, crc_cur=None, dev_bytes=None):
    """One cio_file_rotate_batch_dev.  buf (uint8 array), offs, caps, crc_cur
    (lists of ints, crc_cur the raw states), arena ([top, end]), the three
    list arrays (lists of out_count[1] entries) and out_count ([entries,
    capacity]) are changed IN PLACE; need = None is the records variant's
    malformed list, need = [] every need 0.  Returns (status int32, [total
    bytes, total images], rotated indices)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    status = np.zeros(n, np.int32)
    if need is None:
        status[:] = ERR
        return status, [0, 0], []
    top, end = int(arena[0]), int(arena[1])
    have, room = int(out_count[0]), int(out_count[1])
    reach = []                                # (i, meta) of an image that reaches the placement
    for i in range(n):
        nd = int(need[i]) if len(need) else 0
        if nd == 0 and limit == 0:
            continue
        off, cap = int(offs[i]), int(caps[i])
        img = image_check(buf, dev_bytes, off, cap)
        if img is None or (top < end and cap != 0 and off < end and top < off + cap):
            status[i] = ERR
            continue
        meta, content = img
        used = HDR + meta + content
        if not (content > 0 and (used + nd > cap or (limit != 0 and content + nd > limit))):
            continue
        if HDR + meta > new_cap:
            status[i] = ERR
            continue
        reach.append((i, meta))
    base = min(round_up(top, align), OVER)
    slot = min(round_up(new_cap, align), OVER)
    rotated, cut = [], False
    for j, (i, meta) in enumerate(reach):
        noff = base + j * slot
        if cut or not (end <= dev_bytes and noff + slot < OVER and noff + slot <= end and have + j < room):
            cut = True
            status[i] = ERR
            continue
        off = int(offs[i])
        if flags & CK:
            m_seal(buf, off, int(crc_cur[i]))
        k = have + j
        out_offs[k], out_caps[k], out_img[k] = off, int(caps[i]), i
        raw = m_init(buf, noff, buf[off + HDR:off + HDR + meta].tobytes(), checksum=bool(flags & CK))
        if flags & CK:
            crc_cur[i] = raw
        offs[i], caps[i] = noff, new_cap
        rotated.append(i)
    if rotated:
        arena[0] = base + len(rotated) * slot
        out_count[0] = have + len(rotated)
    slots = min(len(reach) * slot, OVER)
    total = 0 if not reach else OVER if base == OVER else min(base - top + slots, OVER)
    return status, [total, len(reach)], rotated
