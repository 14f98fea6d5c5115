"""The numpy model of recycling drained chunk slots
(include/chunkio_amd/cio_write_dev_pool.h): the header's two rules,
sequentially, in Python integers, over the whole buffer, every array and every
word.  The image check, round_up and the saturation are the grow model's, the
fresh image is m_init's and the seal m_seal's (write_dev_move_model.py), and
with an empty or unusable pool m_rotate_pool is rotate_dev_model.m_rotate
output for output.  The GPU tests compare every output of the device calls
with it."""
import numpy as np

from grow_dev_model import ERR, HDR, OK, OVER, image_check, needs_of, round_up  # noqa: F401
from rotate_dev_model import CK, m_rotate  # noqa: F401
from write_dev_move_model import m_init, m_seal

ZERO, COMPACT = 1, 2                          # CIOA_RELEASE_ZERO, CIOA_RELEASE_COMPACT
NO_IMAGE = 0xFFFFFFFF                         # dev_img of a vacated list entry


def pool_sound(pool):
    count, cap, cls, pal = (int(x) for x in pool)
    return count <= cap and cls >= HDR and 1 <= pal <= 4096 and pal & (pal - 1) == 0


def m_release(buf, offs, caps, img, count, gate, live, flags, pool_offs, pool_caps, pool, dev_bytes=None):
    """One cio_file_release_batch_dev.  buf (uint8 array), offs, caps, img
    (lists of n ints; img may be None), count ([entries, capacity] or None),
    pool_offs, pool_caps (lists of pool[1] ints) and pool (the four words) are
    changed IN PLACE; gate and live are lists of n or None.  Returns (status
    int32, [reach, kept], accepted indices)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    m = n if count is None else min(n, int(count[0]))
    status = np.zeros(n, np.int32)
    sound = pool_sound(pool)
    have, room, cls, pal = (int(x) for x in pool)
    reach = []
    for i in range(m):
        off, cap = int(offs[i]), int(caps[i])
        if live is not None and int(live[i]) == off:
            continue
        if gate is not None and int(gate[i]) != OK:
            status[i] = ERR
            continue
        if not sound or image_check(buf, dev_bytes, off, cap) is None or cap < cls or off % pal:
            status[i] = ERR
            continue
        reach.append(i)
    accepted = []
    for j, i in enumerate(reach):
        if have + j < room:
            accepted.append(i)
        else:
            status[i] = ERR
    for j, i in enumerate(accepted):
        off, cap = int(offs[i]), int(caps[i])
        pool_offs[have + j], pool_caps[have + j] = off, cap
        buf[off:off + 2] = 0
        if flags & ZERO:
            buf[off:off + cap] = 0
    if accepted:
        pool[0] = have + len(accepted)
    gone = set(accepted)
    kept = [i for i in range(m) if i not in gone]
    if flags & COMPACT:
        rows = [(int(offs[i]), int(caps[i]), int(img[i]) if img is not None else 0) for i in kept]
        rows += [(0, 0, NO_IMAGE)] * (m - len(kept))
        for r, (o, c, g) in enumerate(rows):
            offs[r], caps[r] = o, c
            if img is not None:
                img[r] = g
        count[0] = len(kept)
    return status, [len(reach), len(kept)], accepted


def m_rotate_pool(buf, offs, caps, need, limit, new_cap, align, arena, out_offs, out_caps, out_img, out_count,
                  pool_offs, pool_caps, pool, flags=CK, crc_cur=None, dev_bytes=None):
    """One cio_file_rotate_pool_batch_dev: rotate_dev_model.m_rotate with the
    pool in front of the arena.  pool[0] is changed IN PLACE beside everything
    m_rotate changes.  Returns (status, [arena bytes, reach], rotated indices,
    the number of them that came from the pool)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    status = np.zeros(n, np.int32)
    if need is None:
        status[:] = ERR
        return status, [0, 0], [], 0
    top, end = int(arena[0]), int(arena[1])
    have, room = int(out_count[0]), int(out_count[1])
    pcount = int(pool[0])
    F = pcount if pool_sound(pool) and new_cap <= int(pool[2]) and int(pool[3]) % align == 0 else 0
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
    rotated, from_pool, cut = [], 0, False
    for j, (i, meta) in enumerate(reach):
        if j < F:
            noff, ncap = int(pool_offs[pcount - 1 - j]), int(pool_caps[pcount - 1 - j])
            ok = have + j < room
        else:
            noff, ncap = base + (j - F) * slot, new_cap
            ok = end <= dev_bytes and noff + slot < OVER and noff + slot <= end and have + j < room
        if cut or not ok:
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
        offs[i], caps[i] = noff, ncap
        rotated.append(i)
        from_pool += j < F
    if rotated:
        out_count[0] = have + len(rotated)
        if from_pool:
            pool[0] = pcount - from_pool
        if len(rotated) > from_pool:
            arena[0] = base + (len(rotated) - from_pool) * slot
    extra = max(0, len(reach) - F)
    slots = min(extra * slot, OVER)
    total = 0 if not extra else OVER if base == OVER else min(base - top + slots, OVER)
    return status, [total, len(reach)], rotated, from_pool
