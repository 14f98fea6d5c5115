"""The numpy model of growing chunk images out of an arena
(include/chunkio_amd/cio_write_dev_grow.h): the header's rule, sequentially,
in Python integers, over the whole buffer, the two arrays and the arena words.
The GPU tests compare every output of the device calls with it."""
import numpy as np

OK, ERR = 0, -1
HDR = 24
MAX_CONTENT = 0xFFFFFFFF
OVER = (1 << 64) - 1                          # a value that left 64 bits, or reached 2^64 - 1
GROW_ZERO = 1


def round_up(v, a):
    return (v + a - 1) // a * a


def new_capacity(cap, used, need, realloc, page):
    """The reference's loop (cio_file_write), as it is written there."""
    new = cap + realloc
    if realloc < (1 << 20):
        while new < used + need:
            new += realloc
    elif new < used + need:                   # the same value without a long loop
        new = cap + -(-(used + need - cap) // realloc) * realloc
    return round_up(new, page)


def image_check(buf, dev_bytes, off, cap):
    """(meta_len, content_len) of a valid image, or None: the write path's check."""
    if off + cap > dev_bytes or cap < HDR:
        return None
    if buf[off] != 0xC1 or buf[off + 1] != 0x00:
        return None
    meta = (int(buf[off + 22]) << 8) | int(buf[off + 23])
    content = int.from_bytes(bytes(buf[off + 10:off + 14]), "big")
    return (meta, content) if HDR + meta + content <= cap else None


def needs_of(rec_img, rec_lens, n):
    """The records variant's need per image, or None for a malformed list."""
    need = [0] * n
    for img, ln in zip(rec_img, rec_lens):
        if int(img) >= n:
            return None
        need[int(img)] += min(int(ln), 1 << 32)
    return need


def m_grow(buf, offs, caps, need, arena, realloc=32768, page=4096, align=16, flags=0, dev_bytes=None):
    """One cio_file_grow_batch_dev.  buf (uint8 array), offs, caps (lists or
    uint64 arrays) and arena ([top, end]) are changed IN PLACE; need = None is
    the records variant's malformed list.  Returns (status int32, total,
    prev_offs uint64, prev_caps uint64)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    prev_offs = np.asarray([int(x) for x in offs], np.uint64)
    prev_caps = np.asarray([int(x) for x in caps], np.uint64)
    status = np.zeros(n, np.int32)
    if need is None:
        status[:] = ERR
        return status, 0, prev_offs, prev_caps
    top, end = int(arena[0]), int(arena[1])
    plan = [None] * n                         # (used, new_cap) of an image that reaches rule 4
    for i in range(n):
        nd = int(need[i])
        if nd == 0:
            continue
        off, cap = int(offs[i]), int(caps[i])
        img = image_check(buf, dev_bytes, off, cap)
        if img is None or img[1] + nd > MAX_CONTENT or (top < end and off < end and top < off + cap):
            status[i] = ERR
            continue
        used = HDR + img[0] + img[1]
        if used + nd <= cap:
            continue
        ncap = new_capacity(cap, used, nd, realloc, page)
        if ncap >= OVER:
            status[i] = ERR
            continue
        plan[i] = (used, ncap)
    # sums saturate at OVER: once out of 64 bits, out for good
    base = min(round_up(top, align), OVER)
    run, new_top, moves = 0, top, []
    for i in range(n):
        if plan[i] is None:
            continue
        used, ncap = plan[i]
        slot = min(round_up(ncap, align), OVER)
        off = min(base + run, OVER)
        if end <= dev_bytes and off < OVER and off + slot < OVER and off + slot <= end:
            moves.append((i, off, used, ncap))
            new_top = off + slot
        else:
            status[i] = ERR
        run = min(run + slot, OVER)
    total = 0 if run == 0 else OVER if base == OVER else min(base - top + run, OVER)
    for i, noff, used, ncap in moves:
        off = int(offs[i])
        buf[noff:noff + used] = buf[off:off + used].copy()
        if flags & GROW_ZERO:
            buf[noff + used:noff + ncap] = 0
        offs[i] = noff
        caps[i] = ncap
    arena[0] = new_top
    return status, total, prev_offs, prev_caps
