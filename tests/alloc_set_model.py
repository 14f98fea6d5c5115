"""The numpy model of cio_file_alloc_set_batch_dev
(include/chunkio_amd/cio_persist_dev.h): rules A1..A5, sequentially, in Python
integers, over the whole buffer, every array and every word.  The placement is
the pool set's S1..S4, S6 and S7 with new_cap_i := need_i.

m_alloc_set states the rules on its own, because an allocation has no image in
front of it and so cannot be asked of pool_set_model.m_grow_set for every need
(a grow never leaves a capacity where it was, so need == 24 has no grow).  For
every need above 24 it CAN: m_alloc_via_grow builds a 24-byte image per entry
in a scratch buffer and runs pool_set_model.m_grow_set over them with realloc =
page = 1, for which the reference's growth rule gives new_cap = used + need =
24 + (need_i - 24).  tests/test_persist_abi.py holds the two to each other, so
that a divergence between "alloc with need = c" and "grow to new_cap = c"
shows."""
import numpy as np

from pool_set_model import ERR, OK, OVER, m_grow_set, round_up, set_sound
from write_dev_move_model import m_init

ALLOC_ZERO = 1
NONE = (1 << 64) - 1                          # dev_out_offs of an entry without a slot
MIN_NEED = 24


def m_alloc_set(buf, need, gate, arena, set_offs, set_caps, words, n_cls, stride, align=16, flags=0, dev_bytes=None):
    """One cio_file_alloc_set_batch_dev.  buf is changed only with ALLOC_ZERO;
    arena[0] and words[4k] are changed IN PLACE.  Returns (status int32, [arena
    bytes, consumed, entries of class 0, ...], out_offs, out_caps)."""
    n = len(need)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    sound = n_cls > 0 and set_sound(words, n_cls, stride)
    usable = [sound and int(words[4 * k + 3]) % align == 0 for k in range(n_cls)]
    F = [int(words[4 * k]) if usable[k] else 0 for k in range(n_cls)]
    seen = [0] * n_cls
    top, end = int(arena[0]), int(arena[1])
    base = min(round_up(top, align), OVER)
    status = np.full(n, ERR, np.int32)
    out_offs, out_caps = [NONE] * n, [0] * n
    run, new_top = 0, top
    for i in range(n):
        nd = int(need[i])
        if (gate is not None and int(gate[i]) != OK) or nd < MIN_NEED:
            continue
        c = next((k for k in range(n_cls) if usable[k] and int(words[4 * k + 2]) >= nd), None)
        if c is not None:
            j = seen[c]
            seen[c] += 1
            if j < F[c]:                      # S3: the entry, checked before it is handed out
                e = c * stride + F[c] - 1 - j
                eo, ec = int(set_offs[e]), int(set_caps[e])
                if eo + ec <= dev_bytes and ec >= int(words[4 * c + 2]) and eo % align == 0:
                    status[i], out_offs[i], out_caps[i] = OK, eo, ec
                continue                      # consumed either way
        cap = int(words[4 * c + 2]) if c is not None else nd
        slot = min(round_up(cap, align), OVER)
        off = min(base + run, OVER)
        if end <= dev_bytes and off < OVER and off + slot < OVER and off + slot <= end:
            status[i], out_offs[i], out_caps[i] = OK, off, cap
            new_top = off + slot
        run = min(run + slot, OVER)
    total = 0 if run == 0 else OVER if base == OVER else min(base - top + run, OVER)
    if flags & ALLOC_ZERO:
        for i in range(n):
            if status[i] == OK:
                buf[out_offs[i]:out_offs[i] + out_caps[i]] = 0
    arena[0] = new_top
    taken = [min(seen[k], F[k]) for k in range(n_cls)]
    for k in range(n_cls):
        words[4 * k] = int(words[4 * k]) - taken[k]
    return status, [total, sum(taken)] + seen, out_offs, out_caps


def m_alloc_via_grow(need, gate, arena, set_offs, set_caps, words, n_cls, stride, align, dev_bytes):
    """The same allocation asked of pool_set_model.m_grow_set, for needs that
    are below 24 (the entry does not reach) or above it: entry i is a 24-byte
    image that is to grow by need_i - 24 with realloc = page = 1.  The images
    lie in a scratch buffer BEHIND dev_bytes, so that no slot handed out can
    touch them and none lies in the arena.  m_grow_set's dev_bytes bounds the
    images, the pool entries and the arena alike, so it is the scratch
    buffer's length: the cases keep the arena's end inside the real dev_bytes
    and every pool entry inside it or beyond the scratch buffer, where both
    bounds agree.  Returns what m_alloc_set returns."""
    n = len(need)
    buf = np.zeros(dev_bytes + 24 * n, np.uint8)
    offs, caps = [dev_bytes + 24 * i for i in range(n)], [24] * n
    for o in offs:
        m_init(buf, o, b"")
    reach = [(gate is None or int(gate[i]) == OK) and int(need[i]) >= MIN_NEED for i in range(n)]
    assert all(int(need[i]) > MIN_NEED for i in range(n) if reach[i])
    assert int(arena[1]) <= dev_bytes
    for e in range(n_cls * stride):
        end = int(set_offs[e]) + int(set_caps[e])
        assert end <= dev_bytes or end > len(buf)
    nd = [int(need[i]) - 24 if reach[i] else 0 for i in range(n)]
    st, total = m_grow_set(buf, offs, caps, nd, arena, set_offs, set_caps, words, n_cls, stride, realloc=1, page=1,
                           align=align)[:2]
    status = np.full(n, ERR, np.int32)
    out_offs, out_caps = [NONE] * n, [0] * n
    for i in range(n):
        if reach[i] and st[i] == OK:
            status[i], out_offs[i], out_caps[i] = OK, int(offs[i]), int(caps[i])
    return status, total, out_offs, out_caps
