"""The numpy model of the size-classed pool set
(include/chunkio_amd/cio_write_dev_pool_set.h): the header's rules 4', 6', 7'
and S1..S8, sequentially, in Python integers, over the whole buffer, every
array and every word.  It composes the existing models: the image check,
round_up, the reference's growth rule and the saturation are the grow model's,
with no usable class m_grow_set IS grow_dev_model.m_grow, the list's compaction
is pool_dev_model.m_release's, and the steady-state chain (Steady) runs
m_rotate_pool and m_write between them.  The GPU tests compare every output of
the device calls with it."""
import numpy as np

from grow_dev_model import ERR, GROW_ZERO, HDR, MAX_CONTENT, OK, OVER  # noqa: F401
from grow_dev_model import image_check, m_grow, needs_of, new_capacity, round_up  # noqa: F401
from pool_dev_model import CK, COMPACT, NO_IMAGE, ZERO, m_release, m_rotate_pool, pool_sound  # noqa: F401
from write_dev_move_model import m_init, m_write

SET_MAX = 8                                   # CIOA_POOL_SET_MAX


def set_sound(words, n_cls, stride):
    """Every class sound, no capacity above the stride, cls strictly rising."""
    below = None
    for k in range(n_cls):
        count, cap, cls, pal = (int(x) for x in words[4 * k:4 * k + 4])
        if not pool_sound((count, cap, cls, pal)) or cap > stride or (below is not None and cls <= below):
            return False
        below = cls
    return True


def m_release_set(buf, offs, caps, img, count, gate, live, flags, set_offs, set_caps, words, n_cls, stride,
                  dev_bytes=None):
    """One cio_file_release_set_batch_dev.  buf, offs, caps, img, count as in
    m_release; set_offs, set_caps (lists of n_cls * stride ints) and words (4 *
    n_cls ints) are changed IN PLACE.  Returns (status int32, [reach, kept,
    reach of class 0, ...], accepted indices)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    m = n if count is None else min(n, int(count[0]))
    status = np.zeros(n, np.int32)
    sound = set_sound(words, n_cls, stride)
    reach = []                                # (i, class)
    for i in range(m):
        off, cap = int(offs[i]), int(caps[i])
        if live is not None and int(live[i]) == off:
            continue
        if gate is not None and int(gate[i]) != OK:
            status[i] = ERR
            continue
        k = None
        if sound and image_check(buf, dev_bytes, off, cap) is not None:
            for c in range(n_cls):
                if int(words[4 * c + 2]) <= cap and off % int(words[4 * c + 3]) == 0:
                    k = c
        if k is None:
            status[i] = ERR
            continue
        reach.append((i, k))
    seen, accepted = [0] * n_cls, []
    for i, k in reach:
        j, have, room = seen[k], int(words[4 * k]), int(words[4 * k + 1])
        seen[k] += 1
        if have + j < room:
            off, cap = int(offs[i]), int(caps[i])
            set_offs[k * stride + have + j], set_caps[k * stride + have + j] = off, cap
            buf[off:off + 2] = 0
            if flags & ZERO:
                buf[off:off + cap] = 0
            accepted.append(i)
        else:
            status[i] = ERR
    for k in range(n_cls):                    # seen[k] is 0 in an unsound set
        words[4 * k] = int(words[4 * k]) + min(seen[k], max(0, int(words[4 * k + 1]) - int(words[4 * k])))
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
    return status, [len(reach), len(kept)] + seen, accepted


def m_grow_set(buf, offs, caps, need, arena, set_offs, set_caps, words, n_cls, stride, realloc=32768, page=4096,
               align=16, flags=0, dev_bytes=None):
    """One cio_file_grow_set_batch_dev.  buf, offs, caps and arena as in
    m_grow; words[4k] is changed IN PLACE; need = None is the records variant's
    malformed list.  Returns (status int32, [arena bytes, consumed, images of
    class 0, ...], prev_offs, prev_caps, the indices served from the pool)."""
    n = len(offs)
    dev_bytes = len(buf) if dev_bytes is None else dev_bytes
    sound = set_sound(words, n_cls, stride)
    usable = [sound and int(words[4 * k + 3]) % align == 0 for k in range(n_cls)]
    if need is None or not any(usable):       # S8: the plain grow, output for output
        st, total, po, pc = m_grow(buf, offs, caps, need, arena, realloc=realloc, page=page, align=align,
                                   flags=flags, dev_bytes=dev_bytes)
        return st, [total, 0] + [0] * n_cls, po, pc, []
    prev_offs = np.asarray([int(x) for x in offs], np.uint64)
    prev_caps = np.asarray([int(x) for x in caps], np.uint64)
    status = np.zeros(n, np.int32)
    top, end = int(arena[0]), int(arena[1])
    plan = [None] * n                         # (used, new_cap) of an image that reaches rule 4, as in m_grow
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
    F = [int(words[4 * k]) if usable[k] else 0 for k in range(n_cls)]
    seen = [0] * n_cls
    base = min(round_up(top, align), OVER)
    run, new_top, moves, served = 0, top, [], []
    for i in range(n):
        if plan[i] is None:
            continue
        used, ncap = plan[i]
        c = next((k for k in range(n_cls) if usable[k] and int(words[4 * k + 2]) >= ncap), None)
        if c is not None:
            j = seen[c]
            seen[c] += 1
            if j < F[c]:                      # S3: the entry, checked before a byte of it is touched
                e = c * stride + F[c] - 1 - j
                eo, ec = int(set_offs[e]), int(set_caps[e])
                if eo + ec <= dev_bytes and ec >= int(words[4 * c + 2]) and eo % align == 0:
                    moves.append((i, eo, used, ec))
                    served.append(i)
                else:
                    status[i] = ERR           # consumed
                continue
        cap = int(words[4 * c + 2]) if c is not None else ncap
        slot = min(round_up(cap, align), OVER)
        off = min(base + run, OVER)
        if end <= dev_bytes and off < OVER and off + slot < OVER and off + slot <= end:
            moves.append((i, off, used, cap))
            new_top = off + slot
        else:
            status[i] = ERR
        run = min(run + slot, OVER)
    total = 0 if run == 0 else OVER if base == OVER else min(base - top + run, OVER)
    for i, noff, used, cap in moves:
        off = int(offs[i])
        buf[noff:noff + used] = buf[off:off + used].copy()
        if flags & GROW_ZERO:
            buf[noff + used:noff + cap] = 0
        offs[i] = noff
        caps[i] = cap
    arena[0] = new_top
    taken = [min(seen[k], F[k]) for k in range(n_cls)]
    for k in range(n_cls):
        words[4 * k] = int(words[4 * k]) - taken[k]
    return status, [total, sum(taken)] + seen, prev_offs, prev_caps, served


# ---------------------------------------------------------------- the steady state

STEADY = dict(n=12, meta=3, size=300, limit=2000, new_cap=527, realloc=512, page=256, align=32,
              classes=(527, 1280, 1792, 2304), seed=1, rounds=40, stride=16, arena_room=81920, list_cap=12)


class Steady:
    """The chain rotate_pool (class 0) -> grow_set -> release_set of the
    previous slots (dev_live_offs = dev_img_offs) -> append -> verify ->
    read_packed -> release_set(ZERO | COMPACT) of the list, round by round on
    the model.  Every image appends 1 .. size bytes per round, except image k %
    n in round k, which appends 0.  plain=True runs m_grow in place of the set
    grow: the larger slots then come from the arena every time."""

    def __init__(self, plain=False, **kw):
        p = dict(STEADY, **kw)
        self.p, self.plain = p, plain
        n, align = p["n"], p["align"]
        slot = round_up(p["new_cap"], align)
        self.offs, self.caps = [2 * align + i * slot for i in range(n)], [p["new_cap"]] * n
        top = self.offs[-1] + slot
        self.arena = [top, top + p["arena_room"]]
        i = np.arange(top + p["arena_room"] + 41, dtype=np.uint64)
        self.buf = ((i * 37 + (i >> 8) * 11) % 253 + 1).astype(np.uint8)      # test_gpu_grow_dev's sentinel
        self.crc = [m_init(self.buf, self.offs[i], bytes([1 + i] * p["meta"])) for i in range(n)]
        k = p["list_cap"]
        self.lo, self.lc, self.li, self.count = [0] * k, [0] * k, [NO_IMAGE] * k, [0, k]
        self.n_cls, self.stride = len(p["classes"]), p["stride"]
        self.so, self.sc = [0] * (self.n_cls * self.stride), [0] * (self.n_cls * self.stride)
        self.words = [w for c in p["classes"] for w in (0, self.stride, c, align)]
        self.rng = np.random.default_rng(p["seed"])
        self.src_offs = np.arange(n, dtype=np.uint64) * (p["size"] + 3)
        self.wrote, self.drained = [b""] * n, [b""] * n
        self.served = [0] * self.n_cls        # images served from the pool, by class
        self.odd = 0                          # capacities seen that are no class's (the growth rule went beyond them)

    def draw(self, k):
        """Round k's lengths and source bytes."""
        p = self.p
        lens = self.rng.integers(1, p["size"] + 1, p["n"]).astype(np.uint64)
        lens[k % p["n"]] = 0
        src = np.zeros(p["n"] * (p["size"] + 3) + 16, np.uint8)
        for i in range(p["n"]):
            o, ln = int(self.src_offs[i]), int(lens[i])
            src[o:o + ln] = self.rng.integers(0, 256, ln, dtype=np.uint8)
        return lens, src

    def round(self, k):
        """Round k on the model.  Returns a dict of what every call of the
        round answers."""
        p, out = self.p, {}
        lens, src = self.draw(k)
        out["lens"], out["src"] = lens, src
        cls0 = (self.so[:self.stride], self.sc[:self.stride], self.words[:4])
        # the rotation gets NO needs: with them rotate counts an image that lacks room as full, and nothing ever grows
        out["rotate"] = m_rotate_pool(self.buf, self.offs, self.caps, [], p["limit"], p["new_cap"], p["align"],
                                      self.arena, self.lo, self.lc, self.li, self.count, cls0[0], cls0[1], cls0[2],
                                      flags=CK, crc_cur=self.crc)
        self.words[0] = cls0[2][0]
        if self.plain:
            g = m_grow(self.buf, self.offs, self.caps, lens, self.arena, realloc=p["realloc"], page=p["page"],
                       align=p["align"])
            out["grow"] = (g[0], [g[1], 0] + [0] * self.n_cls, g[2], g[3], [])
        else:
            before = list(self.caps)
            out["grow"] = m_grow_set(self.buf, self.offs, self.caps, lens, self.arena, self.so, self.sc, self.words,
                                     self.n_cls, self.stride, realloc=p["realloc"], page=p["page"], align=p["align"])
            for i in out["grow"][4]:              # an entry's class is the largest one its capacity reaches
                assert self.caps[i] > before[i]
                self.served[max(k for k, c in enumerate(p["classes"]) if c <= self.caps[i])] += 1
        self.odd += sum(1 for c in self.caps if c not in p["classes"])
        if out["rotate"][0].any() or out["grow"][0].any():     # the append behind it would be refused for room
            out["ok"] = False
            return out
        prev_o, prev_c = [int(x) for x in out["grow"][2]], [int(x) for x in out["grow"][3]]
        out["prev"] = (list(prev_o), list(prev_c))
        out["release_prev"] = m_release_set(self.buf, prev_o, prev_c, None, None, None, list(self.offs), 0, self.so,
                                            self.sc, self.words, self.n_cls, self.stride)
        for i in range(p["n"]):
            o, ln = int(self.src_offs[i]), int(lens[i])
            data = src[o:o + ln].tobytes()
            self.crc[i] = m_write(self.buf, self.offs[i], data, self.crc[i])
            self.wrote[i] += data
        m = self.count[0]
        out["listed"] = (m, list(self.lo), list(self.lc), list(self.li))
        for e in range(m):
            meta, content = image_check(self.buf, len(self.buf), self.lo[e], self.lc[e])
            self.drained[self.li[e]] += self.buf[self.lo[e] + HDR + meta:self.lo[e] + HDR + meta + content].tobytes()
        out["release_list"] = m_release_set(self.buf, self.lo, self.lc, self.li, self.count, [0] * len(self.lo), None,
                                            ZERO | COMPACT, self.so, self.sc, self.words, self.n_cls, self.stride)
        out["ok"] = not (out["release_prev"][0].any() or out["release_list"][0].any())
        return out
