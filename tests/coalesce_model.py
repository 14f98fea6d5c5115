"""The numpy model of coalescing a pool set's free slots
(include/chunkio_amd/cio_write_dev_coalesce.h): the header's rules C0..C9,
sequentially, in Python integers, entry by entry -- no sort network, no scan,
no search: a sorted list and one walk over it.  The GPU tests compare every
word the device call writes with it.  Drift is the scenario the call exists
for: a producer whose chunks drift to a larger class, on the models of the
whole chain, with and without the call."""
import numpy as np

from pool_set_model import (ERR, HDR, OK, m_grow_set, m_release_set, m_rotate_pool, round_up,  # noqa: F401
                            set_sound)
from pool_dev_model import CK, NO_IMAGE
from write_dev_move_model import m_init, m_write

DRY = 1                                       # CIOA_COALESCE_DRY
M64 = (1 << 64) - 1


def file_class(words, n_cls, off, cap):
    """Release's rule 4': the largest k with cls_k <= cap and off a multiple of
    pal_k, or None."""
    k = None
    for c in range(n_cls):
        if int(words[4 * c + 2]) <= cap and off % int(words[4 * c + 3]) == 0:
            k = c
    return k


def survivors_of(set_offs, set_caps, words, n_cls, stride, dev_bytes, align):
    """C1 and C2 of a sound set: (the survivors [(off, cap)] in ascending off,
    the ill-formed entries, the collisions)."""
    entries = []
    ill = 0
    for k in range(n_cls):
        for j in range(int(words[4 * k])):
            off, cap = int(set_offs[k * stride + j]), int(set_caps[k * stride + j])
            if cap >= 1 and off + cap <= dev_bytes and off + cap <= M64 and off % align == 0:
                entries.append((off, len(entries), cap))
            else:
                ill += 1
    entries.sort(key=lambda e: (e[0], e[1]))  # by off, stably in enumeration order
    out, reach, hit = [], 0, 0
    for off, _, cap in entries:
        if off < reach:
            hit += 1
        else:
            out.append((off, cap))
        reach = max(reach, off + cap)
    return out, ill, hit


def outputs_of(surv, T, P, align):
    """C3 and C4: ([(off, cap)] of the outputs in ascending off, the groups of
    two or more entries, the entries in them)."""
    outs, groups, absorbed = [], 0, 0
    i, n = 0, len(surv)
    while i < n:
        if surv[i][1] >= T:                   # a non-candidate: never part of a run
            outs.append(surv[i])
            i += 1
            continue
        e = i + 1                             # the run [i, e)
        while e < n and surv[e][1] < T and round_up(surv[e - 1][0] + surv[e - 1][1], align) == surv[e][0]:
            e += 1
        g = i
        while g < e and surv[g][0] % P != 0:
            outs.append(surv[g])              # before g_0: single
            g += 1
        while g < e:
            h = g + 1                         # g_{m+1}
            while h < e and not (surv[h][0] >= surv[g][0] + T and surv[h][0] % P == 0):
                h += 1
            end = surv[h - 1][0] + surv[h - 1][1]
            if h == e and end - surv[g][0] < T:
                outs.extend(surv[g:e])        # the tail stays single
            else:
                outs.append((surv[g][0], end - surv[g][0]))
                if h - g >= 2:                # a group of one entry is that entry
                    groups += 1
                    absorbed += h - g
            g = h
        i = e
    return outs, groups, absorbed


def m_coalesce_set(set_offs, set_caps, words, n_cls, stride, dev_bytes, target, align=16, flags=0):
    """One cio_file_coalesce_set_dev.  set_offs, set_caps (n_cls * stride ints)
    and words (4 * n_cls ints) are changed IN PLACE.  Returns dev_total, 5 +
    n_cls ints."""
    if not set_sound(words, n_cls, stride):
        return [1] + [0] * (4 + n_cls)
    T, P = int(words[4 * target + 2]), int(words[4 * target + 3])
    surv, ill, hit = survivors_of(set_offs, set_caps, words, n_cls, stride, dev_bytes, align)
    outs, groups, absorbed = outputs_of(surv, T, P, align)
    filed = [[] for _ in range(n_cls)]
    for off, cap in outs:
        k = file_class(words, n_cls, off, cap)
        if k is None:
            ill += 1
        else:
            filed[k].append((off, cap))
    counts = [len(f) for f in filed]
    over = any(counts[k] > int(words[4 * k + 1]) for k in range(n_cls))
    if not over and not flags & DRY:
        for k in range(n_cls):
            for j, (off, cap) in enumerate(filed[k]):
                set_offs[k * stride + j], set_caps[k * stride + j] = off, cap
            words[4 * k] = counts[k]
    return [2 if over else 0, ill, hit, groups, absorbed] + counts


# ---------------------------------------------------------------- sets to coalesce

def make_set(seed, classes, stride, entries, dev_bytes, align, adjacent=0.7, bad=0.08, caps=None, room=None):
    """A set of `entries` entries for the tests: slots laid from a cursor, the
    next one adjacent with probability `adjacent` and otherwise behind a gap
    drawn so that the offsets spread over the whole of dev_bytes (every digit
    of the sort key is in use); a fraction `bad` of the entries are duplicates,
    nested and partial overlaps and ill-formed entries of each kind; the last
    slot ends exactly at dev_bytes.  An entry goes to the class release would
    file it in while that has room and to any class with room otherwise, and
    each class's entries are shuffled.  Fewer entries come back when dev_bytes
    or the classes' room (`room` words per class, default stride) cannot hold
    them.  Returns (set_offs, set_caps, words) as lists."""
    rng = np.random.default_rng(seed)
    n_cls = len(classes)
    room = [stride] * n_cls if room is None else list(room)
    sizes = caps or sorted({c for c, _ in classes} | {classes[0][0] + 5, classes[-1][0] // 2 + 1, 3 * align, 1})
    slots, cur = [], align * int(rng.integers(0, 3))
    while len(slots) < entries:
        cap = int(sizes[int(rng.integers(0, len(sizes)))])
        left = entries - len(slots)
        if left == 1 and (dev_bytes - 1) // align * align >= cur:
            cur = (dev_bytes - 1) // align * align            # the highest key there is
            cap = dev_bytes - cur
        if cur + cap > dev_bytes:
            break
        slots.append((cur, cap))
        cur = round_up(cur + cap, align)
        if rng.random() >= adjacent:
            units = max(2, (dev_bytes - cur) // align // (2 * left))
            cur += align * int(rng.integers(1, units))
    last = (dev_bytes - 1) // align * align
    if slots and slots[-1][0] != last and (len(slots) == 1 or round_up(sum(slots[-2]), align) <= last):
        slots[-1] = (last, dev_bytes - last)                  # whatever the gaps did: an entry with the last key
    for i in range(len(slots) - 1):
        if i == 0 or rng.random() >= bad:
            continue
        o, c = slots[int(rng.integers(0, i))]
        kind = int(rng.integers(0, 8))
        slots[i] = [(o, c), (o, max(1, c // 2)), (o + align * ((c // 2) // align), c), (o, 0),
                    (o + 1, c) if align > 1 else (o, 0), (dev_bytes - align, 2 * align + 1), (M64 - 5, 6 + kind),
                    (M64 // align * align, M64)][kind]
        slots[i] = (slots[i][0] & M64, slots[i][1] & M64)     # a bad entry of a bad entry may leave 64 bits
    words = [w for k, (c, p) in enumerate(classes) for w in (0, room[k], c, p)]
    per = [[] for _ in range(n_cls)]
    order = rng.permutation(len(slots))
    for i in order:
        off, cap = slots[int(i)]
        k = file_class(words, n_cls, off, cap)
        if k is None or len(per[k]) >= room[k]:
            free = [c for c in range(n_cls) if len(per[c]) < room[c]]
            if not free:
                break
            k = free[int(rng.integers(0, len(free)))]
        per[k].append((off, cap))
    so, sc = [0] * (n_cls * stride), [0] * (n_cls * stride)
    for k in range(n_cls):
        words[4 * k] = len(per[k])
        for j, (off, cap) in enumerate(per[k]):
            so[k * stride + j], sc[k * stride + j] = off, cap
    return so, sc, words


# ---------------------------------------------------------------- the drift

DRIFT = dict(n=12, meta=3, size=600, limit=500, new_cap=527, realloc=512, page=256, align=32,
             classes=(527, 1280, 1792, 2304), stride=32, list_cap=24, need1=600, need2=1900, target=3,
             arena_room=24 * 1280 + 6 * 2304)


class Drift:
    """A producer whose chunks drift to a larger class, on the models of the
    whole chain.  Phase 1, twice: every image grows from 527 to class 1 (1280)
    in ONE grow_set call -- the class is empty, so the twelve slots come side
    by side from the arena --, its old slot is released, it is written, and it
    is rotated (limit) into the list, the fresh images taking the released
    527-byte slots.  Then the list is released: class 1 holds 24 entries, one
    run in memory (1280 is a multiple of align).  Twelve of them would be 15360
    bytes, not enough for twelve class-3 slots; two generations are.  Phase 2:
    every image needs class 3 (2304).  With coalesce=True the call stands in
    front of the grow: pairs of 1280-byte slots become 2560-byte class-3 slots,
    all twelve images are served from the set and the arena's top does not
    move.  Without it the same grow asks the arena for twelve class-3 slots."""

    def __init__(self, coalesce=True, **kw):
        p = dict(DRIFT, **kw)
        self.p, self.coalesce = p, coalesce
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
        self.src_offs = np.arange(n, dtype=np.uint64) * (p["size"] + 3)
        j = np.arange(n * (p["size"] + 3) + 16, dtype=np.uint64)
        self.src = ((j * 29 + 5) % 251 + 1).astype(np.uint8)
        self.prev = None

    def grow(self, need):
        """grow_set of every image by `need` bytes: (status, total, prev_offs,
        prev_caps, served)."""
        p = self.p
        out = m_grow_set(self.buf, self.offs, self.caps, [need] * p["n"], self.arena, self.so, self.sc, self.words,
                         self.n_cls, self.stride, realloc=p["realloc"], page=p["page"], align=p["align"])
        self.prev = ([int(x) for x in out[2]], [int(x) for x in out[3]])
        return out

    def release_prev(self):
        """release_set of the slots the grow left (live = the images' offsets)."""
        return m_release_set(self.buf, self.prev[0], self.prev[1], None, None, None, list(self.offs), 0, self.so,
                             self.sc, self.words, self.n_cls, self.stride)

    def write(self):
        p = self.p
        for i in range(p["n"]):
            o = int(self.src_offs[i])
            self.crc[i] = m_write(self.buf, self.offs[i], self.src[o:o + p["size"]].tobytes(), self.crc[i])

    def rotate(self):
        """rotate_pool into class 0, no needs: every image above limit."""
        p = self.p
        cls0 = (self.so[:self.stride], self.sc[:self.stride], self.words[:4])
        out = m_rotate_pool(self.buf, self.offs, self.caps, [], p["limit"], p["new_cap"], p["align"], self.arena,
                            self.lo, self.lc, self.li, self.count, cls0[0], cls0[1], cls0[2], flags=CK,
                            crc_cur=self.crc)
        self.words[0] = cls0[2][0]
        return out

    def release_list(self):
        """release_set(ZERO | COMPACT) of the list of rotated images."""
        from pool_dev_model import COMPACT, ZERO
        return m_release_set(self.buf, self.lo, self.lc, self.li, self.count, None, None, ZERO | COMPACT, self.so,
                             self.sc, self.words, self.n_cls, self.stride)

    def coalesce_set(self, flags=0):
        return m_coalesce_set(self.so, self.sc, self.words, self.n_cls, self.stride, len(self.buf), self.p["target"],
                              self.p["align"], flags)

    def run(self):
        """The whole scenario on the model.  Returns what the test asserts:
        the tops after phase 1 and after phase 2, every status seen, the
        coalesce totals, the images served from the set in phase 2."""
        p, bad = self.p, 0
        for _ in range(2):
            g = self.grow(p["need1"])
            bad += int(g[0].any()) + int(self.release_prev()[0].any())
            self.write()
            bad += int(self.rotate()[0].any())
        bad += int(self.release_list()[0].any())
        top1 = self.arena[0]
        total = self.coalesce_set() if self.coalesce else None
        g = self.grow(p["need2"])
        self.release_prev()
        return dict(top1=top1, top2=self.arena[0], phase1_bad=bad, grow_status=g[0], grow_total=g[1],
                    served=g[4], coalesce=total)
