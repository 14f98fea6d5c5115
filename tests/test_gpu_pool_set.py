"""The size-classed pool set in device memory
(include/chunkio_amd/cio_write_dev_pool_set.h) against the numpy model
(pool_set_model.py).  Every call is compared bit for bit in ALL it may touch:
the WHOLE buffer (a position-dependent sentinel fills every slack, the arena
and the free slots, so a stray or missing store shows), every array including
the entries that must stay untouched, the set's arrays (two sentinel entries
behind them) and words, the arena, the counts, every word of dev_total and the
statuses.  No tolerance anywhere.  State, sentinel and layout are those of
test_gpu_grow_dev.py, test_gpu_rotate_dev.py and test_gpu_pool_dev.py."""
import hashlib

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import grow_dev_model as gmodel
import pool_set_model as model
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, layout, put_image, u64
from test_gpu_pool_dev import Pool, free_slots, same_bytes
from test_gpu_rotate_dev import CK, MANIFEST, S64, u32
from write_dev_move_model import m_init, m_seal, m_write, pattern

pytestmark = pytest.mark.gpu

ZERO, COMPACT = cf.CIOA_RELEASE_ZERO, cf.CIOA_RELEASE_COMPACT
SIZES = [1, 63, 64, 65, 1023, 1024, 1025, 2055]    # both sides of a wave (64) and of a workgroup (1024)


class PoolSet:
    """A pool set on the device and the host copy beside it.  The arrays hold
    two entries more than n_cls * stride, so that a push beyond them shows."""

    def __init__(self, cuda, classes, stride, entries=None, words=None):
        self.cuda, self.n_cls, self.stride = cuda, len(classes), stride
        self.so, self.sc = [S64] * (self.n_cls * stride + 2), [S64] * (self.n_cls * stride + 2)
        self.words = []
        for k, (cls, pal) in enumerate(classes):
            ent = [] if entries is None else entries[k]
            for e, (o, c) in enumerate(ent):
                self.so[k * stride + e], self.sc[k * stride + e] = int(o), int(c)
            self.words += [len(ent), stride, cls, pal]
        if words is not None:
            self.words = list(words)
        self.so_t, self.sc_t, self.words_t = dev_i64(self.so, cuda), dev_i64(self.sc, cuda), dev_i64(self.words, cuda)

    def arg(self):
        return (self.so_t, self.sc_t, self.words_t, self.n_cls, self.stride)

    def model_args(self):
        return (self.so, self.sc, self.words, self.n_cls, self.stride)

    def check(self, what=""):
        assert u64(self.words_t).tolist() == self.words, (what, "set words", u64(self.words_t).tolist(), self.words)
        assert u64(self.so_t).tolist() == self.so, (what, "set offsets")
        assert u64(self.sc_t).tolist() == self.sc, (what, "set capacities")


class Entries:
    """A list of slots (offs, caps, img, count) over one buffer, on the device
    and on the host, released into a set."""

    def __init__(self, cuda, buf, offs, caps, img=None, count=None, base_t=None):
        self.cuda, self.buf, self.n = cuda, buf, len(offs)
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.img = list(range(100, 100 + self.n)) if img is None else [int(x) for x in img]
        self.count = None if count is None else [int(count), self.n]
        self.base_t = dev_u8(buf, cuda) if base_t is None else base_t
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.img_t = dev_i32(self.img, cuda)
        self.count_t = None if count is None else dev_i64(self.count, cuda)

    def release(self, w, pset, gate=None, live=None, flags=0, what=""):
        """One device call and the model's, compared in everything.  Returns
        the model's (status, total, accepted)."""
        import torch
        total = dev_i64([0x55] * (2 + pset.n_cls), self.cuda)
        status = torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda)
        cf.release_set_batch_dev(w, self.base_t, self.offs_t, self.caps_t, pset.arg(), img=self.img_t,
                                 count=self.count_t,
                                 gate=None if gate is None else dev_i32(np.asarray(gate, np.int32).view(np.uint32),
                                                                        self.cuda),
                                 live_offs=None if live is None else dev_i64(live, self.cuda), flags=flags,
                                 total=total, status=status)
        want = model.m_release_set(self.buf, self.offs, self.caps, self.img, self.count, gate, live, flags,
                                   *pset.model_args())
        assert np.array_equal(status.cpu().numpy(), want[0]), (what, "status", status.cpu().numpy(), want[0])
        assert u64(total).tolist() == want[1], (what, "total", u64(total).tolist(), want[1])
        self.check(pset, what)
        return want

    def check(self, pset, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u32(self.img_t).tolist() == self.img, (what, "images")
        if self.count is not None:
            assert u64(self.count_t).tolist() == self.count, (what, "count", u64(self.count_t).tolist(), self.count)
        pset.check(what)
        same_bytes(self.base_t, self.buf, what)


class Images:
    """Images, an arena and a pool set in one device buffer, the host copy
    beside them; grown out of the set."""

    def __init__(self, cuda, buf, offs, caps, arena, pset):
        self.cuda, self.buf, self.pset = cuda, buf, pset
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.arena, self.n = [int(arena[0]), int(arena[1])], len(offs)
        self.base_t = dev_u8(buf, cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.arena_t = dev_i64(self.arena, cuda)

    def grow(self, w, need=None, recs=None, what="", **kw):
        """One device call (the records variant with recs = (rec_img,
        rec_lens)) and the model's, compared in everything.  Returns the
        model's (status, total, prev_offs, prev_caps, served)."""
        import torch
        o = dict(prev_offs=dev_i64(np.full(self.n, 0x77, np.uint64), self.cuda),
                 prev_caps=dev_i64(np.full(self.n, 0x77, np.uint64), self.cuda),
                 total=dev_i64([0x55] * (2 + self.pset.n_cls), self.cuda),
                 status=torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda))
        if recs is None:
            cf.grow_set_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_i64(need, self.cuda), self.arena_t,
                                  self.pset.arg(), **kw, **o)
        else:
            cf.grow_set_records_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_i32(recs[0], self.cuda),
                                          dev_i64(recs[1], self.cuda), self.arena_t, self.pset.arg(), **kw, **o)
            need = model.needs_of(recs[0], recs[1], self.n)
        want = model.m_grow_set(self.buf, self.offs, self.caps, need, self.arena, *self.pset.model_args(), **kw)
        got = (o["status"].cpu().numpy(), u64(o["total"]).tolist(), u64(o["prev_offs"]), u64(o["prev_caps"]))
        for g, m, name in zip(got, want, ("status", "total", "prev_offs", "prev_caps")):
            assert np.array_equal(g, m), (what, name, g, m)
        self.check(what)
        return want

    def check(self, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u64(self.arena_t).tolist() == self.arena, (what, "arena", u64(self.arena_t).tolist(), self.arena)
        self.pset.check(what)
        same_bytes(self.base_t, self.buf, what)


# ------------------------------------------------------------------ 1. release, mixed batches

REL_KINDS = ("ok", "ok", "gate", "ok", "live", "magic", "below", "ok", "misaligned", "ok")
PAL, SLOT = 16, 64 + 32 * 8 + 16
MODES = ("none", "first", "middle", "full")


def classes_of(n_cls):
    return [(64 + 32 * k, PAL) for k in range(n_cls)]


def rel_mixed(n, n_cls):
    """Entry i of kind REL_KINDS[i % 10] in a slot of SLOT bytes at a multiple
    of PAL: releasable, its capacity spread over all classes (the class's cls
    plus 0, 8 or 16); valid but gate-failed; valid and still live; bad magic; a
    valid image of one byte less than class 0; a valid image at an offset that
    is 8 modulo PAL.  Returns (buf, offs, caps, gate, live, kinds, class of
    entry i or None)."""
    buf = fill(32 + n * SLOT + 48)
    offs, caps, gate, live, kinds, cls = [], [], [], [], [], []
    for i in range(n):
        kind = REL_KINDS[i % 10]
        k = (i // 2 + i // 10) % n_cls
        off, cap = 32 + i * SLOT, 64 + 32 * k + 8 * (i % 3)
        if kind == "below":
            cap = 63
        elif kind == "misaligned":
            off += 8
        put_image(buf, off, i % 5, (7 * i) % 30)
        if kind == "magic":
            buf[off] = 0xC0
        offs.append(off)
        caps.append(cap)
        gate.append(-1 if kind == "gate" else 0)
        live.append(off if kind == "live" else off + 16)
        kinds.append(kind)
        cls.append(k if kind == "ok" else None)
    return buf, offs, caps, gate, live, kinds, cls


def set_for(cuda, n_cls, reach, shift=0, entry=lambda k, e: (1 << 40) + 4096 * (8 * e + k)):
    """Class k in mode MODES[(k + shift) % 4]: room for everything; an empty
    class of capacity 0; room for half; full on entry with three entries.
    Returns (set, room per class)."""
    have, room = [], []
    for k in range(n_cls):
        mode = MODES[(k + shift) % 4]
        have.append({"none": 2, "first": 0, "middle": 1, "full": 3}[mode])
        room.append({"none": reach[k] + 3, "first": 0, "middle": reach[k] // 2, "full": 0}[mode])
    stride = max(h + r for h, r in zip(have, room)) + 1
    pset = PoolSet(cuda, classes_of(n_cls), stride,
                   entries=[[(entry(k, e), 64 + 32 * k) for e in range(have[k])] for k in range(n_cls)])
    for k in range(n_cls):                        # each class's own capacity, below the stride
        pset.words[4 * k + 1] = have[k] + room[k]
    pset.words_t.copy_(dev_i64(pset.words, cuda))
    return pset, room


@pytest.mark.parametrize("n_cls", [1, 3, 8])
@pytest.mark.parametrize("n", SIZES)
def test_release_set_mixed_batches(cuda, n, n_cls):
    buf, offs, caps, gate, live, kinds, cls = rel_mixed(n, n_cls)
    reach = [sum(1 for c in cls if c == k) for k in range(n_cls)]
    pset, room = set_for(cuda, n_cls, reach, shift=n % 4)
    have = [pset.words[4 * k] for k in range(n_cls)]
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pset, gate=gate, live=live, what=f"release {n} {n_cls}")
    want_acc = []
    for k in range(n_cls):
        want_acc += [i for i in range(n) if cls[i] == k][:room[k]]
    assert sorted(acc) == sorted(want_acc) and total == [sum(reach), n - len(acc)] + reach
    assert st.tolist() == [0 if i in set(acc) or kinds[i] == "live" else -1 for i in range(n)]
    for k in range(n_cls):
        mine = [i for i in acc if cls[i] == k]
        assert pset.words[4 * k] == have[k] + len(mine)
        assert pset.so[k * pset.stride + have[k]:k * pset.stride + have[k] + len(mine)] == [offs[i] for i in mine]
    for i in acc:
        assert buf[offs[i]] == 0 and buf[offs[i] + 1] == 0 and buf[offs[i] + 24 + i % 5 + (7 * i) % 30] != 0


# ------------------------------------------------------------------ 2. one class: the single-pool call

@pytest.mark.parametrize("flags", [0, ZERO | COMPACT])
@pytest.mark.parametrize("n", [65, 1025])
def test_release_set_with_one_class_is_release(cuda, n, flags):
    """n_cls = 1 against cio_file_release_batch_dev on a copy, the pool cutting
    in the middle: output for output."""
    import torch
    buf, offs, caps, gate, live, kinds, cls = rel_mixed(n, 1)
    room = sum(1 for c in cls if c == 0) // 2
    pset = PoolSet(cuda, [(64, PAL)], room + 2, entries=[[(1 << 40, 80), ((1 << 40) + 4096, 96)]])
    pool = Pool(cuda, room + 2, 64, PAL, entries=[(1 << 40, 80), ((1 << 40) + 4096, 96)])
    a, b = Entries(cuda, buf, offs, caps, count=n), Entries(cuda, buf.copy(), offs, caps, count=n)
    gate_t = dev_i32(np.asarray(gate, np.int32).view(np.uint32), cuda)
    with cio.DevWriter(n) as w:
        st, total, acc = a.release(w, pset, gate=gate, flags=flags, what="the set")
        total_b = dev_i64([0x55, 0x55], cuda)
        status_b = torch.full((n,), 99, dtype=torch.int32, device=cuda)
        cf.release_batch_dev(w, b.base_t, b.offs_t, b.caps_t, img=b.img_t, count=b.count_t, gate=gate_t, flags=flags,
                             total=total_b, status=status_b, **pool.args())
    assert len(acc) == room > 0 and total[:2] == u64(total_b).tolist() and total[2] == total[0]
    assert np.array_equal(status_b.cpu().numpy(), st)
    assert torch.equal(a.base_t, b.base_t) and torch.equal(a.offs_t, b.offs_t) and torch.equal(a.caps_t, b.caps_t)
    assert torch.equal(a.img_t, b.img_t) and torch.equal(a.count_t, b.count_t)
    assert u64(pool.words_t).tolist() == pset.words and u64(pool.po_t).tolist() == pset.so
    assert u64(pool.pc_t).tolist() == pset.sc


# ------------------------------------------------------------------ 3. COMPACT and ZERO

@pytest.mark.parametrize("flags", [COMPACT, COMPACT | ZERO])
@pytest.mark.parametrize("kept", ["none", "all", "alternating"])
def test_release_set_compacts_with_cuts_in_several_classes(cuda, kept, flags):
    """1025 drained chunks over four classes, of which two cut in the middle;
    beside the cuts the gate keeps none, all or every other entry.  The kept
    entries move to the front in their order, the vacated ones are (0, 0,
    0xffffffff), the statuses stay where the entries were."""
    n, n_cls = 1025, 4
    buf = fill(32 + n * SLOT + 48)
    offs = [32 + i * SLOT for i in range(n)]
    caps = [64 + 32 * ((i // 3) % n_cls) + 8 * (i % 3) for i in range(n)]
    for i in range(n):
        put_image(buf, offs[i], i % 5, (7 * i) % 30)
    gate = {"none": [0] * n, "all": [-3] * n, "alternating": [-(i % 2) for i in range(n)]}[kept]
    reach = [sum(1 for i in range(n) if gate[i] == 0 and (i // 3) % n_cls == k) for k in range(n_cls)]
    pset, room = set_for(cuda, n_cls, reach, shift=3)      # classes 0 and 3 cut: "full" and "middle"
    e = Entries(cuda, buf, offs + [S64] * 3, caps + [S64] * 3, count=n)
    e.count[1] = n
    e.count_t.copy_(dev_i64(e.count, cuda))
    with cio.DevWriter(n + 3) as w:
        st, total, acc = e.release(w, pset, gate=gate + [0] * 3, flags=flags, what=f"compact {kept}")
    stay = [i for i in range(n) if i not in set(acc)]
    assert total == [sum(reach), len(stay)] + reach and len(acc) == sum(min(r, m) for r, m in zip(reach, room))
    assert (kept == "all") == (not acc) and (kept == "all" or 0 < len(acc) < sum(reach))
    assert e.offs[:len(stay)] == [offs[i] for i in stay] and e.img[:len(stay)] == [100 + i for i in stay]
    assert e.offs[len(stay):n] == [0] * len(acc) and e.caps[len(stay):n] == [0] * len(acc)
    assert e.img[len(stay):n] == [model.NO_IMAGE] * len(acc) and e.offs[n:] == [S64] * 3
    assert e.count == [len(stay), n]


def test_release_set_zero_over_every_destination_residue(cuda):
    """Slots of two classes at every offset residue modulo 16, full of image
    bytes, 1 .. 16 sentinel bytes between them: the whole slot becomes zero and
    no byte beside it changes."""
    offs, caps, pos = [], [], 5
    for r in range(16):
        for c in (24, 41, 4096 + 17, 5000):
            pos += (r - pos) % 16 or 16
            offs.append(pos)
            caps.append(c)
            pos += c
    buf = fill(pos + 33)
    for o, c in zip(offs, caps):
        put_image(buf, o, min(c - 24, 3), c - 24 - min(c - 24, 3))
    before, n = buf.copy(), len(offs)
    pset = PoolSet(cuda, [(24, 1), (4096, 1)], n)
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pset, flags=ZERO, what="zero")
    assert not st.any() and acc == list(range(n)) and total == [n, 0, n // 2, n // 2]
    keep = np.ones(len(buf), bool)
    for o, c in zip(offs, caps):
        assert not buf[o:o + c].any()
        keep[o:o + c] = False
    assert np.array_equal(buf[keep], before[keep]) and buf[keep].all()


# ------------------------------------------------------------------ 5. grow, mixed batches

GROW_KINDS = ("c0", "none", "c1", "room", "c2", "magic", "c3", "above", "arena", "c0")
GCLS = (256, 512, 768, 1024)
REALLOC, PAGE = 3, 256


def grow_mixed(n, arena_room=None):
    """Image i of kind GROW_KINDS[i % 10]: grows into class 0 .. 3 (the
    reference's rule gives exactly the class's size); no need; a need below the
    room; bad magic; grows above the largest class (1536); an image inside the
    arena's free part.  Returns (buf, offs, caps, arena, need, kinds)."""
    items, need, kinds = [], [], []
    for i in range(n):
        kind = GROW_KINDS[i % 10]
        meta, content, room = i % 4, 20 + (7 * i) % 50, 10 + i % 7
        used = 24 + meta + content
        items.append((meta, content, room))
        need.append(GCLS[int(kind[1])] - 10 - used if kind[0] == "c" else
                    {"none": 0, "room": room, "above": 1536 - 10 - used}.get(kind, room + 7))
        kinds.append(kind)
    bound = (n // 10 + 1) * (2 * 256 + 512 + 768 + 1024 + 1536 + 6 * 64) if arena_room is None else arena_room
    resident = [i for i in range(n) if kinds[i] == "arena"]
    buf, offs, caps, arena = layout(items, bound, resident=resident)
    for i in range(n):
        if kinds[i] == "magic":
            buf[offs[i] + 1] = 0x01
    return buf, offs, caps, arena, need, kinds


def grow_set_for(cuda, buf, demand, shift, pals=(64, 64, 32, 64)):
    """Class k with F_k 0, below, equal to or above its demand, by (k + shift) %
    4; the entries are free slots behind buf, of the class's size plus 0, 8 or
    16 bytes.  Returns (buf, set, F)."""
    F = [(0, demand[k] // 2, demand[k], demand[k] + 2)[(k + shift) % 4] for k in range(4)]
    entries = []
    for k in range(4):
        buf, ent = free_slots(buf, F[k], lambda e, k=k: GCLS[k] + 8 * (e % 3), 64)
        entries.append(ent)
    pset = PoolSet(cuda, list(zip(GCLS, pals)), max(F) + 2, entries=entries)
    return buf, pset, F


@pytest.mark.parametrize("shift", [0, 1, 2, 3])
@pytest.mark.parametrize("n", SIZES)
def test_grow_set_mixed_batches(cuda, n, shift):
    """An odd shift runs with align 64, which makes class 2 (pal 32) unusable:
    its images then ask class 3."""
    align = 64 if shift % 2 else 32
    buf, offs, caps, arena, need, kinds = grow_mixed(n)
    cls_of = {"c0": 0, "c1": 1, "c2": 3 if align == 64 else 2, "c3": 3}
    demand = [sum(1 for k in kinds if cls_of.get(k) == c) for c in range(4)]
    buf, pset, F = grow_set_for(cuda, buf, demand, shift)
    if align == 64:
        F[2] = 0
    s = Images(cuda, buf, offs, caps, arena, pset)
    flags = cf.CIOA_GROW_ZERO * (n % 2)
    with cio.DevWriter(n) as w:
        st, total, po, pc, served = s.grow(w, need, realloc=REALLOC, page=PAGE, align=align, flags=flags,
                                           what=f"grow {n} {shift}")
        assert st.tolist() == [-1 if k in ("magic", "arena") else 0 for k in kinds]
        assert total[2:] == demand and total[1] == len(served) == sum(min(d, f) for d, f in zip(demand, F))
        for c in range(4):                        # the pool is a stack, and the image gets the entry's whole capacity
            mine = [i for i in served if cls_of[kinds[i]] == c]
            top = pset.words[4 * c] + len(mine)
            assert [(s.offs[i], s.caps[i]) for i in mine] == \
                [(pset.so[c * pset.stride + top - 1 - j], pset.sc[c * pset.stride + top - 1 - j])
                 for j in range(len(mine))]
        for i in range(n):                        # an arena-bound image has its class's size, or its own without one
            if kinds[i][0] == "c" and i not in set(served):
                assert s.caps[i] == GCLS[cls_of[kinds[i]]]
            elif kinds[i] == "above":
                assert s.caps[i] == 1536
        # the same call again: everything now has room (or is still invalid), nothing moves
        top, words = s.arena[0], list(pset.words)
        st2 = s.grow(w, need, realloc=REALLOC, page=PAGE, align=align, what="again")[0]
        assert st2.tolist() == st.tolist() and s.arena[0] == top and pset.words == words


# ------------------------------------------------------------------ 4. an unsound set

UNSOUND = {"count above capacity": (0, 0, 9), "cls below 24": (0, 2, 23), "pal no power of two": (1, 3, 48),
           "capacity above the stride": (2, 1, 9), "cls not increasing": (2, 2, 512)}


@pytest.mark.parametrize("why", sorted(UNSOUND))
def test_unsound_set_release_changes_nothing_and_grow_is_plain_grow(cuda, why):
    import torch
    k, word, value = UNSOUND[why]
    n = 65
    buf, offs, caps, gate, live, kinds, cls = rel_mixed(n, 4)
    before = buf.copy()
    pset = PoolSet(cuda, classes_of(4), 8)
    pset.words[4 * k + word] = value
    pset.words_t.copy_(dev_i64(pset.words, cuda))
    words = list(pset.words)
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pset, gate=gate, live=live, what=f"unsound {why}")
    assert acc == [] and total == [0, n, 0, 0, 0, 0] and np.array_equal(buf, before) and pset.words == words
    assert st.tolist() == [0 if x == "live" else -1 for x in kinds]
    # grow: the same set's fault in a set of grow's classes, full of entries; the call is cio_file_grow_batch_dev
    buf, offs, caps, arena, need, kinds = grow_mixed(n)
    buf, pset, F = grow_set_for(cuda, buf, [7] * 4, 3)
    pset.words[4 * k + word] = {"cls not increasing": GCLS[1], "count above capacity": pset.stride + 1,
                                "capacity above the stride": pset.stride + 1}.get(why, value)
    pset.words_t.copy_(dev_i64(pset.words, cuda))
    s = Images(cuda, buf, offs, caps, arena, pset)
    plain = dict(base=dev_u8(buf, cuda), offs=dev_i64(offs, cuda), caps=dev_i64(caps, cuda), arena=dev_i64(arena, cuda))
    with cio.DevWriter(n) as w:
        st, total, po, pc, served = s.grow(w, need, realloc=REALLOC, page=PAGE, align=32, flags=1, what=why)
        pst, ptotal = cf.grow_batch_dev(w, plain["base"], plain["offs"], plain["caps"], dev_i64(need, cuda),
                                        plain["arena"], realloc=REALLOC, page=PAGE, align=32, flags=1)
    assert served == [] and total[1:] == [0] * 5 and total[0] == int(u64(ptotal)[0]) > 0
    assert np.array_equal(pst.cpu().numpy(), st) and torch.equal(plain["base"], s.base_t)
    assert torch.equal(plain["offs"], s.offs_t) and torch.equal(plain["caps"], s.caps_t)
    assert torch.equal(plain["arena"], s.arena_t)


# ------------------------------------------------------------------ 6. the arena cut

def test_grow_set_arena_cut_with_pool_served_images_behind_it(cuda):
    """Twenty images: class 1 serves the first two of its images, every other
    growing image is arena-bound.  The arena ends inside the arena-bound part:
    every arena-bound image from the first that does not fit is cut, and the
    pool-served images behind the cut are still accepted."""
    n = 20
    buf, offs, caps, arena, need, kinds = grow_mixed(n, arena_room=256 + 64 + 768 + 100)
    buf, ent = free_slots(buf, 2, lambda e: 520 + 8 * e, 64)
    pset = PoolSet(cuda, list(zip(GCLS, (64,) * 4)), 4, entries=[[], ent, [], []])
    s = Images(cuda, buf, offs, caps, arena, pset)
    with cio.DevWriter(n) as w:
        st, total, po, pc, served = s.grow(w, need, realloc=REALLOC, page=PAGE, align=64, what="arena cut")
    # image 0 (256) and 4 (768) fit; 6 (1024) does not, nor any arena-bound image behind it; 2 and 12 are served
    assert served == [2, 12] and st.tolist()[:10] == [0, 0, 0, 0, 0, -1, -1, -1, -1, -1]
    assert st.tolist()[10:] == [-1, 0, 0, 0, -1, -1, -1, -1, -1, -1]
    assert (s.offs[12], s.caps[12]) == ent[0] and (s.offs[2], s.caps[2]) == ent[1] and total[1:] == [2, 4, 2, 2, 2]
    base = gmodel.round_up(arena[0], 64)
    assert s.arena[0] == base + 256 + 768 and total[0] == base - arena[0] + 4 * 256 + 2 * 768 + 2 * 1024 + 2 * 1536


# ------------------------------------------------------------------ 7. a bad pool entry

def test_grow_set_entry_below_its_class_is_consumed(cuda):
    """Class 1's top entry has 500 bytes, below its class (512); it lies inside
    the buffer.  The image that would take it gets CIO_ERROR and stays where it
    was, the entry is consumed, and the class's next image takes the next
    entry."""
    n = 20
    buf, offs, caps, arena, need, kinds = grow_mixed(n)
    buf, ent = free_slots(buf, 2, lambda e: 520 - 20 * e, 64)         # entry 1, the top one, has 500 bytes
    pset = PoolSet(cuda, list(zip(GCLS, (64,) * 4)), 4, entries=[[], ent, [], []])
    s = Images(cuda, buf, offs, caps, arena, pset)
    before = (offs[2], caps[2])
    with cio.DevWriter(n) as w:
        st, total, po, pc, served = s.grow(w, need, realloc=REALLOC, page=PAGE, align=64, what="bad entry")
    assert st[2] == -1 and (s.offs[2], s.caps[2]) == before and served == [12] and (s.offs[12], s.caps[12]) == ent[0]
    assert total[1] == 2 and pset.words[4] == 0 and [i for i in range(n) if st[i]] == [2, 5, 8, 15, 18]


# ------------------------------------------------------------------ 8. the records variant

def records_images(cuda, n_img=300, have=40):
    """n_img images of 40 .. 59 used bytes and 64 of capacity, classes 256 and
    1024 with `have` entries each."""
    items = [(i % 4, 16 + i % 17, 64 - 24 - i % 4 - 16 - i % 17) for i in range(n_img)]
    buf, offs, caps, arena = layout(items, 1 << 19, residue=lambda i: 0)
    entries = []
    for c in (256, 1024):
        buf, ent = free_slots(buf, have, lambda e, c=c: c + 16 * (e % 2), 64)
        entries.append(ent)
    return Images(cuda, buf, offs, caps, arena, PoolSet(cuda, [(256, 64), (1024, 64)], 48, entries=entries))


def test_grow_set_records_cross_wave_and_workgroup_boundaries(cuda):
    """Runs of 1 .. 1000 records per image, in random order: the records
    variant against the model and against the need variant fed the model's
    sums."""
    rng = np.random.default_rng(5)
    rec_img = list(rng.integers(0, 300, 37))
    for rep in range(3):
        for k, run in enumerate((1, 2, 63, 64, 65, 1000)):
            rec_img += [10 * k + rep] * run
    rec_img = rng.permutation(np.asarray(rec_img, np.uint32))
    rec_lens = rng.integers(0, 3, len(rec_img)).astype(np.uint64)
    rec_lens[100] = 1 << 40                       # clamped to 2^32: its image is rejected
    a, b = records_images(cuda, have=4), records_images(cuda, have=4)
    kw = dict(realloc=64, page=64, align=64)
    with cio.DevWriter(len(rec_img)) as w:
        st, total, po, pc, served = a.grow(w, recs=(rec_img, rec_lens), what="runs, records", **kw)
        b.grow(w, model.needs_of(rec_img, rec_lens, 300), what="runs, needs", **kw)
    assert st.tolist().count(-1) == 1 and total[1] == len(served) == min(4, total[2]) + min(4, total[3])
    assert 4 < total[2] and total[0] > 0        # class 0 serves four of its images, the arena the others
    assert a.offs == b.offs and a.caps == b.caps and a.pset.words == b.pset.words and np.array_equal(a.buf, b.buf)


@pytest.mark.parametrize("at", [0, 256, 2999])
def test_grow_set_malformed_records_list_changes_nothing(cuda, at):
    rng = np.random.default_rng(at)
    s = records_images(cuda)
    arena, before, words = list(s.arena), s.buf.copy(), list(s.pset.words)
    rec_img = rng.integers(0, 300, 3000).astype(np.uint32)
    rec_img[at] = 300 + (at % 2) * 0xFFFFFED3
    rec_lens = rng.integers(1, 100, 3000).astype(np.uint64)
    kw = dict(realloc=64, page=64, align=64)
    with cio.DevWriter(3000) as w:
        st, total, po, pc, served = s.grow(w, recs=(rec_img, rec_lens), what=f"malformed at {at}", **kw)
        assert st.tolist() == [-1] * 300 and total == [0, 0, 0, 0] and s.arena == arena
        assert s.pset.words == words and np.array_equal(s.buf, before)
        rec_img[at] = 0                           # the writer is not left marked: the same list, mended, grows
        st, total, po, pc, served = s.grow(w, recs=(rec_img, rec_lens), what="mended", **kw)
        assert not st.any() and len(served) == total[1] == min(40, total[2]) + min(40, total[3]) > 40 and total[0] > 0


# ------------------------------------------------------------------ 9. CIOA_GROW_ZERO

def test_grow_set_zero_reaches_the_entrys_whole_capacity(cuda):
    """Entries of the class's size plus 0 .. 4113 bytes at every offset residue
    modulo 16, full of sentinel bytes: behind the copied bytes the WHOLE entry
    becomes zero, and no byte beside it changes."""
    extra = (0, 1, 15, 16, 17, 4096 + 17)
    n = 16 * len(extra)
    items = [(i % 4, 20 + i % 30, 5) for i in range(n)]
    need = [150] * n                              # used + 150 <= 227, rounded up to the page: 256
    buf, offs, caps, arena = layout(items, 64)
    pos, ent = len(buf), []
    for r in range(16):
        for x in extra:
            pos += (r - pos) % 16 or 16
            ent.append((pos, 256 + x))
            pos += 256 + x
    big = fill(pos + 33)
    big[:len(buf)] = buf
    for o, _ in ent:
        big[o:o + 2] = 0
    before = big.copy()
    pset = PoolSet(cuda, [(256, 1)], n, entries=[ent])
    s = Images(cuda, big, offs, caps, arena, pset)
    with cio.DevWriter(n) as w:
        st, total, po, pc, served = s.grow(w, need, realloc=1, page=256, align=1, flags=cf.CIOA_GROW_ZERO,
                                           what="zero")
    assert not st.any() and served == list(range(n)) and total == [0, n, n] and s.arena == arena
    keep = np.ones(len(big), bool)
    for i in range(n):
        o, c = ent[n - 1 - i]
        used = 24 + items[i][0] + items[i][1]
        assert (s.offs[i], s.caps[i]) == (o, c) and not s.buf[o + used:o + c].any()
        assert np.array_equal(s.buf[o:o + used], before[offs[i]:offs[i] + used])
        keep[o:o + c] = False
    assert np.array_equal(s.buf[keep], before[keep])


# ------------------------------------------------------------------ 10. the reference pin

def test_reference_fixture_in_a_slot_grown_out_of_the_set(cuda):
    """A slot of the fixture's size, full of another chunk's bytes, is released
    with CIOA_RELEASE_ZERO into a class of that size; a small image with
    c03_meta_content's metadata is grown into it by grow_set; the fixture's
    writes and a seal follow.  The image in the recycled slot has the manifest's
    SHA-256 -- its tail is the file's zero tail -- and nothing beside the slot
    changed."""
    spec = [c for c in MANIFEST["chunks"] if c["name"] == "c03_meta_content"][0]
    size, ld = spec["size"], spec["load"]
    meta = spec["ops"][0]["meta"].encode()
    writes = [pattern(o["len"], o["seed"]) for o in spec["ops"] if o["op"] == "write"]
    content = sum(len(x) for x in writes)
    small, slot_off = 24 + len(meta) + 8, 4096
    buf = fill(slot_off + size + 64 + 77)
    put_image(buf, slot_off, 5, size - 24 - 5)    # the drained chunk: every byte of the slot is in use
    crc0 = m_init(buf, 48, meta)
    pset = PoolSet(cuda, [(64, 16), (size, 16)], 2)
    top = slot_off + size + 16
    s = Images(cuda, buf, [48], [small], [top, top + 48], pset)
    crc = [crc0]
    crc_t = dev_i32(crc, cuda)
    src_t = dev_u8(np.frombuffer(b"".join(writes), np.uint8).copy(), cuda)
    with cio.DevWriter(1) as w:
        e = Entries(cuda, buf, [slot_off], [size], base_t=s.base_t)
        st, total, acc = e.release(w, pset, flags=ZERO, what="release the slot")
        assert acc == [0] and total == [1, 0, 0, 1] and not buf[slot_off:slot_off + size].any()
        assert buf[slot_off + size] != 0
        st, total, po, pc, served = s.grow(w, [content], realloc=64, page=1, align=16, what="grow into the slot")
        assert st.tolist() == [0] and served == [0] and total == [0, 1, 0, 1]
        assert (s.offs[0], s.caps[0]) == (slot_off, size) and s.arena[0] == top and pset.words[4] == 0
        pos = 0
        for k, x in enumerate(writes):
            wst = cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, dev_i64([pos], cuda),
                                     dev_i64([len(x)], cuda), crc_t, flags=CK)
            assert not wst.cpu().numpy().any()
            crc[0] = m_write(s.buf, s.offs[0], x, crc[0])
            pos += len(x)
            s.check(f"write {k}")
        assert crc[0] == ld["crc_cur"] and u32(crc_t).tolist() == crc
        assert not cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, crc_t, flags=CK).cpu().numpy().any()
        m_seal(s.buf, slot_off, crc[0])
        s.check("sealed")
    got = s.base_t.cpu().numpy()
    assert hashlib.sha256(got[slot_off:slot_off + size].tobytes()).hexdigest() == spec["sha256"]
    used = 24 + len(meta) + content
    assert not got[slot_off + used:slot_off + size].any() and got[slot_off + size:].all()


# ------------------------------------------------------------------ 11. the steady state, captured

def test_steady_state_chain_with_growth_replays_in_a_bounded_buffer(cuda):
    """The shape test_pool_set_abi.py fixes on the model: rotate_pool (class 0,
    no needs) -> grow_set -> release_set of the previous slots (dev_live_offs =
    dev_img_offs) -> write -> verify over the list's whole capacity ->
    read_packed gated by verify -> release_set(ZERO | COMPACT, gated by the
    read), captured once on one stream with no parallel branches: a warm-up and
    39 replays, each compared with the model in everything.  No status but
    CIO_OK, the arena's top stands still over the last half, and the drained
    bytes followed by the live images' contents are what was written."""
    import torch
    m = model.Steady()
    p = m.p
    n, list_cap, align = p["n"], p["list_cap"], p["align"]
    pset = PoolSet(cuda, [(c, align) for c in p["classes"]], p["stride"])
    assert pset.words == m.words
    pset.so_t.copy_(dev_i64(m.so + [S64] * 2, cuda))      # the model's empty set holds zeros
    pset.sc_t.copy_(dev_i64(m.sc + [S64] * 2, cuda))
    base_t, offs_t, caps_t = dev_u8(m.buf, cuda), dev_i64(m.offs, cuda), dev_i64(m.caps, cuda)
    arena_t, crc_t, count_t = dev_i64(m.arena, cuda), dev_i32(m.crc, cuda), dev_i64(m.count, cuda)
    lo_t, lc_t, li_t = dev_i64(m.lo, cuda), dev_i64(m.lc, cuda), dev_i32(m.li, cuda)
    src_t = dev_u8(np.zeros(n * (p["size"] + 3) + 16, np.uint8), cuda)
    so_t, sl_t = dev_i64(m.src_offs, cuda), dev_i64(np.zeros(n, np.uint64), cuda)
    cls0 = cf.pool_set_class(pset.arg(), 0)

    def st(k):
        return torch.full((k,), 99, dtype=torch.int32, device=cuda)
    ro = dict(total=dev_i64([0, 0], cuda), status=st(n))
    go = dict(total=dev_i64([0] * 6, cuda), status=st(n), prev_offs=dev_i64([0] * n, cuda),
              prev_caps=dev_i64([0] * n, cuda))
    rp = dict(total=dev_i64([0] * 6, cuda), status=st(n))
    wst = st(n)
    out_t = torch.zeros(list_cap * (p["limit"] + p["size"]) + 64, dtype=torch.uint8, device=cuda)
    rd = dict(out_offs=dev_i64([0] * list_cap, cuda), out_lens=dev_i64([0] * list_cap, cuda),
              total=dev_i64([0], cuda), status=st(list_cap))
    rl = dict(total=dev_i64([0] * 6, cuda), status=st(list_cap))
    got = [b""] * n

    def call():
        cf.rotate_pool_batch_dev(w, base_t, offs_t, caps_t, None, limit=p["limit"], new_cap=p["new_cap"], align=align,
                                 arena=arena_t, pool_offs=cls0[0], pool_caps=cls0[1], pool=cls0[2], out_offs=lo_t,
                                 out_caps=lc_t, out_img=li_t, out_count=count_t, flags=CK, crc_cur=crc_t, **ro)
        cf.grow_set_batch_dev(w, base_t, offs_t, caps_t, sl_t, arena_t, pset.arg(), realloc=p["realloc"],
                              page=p["page"], align=align, **go)
        cf.release_set_batch_dev(w, base_t, go["prev_offs"], go["prev_caps"], pset.arg(), live_offs=offs_t, **rp)
        cf.write_batch_dev(w, base_t, offs_t, caps_t, src_t, so_t, sl_t, crc_t, flags=CK, status=wst)
        vst = cf.verify_batch_dev(plan, base_t, lo_t, lc_t, flags=CK)[0]
        cf.read_packed_batch_dev(w, base_t, lo_t, lc_t, cf.CIOA_READ_CONTENT, out_t, gate=vst, **rd)
        cf.release_set_batch_dev(w, base_t, lo_t, lc_t, pset.arg(), img=li_t, count=count_t, gate=rd["status"],
                                 flags=ZERO | COMPACT, **rl)
        return vst

    def stage(k):
        want = m.round(k)
        src_t.copy_(torch.from_numpy(want["src"]))
        sl_t.copy_(torch.from_numpy(want["lens"].view(np.int64)))
        return want

    def settle(k, vst, want):
        torch.cuda.synchronize()
        what = f"round {k}"
        assert want["ok"], what
        for name, o in (("rotate", ro), ("grow", go), ("release_prev", rp), ("release_list", rl)):
            assert np.array_equal(o["status"].cpu().numpy(), want[name][0]), (what, name, "status")
            assert u64(o["total"]).tolist() == want[name][1], (what, name, "total", u64(o["total"]).tolist())
            assert not want[name][0].any(), (what, name)
        assert u64(go["prev_offs"]).tolist() == want["prev"][0] and u64(go["prev_caps"]).tolist() == want["prev"][1]
        assert not wst.cpu().numpy().any(), (what, "write")
        cnt, lo, lc, owners = want["listed"]
        assert not vst.cpu().numpy()[:cnt].any() and not rd["status"].cpu().numpy()[:cnt].any(), (what, "verify, read")
        assert vst.cpu().numpy()[cnt:].all(), (what, "an empty list entry passed verify")
        packed, po, pl = out_t.cpu().numpy(), u64(rd["out_offs"]), u64(rd["out_lens"])
        for e in range(cnt):
            got[owners[e]] += packed[int(po[e]):int(po[e] + pl[e])].tobytes()
        for t, v, name in ((offs_t, m.offs, "offsets"), (caps_t, m.caps, "capacities"), (arena_t, m.arena, "arena"),
                           (count_t, m.count, "count"), (lo_t, m.lo, "list offsets"), (lc_t, m.lc, "list caps"),
                           (pset.words_t, m.words, "set words"),
                           (pset.so_t, m.so + [S64] * 2, "set offsets"), (pset.sc_t, m.sc + [S64] * 2, "set caps")):
            assert u64(t).tolist() == v, (what, name, u64(t).tolist(), v)
        assert u32(crc_t).tolist() == m.crc and u32(li_t).tolist() == m.li, (what, "crc, list images")
        same_bytes(base_t, m.buf, what)

    tops = []
    with cio.DevWriter(max(n, list_cap)) as w, cio.Crc32DevPlan(list_cap) as plan:
        want = stage(0)
        vst = call()                              # warm-up outside the capture (a round like the others)
        settle(0, vst, want)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vst = call()
        torch.cuda.synchronize()
        same_bytes(base_t, m.buf, "capture runs nothing")
        for k in range(1, p["rounds"]):
            want = stage(k)
            for t in (ro["status"], go["status"], rp["status"], wst, rd["status"], rl["status"]):
                t.fill_(99)
            graph.replay()
            settle(k, vst, want)
            tops.append(m.arena[0])
        del graph
    assert len(set(tops[-p["rounds"] // 2:])) == 1 and tops[-1] < m.arena[1]
    assert m.odd == 0 and all(x >= 1 for x in m.served[1:])
    assert got == m.drained
    final = base_t.cpu().numpy()
    for i in range(n):
        meta, content = model.image_check(m.buf, len(m.buf), m.offs[i], m.caps[i])
        live = final[m.offs[i] + 24 + meta:m.offs[i] + 24 + meta + content].tobytes()
        assert got[i] + live == m.wrote[i], i


# ------------------------------------------------------------------ 12. rounds without a graph

def test_rounds_of_records_on_tiny_classes(cuda):
    """Five images through ten rounds of grow_set_records ->
    write_records_ungrouped -> release_set of the previous slots
    (dev_live_offs = dev_img_offs), each call on its own.  Classes 128, 256 and
    512 with a stride of 2: a release of more than two slots of one class is
    cut, and the next grow takes what the set holds and the arena for the rest,
    so that one call serves from both.  After round 5 the images start over
    small, so that the set is asked again.  Every call equals the model, and
    each image's content is its records in order."""
    n_img, n_rec, rounds = 5, 20, 10
    rng = np.random.default_rng(12)
    items = [(2 * i + 1, 0, 64 - 24 - 2 * i - 1) for i in range(n_img)]
    buf, offs, caps, arena = layout(items, 1 << 16, residue=lambda i: 0)
    pset = PoolSet(cuda, [(128, 16), (256, 16), (512, 16)], 2)
    s = Images(cuda, buf, offs, caps, arena, pset)
    crc = [m_init(s.buf, offs[i], bytes([7 + i] * (2 * i + 1))) for i in range(n_img)]
    s.base_t.copy_(dev_u8(s.buf, cuda))
    crc_t = dev_i32(crc, cuda)
    wrote = [b""] * n_img
    both = cuts = 0
    with cio.DevWriter(max(n_img, n_rec)) as w:
        for k in range(rounds):
            if k == 6:                            # start over in fresh small images, so that the set is asked again
                for i in range(n_img):
                    s.offs[i], s.caps[i] = offs[i], caps[i]
                    crc[i] = m_init(s.buf, offs[i], bytes([7 + i] * (2 * i + 1)))
                    wrote[i] = b""
                s.base_t.copy_(dev_u8(s.buf, cuda))
                s.offs_t.copy_(dev_i64(s.offs, cuda))
                s.caps_t.copy_(dev_i64(s.caps, cuda))
                crc_t.copy_(dev_i32(crc, cuda))
            rec_img = rng.integers(0, n_img, n_rec).astype(np.uint32)
            rec_lens = rng.integers(0, 31, n_rec).astype(np.uint64)
            rec_offs = np.concatenate(([0], np.cumsum(rec_lens)[:-1])).astype(np.uint64)
            src = rng.integers(0, 256, int(rec_lens.sum()) + 16, dtype=np.uint8)
            st, total, po, pc, served = s.grow(w, recs=(rec_img, rec_lens), realloc=64, page=64, align=16,
                                               what=f"round {k}: grow")
            assert not st.any()
            both += 0 < len(served) and total[0] > 0
            img_t, lens_t = dev_i32(rec_img, cuda), dev_i64(rec_lens, cuda)
            ist, rst = cf.write_records_ungrouped_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(src, cuda), img_t,
                                                            dev_i64(rec_offs, cuda), lens_t, crc_t, flags=CK)
            assert not rst.cpu().numpy().any() and not ist.cpu().numpy().any()
            for r in range(n_rec):
                i, data = int(rec_img[r]), src[int(rec_offs[r]):int(rec_offs[r] + rec_lens[r])].tobytes()
                crc[i] = m_write(s.buf, s.offs[i], data, crc[i])
                wrote[i] += data
            s.check(f"round {k}: append")
            e = Entries(cuda, s.buf, [int(x) for x in po], [int(x) for x in pc], base_t=s.base_t)
            rwant = e.release(w, pset, live=list(s.offs), what=f"round {k}: release")
            cuts += bool(rwant[0].any())
    assert both >= 1 and cuts >= 1
    for i in range(n_img):
        meta, content = model.image_check(s.buf, len(s.buf), s.offs[i], s.caps[i])
        assert s.buf[s.offs[i] + 24 + meta:s.offs[i] + 24 + meta + content].tobytes() == wrote[i], i
