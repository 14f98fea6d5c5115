"""Recycling drained chunk slots in device memory
(include/chunkio_amd/cio_write_dev_pool.h) against the numpy model
(pool_dev_model.py).  Every call is compared in ALL it may touch: the WHOLE
buffer (a position-dependent sentinel fills every slack, the arena and the
slots around a released one, so a stray or missing store shows), every array
including the entries that must stay untouched, the four pool words, the
arena, the counts, dev_total and the statuses.  State, sentinel and layout are
those of test_gpu_grow_dev.py and test_gpu_rotate_dev.py."""
import hashlib

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import grow_dev_model as gmodel
import pool_dev_model as model
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, layout, put_image, u64
from test_gpu_rotate_dev import BLOCK, CK, KINDS, LIMIT, MANIFEST, NEW_CAP, S64, State, mixed, records_state, u32
from write_dev_move_model import m_init, m_seal, m_write, pattern

pytestmark = pytest.mark.gpu

ZERO, COMPACT = cf.CIOA_RELEASE_ZERO, cf.CIOA_RELEASE_COMPACT


class Pool:
    """A pool on the device and the host copy beside it.  The arrays hold
    `cap` + 2 entries, so that a push beyond the capacity shows."""

    def __init__(self, cuda, cap, cls, pal, entries=(), words=None):
        self.po, self.pc = [S64] * (cap + 2), [S64] * (cap + 2)
        for k, (o, c) in enumerate(entries):
            self.po[k], self.pc[k] = int(o), int(c)
        self.words = [len(entries), cap, cls, pal] if words is None else list(words)
        self.po_t, self.pc_t, self.words_t = dev_i64(self.po, cuda), dev_i64(self.pc, cuda), dev_i64(self.words, cuda)

    def args(self):
        return dict(pool_offs=self.po_t, pool_caps=self.pc_t, pool=self.words_t)

    def check(self, what=""):
        assert u64(self.words_t).tolist() == self.words, (what, "pool words", u64(self.words_t).tolist(), self.words)
        assert u64(self.po_t).tolist() == self.po, (what, "pool offsets")
        assert u64(self.pc_t).tolist() == self.pc, (what, "pool capacities")


def same_bytes(base_t, buf, what):
    got = base_t.cpu().numpy()
    if not np.array_equal(got, buf):
        bad = np.flatnonzero(got != buf)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:6]} of {len(got)}")


class Entries:
    """A list of slots (offs, caps, img, count) over one buffer, on the device
    and on the host, released into a pool."""

    def __init__(self, cuda, buf, offs, caps, img=None, count=None):
        self.cuda, self.buf, self.n = cuda, buf, len(offs)
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.img = list(range(100, 100 + self.n)) if img is None else [int(x) for x in img]
        self.count = None if count is None else [int(count), self.n]
        self.base_t = dev_u8(buf, cuda)
        self.offs_t, self.caps_t, self.img_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda), dev_i32(self.img, cuda)
        self.count_t = None if count is None else dev_i64(self.count, cuda)

    def release(self, w, pool, gate=None, live=None, flags=0, with_img=True, what=""):
        """One device call and the model's, compared in everything.  Returns
        the model's (status, total, accepted)."""
        import torch
        total = dev_i64([0x55, 0x55], self.cuda)
        status = torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda)
        cf.release_batch_dev(w, self.base_t, self.offs_t, self.caps_t, img=self.img_t if with_img else None,
                             count=self.count_t, gate=None if gate is None else dev_i32(np.asarray(gate, np.int32)
                                                                                          .view(np.uint32), self.cuda),
                             live_offs=None if live is None else dev_i64(live, self.cuda), flags=flags,
                             total=total, status=status, **pool.args())
        want = model.m_release(self.buf, self.offs, self.caps, self.img if with_img else None, self.count, gate, live,
                               flags, pool.po, pool.pc, pool.words)
        assert np.array_equal(status.cpu().numpy(), want[0]), (what, "status", status.cpu().numpy(), want[0])
        assert u64(total).tolist() == want[1], (what, "total", u64(total).tolist(), want[1])
        self.check(pool, what)
        return want

    def check(self, pool, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u32(self.img_t).tolist() == self.img, (what, "images")
        if self.count is not None:
            assert u64(self.count_t).tolist() == self.count, (what, "count", u64(self.count_t).tolist(), self.count)
        pool.check(what)
        same_bytes(self.base_t, self.buf, what)


# ------------------------------------------------------------------ 1. release, mixed batches

REL_KINDS = ("ok", "gate", "live", "magic", "small", "misaligned", "outside", "ok")
CLS, PAL, STRIDE = 64, 16, 112


def rel_mixed(n):
    """Entry i of kind REL_KINDS[i % 8] in a slot of STRIDE bytes at a multiple
    of PAL: releasable (capacity CLS .. CLS + 32); valid but gate-failed; valid
    and still live; bad magic; a valid image of capacity CLS - 1; a valid image
    at an offset that is 8 modulo PAL; outside dev_bytes (one by a byte, one
    wrapping 2^64).  Returns (buf, offs, caps, gate, live, kinds)."""
    buf = fill(32 + n * STRIDE + 48)
    offs, caps, gate, live, kinds = [], [], [], [], []
    for i in range(n):
        kind = REL_KINDS[i % 8]
        off, cap = 32 + i * STRIDE, CLS + 16 * (i % 3)
        if kind == "small":
            cap = CLS - 1
        elif kind == "misaligned":
            off += 8
        put_image(buf, off, i % 5, (7 * i) % 30)
        if kind == "magic":
            buf[off] = 0xC0
        elif kind == "outside":
            off, cap = (len(buf) - CLS + 1, CLS) if i % 16 < 8 else ((1 << 64) - 32, CLS)
        offs.append(off)
        caps.append(cap)
        gate.append(-1 if kind == "gate" else 0)
        live.append(off if kind == "live" else off + 16)
        kinds.append(kind)
    return buf, offs, caps, gate, live, kinds


@pytest.mark.parametrize("cut", ["first", "middle", "none"])
@pytest.mark.parametrize("n", [1, 64, 65, BLOCK - 1, BLOCK + 1, 2 * BLOCK + 1])
def test_release_mixed_batches(cuda, n, cut):
    buf, offs, caps, gate, live, kinds = rel_mixed(n)
    ok = [i for i in range(n) if kinds[i] == "ok"]
    room = {"first": 0, "middle": len(ok) // 2, "none": len(ok) + 3}[cut]
    have = 2
    pool = Pool(cuda, have + room, CLS, PAL, entries=[(4096 * 1024, 80), (4097 * 1024, 96)])
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pool, gate=gate, live=live, what=f"release {n} {cut}")
    assert acc == ok[:room] and total == [len(ok), n - len(acc)]
    assert st.tolist() == [0 if i in acc or kinds[i] == "live" else -1 for i in range(n)]
    assert pool.words[0] == have + len(acc)
    for i in acc:
        assert buf[offs[i]] == 0 and buf[offs[i] + 1] == 0 and buf[offs[i] + 24 + i % 5 + (7 * i) % 30] != 0


@pytest.mark.parametrize("words", [[5, 4, CLS, PAL], [0, 8, 23, PAL], [0, 8, CLS, 24], [0, 8, CLS, 8192],
                                   [0, 8, CLS, 0]])
def test_release_into_an_unsound_pool_changes_nothing(cuda, words):
    buf, offs, caps, gate, live, kinds = rel_mixed(65)
    before = buf.copy()
    pool = Pool(cuda, 8, CLS, PAL, words=words)
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(65) as w:
        st, total, acc = e.release(w, pool, gate=gate, live=live, what=f"unsound {words}")
    assert acc == [] and total == [0, 65] and np.array_equal(buf, before)
    assert st.tolist() == [0 if k == "live" else -1 for k in kinds]


@pytest.mark.parametrize("flags", [0, COMPACT])
@pytest.mark.parametrize("count", [0, 700, BLOCK + 1, 5000])
def test_release_looks_at_the_first_count_entries(cuda, count, flags):
    n = BLOCK + 1
    buf, offs, caps, gate, live, kinds = rel_mixed(n)
    pool = Pool(cuda, n, CLS, PAL)
    e = Entries(cuda, buf, offs, caps, count=count)
    m = min(n, count)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pool, gate=gate, flags=flags, what=f"count {count} {flags}")
    assert acc == [i for i in range(m) if kinds[i] in ("ok", "live")] and not st[m:].any()
    assert total == [len(acc), m - len(acc)]
    if flags:
        assert e.count == [m - len(acc), n] and e.offs[m:] == offs[m:]
        assert e.offs[m - len(acc):m] == [0] * len(acc) and e.img[m - len(acc):m] == [model.NO_IMAGE] * len(acc)
    else:
        assert e.count == [count, n] and e.offs == offs


# ------------------------------------------------------------------ 2. CIOA_RELEASE_ZERO

ZERO_CAPS = (24, 25, 39, 40, 41, 4096 + 17)


def test_release_zero_every_residue_and_size(cuda):
    """Slots of 24 .. 4113 bytes at every offset residue modulo 16, and one of
    300 000 bytes, each full of image bytes, 1 .. 16 sentinel bytes between
    them: the whole slot becomes zero and no byte beside it changes."""
    offs, caps, pos = [], [], 5
    for r in range(16):
        for c in ZERO_CAPS:
            pos += (r - pos) % 16 or 16
            offs.append(pos)
            caps.append(c)
            pos += c
    pos += 7
    offs.append(pos)
    caps.append(300000)
    buf = fill(pos + 300000 + 33)
    for o, c in zip(offs, caps):
        put_image(buf, o, min(c - 24, 3), c - 24 - min(c - 24, 3))
    assert {o % 16 for o in offs[:-1]} == set(range(16))
    before = buf.copy()
    n = len(offs)
    pool = Pool(cuda, n, 24, 1)
    e = Entries(cuda, buf, offs, caps)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pool, flags=ZERO, what="zero")
    assert not st.any() and acc == list(range(n)) and pool.po[:n] == offs and pool.pc[:n] == caps
    keep = np.ones(len(buf), bool)
    for o, c in zip(offs, caps):
        assert not buf[o:o + c].any()
        keep[o:o + c] = False
    assert np.array_equal(buf[keep], before[keep]) and buf[keep].all()


# ------------------------------------------------------------------ 3. CIOA_RELEASE_COMPACT

@pytest.mark.parametrize("flags", [COMPACT, COMPACT | ZERO])
@pytest.mark.parametrize("kept", ["none", "all", "alternating", "random", "pool"])
def test_release_compacts_the_list_in_place(cuda, kept, flags):
    """1025 drained chunks; the gate (or, for "pool", the pool's capacity)
    decides which are kept.  The kept entries move to the front in their order,
    the vacated ones are (0, 0, 0xffffffff), the statuses stay where the
    entries were."""
    n = BLOCK + 1
    rng = np.random.default_rng(3)
    buf = fill(32 + n * STRIDE + 48)
    offs, caps = [32 + i * STRIDE for i in range(n)], [CLS + 16 * (i % 3) for i in range(n)]
    for i in range(n):
        put_image(buf, offs[i], i % 5, (7 * i) % 30)
    gate = {"none": [0] * n, "all": [-3] * n, "alternating": [-(i % 2) for i in range(n)],
            "random": [-int(x) for x in rng.integers(0, 2, n)], "pool": [0] * n}[kept]
    pool = Pool(cuda, 300 if kept == "pool" else n, CLS, PAL)
    alloc = n + 3                                  # the list's arrays are longer than the count says
    e = Entries(cuda, buf, offs + [S64] * 3, caps + [S64] * 3, count=n)
    e.count[1] = n
    e.count_t.copy_(dev_i64(e.count, cuda))
    with cio.DevWriter(alloc) as w:
        st, total, acc = e.release(w, pool, gate=gate + [0] * 3, flags=flags, what=f"compact {kept}")
    stay = [i for i in range(n) if i not in set(acc)]
    assert acc == [i for i in range(n) if gate[i] == 0][:pool.words[1]]
    assert st[:n].tolist() == [0 if i in set(acc) else -1 for i in range(n)]
    assert e.offs[:len(stay)] == [offs[i] for i in stay] and e.img[:len(stay)] == [100 + i for i in stay]
    assert e.offs[len(stay):n] == [0] * len(acc) and e.caps[len(stay):n] == [0] * len(acc)
    assert e.img[len(stay):n] == [model.NO_IMAGE] * len(acc) and e.offs[n:] == [S64] * 3
    assert e.count == [len(stay), n] and total == [sum(1 for g in gate if g == 0), len(stay)]


def test_release_without_the_list_images(cuda):
    """dev_img = NULL: offsets and capacities are compacted alone."""
    n = 70
    buf, offs, caps, gate, live, kinds = rel_mixed(n)
    pool = Pool(cuda, n, CLS, PAL)
    e = Entries(cuda, buf, offs, caps, count=n)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pool, gate=gate, flags=COMPACT, with_img=False, what="no images")
    assert len(acc) > 0 and e.img == list(range(100, 100 + n)) and e.count[0] == n - len(acc)


# ------------------------------------------------------------------ 4. double release

@pytest.mark.parametrize("flags", [0, ZERO])
def test_double_release_is_caught(cuda, flags):
    n = 200
    buf = fill(32 + n * STRIDE + 48)
    offs, caps = [32 + i * STRIDE for i in range(n)], [CLS + 16 * (i % 3) for i in range(n)]
    for i in range(n):
        put_image(buf, offs[i], i % 5, (7 * i) % 30)
    pool = Pool(cuda, 2 * n, CLS, PAL)
    e = Entries(cuda, buf, offs, caps, count=n)
    with cio.DevWriter(n) as w:
        st, total, acc = e.release(w, pool, flags=flags, what="first release")
        assert not st.any() and acc == list(range(n)) and pool.words[0] == n
        after = buf.copy()
        st, total, acc = e.release(w, pool, flags=flags, what="second release")
    assert st.tolist() == [-1] * n and acc == [] and total == [0, n]
    assert pool.words[0] == n and np.array_equal(buf, after)


# ------------------------------------------------------------------ 5. rotate from the pool

class PoolState(State):
    """test_gpu_rotate_dev's State with a pool beside the arena."""

    def __init__(self, cuda, buf, offs, caps, arena, pool, **kw):
        super().__init__(cuda, buf, offs, caps, arena, **kw)
        self.pool = pool

    def model(self, need, limit, new_cap, align, flags):
        return model.m_rotate_pool(self.buf, self.offs, self.caps, need, limit, new_cap, align, self.arena, self.lo,
                                   self.lc, self.li, self.count, self.pool.po, self.pool.pc, self.pool.words,
                                   flags=flags, crc_cur=self.crc)

    def rotate(self, w, need=None, recs=None, limit=0, new_cap=24, align=16, flags=CK, what=""):
        o = self.outs()
        kw = dict(limit=limit, new_cap=new_cap, align=align, flags=flags, **self.lists(), **self.pool.args(), **o)
        if recs is None:
            cf.rotate_pool_batch_dev(w, self.base_t, self.offs_t, self.caps_t,
                                     None if need is None else dev_i64(need, self.cuda), **kw)
            need = [] if need is None else need
        else:
            cf.rotate_pool_records_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_i32(recs[0], self.cuda),
                                             dev_i64(recs[1], self.cuda), **kw)
            need = model.needs_of(recs[0], recs[1], self.n)
        want = self.model(need, limit, new_cap, align, flags)
        self.compare(o, want[:3], what)
        return want

    def check(self, what=""):
        super().check(what)
        self.pool.check(what)


def free_slots(buf, count, cap_of, pal):
    """`count` released slots behind buf: sentinel bytes, bytes 0..1 zero, slot
    k of cap_of(k) bytes at a multiple of pal.  Returns (buf, entries)."""
    pos, entries = len(buf), []
    for k in range(count):
        pos = gmodel.round_up(pos + 1 + k % 5, pal)
        entries.append((pos, cap_of(k)))
        pos += cap_of(k)
    out = fill(pos + 37)
    out[:len(buf)] = buf
    for o, _ in entries:
        out[o:o + 2] = 0
    return out, entries


def reach_of(n, limit):
    return sum(1 for i in range(n) if KINDS[i % 8] in (("room", "limit", "cut") if limit else ("room", "cut")))


@pytest.mark.parametrize("fsel", ["0", "1", "reach-1", "reach", "reach+3"])
@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_rotate_pool_mixed_batches(cuda, n, align, fsel):
    flags, limit = [(CK, LIMIT), (0, LIMIT), (CK, 0)][(n + align + len(fsel)) % 3]
    buf, offs, caps, arena, need, status, rotated = mixed(n, limit, align)
    reach = reach_of(n, limit)
    F = max(0, {"0": 0, "1": 1, "reach-1": reach - 1, "reach": reach, "reach+3": reach + 3}[fsel])
    buf, entries = free_slots(buf, F, lambda k: NEW_CAP + 8 * (k % 3), align)
    pool = Pool(cuda, F + 2, NEW_CAP, align, entries=entries)
    s = PoolState(cuda, buf, offs, caps, arena, pool, list_cap=n + 1, have=1)
    with cio.DevWriter(n) as w:
        st, total, rot, fp = s.rotate(w, need, limit=limit, new_cap=NEW_CAP, align=align, flags=flags,
                                      what=f"pool mixed {n} {align} {fsel}")
        assert total[1] == reach and fp == min(F, len(rot)) and pool.words[0] == F - fp
        for j in range(fp):                       # the pool is a stack, and the image gets the slot's whole capacity
            assert (s.offs[rot[j]], s.caps[rot[j]]) == entries[F - 1 - j]
        if F >= reach:
            assert total[0] == 0 and len(rot) == reach and s.arena == arena
        # the same call again: the fresh images are empty, and an empty image is never rotated
        st2, total2, rot2, fp2 = s.rotate(w, need, limit=limit, new_cap=NEW_CAP, align=align, flags=flags,
                                          what="again")
        assert rot2 == [] and fp2 == 0 and total2[1] == reach - len(rot)


@pytest.mark.parametrize("mode", ["list in the pool part", "list in the arena part", "arena", "list full"])
def test_rotate_pool_cuts(cuda, mode):
    """7 full images and one that is not, 3 pool entries.  The list ends inside
    the pool part (2 entries), or inside the arena part (5), or the arena ends
    one byte short of its third slot (3 + 2 rotate), or the list is full."""
    align, new_cap = 64, 200
    slot = gmodel.round_up(new_cap, align)
    items = [(i, 50 + 30 * i, 5) for i in range(7)] + [(0, 10, 50)]
    need = [6 + 100 * i for i in range(7)] + [3]
    buf, offs, caps, arena = layout(items, 20 * slot)
    top, base = arena[0], gmodel.round_up(arena[0], align)
    fit = {"list in the pool part": 2, "list in the arena part": 5, "arena": 5, "list full": 0}[mode]
    end = base + 2 * slot + slot - 1 if mode == "arena" else arena[1]
    buf, entries = free_slots(buf, 3, lambda k: 256 + 64 * k, 128)
    pool = Pool(cuda, 8, 256, 128, entries=entries)
    s = PoolState(cuda, buf, offs, caps, [top, end], pool, list_cap=2 + (7 if mode == "arena" else fit), have=2,
                  alloc=20)
    with cio.DevWriter(8) as w:
        st, total, rot, fp = s.rotate(w, need, new_cap=new_cap, align=align, what=mode)
    assert rot == list(range(fit)) and fp == min(fit, 3) and st.tolist() == [0] * fit + [-1] * (7 - fit) + [0]
    assert total == [base - top + 4 * slot, 7] and pool.words[0] == 3 - fp
    assert s.arena[0] == (base + (fit - 3) * slot if fit > 3 else top) and s.count[0] == 2 + fit


@pytest.mark.parametrize("why", ["new_cap above the class", "alignment", "unsound"])
def test_rotate_pool_that_cannot_be_used_is_plain_rotate(cuda, why):
    n, align = 65, 16
    buf, offs, caps, arena, need, status, rotated = mixed(n, LIMIT, align)
    buf, entries = free_slots(buf, 4, lambda k: NEW_CAP + 16, 16)
    words = {"new_cap above the class": [4, 6, NEW_CAP - 1, 16], "alignment": [4, 6, NEW_CAP, 8],
             "unsound": [4, 3, NEW_CAP, 16]}[why]
    pool = Pool(cuda, 6, NEW_CAP, 16, entries=entries, words=words)
    s = PoolState(cuda, buf, offs, caps, arena, pool, list_cap=n + 1, have=1)
    plain = State(cuda, buf.copy(), offs, caps, arena, list_cap=n + 1, have=1)
    with cio.DevWriter(n) as w:
        st, total, rot, fp = s.rotate(w, need, limit=LIMIT, new_cap=NEW_CAP, align=align, what=why)
        pst, ptotal, prot = plain.rotate(w, need, limit=LIMIT, new_cap=NEW_CAP, align=align, what="plain")
    assert fp == 0 and rot == rotated == prot and st.tolist() == status and total == ptotal and pool.words == words
    assert np.array_equal(s.buf, plain.buf) and s.offs == plain.offs and s.arena == plain.arena and s.li == plain.li


def pool_records_state(cuda, F):
    s0 = records_state(cuda)
    buf, entries = free_slots(s0.buf, F, lambda k: 128 + 16 * (k % 4), 16)
    return PoolState(cuda, buf, s0.offs, s0.caps, s0.arena, Pool(cuda, F + 5, 128, 16, entries=entries))


def test_rotate_pool_records_cross_wave_and_workgroup_boundaries(cuda):
    """test_gpu_rotate_dev's runs of 1 .. 1000 records per image: the records
    variant against the model and against the need variant fed the model's
    sums, 3 rotations from the pool and the others from the arena."""
    rng = np.random.default_rng(5)
    rec_img = list(rng.integers(0, 300, 37))
    for rep in range(3):
        for k, run in enumerate((1, 2, 63, 64, 65, 1000)):
            rec_img += [10 * k + rep] * run
    rec_img = np.asarray(rec_img, np.uint32)
    rec_lens = rng.integers(0, 3, len(rec_img)).astype(np.uint64)
    rec_lens[100] = 1 << 40                       # clamped to 2^32
    a, b = pool_records_state(cuda, 3), pool_records_state(cuda, 3)
    with cio.DevWriter(len(rec_img)) as w:
        st, total, rot, fp = a.rotate(w, recs=(rec_img, rec_lens), new_cap=128, align=16, what="runs, records")
        b.rotate(w, model.needs_of(rec_img, rec_lens, 300), new_cap=128, align=16, what="runs, needs")
    assert not st.any() and fp == 3 < len(rot) < 300 and a.pool.words[0] == 0
    assert a.offs == b.offs and a.li == b.li and a.crc == b.crc and np.array_equal(a.buf, b.buf)


@pytest.mark.parametrize("at", [0, 256, 2999])
def test_rotate_pool_malformed_records_list_changes_nothing(cuda, at):
    rng = np.random.default_rng(at)
    s = pool_records_state(cuda, 9)
    arena, before = list(s.arena), s.buf.copy()
    rec_img = rng.integers(0, 300, 3000).astype(np.uint32)
    rec_img[at] = 300 + (at % 2) * 0xFFFFFED3
    rec_lens = rng.integers(1, 100, 3000).astype(np.uint64)
    with cio.DevWriter(3000) as w:
        st, total, rot, fp = s.rotate(w, recs=(rec_img, rec_lens), new_cap=128, what=f"malformed at {at}")
        assert st.tolist() == [-1] * 300 and total == [0, 0] and s.arena == arena and s.count[0] == 0
        assert s.pool.words[0] == 9 and np.array_equal(s.buf, before)
        rec_img[at] = 0                           # the writer is not left marked: the same list, mended, rotates
        st, total, rot, fp = s.rotate(w, recs=(rec_img, rec_lens), new_cap=128, what="mended")
        assert not st.any() and fp == 9 and len(rot) > 9


# ------------------------------------------------------------------ 6. grow's leftovers

def test_grow_leftovers_enter_the_pool(cuda):
    """grow_batch_dev with dev_prev_*, then a release of the previous slots
    with dev_live_offs = dev_img_offs: exactly the old slots of the moved images
    enter the pool; an image that stayed is still live and is kept."""
    n = 40
    items = [(i % 4, 10 + i, 64 + 40 * (i % 3)) for i in range(n)]
    need = [[0, 30, 200, 500][i % 4] for i in range(n)]
    buf, offs, caps, arena = layout(items, 1 << 16)
    base_t, offs_t, caps_t, arena_t = dev_u8(buf, cuda), dev_i64(offs, cuda), dev_i64(caps, cuda), dev_i64(arena, cuda)
    prev_o, prev_c = dev_i64([0] * n, cuda), dev_i64([0] * n, cuda)
    pool = Pool(cuda, n, 24, 1)
    with cio.DevWriter(n) as w:
        gst, gtotal = cf.grow_batch_dev(w, base_t, offs_t, caps_t, dev_i64(need, cuda), arena_t, realloc=256, page=64,
                                        align=16, prev_offs=prev_o, prev_caps=prev_c)
        new_offs, new_caps = list(offs), list(caps)
        gwant = gmodel.m_grow(buf, new_offs, new_caps, need, arena, realloc=256, page=64, align=16)
        assert not gwant[0].any() and np.array_equal(gst.cpu().numpy(), gwant[0])
        assert u64(prev_o).tolist() == offs and u64(prev_c).tolist() == caps and u64(offs_t).tolist() == new_offs
        e = Entries(cuda, buf, offs, caps)
        e.base_t, e.offs_t, e.caps_t = base_t, prev_o, prev_c
        st, total, acc = e.release(w, pool, live=new_offs, what="leftovers")
    moved = [i for i in range(n) if new_offs[i] != offs[i]]
    assert 0 < len(moved) < n and acc == moved and not st.any() and total == [len(moved), n - len(moved)]
    assert pool.po[:len(moved)] == [offs[i] for i in moved] and pool.pc[:len(moved)] == [caps[i] for i in moved]
    for i in range(n):                            # every live image is still an image
        assert model.image_check(buf, len(buf), new_offs[i], new_caps[i]) is not None


# ------------------------------------------------------------------ 7. the reference pin

def test_reference_fixture_in_a_recycled_slot(cuda):
    """A slot of the fixture's size, full of another chunk's bytes, is released
    with CIOA_RELEASE_ZERO; a small full image with c03_meta_content's metadata
    rotates into it; the fixture's writes and a seal follow.  The image in the
    recycled slot has the manifest's SHA-256 -- its tail is the file's zero
    tail -- and nothing beside the slot changed."""
    spec = [c for c in MANIFEST["chunks"] if c["name"] == "c03_meta_content"][0]
    size, ld = spec["size"], spec["load"]
    meta = spec["ops"][0]["meta"].encode()
    writes = [pattern(o["len"], o["seed"]) for o in spec["ops"] if o["op"] == "write"]
    content = sum(len(x) for x in writes)
    small, slot_off = 24 + len(meta) + 8, 4096
    buf = fill(slot_off + size + 64 + 77)
    put_image(buf, slot_off, 5, size - 24 - 5)    # the drained chunk: every byte of the slot is in use
    crc0 = m_init(buf, 48, meta)
    pool = Pool(cuda, 2, size, 16)
    top = slot_off + size + 16
    s = PoolState(cuda, buf, [48], [small], [top, top + 48], pool, crc=[crc0], list_cap=1)
    src_t = dev_u8(np.frombuffer(b"junk" + b"".join(writes), np.uint8).copy(), cuda)
    with cio.DevWriter(1) as w:
        e = Entries(cuda, buf, [slot_off], [size])
        e.base_t = s.base_t
        st, total, acc = e.release(w, pool, flags=ZERO, what="release the slot")
        assert acc == [0] and not buf[slot_off:slot_off + size].any() and buf[slot_off + size] != 0

        def write(pos, ln, what):
            wst = cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, dev_i64([pos], cuda), dev_i64([ln], cuda),
                                     s.crc_t, flags=CK)
            assert not wst.cpu().numpy().any()
            s.crc[0] = m_write(s.buf, s.offs[0], bytes(src_t[pos:pos + ln].cpu().numpy()), s.crc[0])
            s.check(what)

        write(0, 4, "four bytes into the small image")
        st, total, rot, fp = s.rotate(w, [8], new_cap=size, align=16, what="rotate into the recycled slot")
        assert st.tolist() == [0] and rot == [0] and fp == 1 and total == [0, 1]
        assert (s.offs[0], s.caps[0]) == (slot_off, size) and s.arena[0] == top and pool.words[0] == 0
        pos = 4
        for k, x in enumerate(writes):
            write(pos, len(x), f"write {k}")
            pos += len(x)
        assert s.crc[0] == ld["crc_cur"]
        assert not cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.crc_t, flags=CK).cpu().numpy().any()
        m_seal(s.buf, slot_off, s.crc[0])
        s.check("sealed")
    got = s.base_t.cpu().numpy()
    assert hashlib.sha256(got[slot_off:slot_off + size].tobytes()).hexdigest() == spec["sha256"]
    used = 24 + len(meta) + content
    assert not got[slot_off + used:slot_off + size].any() and got[slot_off + size:].all()


# ------------------------------------------------------------------ 8. the steady state, captured

def steady_layout(n, new_cap, align, arena_room):
    """n empty images of new_cap bytes with 3 bytes of metadata at multiples of
    align, the arena behind them."""
    slot = gmodel.round_up(new_cap, align)
    offs, caps = [2 * align + i * slot for i in range(n)], [new_cap] * n
    top = offs[-1] + slot
    buf = fill(top + arena_room + 41)
    crc = [m_init(buf, offs[i], bytes([1 + i] * 3)) for i in range(n)]
    return buf, offs, caps, [top, top + arena_room], crc


def empty_list(s):
    """The list as a consumer that passes its whole capacity wants it: every
    entry (0, 0, 0xffffffff), which verify and read reject by cap < 24."""
    k = len(s.lo)
    s.lo[:], s.lc[:], s.li[:] = [0] * k, [0] * k, [model.NO_IMAGE] * k
    s.lo_t.zero_()
    s.lc_t.zero_()
    s.li_t.fill_(-1)


def drain_model(s, drained):
    """What the read of the list's chunks gives, from the model's buffer."""
    for e in range(s.count[0]):
        meta, content = model.image_check(s.buf, len(s.buf), s.lo[e], s.lc[e])
        drained[s.li[e]] += s.buf[s.lo[e] + 24 + meta:s.lo[e] + 24 + meta + content].tobytes()


def test_steady_state_chain_replays_in_a_bounded_buffer(cuda):
    """rotate_pool -> grow -> write -> verify over the list's whole capacity ->
    read_packed gated by verify -> release(ZERO | COMPACT, gated by the read),
    captured once on one stream: a warm-up and 40 replays, each compared with
    the model in everything.  No status but CIO_OK, the arena's top stands
    still over the last 30 replays, and the drained bytes followed by the live
    images' contents are what was written.  (On the model alone, seed 7: no
    cut in 40 rounds, the top stops after round 3 at 3808 of 13120 arena
    bytes; without the pool the arena runs out after round 7.)"""
    import torch
    n, size, limit, align, list_cap, pool_cap = 12, 300, 500, 32, 12, 24
    new_cap = 24 + 3 + limit
    slot = gmodel.round_up(new_cap, align)
    assert slot == 544
    rng = np.random.default_rng(7)
    buf, offs, caps, arena, crc = steady_layout(n, new_cap, align, 64 + 2 * n * slot)
    pool = Pool(cuda, pool_cap, new_cap, align)
    s = PoolState(cuda, buf, offs, caps, arena, pool, crc=crc, list_cap=list_cap, alloc=list_cap)
    empty_list(s)
    so = np.arange(n, dtype=np.uint64) * (size + 3)
    src_t = dev_u8(np.zeros(n * (size + 3) + 16, np.uint8), cuda)
    so_t, sl_t = dev_i64(so, cuda), dev_i64(np.zeros(n, np.uint64), cuda)
    o = s.outs()
    go = dict(total=dev_i64([0], cuda), status=torch.full((n,), 99, dtype=torch.int32, device=cuda))
    wst = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    out_t = torch.zeros(list_cap * limit + 64, dtype=torch.uint8, device=cuda)
    rd = dict(out_offs=dev_i64([0] * list_cap, cuda), out_lens=dev_i64([0] * list_cap, cuda),
              total=dev_i64([0], cuda), status=torch.full((list_cap,), 99, dtype=torch.int32, device=cuda))
    rl = dict(total=dev_i64([0, 0], cuda), status=torch.full((list_cap,), 99, dtype=torch.int32, device=cuda))
    wrote, drained, got = [b""] * n, [b""] * n, [b""] * n

    def stage(k):
        """Round k on the model.  Returns the rotate's result, the list as the
        drain sees it, and the release's result."""
        lens = rng.integers(1, size + 1, n).astype(np.uint64)
        lens[k % n] = 0
        src = np.zeros(src_t.numel(), np.uint8)
        for i in range(n):                        # one draw per image, behind the lengths
            src[int(so[i]):int(so[i]) + int(lens[i])] = rng.integers(0, 256, int(lens[i]), dtype=np.uint8)
        src_t.copy_(torch.from_numpy(src))
        sl_t.copy_(torch.from_numpy(lens.view(np.int64)))
        want = s.model(lens, limit, new_cap, align, CK)
        gwant = gmodel.m_grow(s.buf, s.offs, s.caps, lens, s.arena, realloc=512, page=256, align=align)
        assert not gwant[0].any()
        for i in range(n):
            data = src[int(so[i]):int(so[i]) + int(lens[i])].tobytes()
            s.crc[i] = m_write(s.buf, s.offs[i], data, s.crc[i])
            wrote[i] += data
        drain_model(s, drained)
        listed = (s.count[0], list(s.li))
        rwant = model.m_release(s.buf, s.lo, s.lc, s.li, s.count, [0] * list_cap, None, ZERO | COMPACT, pool.po,
                                pool.pc, pool.words)
        return want, listed, rwant

    def call():
        cf.rotate_pool_batch_dev(w, s.base_t, s.offs_t, s.caps_t, sl_t, limit=limit, new_cap=new_cap, align=align,
                                 flags=CK, **s.lists(), **pool.args(), **o)
        cf.grow_batch_dev(w, s.base_t, s.offs_t, s.caps_t, sl_t, s.arena_t, realloc=512, page=256, align=align, **go)
        cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, so_t, sl_t, s.crc_t, flags=CK, status=wst)
        vst = cf.verify_batch_dev(plan, s.base_t, s.lo_t, s.lc_t, flags=CK)[0]
        cf.read_packed_batch_dev(w, s.base_t, s.lo_t, s.lc_t, cf.CIOA_READ_CONTENT, out_t, gate=vst, **rd)
        cf.release_batch_dev(w, s.base_t, s.lo_t, s.lc_t, img=s.li_t, count=s.count_t, gate=rd["status"],
                             flags=ZERO | COMPACT, **pool.args(), **rl)
        return vst

    def settle(k, vst, want, listed, rwant):
        torch.cuda.synchronize()
        what = f"round {k}"
        assert np.array_equal(o["status"].cpu().numpy(), want[0]) and not want[0].any(), (what, "rotate", want[0])
        assert u64(o["total"]).tolist() == want[1], (what, "rotate total")
        assert not go["status"].cpu().numpy().any() and not wst.cpu().numpy().any(), (what, "grow, write")
        m, owners = listed
        assert not vst.cpu().numpy()[:m].any() and not rd["status"].cpu().numpy()[:m].any(), (what, "verify, read")
        assert vst.cpu().numpy()[m:].all(), (what, "an empty list entry passed verify")
        assert np.array_equal(rl["status"].cpu().numpy(), rwant[0]) and not rwant[0].any(), (what, "release")
        assert u64(rl["total"]).tolist() == rwant[1] == [m, 0], (what, "release total")
        packed, po, pl = out_t.cpu().numpy(), u64(rd["out_offs"]), u64(rd["out_lens"])
        for e in range(m):
            got[owners[e]] += packed[int(po[e]):int(po[e] + pl[e])].tobytes()
        s.check(what)

    tops = []
    with cio.DevWriter(max(n, list_cap)) as w, cio.Crc32DevPlan(list_cap) as plan:
        staged = stage(0)
        vst = call()                              # warm-up outside the capture (a round like the others)
        settle(0, vst, *staged)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            vst = call()
        torch.cuda.synchronize()
        s.check("capture runs nothing")
        for k in range(1, 41):
            staged = stage(k)
            for t in (o["status"], go["status"], wst, rd["status"], rl["status"]):
                t.fill_(99)
            graph.replay()
            settle(k, vst, *staged)
            tops.append(s.arena[0])
        del graph
    assert len(set(tops[-30:])) == 1 and tops[-1] < s.arena[1]
    assert got == drained
    for i in range(n):
        meta, content = model.image_check(s.buf, len(s.buf), s.offs[i], s.caps[i])
        live = s.base_t.cpu().numpy()[s.offs[i] + 24 + meta:s.offs[i] + 24 + meta + content].tobytes()
        assert got[i] + live == wrote[i], i


# ------------------------------------------------------------------ 9. rounds without a graph

def test_rounds_of_records_with_a_small_pool(cuda):
    """Five images through eight rounds of rotate_pool_records -> grow_records
    -> write_records_ungrouped -> verify -> read_packed -> release, as
    test_lifecycle_rotate_grow_append, with a pool of two entries: a release of
    more than two chunks is cut by the pool's capacity and retried into a
    second pool of the same class, and a call with more rotations than the pool
    holds serves them from both the pool and the arena.  Every call equals the
    model, and the drained bytes followed by the live images' contents are the
    records of each image in order."""
    import torch
    n_img, n_rec, rounds, limit, new_cap = 5, 20, 8, 150, 24 + 9 + 150
    rng = np.random.default_rng(12)
    metas = [bytes(rng.integers(1, 255, 2 * i + 1, dtype=np.uint8)) for i in range(n_img)]
    items = [(0, 0, new_cap - 24) for m in metas]     # every slot of the pool's class, at a multiple of 16
    buf, offs, caps, arena = layout(items, 1 << 16, residue=lambda i: 0)
    buf = fill(len(buf))
    pool, spare = Pool(cuda, 2, new_cap, 16), Pool(cuda, 64, new_cap, 16)
    s = PoolState(cuda, buf, offs, caps, arena, pool, list_cap=16, alloc=16)
    empty_list(s)
    msrc = np.frombuffer(b"".join(metas) + b"\0", np.uint8).copy()
    mlens = np.asarray([len(m) for m in metas], np.uint64)
    moffs = np.concatenate(([0], np.cumsum(mlens)[:-1])).astype(np.uint64)
    wrote, got = [b""] * n_img, [b""] * n_img
    both, cut_releases = 0, 0
    out_t = torch.zeros(16 * (limit + n_rec * 60) + 64, dtype=torch.uint8, device=cuda)
    with cio.DevWriter(max(n_img, n_rec)) as w, cio.Crc32DevPlan(16) as plan:
        st, crc = cf.init_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(msrc, cuda), dev_i64(moffs, cuda),
                                    dev_i64(mlens, cuda), flags=CK, crc_cur=s.crc_t)
        assert not st.cpu().numpy().any()
        s.crc = [m_init(s.buf, offs[i], m) for i, m in enumerate(metas)]
        s.check("init")
        for k in range(rounds):
            rec_img = rng.integers(0, n_img, n_rec).astype(np.uint32)
            rec_lens = rng.integers(0, 61, n_rec).astype(np.uint64)
            rec_offs = np.concatenate(([0], np.cumsum(rec_lens)[:-1])).astype(np.uint64)
            src = rng.integers(0, 256, int(rec_lens.sum()) + 16, dtype=np.uint8)
            st, total, rot, fp = s.rotate(w, recs=(rec_img, rec_lens), limit=limit, new_cap=new_cap, align=16,
                                          what=f"round {k}: rotate")
            assert not st.any()
            both += 0 < fp < len(rot)
            img_t, lens_t = dev_i32(rec_img, cuda), dev_i64(rec_lens, cuda)
            gst, gtotal = cf.grow_records_batch_dev(w, s.base_t, s.offs_t, s.caps_t, img_t, lens_t, s.arena_t,
                                                    realloc=256, page=64, align=16)
            gwant = gmodel.m_grow(s.buf, s.offs, s.caps, gmodel.needs_of(rec_img, rec_lens, n_img), s.arena,
                                  realloc=256, page=64, align=16)
            assert np.array_equal(gst.cpu().numpy(), gwant[0]) and not gwant[0].any()
            s.check(f"round {k}: grow")
            ist, rst = cf.write_records_ungrouped_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(src, cuda), img_t,
                                                            dev_i64(rec_offs, cuda), lens_t, s.crc_t, flags=CK)
            assert not rst.cpu().numpy().any() and not ist.cpu().numpy().any()
            for r in range(n_rec):
                i, data = int(rec_img[r]), src[int(rec_offs[r]):int(rec_offs[r] + rec_lens[r])].tobytes()
                s.crc[i] = m_write(s.buf, s.offs[i], data, s.crc[i])
                wrote[i] += data
            s.check(f"round {k}: append")
            m, owners = s.count[0], list(s.li)
            vst = cf.verify_batch_dev(plan, s.base_t, s.lo_t, s.lc_t, flags=CK)[0]
            rst, o_offs, o_lens, rtotal = cf.read_packed_batch_dev(w, s.base_t, s.lo_t, s.lc_t, cf.CIOA_READ_CONTENT,
                                                                   out_t, gate=vst)
            assert not rst.cpu().numpy()[:m].any() and rst.cpu().numpy()[m:].all()
            packed, o_offs, o_lens = out_t.cpu().numpy(), u64(o_offs), u64(o_lens)
            for e in range(m):
                got[owners[e]] += packed[int(o_offs[e]):int(o_offs[e] + o_lens[e])].tobytes()
            lst = Entries(cuda, s.buf, s.lo, s.lc, img=s.li, count=m)
            lst.count[1] = s.count[1]
            lst.base_t, lst.offs_t, lst.caps_t, lst.img_t, lst.count_t = s.base_t, s.lo_t, s.lc_t, s.li_t, s.count_t
            rwant = lst.release(w, pool, gate=rst.cpu().numpy().tolist(), flags=ZERO | COMPACT,
                                what=f"round {k}: release")
            if rwant[1][1]:                       # cut by the pool's capacity: the kept chunks go to the spare pool
                cut_releases += 1
                assert rwant[1] == [m, m - len(rwant[2])] and lst.count[0] == rwant[1][1]
                again = lst.release(w, spare, flags=ZERO | COMPACT, what=f"round {k}: retry")
                assert len(again[2]) == rwant[1][1] and lst.count[0] == 0
            s.lo, s.lc, s.li, s.count = lst.offs, lst.caps, lst.img, lst.count
            s.check(f"round {k}: released")
    assert both >= 1 and cut_releases >= 1
    for i in range(n_img):
        meta, content = model.image_check(s.buf, len(s.buf), s.offs[i], s.caps[i])
        assert got[i] + s.buf[s.offs[i] + 24 + meta:s.offs[i] + 24 + meta + content].tobytes() == wrote[i], i
