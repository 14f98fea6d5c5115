"""Rotating full chunk images in device memory
(include/chunkio_amd/cio_write_dev_rotate.h) against the numpy model
(rotate_dev_model.py).  Every rotate call is compared in ALL it may touch: the
WHOLE buffer (a position-dependent sentinel fills every slack and the arena, so
a stray or missing store shows), both arrays, crc_cur, the arena, the three
list arrays including the entries that must stay untouched, the count,
dev_total and the statuses.  State, sentinel and layout are those of
test_gpu_grow_dev.py."""
import hashlib
import json
import os
import zlib

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import grow_dev_model as gmodel
import rotate_dev_model as model
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, layout, u64
from write_dev_move_model import m_init, m_seal, m_write, pattern

pytestmark = pytest.mark.gpu

CK = cf.CIO_CHECKSUM
BLOCK = 1024                                  # kRotBlock: images per workgroup of the header kernel
M32 = 0xFFFFFFFF
S64, S32 = 0x7777777777777777, 0x77777777     # what an unwritten list entry holds
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "chunks", "manifest.json")) as _f:
    MANIFEST = json.load(_f)


def u32(t):
    return t.cpu().numpy().view(np.uint32).copy()


class State:
    """Images, an arena and a list of finished chunks on the device, the host
    copy beside them; all are carried from call to call.  The list arrays hold
    `alloc` entries, of which the call may use count[1]."""

    def __init__(self, cuda, buf, offs, caps, arena, crc=None, list_cap=None, have=0, alloc=None):
        self.cuda, self.buf = cuda, buf
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.n = len(self.offs)
        self.arena = [int(arena[0]), int(arena[1])]
        self.crc = [int(x) for x in (crc if crc is not None else (np.arange(self.n) * 2654435761 + 99) % (1 << 32))]
        list_cap = self.n if list_cap is None else list_cap
        alloc = max(list_cap, have, self.n) + 2 if alloc is None else alloc
        self.lo, self.lc, self.li, self.count = [S64] * alloc, [S64] * alloc, [S32] * alloc, [have, list_cap]
        self.base_t = dev_u8(buf, cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.arena_t, self.crc_t = dev_i64(self.arena, cuda), dev_i32(self.crc, cuda)
        self.lo_t, self.lc_t, self.li_t = dev_i64(self.lo, cuda), dev_i64(self.lc, cuda), dev_i32(self.li, cuda)
        self.count_t = dev_i64(self.count, cuda)

    def set_arena(self, arena):
        self.arena = [int(arena[0]), int(arena[1])]
        self.arena_t.copy_(dev_i64(self.arena, self.cuda))

    def set_list_cap(self, cap):
        self.count[1] = int(cap)
        self.count_t.copy_(dev_i64(self.count, self.cuda))

    def outs(self):
        import torch
        return dict(total=dev_i64([0x55, 0x55], self.cuda),
                    status=torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda))

    def lists(self):
        return dict(arena=self.arena_t, out_offs=self.lo_t, out_caps=self.lc_t, out_img=self.li_t,
                    out_count=self.count_t, crc_cur=self.crc_t)

    def model(self, need, limit, new_cap, align, flags):
        return model.m_rotate(self.buf, self.offs, self.caps, need, limit, new_cap, align, self.arena, self.lo,
                              self.lc, self.li, self.count, flags=flags, crc_cur=self.crc)

    def rotate(self, w, need=None, recs=None, limit=0, new_cap=24, align=16, flags=CK, what=""):
        """One device call (the records variant with recs = (rec_img,
        rec_lens)) and the model's, compared in everything.  Returns the
        model's (status, total, rotated)."""
        o = self.outs()
        kw = dict(limit=limit, new_cap=new_cap, align=align, flags=flags, **self.lists(), **o)
        if recs is None:
            cf.rotate_batch_dev(w, self.base_t, self.offs_t, self.caps_t,
                                None if need is None else dev_i64(need, self.cuda), **kw)
            need = [] if need is None else need
        else:
            cf.rotate_records_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_i32(recs[0], self.cuda),
                                        dev_i64(recs[1], self.cuda), **kw)
            need = model.needs_of(recs[0], recs[1], self.n)
        want = self.model(need, limit, new_cap, align, flags)
        self.compare(o, want, what)
        return want

    def compare(self, o, want, what):
        assert np.array_equal(o["status"].cpu().numpy(), want[0]), (what, "status", o["status"].cpu().numpy(), want[0])
        assert u64(o["total"]).tolist() == want[1], (what, "total", u64(o["total"]).tolist(), want[1])
        self.check(what)

    def check(self, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u32(self.crc_t).tolist() == self.crc, (what, "crc_cur")
        assert u64(self.arena_t).tolist() == self.arena, (what, "arena", u64(self.arena_t).tolist(), self.arena)
        assert u64(self.count_t).tolist() == self.count, (what, "count", u64(self.count_t).tolist(), self.count)
        assert u64(self.lo_t).tolist() == self.lo, (what, "list offsets")
        assert u64(self.lc_t).tolist() == self.lc, (what, "list capacities")
        assert u32(self.li_t).tolist() == self.li, (what, "list images")
        got = self.base_t.cpu().numpy()
        if not np.array_equal(got, self.buf):
            bad = np.flatnonzero(got != self.buf)
            raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:6]} of {len(got)}")


# ------------------------------------------------------------------ 1. mixed batches

KINDS = ("noneed", "notfull", "room", "limit", "empty", "magic", "meta", "cut")
NEW_CAP, LIMIT = 96, 150


def mixed(n, limit, align):
    """Image i of kind KINDS[i % 8], those of the hand-written batch of
    test_rotate_dev_abi.py: no need (and, with limit 0, not an image: it is
    not read); not full; full by room; over the limit by one byte with room to
    spare; empty and over its room; bad magic; full with metadata that does
    not fit NEW_CAP; full -- and the arena ends one byte short of the slot of
    the LAST image of that kind.  Returns (buf, offs, caps, arena, need,
    expected statuses, expected rotated)."""
    rng = np.random.default_rng(n)
    items, need = [], []
    for i in range(n):
        kind = KINDS[i % 8]
        meta = int(rng.integers(0, 41)) * (i % 3 == 0)
        content, room = 1 + int(rng.integers(0, 60)), int(rng.integers(0, 30))
        nd = room + 1
        if kind == "noneed":
            nd = 0
        elif kind == "notfull":
            room += 20
            nd = room - 1
        elif kind == "limit":
            content = 1 + int(rng.integers(0, 100))
            nd = LIMIT + 1 - content
            room = nd + 5
        elif kind == "empty":
            content = 0
        elif kind == "meta":
            meta = NEW_CAP - 24 + 1
        items.append((meta, content, room))
        need.append(nd)
    reach = [i for i in range(n) if KINDS[i % 8] in (("room", "limit", "cut") if limit else ("room", "cut"))]
    last = max([i for i in range(n) if KINDS[i % 8] == "cut"], default=None)
    fit = len(reach) if last is None else reach.index(last)
    slot = gmodel.round_up(NEW_CAP, align)
    buf, offs, caps, arena = layout(items, 3 * align + (len(reach) + 1) * slot)
    arena[1] = gmodel.round_up(arena[0], align) + fit * slot + slot - 1
    for i in range(n):
        if KINDS[i % 8] == "magic" or (KINDS[i % 8] == "noneed" and limit == 0):
            buf[offs[i] + 1] = 0x01
    status = [-1 if KINDS[i % 8] in ("magic", "meta") or i in reach[fit:] else 0 for i in range(n)]
    return buf, offs, caps, arena, need, status, reach[:fit]


@pytest.mark.parametrize("flags,limit", [(CK, LIMIT), (0, LIMIT), (CK, 0)])
@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_mixed_batches(cuda, n, align, flags, limit):
    buf, offs, caps, arena, need, status, rotated = mixed(n, limit, align)
    s = State(cuda, buf, offs, caps, arena, list_cap=n + 1, have=1)
    with cio.DevWriter(n) as w:
        st, total, rot = s.rotate(w, need, limit=limit, new_cap=NEW_CAP, align=align, flags=flags,
                                  what=f"mixed {n} {align} {flags} {limit}")
        assert st.tolist() == status and rot == rotated
        assert s.count == [1 + len(rotated), n + 1] and s.li[1:1 + len(rotated)] == rotated and s.li[0] == S32
        # the same call again: the fresh images are empty and an empty image is never rotated; the cut images are
        # still full and cut again, one byte short; nothing changes
        top = s.arena[0]
        st2, total2, rot2 = s.rotate(w, need, limit=limit, new_cap=NEW_CAP, align=align, flags=flags, what="again")
        assert st2.tolist() == status and rot2 == [] and s.arena[0] == top and total2[1] == total[1] - len(rotated)


# ------------------------------------------------------------------ 2. the cut

@pytest.mark.parametrize("mode", ["arena", "list", "both"])
@pytest.mark.parametrize("fit", range(8))
def test_cut_and_retry(cuda, fit, mode):
    """7 full images and one that is not.  The arena ends exactly behind the
    first `fit` slots and one byte short of the next; or the list ends after
    `fit` entries; or both end, at different places, and the nearer one cuts.
    The cut images stay byte for byte, unsealed and valid; a retry sized from
    dev_total rotates the rest."""
    align, new_cap = 64, 200
    slot = gmodel.round_up(new_cap, align)
    items = [(i, 50 + 30 * i, 5) for i in range(7)] + [(0, 10, 50)]
    need = [6 + 100 * i for i in range(7)] + [3]
    buf, offs, caps, arena = layout(items, 20 * slot)
    top = arena[0]
    base = gmodel.round_up(top, align)
    other = (fit + 3) % 8
    a_fit = fit if mode in ("arena", "both") else 7
    l_fit = fit if mode == "list" else other if mode == "both" else 7
    acc = min(a_fit, l_fit)
    end = base + a_fit * slot + (slot - 1 if a_fit < 7 else 0)
    s = State(cuda, buf, offs, caps, [top, end], list_cap=2 + l_fit, have=2, alloc=20)
    before = buf.copy()
    with cio.DevWriter(8) as w:
        st, total, rot = s.rotate(w, need, new_cap=new_cap, align=align, what=f"cut {fit} {mode}")
        assert st.tolist() == [0] * acc + [-1] * (7 - acc) + [0] and rot == list(range(acc))
        assert total == [base - top + 7 * slot, 7] and s.arena[0] == (base + acc * slot if acc else top)
        assert s.count == [2 + acc, 2 + l_fit]
        for i in range(acc, 7):
            assert (s.offs[i], s.caps[i]) == (offs[i], caps[i])
            assert np.array_equal(s.buf[offs[i]:offs[i] + caps[i]], before[offs[i]:offs[i] + caps[i]])
            assert model.image_check(s.buf, len(s.buf), offs[i], caps[i]) is not None
        # the retry: a fresh arena of dev_total[0] bytes behind the first, at the same residue, and a list that
        # takes dev_total[1] more entries
        top2 = base + 8 * slot + (top - base) % align
        s.set_arena([top2, top2 + total[0]])
        s.set_list_cap(s.count[0] + total[1])
        st, total, rot = s.rotate(w, need, new_cap=new_cap, align=align, what=f"retry {fit} {mode}")
        assert not st.any() and rot == list(range(acc, 7)) and s.count[0] == 9
        assert s.li[2:9] == list(range(7)) and s.lo[2:9] == offs[:7]


# ------------------------------------------------------------------ 3. the metadata copy

def meta_case(cuda, mlen, n, residue):
    """n full images with mlen bytes of metadata, image i at old offset
    residue(i); align 1 and a new_cap that is 1 modulo 16 put fresh image i at
    residue top + i."""
    new_cap = 24 + mlen + (1 - (24 + mlen)) % 16
    items = [(mlen, 1 + i % 3, 0) for i in range(n)]
    buf, offs, caps, arena = layout(items, n * new_cap + 40, residue=residue)
    s = State(cuda, buf, offs, caps, arena)
    old = list(s.offs)
    with cio.DevWriter(n) as w:
        st, total, rot = s.rotate(w, [1] * n, new_cap=new_cap, align=1, what=f"metadata {mlen}")
    assert not st.any() and rot == list(range(n))
    for i in (0, n // 2, n - 1):
        o = s.offs[i]
        assert s.crc[i] == zlib.crc32(s.buf[o + 22:o + 24 + mlen].tobytes()) ^ M32
    return [(a % 16, b % 16) for a, b in zip(old, s.offs)]


@pytest.mark.parametrize("mlen", [0, 1, 3, 4, 15, 16, 17])
def test_metadata_copy_short(cuda, mlen):
    pairs = meta_case(cuda, mlen, 256, lambda i: i // 16)
    assert sorted(pairs) == [(a, b) for a in range(16) for b in range(16)]


@pytest.mark.parametrize("mlen", [4095, 4096, 4097, 65535])
def test_metadata_copy_long(cuda, mlen):
    pairs = meta_case(cuda, mlen, 32, lambda i: i % 16 if i < 16 else (5 * i + 3) % 16)
    assert {a for a, _ in pairs} == set(range(16)) and {b for _, b in pairs} == set(range(16))
    assert len(set(pairs)) > 16


# ------------------------------------------------------------------ 4. the reference pin

def test_reference_fixture_rotated(cuda):
    """c03_meta_content built on the device in a zeroed image of the file's
    size, then rotated by `limit`: the sealed image's SHA-256 is the
    manifest's and verify-on-load over the list gives the manifest's load
    values; the fresh image, after the same writes and a seal, has that
    SHA-256 again."""
    spec = [c for c in MANIFEST["chunks"] if c["name"] == "c03_meta_content"][0]
    size, ld = spec["size"], spec["load"]
    meta = spec["ops"][0]["meta"].encode()
    writes = [pattern(o["len"], o["seed"]) for o in spec["ops"] if o["op"] == "write"]
    content = sum(len(x) for x in writes)
    assert content == ld["content_size"] and len(meta) == ld["meta_size"]
    off, top = 37, 37 + size + 11
    buf = np.zeros(top + size + 64 + 50, np.uint8)
    s = State(cuda, buf, [off], [size], [top, top + size + 64], crc=[0])
    src = np.frombuffer(b"".join(writes), np.uint8).copy()
    src_t = dev_u8(src, cuda)

    def build(what):
        o = s.offs[0]
        pos = 0
        for k, x in enumerate(writes):
            st = cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, dev_i64([pos], cuda),
                                    dev_i64([len(x)], cuda), s.crc_t, flags=CK)
            assert not st.cpu().numpy().any()
            s.crc[0] = m_write(s.buf, o, x, s.crc[0])
            pos += len(x)
        s.check(what)

    with cio.DevWriter(1) as w:
        st, crc = cf.init_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(np.frombuffer(meta, np.uint8).copy(), cuda),
                                    dev_i64([0], cuda), dev_i64([len(meta)], cuda), flags=CK, crc_cur=s.crc_t)
        assert not st.cpu().numpy().any()
        s.crc[0] = m_init(s.buf, off, meta)
        build("built")
        assert s.crc[0] == ld["crc_cur"]
        st, total, rot = s.rotate(w, [1], limit=content, new_cap=size, align=16, what="rotate the fixture")
        assert st.tolist() == [0] and rot == [0] and s.lo[0] == off and s.offs[0] == gmodel.round_up(top, 16)
        got = s.base_t.cpu().numpy()
        assert hashlib.sha256(got[off:off + size].tobytes()).hexdigest() == spec["sha256"]
        with cio.Crc32DevPlan(1) as plan:
            vst, er, cr, ml, cl = cf.verify_batch_dev(plan, s.base_t, s.lo_t[:1], s.lc_t[:1], flags=CK)
            assert ld["ok"] and int(vst[0]) == cf.CIO_OK and int(er[0]) == ld["last_chunk_error"]
            assert int(u32(cr)[0]) == ld["crc_cur"] and (int(ml[0]), int(cl[0])) == (ld["meta_size"], content)
        build("built again")
        assert not cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.crc_t, flags=CK).cpu().numpy().any()
        m_seal(s.buf, s.offs[0], s.crc[0])
        s.check("sealed again")
    got = s.base_t.cpu().numpy()
    assert hashlib.sha256(got[s.offs[0]:s.offs[0] + size].tobytes()).hexdigest() == spec["sha256"]


# ------------------------------------------------------------------ 5. the records variant

N_IMG = 300


def records_state(cuda):
    """300 images with 1..40 bytes of content and 0..199 bytes of room, and an
    arena that takes a fresh image for each."""
    items = [(i % 7, 1 + i % 40, (37 * i) % 200) for i in range(N_IMG)]
    buf, offs, caps, arena = layout(items, N_IMG * 128 + 64)
    return State(cuda, buf, offs, caps, arena)


def both_variants(cuda, rec_img, rec_lens, what):
    """The records variant against the model, and against the need variant fed
    the model's sums, on a second copy of the same state."""
    a, b = records_state(cuda), records_state(cuda)
    with cio.DevWriter(max(N_IMG, len(rec_img))) as w:
        want = a.rotate(w, recs=(rec_img, rec_lens), new_cap=128, align=16, what=what + ", records")
        need = model.needs_of(rec_img, rec_lens, N_IMG)
        b.rotate(w, need, new_cap=128, align=16, what=what + ", needs")
    assert a.offs == b.offs and a.li == b.li and a.crc == b.crc and np.array_equal(a.buf, b.buf)
    return want


def test_records_runs_cross_wave_and_workgroup_boundaries(cuda):
    """Runs of 1, 2, 63, 64, 65 and 1000 records per image, one behind another
    behind a prefix of 37 records: every run starts at another lane, the long
    ones cross waves and the 256-record workgroups of the sums kernel."""
    rng = np.random.default_rng(5)
    rec_img = list(rng.integers(0, N_IMG, 37))
    for rep in range(3):
        for k, run in enumerate((1, 2, 63, 64, 65, 1000)):
            rec_img += [10 * k + rep] * run
    rec_img = np.asarray(rec_img, np.uint32)
    rec_lens = rng.integers(0, 3, len(rec_img)).astype(np.uint64)
    rec_lens[100] = 1 << 40                       # clamped to 2^32
    st, total, rot = both_variants(cuda, rec_img, rec_lens, "runs")
    assert not st.any() and 0 < len(rot) < N_IMG


def test_records_shuffled_and_all_to_one_image(cuda):
    rng = np.random.default_rng(6)
    rec_img = rng.permutation(np.arange(5000) % N_IMG).astype(np.uint32)
    rec_lens = rng.integers(0, 12, 5000).astype(np.uint64)
    st, total, rot = both_variants(cuda, rec_img, rec_lens, "shuffled")
    assert not st.any() and 0 < len(rot) < N_IMG
    st, total, rot = both_variants(cuda, np.full(5000, 131, np.uint32), rec_lens, "one image")
    assert not st.any() and rot == [131]


@pytest.mark.parametrize("at", [0, 255, 256, 2999])
def test_malformed_records_list_changes_nothing(cuda, at):
    rng = np.random.default_rng(at)
    s = records_state(cuda)
    arena = list(s.arena)
    rec_img = rng.integers(0, N_IMG, 3000).astype(np.uint32)
    rec_img[at] = N_IMG + (at % 2) * 0xFFFFFED3
    rec_lens = rng.integers(1, 100, 3000).astype(np.uint64)
    with cio.DevWriter(3000) as w:
        st, total, rot = s.rotate(w, recs=(rec_img, rec_lens), new_cap=128, what=f"malformed at {at}")
        assert st.tolist() == [-1] * N_IMG and total == [0, 0] and s.arena == arena and s.count[0] == 0
        # the writer is not left marked: the same list, mended, rotates
        rec_img[at] = 0
        st, total, rot = s.rotate(w, recs=(rec_img, rec_lens), new_cap=128, what="mended")
        assert not st.any() and len(rot) > 0


# ------------------------------------------------------------------ 6. lifecycle

def test_lifecycle_rotate_grow_append(cuda):
    """Five images initialised with metadata, then eight rounds of rotate ->
    grow_records -> write_records_ungrouped with limit 1500 and at most 1200
    bytes per image and round, so that the images rotate in different rounds.
    Every call equals the model.  At the end verify-on-load accepts every
    chunk of the list, the list's contents followed by the live images' are
    the records of each image in order, and no sealed chunk exceeds the
    limit."""
    import torch
    n_img, n_rec, rounds, limit, new_cap = 5, 20, 8, 1500, 24 + 9 + 150
    rng = np.random.default_rng(12)
    metas = [bytes(rng.integers(1, 255, 2 * i + 1, dtype=np.uint8)) for i in range(n_img)]
    items = [(0, 0, len(m) + 150) for m in metas]
    buf, offs, caps, arena = layout(items, 1 << 20)
    buf = fill(len(buf))
    s = State(cuda, buf, offs, caps, arena, list_cap=64, alloc=66)
    msrc = np.frombuffer(b"".join(metas) + b"\0", np.uint8).copy()
    mlens = np.asarray([len(m) for m in metas], np.uint64)
    moffs = np.concatenate(([0], np.cumsum(mlens)[:-1])).astype(np.uint64)
    wrote = [b""] * n_img
    rotated_in = []
    with cio.DevWriter(max(n_img, n_rec)) as w:
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
            st, total, rot = s.rotate(w, recs=(rec_img, rec_lens), limit=limit, new_cap=new_cap, align=16,
                                      what=f"round {k}: rotate")
            assert not st.any()
            rotated_in.append(rot)
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
        done = s.count[0]
        assert done >= n_img and len({tuple(r) for r in rotated_in}) > 2      # they rotate in different rounds
        with cio.Crc32DevPlan(done) as plan:
            vst, er, cr, ml, cl = cf.verify_batch_dev(plan, s.base_t, s.lo_t[:done], s.lc_t[:done], flags=CK)
            assert not vst.cpu().numpy().any()
            assert int(cl.cpu().numpy().max()) <= limit
        # the list's chunks, then the live images: packed content, in that order
        all_offs = torch.cat([s.lo_t[:done], s.offs_t])
        all_caps = torch.cat([s.lc_t[:done], s.caps_t])
        out = torch.zeros(sum(len(x) for x in wrote) + 16, dtype=torch.uint8, device=cuda)
        with cio.DevWriter(done + n_img) as rw:
            rst, o_offs, o_lens, rtotal = cf.read_packed_batch_dev(rw, s.base_t, all_offs, all_caps,
                                                                   cf.CIOA_READ_CONTENT, out)
            assert not rst.cpu().numpy().any()
            packed, o_offs, o_lens = out.cpu().numpy(), u64(o_offs), u64(o_lens)
    owner = s.li[:done] + list(range(n_img))
    got = [b""] * n_img
    for j, i in enumerate(owner):
        got[i] += packed[int(o_offs[j]):int(o_offs[j] + o_lens[j])].tobytes()
    assert got == wrote
    assert max(int(x) for x in o_lens[:done]) <= limit


# ------------------------------------------------------------------ 7. graph

def test_graph_replay_until_the_list_is_full(cuda):
    """rotate_batch_dev -> grow_batch_dev -> write_batch_dev captured once,
    dev_need = the source lengths array, replayed until the list of 10 entries
    is full and beyond: every replay equals the model; once the list is full
    the cut images stay where they are and keep accepting what grow makes room
    for.  The whole-buffer compare shows that nothing is written out of
    bounds."""
    import torch
    n, size, limit, new_cap = 12, 300, 500, 24 + 3 + 200
    rng = np.random.default_rng(7)
    items = [(i % 4, 0, 250 + 10 * i) for i in range(n)]
    buf, offs, caps, arena = layout(items, 1 << 19)
    crc = [m_init(buf, offs[i], buf[offs[i] + 24:offs[i] + 24 + m].tobytes()) for i, (m, _, _) in enumerate(items)]
    s = State(cuda, buf, offs, caps, arena, crc=crc, list_cap=10, alloc=12)
    so = np.arange(n, dtype=np.uint64) * (size + 3)
    src_t = dev_u8(np.zeros(n * (size + 3) + 16, np.uint8), cuda)
    so_t, sl_t = dev_i64(so, cuda), dev_i64(np.zeros(n, np.uint64), cuda)
    o = s.outs()
    go = dict(total=dev_i64([0], cuda), status=torch.full((n,), 99, dtype=torch.int32, device=cuda))
    wst = torch.full((n,), 99, dtype=torch.int32, device=cuda)

    def stage(k):
        lens = rng.integers(1, size + 1, n).astype(np.uint64)
        lens[k % n] = 0
        src = rng.integers(0, 256, src_t.numel(), dtype=np.uint8)
        src_t.copy_(torch.from_numpy(src))
        sl_t.copy_(torch.from_numpy(lens.view(np.int64)))
        want = s.model(lens, limit, new_cap, 32, CK)
        gwant = gmodel.m_grow(s.buf, s.offs, s.caps, lens, s.arena, realloc=512, page=256, align=32)
        assert not gwant[0].any()
        for i in range(n):
            s.crc[i] = m_write(s.buf, s.offs[i], src[int(so[i]):int(so[i]) + int(lens[i])].tobytes(), s.crc[i])
        return want

    def call():
        cf.rotate_batch_dev(w, s.base_t, s.offs_t, s.caps_t, sl_t, limit=limit, new_cap=new_cap, align=32, flags=CK,
                            **s.lists(), **o)
        cf.grow_batch_dev(w, s.base_t, s.offs_t, s.caps_t, sl_t, s.arena_t, realloc=512, page=256, align=32, **go)
        cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, so_t, sl_t, s.crc_t, flags=CK, status=wst)

    with cio.DevWriter(n) as w:
        want = stage(0)
        call()                                # warm-up outside the capture (a round like the others)
        torch.cuda.synchronize()
        s.compare(o, want, "warm-up")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        s.check("capture runs nothing")
        counts, cut = [s.count[0]], 0
        for k in range(1, 8):
            want = stage(k)
            o["status"].fill_(99)
            wst.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            s.compare(o, want, f"replay {k}")
            assert not wst.cpu().numpy().any() and not go["status"].cpu().numpy().any()
            counts.append(s.count[0])
            cut += int((want[0] != 0).sum())
        del graph
    assert counts[-1] == 10 and counts[0] < 10 and cut > 0 and counts == sorted(counts)
