"""Transactions on chunk images in device memory
(include/chunkio_amd/cio_write_dev_tx.h) against the numpy model
(tx_dev_model.py).  Every call is compared in ALL it may touch: the WHOLE
buffer (a position-dependent sentinel fills every slack, so a stray or missing
store shows, and every image has guard bytes around it), crc_cur, the state
entries and the statuses (pre-filled, so an entry the call forgot shows).
Helpers, sentinel and layout are those of test_gpu_grow_dev.py."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf
from oracle import pyoracle as po

import grow_dev_model as gmodel
import rotate_dev_model as rmodel
import tx_dev_model as model
from grow_dev_model import image_check
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, layout, u64
from write_dev_move_model import M32, m_init, m_meta_write, m_seal, m_write, m_write_at, pattern
from write_dev_records_model import m_write_records
from write_dev_ungrouped_model import m_write_records_ungrouped

pytestmark = pytest.mark.gpu

CK, REC, ZERO = cf.CIO_CHECKSUM, cf.CIOA_TX_RECOMPUTE, cf.CIOA_TX_ZERO
BLOCK = 256                                   # kTxBlock: images per workgroup of every kernel
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "tests", "golden", "chunks", "manifest.json")) as _f:
    MANIFEST = json.load(_f)


def u32(t):
    return t.cpu().numpy().view(np.uint32).copy()


def i32(t):
    return t.cpu().numpy().copy()


class State:
    """Images in one device buffer with crc_cur and the transaction state, the
    host copies beside them; all are carried from call to call."""

    def __init__(self, cuda, buf, offs, caps, crc=None, tx=None):
        self.cuda, self.buf = cuda, buf
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.n = len(self.offs)
        self.crc = [int(x) for x in (crc if crc is not None else (np.arange(self.n) * 2654435761 + 99) % (1 << 32))]
        self.tx = model.new_state(self.n) if tx is None else [list(t) for t in tx]
        self.base_t = dev_u8(buf, cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.crc_t = dev_i32(self.crc, cuda)
        self.tx_t = cf.tx_state(self.n, cuda)
        self.put_tx()

    def put_tx(self):
        import torch
        self.tx_t.copy_(torch.from_numpy(np.asarray(self.tx, np.uint32).view(np.int32)).to(self.cuda))

    def poke(self, pos, value):
        """One byte, on both sides."""
        self.buf[pos] = value
        self.base_t[pos] = value

    def status(self):
        import torch
        return torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda)

    def dev_cond(self, cond):
        return None if cond is None else dev_i32(np.asarray(cond, np.int32).view(np.uint32), self.cuda)

    def begin(self, w, flags=CK, what="begin"):
        st = cf.tx_begin_batch_dev(w, self.base_t, self.offs_t, self.caps_t, self.tx_t,
                                   self.crc_t if flags & CK else None, flags=flags, status=self.status())
        want = model.m_tx_begin(self.buf, self.offs, self.caps, self.tx, self.crc, flags=flags)
        self.compare(st, want, what)
        return want

    def rollback(self, w, cond=None, flags=CK, what="rollback"):
        st = cf.tx_rollback_batch_dev(w, self.base_t, self.offs_t, self.caps_t, self.tx_t,
                                      self.crc_t if flags & CK else None, cond=self.dev_cond(cond), flags=flags,
                                      status=self.status())
        want, rolled = model.m_tx_rollback(self.buf, self.offs, self.caps, self.tx, self.crc, cond, flags=flags)
        self.compare(st, want, what)
        return want, rolled

    def commit(self, w, cond=None, flags=CK, what="commit"):
        st = cf.tx_commit_batch_dev(w, self.base_t, self.offs_t, self.caps_t, self.tx_t,
                                    self.crc_t if flags & CK else None, cond=self.dev_cond(cond), flags=flags,
                                    status=self.status())
        want, done = model.m_tx_commit(self.buf, self.offs, self.caps, self.tx, self.crc, cond, flags=flags)
        self.compare(st, want, what)
        return want, done

    def write(self, w, records, flags=CK, what="append"):
        """write_batch_dev of records[i] (bytes) to image i, and the model's."""
        lens = np.asarray([len(r) for r in records], np.uint64)
        so = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        src = np.frombuffer(b"".join(records) + b"\0" * 16, np.uint8).copy()
        st = cf.write_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_u8(src, self.cuda),
                                dev_i64(so, self.cuda), dev_i64(lens, self.cuda), self.crc_t, flags=flags,
                                status=self.status())
        want = np.zeros(self.n, np.int32)
        for i, r in enumerate(records):
            if len(r) == 0:
                continue
            geo = image_check(self.buf, len(self.buf), self.offs[i], self.caps[i])
            if geo is None or 24 + geo[0] + geo[1] + len(r) > self.caps[i]:
                want[i] = -1
                continue
            self.crc[i] = m_write(self.buf, self.offs[i], r, self.crc[i], checksum=bool(flags & CK))
        self.compare(st, want, what)
        return want

    def compare(self, st, want, what):
        got = i32(st)
        assert np.array_equal(got, want), (what, "status", np.flatnonzero(got != want)[:8], got[:16], want[:16])
        self.check(what)

    def check(self, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u32(self.crc_t).tolist() == self.crc, (what, "crc_cur")
        tx = u32(self.tx_t).reshape(-1, 4).tolist()
        assert tx == self.tx, (what, "state", [i for i in range(self.n) if tx[i] != self.tx[i]][:8])
        got = self.base_t.cpu().numpy()
        if not np.array_equal(got, self.buf):
            bad = np.flatnonzero(got != self.buf)
            raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:6]} of {len(got)}")


def crc_of_images(buf, offs, items):
    """crc_cur of images that put_image wrote: the CRC of bytes [22, used)."""
    return [po.crc_update(0xFFFFFFFF, buf[o + 22:o + 24 + m + c].tobytes()) for o, (m, c, _) in zip(offs, items)]


# ------------------------------------------------------------------ 1. begin / rollback / commit

KINDS = ("ok", "active", "inactive", "broken", "magic", "tiny", "outside")
METAS = (0, 1, 33)


def mixed(n):
    """Image i of kind KINDS[i % 7] with 0 / 1 / 33 bytes of metadata, at
    offsets of every residue: begun and rolled back; active before the begin
    (with a saved length one byte short); made inactive before the rollback;
    broken (its magic) after the begin; and three that are no images: bad
    magic, cap < 24, outside dev_bytes."""
    rng = np.random.default_rng(n)
    items = [(METAS[i % 3], 1 + int(rng.integers(0, 50)), 10 + int(rng.integers(0, 20))) for i in range(n)]
    buf, offs, caps, _ = layout(items, 0)
    for i in range(n):
        kind = KINDS[i % 7]
        if kind == "magic":
            buf[offs[i] + 1] = 0x01
        elif kind == "tiny":
            caps[i] = 23
        elif kind == "outside":
            offs[i], caps[i] = len(buf) - 7, 64
    return buf, offs, caps, items


@pytest.mark.parametrize("flags", [CK, 0])
@pytest.mark.parametrize("n", [1, 2, BLOCK + 1, 4 * BLOCK + 1])
def test_begin_rollback_commit(cuda, n, flags):
    buf, offs, caps, items = mixed(n)
    kinds = [KINDS[i % 7] for i in range(n)]
    valid = [k in ("ok", "active", "inactive", "broken") for k in kinds]
    tx = model.new_state(n)
    for i in range(n):
        if kinds[i] == "active":
            tx[i] = [1, items[i][1] - 1, 0x1234 + i, items[i][0]]
    s = State(cuda, buf, offs, caps, tx=tx)
    with cio.DevWriter(n) as w:
        st = s.begin(w, flags, "begin")
        assert st.tolist() == [0 if v else -1 for v in valid]
        for i in range(n):
            if kinds[i] == "active":
                assert s.tx[i] == tx[i]                                   # begin on an active entry: a no-op
            elif valid[i]:
                assert s.tx[i] == [1, items[i][1], s.crc[i] if flags else 0, items[i][0]]
            else:
                assert s.tx[i] == [0, 0, 0, 0]
        for i in range(n):
            if kinds[i] == "inactive":
                s.tx[i][0] = 0
        s.put_tx()
        st = s.write(w, [bytes([0x40 + i % 64]) * (1 + i % 7) for i in range(n)], flags)
        assert st.tolist() == [0 if v else -1 for v in valid]
        for i in range(n):
            if kinds[i] == "broken":
                s.poke(offs[i] + 1, 0x01)
        snap = s.buf.copy()
        st, rolled = s.rollback(w, None, flags, "rollback")
        assert rolled == [i for i in range(n) if kinds[i] in ("ok", "active")]
        assert st.tolist() == [0 if k in ("ok", "active") else -1 for k in kinds]
        for i in range(n):
            if kinds[i] == "broken":
                assert s.tx[i][0] == 1                                    # the failed check leaves the state active
            if st[i] != 0 and valid[i]:
                assert np.array_equal(s.buf[offs[i]:offs[i] + caps[i]], snap[offs[i]:offs[i] + caps[i]])
        # a second round: begin anew, append, and commit everything; an inactive entry is sealed too
        st = s.begin(w, flags, "begin again")
        assert st.tolist() == [0 if valid[i] else -1 for i in range(n)]    # "broken" is still active: not read
        st = s.write(w, [bytes([0x80 + i % 64]) * (1 + i % 3) for i in range(n)], flags)
        for i in range(n):
            if kinds[i] == "inactive":
                s.tx[i][0] = 0
        s.put_tx()
        st, done = s.commit(w, None, flags, "commit")
        assert done == [i for i in range(n) if kinds[i] in ("ok", "active", "inactive")]
        assert st.tolist() == [0 if i in done else -1 for i in range(n)]
        assert all(s.tx[i][0] == (1 if kinds[i] == "broken" else 0) for i in range(n))


# ------------------------------------------------------------------ 2. dropped lengths

LENS = [0, 1, 15, 16, 17, 4095, 4096, 4097, (1 << 20) + 13]


@pytest.mark.parametrize("flags", [CK, CK | ZERO, ZERO, CK | ZERO | REC, CK | REC])
def test_dropped_lengths(cuda, flags):
    """Every length twice, at two residues and with different metadata: what
    the rollback drops is zeroed (with CIOA_TX_ZERO) or left, the bytes past
    the old end of the content -- sentinel -- are untouched either way."""
    lens = [ln for ln in LENS for _ in range(2)]
    items = [(METAS[i % 3], 7 + i, ln + 9) for i, ln in enumerate(lens)]
    buf, offs, caps, _ = layout(items, 0, residue=lambda i: (7 * i + 1) % 16)
    s = State(cuda, buf, offs, caps, crc=crc_of_images(buf, offs, items))
    rng = np.random.default_rng(3)
    with cio.DevWriter(len(lens)) as w:
        assert not s.begin(w, flags & CK).any()
        assert not s.write(w, [rng.integers(1, 256, ln, dtype=np.uint8).tobytes() for ln in lens], flags & CK).any()
        before = s.buf.copy()
        st, rolled = s.rollback(w, None, flags, f"rollback {flags}")
        assert not st.any() and rolled == list(range(len(lens)))
    for i, ln in enumerate(lens):
        a = offs[i] + 24 + items[i][0] + items[i][1]
        if flags & ZERO:
            assert not s.buf[a:a + ln].any()
        else:
            assert np.array_equal(s.buf[a:a + ln], before[a:a + ln])
        assert np.array_equal(s.buf[a + ln:a + ln + 9], before[a + ln:a + ln + 9]) and s.buf[a + ln:a + ln + 9].all()
        if flags & CK:
            assert s.crc[i] == po.crc_update(0xFFFFFFFF, s.buf[offs[i] + 22:a].tobytes())


# ------------------------------------------------------------------ 3. CIOA_TX_RECOMPUTE

@pytest.mark.parametrize("recompute", [True, False])
def test_recompute_after_write_at_and_metadata(cuda, recompute):
    """Inside the transaction: A write_at that ends longer than at begin; B
    write_at that ends shorter (CIO_ERROR either way: the image shrank); C an
    equal-length metadata rewrite; D a longer and E a shorter metadata; F a
    plain append.  With CIOA_TX_RECOMPUTE A, C, D, E, F are rolled back and
    crc_cur is the CRC of the kept bytes.  Without it D and E are CIO_ERROR
    with the state still active; A and C pass the header's rules -- the
    lengths say nothing -- and get the saved CRC state, which no longer
    matches the image: the case the header tells callers to use
    CIOA_TX_RECOMPUTE for."""
    groups = "AABBCCDDEEFF"
    n = len(groups)
    items = [(4, 20 + i, 60) for i in range(n)]
    buf, offs, caps, _ = layout(items, 0)
    s = State(cuda, buf, offs, caps, crc=crc_of_images(buf, offs, items))
    flags = CK | ZERO | (REC if recompute else 0)
    with cio.DevWriter(n, move=True) as w:
        assert not s.begin(w, CK).any()
        # write_at on A, B (a record of length 0 elsewhere: a no-op)
        recs = [bytes([0x50 + i]) * (30 if g == "A" else 4 if g == "B" else 0) for i, g in enumerate(groups)]
        lens = np.asarray([len(r) for r in recs], np.uint64)
        so = np.concatenate(([0], np.cumsum(lens)[:-1])).astype(np.uint64)
        src = np.frombuffer(b"".join(recs) + b"\0" * 16, np.uint8).copy()
        st = cf.write_at_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_i64([5] * n, cuda), dev_u8(src, cuda),
                                   dev_i64(so, cuda), dev_i64(lens, cuda), s.crc_t, flags=CK)
        assert not i32(st).any()
        for i, r in enumerate(recs):
            s.crc[i] = m_write_at(s.buf, offs[i], 5, r, s.crc[i])
        s.check("write_at")
        # metadata on C, D, E: a contiguous slice of the batch
        a, b = groups.index("C"), groups.index("F")
        metas = [{"C": b"WXYZ", "D": b"nine byte", "E": b"1"}[g] for g in groups[a:b]]
        ml = np.asarray([len(m) for m in metas], np.uint64)
        mo = np.concatenate(([0], np.cumsum(ml)[:-1])).astype(np.uint64)
        msrc = np.frombuffer(b"".join(metas) + b"\0" * 16, np.uint8).copy()
        st = cf.write_metadata_batch_dev(w, s.base_t, s.offs_t[a:b], s.caps_t[a:b], dev_u8(msrc, cuda),
                                         dev_i64(mo, cuda), dev_i64(ml, cuda), s.crc_t[a:b], flags=CK)
        assert not i32(st).any()
        for k, m in enumerate(metas):
            s.crc[a + k] = m_meta_write(s.buf, offs[a + k], m, s.crc[a + k])
        s.check("metadata")
        assert not s.write(w, [b"appended" if g == "F" else b"" for g in groups]).any()
        saved = [t[2] for t in s.tx]
        st, rolled = s.rollback(w, None, flags, f"rollback, recompute {recompute}")
    ok = "ACDEF" if recompute else "ACF"
    assert st.tolist() == [0 if g in ok else -1 for g in groups]
    for i, g in enumerate(groups):
        assert s.tx[i][0] == (0 if g in ok else 1)                        # a rejected entry stays active
        if g in ok:
            meta, content = image_check(s.buf, len(s.buf), offs[i], caps[i])
            assert content == 20 + i
            true = po.crc_update(0xFFFFFFFF, s.buf[offs[i] + 22:offs[i] + 24 + meta + content].tobytes())
            assert s.crc[i] == (true if recompute or g == "F" else saved[i])
            if g in "AC" and not recompute:
                assert saved[i] != true                                   # the documented hazard


# ------------------------------------------------------------------ 4. without CIO_CHECKSUM

@pytest.mark.parametrize("flags", [0, ZERO])
def test_without_checksum_the_crc_is_left_alone(cuda, flags):
    n = 9
    items = [(METAS[i % 3], 5 + i, 20) for i in range(n)]
    buf, offs, caps, _ = layout(items, 0)
    s = State(cuda, buf, offs, caps)
    for i in range(n):
        s.buf[offs[i] + 2:offs[i] + 10] = np.arange(8) + 0x70 + i           # something to keep
    s.base_t.copy_(dev_u8(s.buf, cuda))
    crc0 = list(s.crc)
    with cio.DevWriter(n) as w:
        assert not s.begin(w, 0).any() and all(t[2] == 0 for t in s.tx)
        assert not s.write(w, [b"x" * (i + 1) for i in range(n)], 0).any()
        st, rolled = s.rollback(w, None, flags)
        assert not st.any() and len(rolled) == n
        assert not s.begin(w, 0).any()
        st, done = s.commit(w, None, 0)
        assert not st.any() and len(done) == n
    assert s.crc == crc0 and u32(s.crc_t).tolist() == crc0
    got = s.base_t.cpu().numpy()
    for i in range(n):
        assert got[offs[i] + 2:offs[i] + 10].tolist() == [0x70 + i + k for k in range(8)]


# ------------------------------------------------------------------ 5. dev_cond

@pytest.mark.parametrize("flags", [CK, CK | ZERO | REC])
def test_condition_splits_a_batch_between_rollback_and_commit(cuda, flags):
    n = 2 * BLOCK + 44
    rng = np.random.default_rng(8)
    items = [(METAS[i % 3], 3 + i % 11, 16) for i in range(n)]
    buf, offs, caps, _ = layout(items, 0)
    s = State(cuda, buf, offs, caps, crc=crc_of_images(buf, offs, items))
    cond = rng.choice(np.asarray([0, 0, -1, -3], np.int32), n)
    with cio.DevWriter(n) as w:
        assert not s.begin(w).any()
        assert not s.write(w, [bytes([1 + i % 200]) * (1 + i % 9) for i in range(n)]).any()
        snap, tx0 = s.buf.copy(), [list(t) for t in s.tx]
        st, rolled = s.rollback(w, cond, flags, "rollback(cond)")
        assert not st.any() and rolled == [i for i in range(n) if cond[i] != 0]
        for i in range(n):
            if cond[i] == 0:                      # skipped: byte-identical, state as it was
                assert np.array_equal(s.buf[offs[i]:offs[i] + caps[i]], snap[offs[i]:offs[i] + caps[i]])
                assert s.tx[i] == tx0[i]
        snap = s.buf.copy()
        st, done = s.commit(w, cond, flags & CK, "commit(cond)")
        assert not st.any() and done == [i for i in range(n) if cond[i] == 0]
        assert sorted(rolled + done) == list(range(n)) and not set(rolled) & set(done)
        for i in rolled:
            assert np.array_equal(s.buf[offs[i]:offs[i] + caps[i]], snap[offs[i]:offs[i] + caps[i]])
        assert all(t[0] == 0 for t in s.tx)


# ------------------------------------------------------------------ 6. tx_cond_records

N_IMG = 300


def run_cond(cuda, rec_img, rec_status, n_img, img_status=None, what=""):
    import torch
    cond = torch.full((n_img,), 77, dtype=torch.int32, device=cuda)
    img_t = None if rec_img is None else dev_i32(np.asarray(rec_img, np.uint32), cuda)
    st_t = None if rec_img is None else dev_i32(np.asarray(rec_status, np.int32).view(np.uint32), cuda)
    is_t = None if img_status is None else dev_i32(np.asarray(img_status, np.int32).view(np.uint32), cuda)
    got = i32(cf.tx_cond_records_batch_dev(img_t, st_t, n_img, img_status=is_t, cond=cond))
    want = model.m_tx_cond([] if rec_img is None else rec_img, [] if rec_img is None else rec_status, n_img,
                           img_status)
    assert np.array_equal(got, want), (what, np.flatnonzero(got != want)[:8])
    return want


def test_cond_grouped_and_shuffled_lists(cuda):
    rng = np.random.default_rng(9)
    rec_img = np.sort(rng.integers(0, N_IMG, 5000)).astype(np.uint32)
    rec_st = np.where(rng.integers(0, 40, 5000) == 0, -1, 0).astype(np.int32)
    rec_st[np.flatnonzero(rec_st)[::3]] = -3
    img_st = np.where(rng.integers(0, 25, N_IMG) == 0, -1, 0).astype(np.int32)
    want = run_cond(cuda, rec_img, rec_st, N_IMG, what="grouped")
    assert 0 < (want != 0).sum() < N_IMG
    perm = rng.permutation(5000)
    assert np.array_equal(run_cond(cuda, rec_img[perm], rec_st[perm], N_IMG, what="shuffled"), want)
    folded = run_cond(cuda, rec_img[perm], rec_st[perm], N_IMG, img_st, "image statuses folded in")
    assert (folded != 0).sum() > (want != 0).sum()
    assert np.array_equal(run_cond(cuda, None, None, N_IMG, img_st, "no records"), img_st)
    assert not run_cond(cuda, None, None, N_IMG, None, "nothing at all").any()
    assert not run_cond(cuda, rec_img, np.zeros(5000, np.int32), N_IMG, what="nothing failed").any()


@pytest.mark.parametrize("n_rec", [1, 63, 64, 65, 1000])
def test_cond_runs_to_one_image(cuda, n_rec):
    """All records to image 131: none failing, all failing, and one failing at
    the list's first and last record and at every wave's first and last lane."""
    rec_img = np.full(n_rec, 131, np.uint32)
    assert not run_cond(cuda, rec_img, np.zeros(n_rec, np.int32), N_IMG, what="none").any()
    want = run_cond(cuda, rec_img, np.full(n_rec, -1, np.int32), N_IMG, what="all")
    assert np.flatnonzero(want).tolist() == [131]
    for at in sorted({0, n_rec - 1} | {x for x in (63, 64, 127, 128, 255, 256, 511, 512) if x < n_rec}):
        st = np.zeros(n_rec, np.int32)
        st[at] = -1
        assert np.flatnonzero(run_cond(cuda, rec_img, st, N_IMG, what=f"one at {at}")).tolist() == [131]
        assert np.flatnonzero(run_cond(cuda, rec_img, st, 132, what=f"one at {at}, last image")).tolist() == [131]


@pytest.mark.parametrize("n_img", [1, 2, BLOCK, BLOCK + 1, N_IMG])
@pytest.mark.parametrize("at", [0, 63, 64, 999])
def test_cond_malformed_index_fails_every_image(cuda, at, n_img):
    rng = np.random.default_rng(at + n_img)
    rec_img = rng.integers(0, n_img, 1000).astype(np.uint32)
    rec_st = np.where(rng.integers(0, 9, 1000) == 0, -1, 0).astype(np.int32)
    rec_img[at] = n_img if at % 2 else 0xFFFFFFFF
    assert run_cond(cuda, rec_img, rec_st, n_img, what="malformed").tolist() == [-1] * n_img
    rec_img[at] = 0                               # mended: nothing sticks
    want = run_cond(cuda, rec_img, rec_st, n_img, what="mended")
    assert n_img <= 2 or not want.all()


# ------------------------------------------------------------------ 7. the all-or-nothing append

def written_images(n, room_of, metas=METAS):
    """n images built by init and one append (so bytes 2..9 hold the raw CRC
    state, as the write path leaves them), zero behind the content as a fresh
    file is, sentinel guard bytes around each.  Returns (buf, offs, caps, crc)."""
    items = [(metas[i % len(metas)], 5 + i % 13, room_of(i)) for i in range(n)]
    buf, offs, caps, _ = layout(items, 0)
    crc = []
    for i, (m, c, _) in enumerate(items):
        buf[offs[i]:offs[i] + caps[i]] = 0
        raw = m_init(buf, offs[i], bytes([0x61 + k % 26 for k in range(m)]))
        crc.append(m_write(buf, offs[i], bytes([1 + (i + k) % 250 for k in range(c)]), raw))
    return buf, offs, caps, crc


def batch_of_records(n_img, rng, per=3):
    rec_img = np.repeat(np.arange(n_img, dtype=np.uint32), per)
    rec_lens = rng.integers(10, 61, len(rec_img)).astype(np.uint64)
    rec_lens[1::per][::5] = 0                     # an empty record here and there
    rec_offs = np.concatenate(([0], np.cumsum(rec_lens)[:-1])).astype(np.uint64)
    src = rng.integers(0, 256, int(rec_lens.sum()) + 16, dtype=np.uint8)
    return rec_img, rec_offs, rec_lens, src


@pytest.mark.parametrize("zero", [True, False])
@pytest.mark.parametrize("grouped", [True, False])
def test_all_or_nothing_append(cuda, grouped, zero):
    """begin -> records append -> cond -> rollback(cond) -> commit(cond), queued
    without a look at anything in between.  Every third image lacks one byte
    of room for its last record: it ends byte-identical to before the batch
    (with CIOA_TX_ZERO its whole capacity and the guard bytes; without, its
    used bytes), the others hold the whole batch, are sealed, and pass
    verify-on-load."""
    import torch
    n_img, per = 41, 3
    rng = np.random.default_rng(21 + grouped)
    rec_img, rec_offs, rec_lens, src = batch_of_records(n_img, rng, per)
    need = rec_lens.reshape(n_img, per).sum(axis=1)
    short = [i % 3 == 0 for i in range(n_img)]
    buf, offs, caps, crc = written_images(n_img, lambda i: int(need[i]) - 1 if i % 3 == 0 else int(need[i]) + (i % 4 == 1))
    if not grouped:
        perm = rng.permutation(len(rec_img))
        rec_img, rec_offs, rec_lens = rec_img[perm], rec_offs[perm], rec_lens[perm]
    s = State(cuda, buf, offs, caps, crc=crc)
    before, crc0 = buf.copy(), list(crc)
    flags = CK | (ZERO if zero else 0)
    img_t, ro_t, rl_t, src_t = dev_i32(rec_img, cuda), dev_i64(rec_offs, cuda), dev_i64(rec_lens, cuda), dev_u8(src, cuda)
    append = cf.write_records_batch_dev if grouped else cf.write_records_ungrouped_batch_dev
    with cio.DevWriter(max(n_img, len(rec_img))) as w:
        bst = cf.tx_begin_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, status=s.status())
        ist, rst = append(w, s.base_t, s.offs_t, s.caps_t, src_t, img_t, ro_t, rl_t, s.crc_t, flags=CK)
        cond = cf.tx_cond_records_batch_dev(img_t, rst, n_img, img_status=ist)
        rb = cf.tx_rollback_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, cond=cond, flags=flags,
                                      status=s.status())
        cm = cf.tx_commit_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, cond=cond, status=s.status())
        # the model, call by call
        assert not model.m_tx_begin(s.buf, s.offs, s.caps, s.tx, s.crc).any() and not i32(bst).any()
        if grouped:
            want_ist, want_rst = m_write_records(s.buf, offs, caps, src, rec_img, rec_offs, rec_lens, s.crc)
        else:
            want_ist, want_rst, _ = m_write_records_ungrouped(s.buf, offs, caps, src, rec_img, rec_offs, rec_lens,
                                                              s.crc)
        assert np.array_equal(i32(ist), want_ist) and np.array_equal(i32(rst), want_rst)
        want_cond = model.m_tx_cond(rec_img, want_rst, n_img, want_ist)
        assert np.array_equal(i32(cond), want_cond) and (want_cond != 0).tolist() == short
        want_rb, rolled = model.m_tx_rollback(s.buf, s.offs, s.caps, s.tx, s.crc, want_cond, flags=flags)
        want_cm, done = model.m_tx_commit(s.buf, s.offs, s.caps, s.tx, s.crc, want_cond)
        assert np.array_equal(i32(rb), want_rb) and np.array_equal(i32(cm), want_cm) and not want_rb.any()
        assert rolled == [i for i in range(n_img) if short[i]] and done == [i for i in range(n_img) if not short[i]]
        s.check("all or nothing")
        got = s.base_t.cpu().numpy()
        for i in range(n_img):
            o, c = offs[i], caps[i]
            meta, content = image_check(got, len(got), o, c)
            if short[i]:
                used = 24 + meta + content
                assert np.array_equal(got[o:o + used], before[o:o + used]) and s.crc[i] == crc0[i]
                if zero:
                    assert np.array_equal(got[o - 1:o + c + 1], before[o - 1:o + c + 1])
            else:
                assert content == 5 + i % 13 + int(need[i])
                assert got[o + 2:o + 10].tobytes() == struct.pack(">I", s.crc[i] ^ M32) + b"\0" * 4
        idx = torch.tensor(done, dtype=torch.int64, device=cuda)
        with cio.Crc32DevPlan(len(done)) as plan:
            vst, er, cr, ml, cl = cf.verify_batch_dev(plan, s.base_t, s.offs_t[idx], s.caps_t[idx], flags=CK)
            assert not i32(vst).any() and u32(cr).tolist() == [s.crc[i] for i in done]


# ------------------------------------------------------------------ 8. graph

def test_graph_replay_of_the_all_or_nothing_chain(cuda):
    """The chain of test_all_or_nothing_append captured once and replayed three
    times, the record lists and the source rewritten in place between the
    replays: every replay equals the model.  The images fill up, so more of
    them are rolled back each time."""
    import torch
    n_img, per = 24, 3
    rng = np.random.default_rng(31)
    buf, offs, caps, crc = written_images(n_img, lambda i: 150 + 37 * (i % 9))
    s = State(cuda, buf, offs, caps, crc=crc)
    n_rec = n_img * per
    img_t = dev_i32(np.zeros(n_rec, np.uint32), cuda)
    ro_t, rl_t = dev_i64(np.zeros(n_rec, np.uint64), cuda), dev_i64(np.zeros(n_rec, np.uint64), cuda)
    src_t = dev_u8(np.zeros(n_rec * 61 + 16, np.uint8), cuda)
    bst, rb, cm = s.status(), s.status(), s.status()
    ist, rst = s.status(), torch.full((n_rec,), 99, dtype=torch.int32, device=cuda)
    cond = torch.full((n_img,), 77, dtype=torch.int32, device=cuda)
    flags = CK | ZERO

    def stage():
        rec_img, rec_offs, rec_lens, src = batch_of_records(n_img, rng, per)
        img_t.copy_(dev_i32(rec_img, cuda))
        ro_t.copy_(dev_i64(rec_offs, cuda))
        rl_t.copy_(dev_i64(rec_lens, cuda))
        src_t[:len(src)].copy_(dev_u8(src, cuda))
        full = np.zeros(src_t.numel(), np.uint8)
        full[:len(src)] = src
        want = [model.m_tx_begin(s.buf, s.offs, s.caps, s.tx, s.crc)]
        want += list(m_write_records(s.buf, offs, caps, full, rec_img, rec_offs, rec_lens, s.crc))
        want.append(model.m_tx_cond(rec_img, want[2], n_img, want[1]))
        want.append(model.m_tx_rollback(s.buf, s.offs, s.caps, s.tx, s.crc, want[3], flags=flags)[0])
        want.append(model.m_tx_commit(s.buf, s.offs, s.caps, s.tx, s.crc, want[3])[0])
        return want

    def call():
        cf.tx_begin_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, status=bst)
        cf.write_records_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, img_t, ro_t, rl_t, s.crc_t, flags=CK,
                                   img_status=ist, rec_status=rst)
        cf.tx_cond_records_batch_dev(img_t, rst, n_img, img_status=ist, cond=cond)
        cf.tx_rollback_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, cond=cond, flags=flags, status=rb)
        cf.tx_commit_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.tx_t, s.crc_t, cond=cond, status=cm)

    def compare(want, what):
        for t, m, name in zip((bst, ist, rst, cond, rb, cm), want, ("begin", "img", "rec", "cond", "rollback", "commit")):
            assert np.array_equal(i32(t), m), (what, name)
        s.check(what)

    with cio.DevWriter(n_rec) as w:
        want = stage()
        call()                                # warm-up outside the capture (a round like the others)
        torch.cuda.synchronize()
        compare(want, "warm-up")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        s.check("capture runs nothing")
        failed = [int((want[3] != 0).sum())]
        for k in range(3):
            want = stage()
            for t in (bst, rb, cm, ist, rst):
                t.fill_(99)
            cond.fill_(77)
            graph.replay()
            torch.cuda.synchronize()
            compare(want, f"replay {k}")
            failed.append(int((want[3] != 0).sum()))
        del graph
    assert failed[0] < failed[-1] < n_img


# ------------------------------------------------------------------ 9. with grow and rotate

def test_rotate_grow_begin_append_rollback(cuda):
    """rotate -> grow -> begin -> append -> rollback: the images have moved,
    and the state is by index."""
    n = 12
    items = [(i % 4, 30 + 5 * i, 6 + i) for i in range(n)]
    buf, offs, caps, arena = layout(items, 1 << 16)
    s = State(cuda, buf, offs, caps, crc=crc_of_images(buf, offs, items))
    need = [40 if i % 3 == 0 else 12 if i % 3 == 1 else 2 for i in range(n)]
    limit, new_cap = 60, 24 + 3 + 30
    lo, lc, li, count = [0] * n, [0] * n, [0] * n, [0, n]
    arena_t, count_t = dev_i64(arena, cuda), dev_i64(count, cuda)
    need_t = dev_i64(need, cuda)
    with cio.DevWriter(n) as w:
        rst = cf.rotate_batch_dev(w, s.base_t, s.offs_t, s.caps_t, need_t, limit=limit, new_cap=new_cap, align=16,
                                  arena=arena_t, out_count=count_t, flags=CK, crc_cur=s.crc_t)[0]
        want, _, rotated = rmodel.m_rotate(s.buf, s.offs, s.caps, need, limit, new_cap, 16, arena, lo, lc, li, count,
                                           crc_cur=s.crc)
        assert np.array_equal(i32(rst), want) and not want.any() and rotated
        gst = cf.grow_batch_dev(w, s.base_t, s.offs_t, s.caps_t, need_t, arena_t, realloc=64, page=32, align=16)[0]
        gwant = gmodel.m_grow(s.buf, s.offs, s.caps, need, arena, realloc=64, page=32, align=16)
        assert np.array_equal(i32(gst), gwant[0]) and not gwant[0].any()
        s.check("rotate, grow")
        moved = [i for i in range(n) if s.offs[i] != offs[i]]
        assert moved and len(moved) < n and set(rotated) <= set(moved)
        assert not s.begin(w).any()
        assert not s.write(w, [bytes([0x21 + i]) * need[i] for i in range(n)]).any()
        st, rolled = s.rollback(w, None, CK | ZERO, "rollback of moved images")
        assert not st.any() and rolled == list(range(n))
        for i in range(n):
            meta, content = image_check(s.buf, len(s.buf), s.offs[i], s.caps[i])
            assert content == (0 if i in rotated else items[i][1])


def test_rotate_inside_a_transaction_is_an_error_at_rollback(cuda):
    """begin -> append -> rotate -> rollback: the fresh image is shorter than
    the transaction's start, so the rollback reports CIO_ERROR, leaves it
    alone and the state active; the images that were not rotated roll back."""
    n = 6
    items = [(2, 20 + i, 30) for i in range(n)]
    buf, offs, caps, arena = layout(items, 4096)
    s = State(cuda, buf, offs, caps, crc=crc_of_images(buf, offs, items))
    need = [100 if i % 2 else 1 for i in range(n)]                        # the odd images are full
    lo, lc, li, count = [0] * n, [0] * n, [0] * n, [0, n]
    arena_t, count_t = dev_i64(arena, cuda), dev_i64(count, cuda)
    with cio.DevWriter(n) as w:
        assert not s.begin(w).any()
        assert not s.write(w, [b"inside" for _ in range(n)]).any()
        rst = cf.rotate_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_i64(need, cuda), new_cap=128, align=16,
                                  arena=arena_t, out_count=count_t, flags=CK, crc_cur=s.crc_t)[0]
        want, _, rotated = rmodel.m_rotate(s.buf, s.offs, s.caps, need, 0, 128, 16, arena, lo, lc, li, count,
                                           crc_cur=s.crc)
        assert np.array_equal(i32(rst), want) and rotated == [1, 3, 5]
        s.check("rotate")
        snap = s.buf.copy()
        for flags in (CK, CK | ZERO | REC):
            st, rolled = s.rollback(w, None, flags, f"rollback {flags}")
            assert st.tolist() == [0 if flags == CK else -1, -1] * 3 and rolled == ([0, 2, 4] if flags == CK else [])
        for i in rotated:
            assert s.tx[i][0] == 1
            assert np.array_equal(s.buf[s.offs[i]:s.offs[i] + 128], snap[s.offs[i]:s.offs[i] + 128])


# ------------------------------------------------------------------ 10. reference pins

def one_image(cuda, size, meta, w):
    """A zeroed image of `size` bytes at offset 37 with guards, initialised
    with `meta` on the device."""
    off = 37
    buf = np.zeros(off + size + 50, np.uint8)
    buf[:off], buf[off + size:] = 0xEE, 0xEE
    s = State(cuda, buf, [off], [size], crc=[0])
    msrc = np.frombuffer(bytes(meta) + b"\0", np.uint8).copy()
    st, _ = cf.init_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(msrc, cuda), dev_i64([0], cuda),
                              dev_i64([len(meta)], cuda), flags=CK, crc_cur=s.crc_t)
    assert not i32(st).any()
    s.crc[0] = m_init(s.buf, off, meta)
    s.check("init")
    return s


def test_reference_pin_host_chunk_layer(cuda, tmp_path):
    """metadata, write A, begin, write B, rollback, write C, begin, write D,
    commit -- through the host chunk layer (Context / Chunk, the reference's
    semantics) and through the device calls: the used bytes are equal and
    crc_cur is the CRC over the length bytes, the metadata, A, C and D."""
    rng = np.random.default_rng(41)
    meta = b"fluent-bit tag"
    a, b, c, d = (rng.integers(0, 256, k, dtype=np.uint8).tobytes() for k in (3000, 6000, 500, 9))
    with cf.Context(str(tmp_path), CK) as ctx:
        ch, _ = ctx.stream("s").open("t")
        assert ch.meta_write(meta) == 0 and ch.write(a) == 0
        assert ch.tx_begin() == cf.CIO_OK and ch.write(b) == 0 and ch.tx_rollback() == cf.CIO_OK
        assert ch.write(c) == 0
        assert ch.tx_begin() == cf.CIO_OK and ch.write(d) == 0 and ch.tx_commit() == cf.CIO_OK
        used = 24 + len(meta) + ch.data_size
        host, host_crc = bytes(ch.map[:used]), ch.crc_cur
    assert used == 24 + len(meta) + len(a) + len(c) + len(d)
    with cio.DevWriter(1) as w:
        s = one_image(cuda, 16384, meta, w)
        assert not s.write(w, [a]).any()
        assert not s.begin(w).any() and not s.write(w, [b]).any()
        st, rolled = s.rollback(w)
        assert not st.any() and rolled == [0]
        assert not s.write(w, [c]).any()
        assert not s.begin(w).any() and not s.write(w, [d]).any()
        st, done = s.commit(w)
        assert not st.any() and done == [0]
    got = s.base_t.cpu().numpy()
    assert got[37:37 + used].tobytes() == host
    want = po.crc_update(0xFFFFFFFF, struct.pack(">H", len(meta)) + meta + a + c + d)
    assert u32(s.crc_t).tolist() == [want] and host_crc == want


def test_reference_pin_fixture_with_a_rolled_back_append(cuda):
    """c03_meta_content built on the device in a zeroed image of the file's
    size, with a junk append begun and rolled back (CIOA_TX_ZERO) after its
    first write, then sealed: the image has the manifest's SHA-256."""
    spec = [c for c in MANIFEST["chunks"] if c["name"] == "c03_meta_content"][0]
    size, ld = spec["size"], spec["load"]
    meta = spec["ops"][0]["meta"].encode()
    writes = [pattern(o["len"], o["seed"]) for o in spec["ops"] if o["op"] == "write"]
    assert writes and sum(len(x) for x in writes) == ld["content_size"] and len(meta) == ld["meta_size"]
    junk = bytes(range(1, 200)) * 3
    with cio.DevWriter(1) as w:
        s = one_image(cuda, size, meta, w)
        for k, x in enumerate(writes):
            assert not s.write(w, [x]).any()
            if k == 0:
                assert not s.begin(w).any() and not s.write(w, [junk]).any()
                st, rolled = s.rollback(w, None, CK | ZERO)
                assert not st.any() and rolled == [0]
        assert s.crc[0] == ld["crc_cur"]
        assert not i32(cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, s.crc_t, flags=CK)).any()
        m_seal(s.buf, 37, s.crc[0])
        s.check("sealed")
    got = s.base_t.cpu().numpy()
    assert hashlib.sha256(got[37:37 + size].tobytes()).hexdigest() == spec["sha256"]
