"""A seeded random walk over the whole device API on chunk images in HBM: the
calls of cio_write_dev.h, _move.h, _records.h, _ungrouped.h, _grow.h,
_rotate.h, _tx.h and cio_read_dev.h mixed on ONE writer, over slices of one
set of images, with rejected entries in every call.

  Store    the composed model: one numpy buffer (layout() and the sentinel
           fill() of test_gpu_grow_dev.py) with everything the device keeps
           beside it, and every op applied through the existing models.
  Ledger   what a consumer must find: per image the finished chunks and the
           bytes of the open one, kept from statuses and arguments alone.
  ops()    the generator: it draws from the seed and from the Store only, so
           the sequence is the same with and without a GPU.
  walk()   the driver: Store, Ledger and (with a device) the kernels in lock
           step, the ledger checkpoints, and the coverage floors.

Shared by test_lifecycle_walk_model.py (models and ledger alone) and
test_gpu_lifecycle_walk.py (the device against both).  Not a test."""
import struct
import zlib
from collections import Counter

import numpy as np

import grow_dev_model as gmodel
import read_dev_model as rmodel
import rotate_dev_model as rotmodel
import tx_dev_model as txmodel
from grow_dev_model import image_check, needs_of
from test_gpu_grow_dev import layout
from write_dev_move_model import (M32, m_init, m_meta_write, m_region_crc, m_seal, m_write, m_write_at,
                                  raw_update)
from write_dev_records_model import m_write_records
from write_dev_ungrouped_model import m_write_records_ungrouped

OK, ERR = 0, -1
CK, SEAL_REC, GROW_ZERO, TX_REC, TX_ZERO, NUL = 4, 256, 1, 256, 512, 1
S64, S32 = 0x7777777777777777, 0x77777777     # what an unwritten list entry holds
MARK = 0xA7                                   # what an unwritten output byte holds

PROFILES = {
    # 13 images of a few hundred bytes; after two thirds of the walk the producer gives all but 2 entries
    # of the list away and, once it is full, all but 700 bytes of the arena: both run out in the last third
    "narrow": dict(n_img=13, meta=12, content=40, room=(100, 300), rec_len=120, max_rec=40, n_ops=200,
                   arena=80000, list_cap=40, run_out=(700, 2), new_cap=320, clip=0.85, limit=260, each=3,
                   chains=(10, 6, 6),
                   realloc=(1, 32, 100), page=(1, 16, 64), align=(1, 16, 64)),
    # 1024 + 61 images: every per-image block (256, 1024) and, with 3 x as many records, every
    # per-record block is crossed
    "wide": dict(n_img=1085, meta=8, content=30, room=(20, 70), rec_len=24, max_rec=3 * 1085, n_ops=48,
                 arena=6_000_000, clip=0.4, list_cap=2 * 1085, new_cap=160, limit=120, each=1, chains=(2, 1, 3),
                 realloc=(32, 100), page=(1, 16), align=(16, 64)),
}
SEEDS = list(range(1, 21))
SINGLES = ("init", "write", "write_at", "meta", "records", "ungrouped", "grow", "grow_records", "rotate",
           "rotate_records", "tx_begin", "tx_rollback", "tx_commit", "seal", "verify", "read", "read_packed",
           "meta_cmp")
KINDS = SINGLES + ("tx_cond",)


def checksum_of(seed):
    """CIO_CHECKSUM is a property of the walk: off for every fourth seed."""
    return 0 if seed % 4 == 0 else CK


def packed(lens, rng, gap=4):
    """Offsets of records of `lens` bytes in one source, a few bytes apart; (offs, source bytes)."""
    lens = np.asarray(lens, np.uint64)
    gaps = rng.integers(0, gap, len(lens)).astype(np.uint64)
    offs = (np.cumsum(lens + gaps) - lens).astype(np.uint64)
    return offs, rng.integers(0, 256, int((lens + gaps).sum()) + 16, dtype=np.uint8)


# ------------------------------------------------------------------ the composed model

class Store:
    """The images, the arena and the list of finished chunks in one numpy
    buffer with crc_cur, the transaction state and the metadata beside it.
    apply(op) runs one call's model and returns what the call must leave in its
    output arrays; self.info says what happened, for the coverage counters."""

    def __init__(self, profile, seed):
        p = self.p = PROFILES[profile]
        self.ck = checksum_of(seed)
        rng = np.random.default_rng([seed, 0x57])
        n = self.n = p["n_img"]
        items = [(int(rng.integers(0, p["meta"] + 1)), int(rng.integers(0, p["content"] + 1)),
                  int(rng.integers(*p["room"]))) for _ in range(n)]
        self.buf, offs, caps, arena = layout(items, p["arena"])
        self.offs, self.caps, self.arena = [int(x) for x in offs], [int(x) for x in caps], [int(x) for x in arena]
        # three that are no images for the whole walk
        self.bad = {n // 4: "magic", n // 2: "tiny", n - 2: "outside"}
        self.buf[self.offs[n // 4] + 1] = 0x01
        self.caps[n // 2] = 23
        self.offs[n - 2], self.caps[n - 2] = len(self.buf) - 7, 64
        self.crc = [raw_update(M32, self.buf[o + 22:o + 24 + m + c].tobytes()) if i not in self.bad
                    else 0x12345600 + i for i, (o, (m, c, _)) in enumerate(zip(offs, items))]
        self.meta = [self.buf[o + 24:o + 24 + m].tobytes() for o, (m, c, _) in zip(offs, items)]
        self.tx = txmodel.new_state(n)
        alloc = p["list_cap"] + 2
        self.lo, self.lc, self.li, self.count = [S64] * alloc, [S64] * alloc, [S32] * alloc, [0, p["list_cap"]]
        self.taint = [False] * n              # write_at / metadata / init / rotate inside the transaction
        self.last_append = self.last_cond = None
        self.info = {}

    def geo(self, i):
        return image_check(self.buf, len(self.buf), self.offs[i], self.caps[i])

    def room(self, i):
        g = self.geo(i)
        return None if g is None else self.caps[i] - 24 - g[0] - g[1]

    def good(self, a, b):
        return [i for i in range(a, b) if i not in self.bad]

    def apply(self, op):
        self.info = {}
        return getattr(self, "_" + op["kind"])(op)

    def _trim(self, op):
        """The caller's own words: the arena's end and the list's capacity."""
        self.arena[1], self.count[1] = op["arena_end"], op["list_cap"]
        return {}

    # -- the per-image calls: the rejection rules of cio_write_dev.h and cio_write_dev_move.h

    def _init(self, op):
        a, b, src = op["a"], op["b"], op["src"]
        st = np.zeros(b - a, np.int32)
        for k, i in enumerate(range(a, b)):
            off, cap, o, ln = self.offs[i], self.caps[i], int(op["so"][k]), int(op["sl"][k])
            if off + cap > len(self.buf) or cap < 24 or ln > 65535 or 24 + ln > cap or o + ln > len(src):
                st[k] = ERR
                continue
            raw = m_init(self.buf, off, src[o:o + ln].tobytes(), checksum=bool(op["flags"] & CK))
            if op["flags"] & CK:
                self.crc[i] = raw
            self.meta[i] = src[o:o + ln].tobytes()
            self.taint[i] = self.taint[i] or bool(self.tx[i][0])
        return {"status": st}

    def _write(self, op):
        a, b, src = op["a"], op["b"], op["src"]
        st = np.zeros(b - a, np.int32)
        for k, i in enumerate(range(a, b)):
            o, ln = int(op["so"][k]), int(op["sl"][k])
            if ln == 0:
                continue
            g = self.geo(i)
            if g is None or 24 + g[0] + g[1] + ln > self.caps[i] or o + ln > len(src):
                st[k] = ERR
                continue
            self.crc[i] = m_write(self.buf, self.offs[i], src[o:o + ln].tobytes(), self.crc[i],
                                  checksum=bool(op["flags"] & CK))
        return {"status": st}

    def _write_at(self, op):
        a, b, src = op["a"], op["b"], op["src"]
        st = np.zeros(b - a, np.int32)
        for k, i in enumerate(range(a, b)):
            o, ln, at = int(op["so"][k]), int(op["sl"][k]), int(op["at"][k])
            if ln == 0:
                continue
            g = self.geo(i)
            if g is None or at > g[1] or 24 + g[0] + at + ln > self.caps[i] or o + ln > len(src):
                st[k] = ERR
                continue
            self.crc[i] = m_write_at(self.buf, self.offs[i], at, src[o:o + ln].tobytes(), self.crc[i],
                                     checksum=bool(op["flags"] & CK))
            self.taint[i] = self.taint[i] or bool(self.tx[i][0])
        return {"status": st}

    def _meta(self, op):
        a, b, src = op["a"], op["b"], op["src"]
        st = np.zeros(b - a, np.int32)
        for k, i in enumerate(range(a, b)):
            o, ln = int(op["so"][k]), int(op["sl"][k])
            g = self.geo(i)
            if g is None or ln > 65535 or 24 + ln + g[1] > self.caps[i] or o + ln > len(src):
                st[k] = ERR
                continue
            self.crc[i] = m_meta_write(self.buf, self.offs[i], src[o:o + ln].tobytes(), self.crc[i],
                                       checksum=bool(op["flags"] & CK))
            self.meta[i] = src[o:o + ln].tobytes()
            self.taint[i] = self.taint[i] or bool(self.tx[i][0])
        return {"status": st}

    def _seal(self, op):
        a, b = op["a"], op["b"]
        st = np.zeros(b - a, np.int32)
        for k, i in enumerate(range(a, b)):
            if self.geo(i) is None:
                st[k] = ERR
                continue
            if op["flags"] & CK:
                if op["flags"] & SEAL_REC:
                    self.crc[i] = m_region_crc(self.buf, self.offs[i])
                m_seal(self.buf, self.offs[i], self.crc[i])
        return {"status": st}

    def _seal_list(self, op):
        """CIOA_SEAL_RECOMPUTE over the finished chunks, with a crc_cur of their own."""
        cnt = self.count[0]
        crc = np.zeros(cnt, np.uint32)
        for k in range(cnt):
            assert image_check(self.buf, len(self.buf), self.lo[k], self.lc[k]) is not None
            crc[k] = m_region_crc(self.buf, self.lo[k])
            m_seal(self.buf, self.lo[k], int(crc[k]))
        return {"status": np.zeros(cnt, np.int32), "crc": crc}

    # -- the record lists

    def _append(self, op, grouped):
        a, b = op["a"], op["b"]
        crc = self.crc[a:b]
        args = (self.buf, self.offs[a:b], self.caps[a:b], op["src"], op["rec_img"], op["ro"], op["rl"], crc)
        if grouped:
            ist, rst = m_write_records(*args, checksum=bool(op["flags"] & CK))
        else:
            ist, rst, _ = m_write_records_ungrouped(*args, checksum=bool(op["flags"] & CK))
        self.crc[a:b] = crc
        self.last_append = (a, b, op["rec_img"], ist, rst)
        self.info = dict(accepted=int((rst == OK).sum()), rejected=int((rst != OK).sum()),
                         whole=bool((np.asarray(op["rec_img"], np.uint64) >= b - a).any()))
        return {"img_status": ist, "rec_status": rst}

    def _records(self, op):
        return self._append(op, True)

    def _ungrouped(self, op):
        return self._append(op, False)

    # -- grow and rotate

    def _grow(self, op, need=None):
        a, b = op["a"], op["b"]
        need = op["need"] if op["kind"] == "grow" else need
        offs, caps, top = self.offs[a:b], self.caps[a:b], self.arena[0]
        st, total, po, pc = gmodel.m_grow(self.buf, offs, caps, need, self.arena, realloc=op["realloc"],
                                          page=op["page"], align=op["align"], flags=op["flags"])
        moved = sum(1 for k in range(b - a) if offs[k] != self.offs[a + k])
        self.offs[a:b], self.caps[a:b] = offs, caps
        self.info = dict(moved=moved, cut=total > 0 and top + total > self.arena[1], whole=need is None)
        return {"status": st, "total": np.asarray([total], np.uint64), "prev_offs": po, "prev_caps": pc}

    def _grow_records(self, op):
        return self._grow(op, needs_of(op["rec_img"], op["rl"], op["b"] - op["a"]))

    def _rotate(self, op, need=None):
        a, b = op["a"], op["b"]
        need = op["need"] if op["kind"] == "rotate" else need
        offs, caps, crc, have = self.offs[a:b], self.caps[a:b], self.crc[a:b], self.count[0]
        st, total, rotated = rotmodel.m_rotate(self.buf, offs, caps, need, op["limit"], op["new_cap"], op["align"],
                                               self.arena, self.lo, self.lc, self.li, self.count,
                                               flags=op["flags"], crc_cur=crc)
        self.offs[a:b], self.caps[a:b], self.crc[a:b] = offs, caps, crc
        for k in rotated:
            self.taint[a + k] = self.taint[a + k] or bool(self.tx[a + k][0])
        cut = total[1] > len(rotated)
        self.info = dict(rotated=len(rotated), cut=cut, full=cut and self.count[0] == self.count[1],
                         in_tx=sum(1 for k in rotated if self.tx[a + k][0]), whole=need is None)
        # the new list entries, as the list arrays hold them: (list index, image index of the slice)
        return {"status": st, "total": np.asarray(total, np.uint64),
                "list_new": [(k, self.li[k]) for k in range(have, self.count[0])]}

    def _rotate_records(self, op):
        return self._rotate(op, needs_of(op["rec_img"], op["rl"], op["b"] - op["a"]))

    # -- transactions

    def cond_of(self, op):
        return self.last_cond if isinstance(op["cond"], str) else op["cond"]

    def _tx_begin(self, op):
        a, b = op["a"], op["b"]
        tx, was = self.tx[a:b], [t[0] for t in self.tx[a:b]]
        st = txmodel.m_tx_begin(self.buf, self.offs[a:b], self.caps[a:b], tx, self.crc[a:b], flags=op["flags"])
        self.tx[a:b] = tx
        for k in range(b - a):
            if not was[k] and tx[k][0]:
                self.taint[a + k] = False
        return {"status": st}

    def _tx_rollback(self, op):
        a, b = op["a"], op["b"]
        tx, crc = self.tx[a:b], self.crc[a:b]
        before = [self.geo(i) for i in range(a, b)]
        st, rolled = txmodel.m_tx_rollback(self.buf, self.offs[a:b], self.caps[a:b], tx, crc, self.cond_of(op),
                                           flags=op["flags"])
        self.tx[a:b], self.crc[a:b] = tx, crc
        self.info = dict(dropped=sum(1 for k in rolled if before[k][1] > tx[k][1]), rolled=len(rolled))
        return {"status": st}

    def _tx_commit(self, op):
        a, b = op["a"], op["b"]
        tx = self.tx[a:b]
        st, _ = txmodel.m_tx_commit(self.buf, self.offs[a:b], self.caps[a:b], tx, self.crc[a:b], self.cond_of(op),
                                    flags=op["flags"])
        self.tx[a:b] = tx
        return {"status": st}

    def _tx_cond(self, op):
        a, b, rec_img, ist, rst = self.last_append
        assert (a, b) == (op["a"], op["b"])
        self.last_cond = txmodel.m_tx_cond(rec_img, rst, b - a, ist)
        return {"cond": self.last_cond}

    # -- the read-only calls

    def _verify(self, op):
        """Every finished chunk loads: the checks of cio_verify.h, stated on the spot."""
        cnt = self.count[0]
        cr, ml, cl = np.zeros(cnt, np.uint32), np.zeros(cnt, np.int32), np.zeros(cnt, np.uint64)
        for k in range(cnt):
            off = self.lo[k]
            ml[k], cl[k] = image_check(self.buf, len(self.buf), off, self.lc[k])
            if op["flags"] & CK:
                cr[k] = m_region_crc(self.buf, off)
                assert self.buf[off + 2:off + 10].tobytes() == struct.pack(">I", int(cr[k]) ^ M32) + b"\0" * 4, k
        return {"status": np.zeros(cnt, np.int32), "error": np.zeros(cnt, np.int32), "crc": cr, "meta_len": ml,
                "content_len": cl}

    def _read(self, op):
        a, b = op["a"], op["b"]
        st, lens, out = rmodel.read_placed(self.buf, self.offs[a:b], self.caps[a:b], op["what"],
                                           np.full(op["out_size"], MARK, np.uint8), op["out_offs"], op["out_caps"],
                                           flags=op["flags"])
        return {"status": st, "out_lens": lens, "out": out}

    def _read_packed(self, op):
        a, b = op["a"], op["b"]
        st, po, lens, total, out = rmodel.read_packed(self.buf, self.offs[a:b], self.caps[a:b], op["what"],
                                                      np.full(op["out_size"], MARK, np.uint8), align=op["align"],
                                                      flags=op["flags"])
        return {"status": st, "out_offs": po, "out_lens": lens, "total": total, "out": out}

    def _meta_cmp(self, op):
        a, b = op["a"], op["b"]
        res, st = rmodel.meta_cmp(self.buf, self.offs[a:b], self.caps[a:b], op["src"], op["so"], op["sl"])
        return {"result": res, "status": st}

    # -- what a consumer reads: the list, then the live images

    def chunks(self):
        cnt = self.count[0]
        return self.lo[:cnt] + self.offs, self.lc[:cnt] + self.caps

    def contents(self, what):
        """[bytes or None] of record `what` of list + live, through read_dev_model."""
        offs, caps = self.chunks()
        size = sum(caps)
        st, po, lens, _, out = rmodel.read_packed(self.buf, offs, caps, what, np.zeros(size, np.uint8))
        return [out[int(o):int(o + ln)].tobytes() if s == OK else None for s, o, ln in zip(st, po, lens)]


# ------------------------------------------------------------------ the ledger

class Ledger:
    """Per image the finished chunks and the bytes of the open one.  It never
    looks at the buffer: update() takes a call's arguments and the statuses
    (and, for a rotate, the entries the call added to the list)."""

    def __init__(self, store):
        self.n = store.n
        self.open, self.meta = [None] * store.n, [None] * store.n
        for i in store.good(0, store.n):      # what the images are set up with
            m, c = store.geo(i)
            o = store.offs[i] + 24
            self.meta[i], self.open[i] = store.buf[o:o + m].tobytes(), bytearray(store.buf[o + m:o + m + c].tobytes())
        self.done = []                        # by list index: (image, metadata, content)
        self.active, self.saved = [False] * store.n, [0] * store.n
        self.cond = None

    def update(self, op, out):
        kind, a = op["kind"], op.get("a", 0)
        st = out.get("status")
        if kind == "init":
            for k in np.flatnonzero(st == OK):
                o, ln = int(op["so"][k]), int(op["sl"][k])
                self.meta[a + k], self.open[a + k] = op["src"][o:o + ln].tobytes(), bytearray()
        elif kind in ("write", "write_at"):
            for k in np.flatnonzero((st == OK) & (op["sl"] != 0)):
                o, ln = int(op["so"][k]), int(op["sl"][k])
                if kind == "write_at":
                    del self.open[a + k][int(op["at"][k]):]
                self.open[a + k] += op["src"][o:o + ln].tobytes()
        elif kind == "meta":
            for k in np.flatnonzero(st == OK):
                o, ln = int(op["so"][k]), int(op["sl"][k])
                self.meta[a + k] = op["src"][o:o + ln].tobytes()
        elif kind in ("records", "ungrouped"):
            rst = out["rec_status"]
            for img in np.unique(op["rec_img"][rst != OK]):           # the prefix rule, from the statuses alone
                run = rst[op["rec_img"] == img]
                assert (run[int(np.argmax(run != OK)):] != OK).all(), (int(img), "accepted after a rejected record")
            for r in np.flatnonzero((rst == OK) & (op["rl"] != 0)):
                o, ln = int(op["ro"][r]), int(op["rl"][r])
                self.open[a + int(op["rec_img"][r])] += op["src"][o:o + ln].tobytes()
        elif kind in ("rotate", "rotate_records"):
            for k, img in out["list_new"]:
                assert k == len(self.done) and img < len(st) and st[img] == OK, ("list entry", k, "image", img)
                i = a + img                   # the list holds the index inside the slice
                self.done.append((i, self.meta[i], bytes(self.open[i])))
                self.open[i] = bytearray()
        elif kind == "tx_begin":
            for k in np.flatnonzero(st == OK):
                if not self.active[a + k]:
                    self.active[a + k], self.saved[a + k] = True, len(self.open[a + k])
        elif kind == "tx_cond":
            self.cond = out["cond"]
        elif kind in ("tx_rollback", "tx_commit"):
            cond = self.cond if isinstance(op["cond"], str) else op["cond"]
            for k in np.flatnonzero(st == OK):
                taken = cond is None or (cond[k] != OK) == (kind == "tx_rollback")
                if taken and kind == "tx_rollback":
                    assert self.active[a + k] and len(self.open[a + k]) >= self.saved[a + k], (a + k, "rolled back")
                    del self.open[a + k][self.saved[a + k]:]
                if taken:
                    self.active[a + k] = False

    def expected(self, what):
        """Record `what` (read_dev_model.META / CONTENT) of list + live."""
        pick = (lambda m, c: m) if what == rmodel.META else (lambda m, c: c)
        return [pick(m, c) for _, m, c in self.done] + \
               [None if self.open[i] is None else pick(self.meta[i], bytes(self.open[i])) for i in range(self.n)]


# ------------------------------------------------------------------ the generator

def ops(profile, seed, store=None):
    """Yields (op, want): the op's description -- a dict of its kind, the slice
    [a, b), flags and numpy arguments -- and what the Store says the call must
    leave in its output arrays.  The op is already applied to the Store when it
    is yielded.  Everything is drawn from default_rng(seed) and the Store."""
    p = PROFILES[profile]
    s = store if store is not None else Store(profile, seed)
    rng = np.random.default_rng(seed)
    n, ck, n_ops = s.n, s.ck, p["n_ops"]
    last_third = [False]
    rolled = {(0, 0): 0, (TX_ZERO, 0): 0, (TX_ZERO, TX_REC): 0, (0, TX_REC): 0}     # rollbacks that took an image
    wholes = [0]
    entries = [0, 0]                          # record entries accepted, rejected so far
    trimmed = [False, False]                  # the list, the arena

    def rejected_share():
        return entries[1] / max(sum(entries), 1)

    def a_slice():
        r = rng.random()
        if r < 0.3:
            return 0, n
        if r < 0.4:
            a = int(rng.integers(0, n))
            return a, a + 1
        a = int(rng.integers(1, n - 1))
        return a, int(rng.integers(a + 1, n + 1))

    def sources(lens):
        so, src = packed(lens, rng)
        return dict(src=src, so=so, sl=np.asarray(lens, np.uint64))

    def chain_slice():
        while True:
            a, b = a_slice()
            if len(s.good(a, b)) >= min(3, n - 3):
                return a, b

    def record_list(a, b, tight, single=False):
        """A list for the images of [a, b): the three that are no images get a
        third of a share; empty records; one index outside the batch now and
        then (the whole call is rejected); and, when nothing is queued to make
        room (tight), a record that lacks exactly one byte."""
        m = b - a
        n_rec = int(rng.integers(1, min(p["max_rec"], 3 * m) + 1))
        w = np.asarray([0.3 if i in s.bad else 1.0 for i in range(a, b)])
        rec_img = rng.choice(m, n_rec, p=w / w.sum()).astype(np.uint32)
        rl = rng.integers(0, p["rec_len"] + 1, n_rec).astype(np.uint64)
        rl[rng.random(n_rec) < 0.08] = 0
        share = rejected_share()              # kept between the floors: more lacking bytes, or more cut to fit
        if tight:                             # nothing is queued to make room: most records are cut to fit
            left = {}
            for r in np.flatnonzero(rng.random(n_rec) < (1.0 if share > 0.25 else p["clip"])):
                i = int(rec_img[r])
                if i not in left:
                    left[i] = s.room(a + i) or 0
                rl[r] = min(int(rl[r]), left[i])
                left[i] -= int(rl[r])
        lacking = max(1, n_rec // 4) if share < 0.08 else max(1, n_rec // 10) if share < 0.25 else 0
        for r in rng.integers(0, n_rec, lacking if tight else 0):
            room = s.room(a + int(rec_img[r]))
            if room is not None:
                ahead = int(rl[:r][rec_img[:r] == rec_img[r]].sum())
                if 0 < room + 1 - ahead <= 4 * p["rec_len"] + 64:
                    rl[r] = room + 1 - ahead
        # an index outside the batch: the whole call is rejected (at most 4 % of the calls)
        if single and (wholes[0] == 0 or (rng.random() < 0.1 and wholes[0] < n_ops // 25)):
            wholes[0] += 1
            rec_img[int(rng.integers(0, n_rec))] = m if rng.random() < 0.5 else 0xFFFFFF00
        ro, src = packed(rl, rng)
        return dict(a=a, b=b, rec_img=rec_img, ro=ro, rl=rl, src=src)

    def grow_args():
        big = trimmed[1] and s.arena[0] < s.arena[1]
        return dict(realloc=1024 if big else int(rng.choice(p["realloc"])), page=int(rng.choice(p["page"])),
                    align=int(rng.choice(p["align"])), flags=GROW_ZERO if rng.random() < 0.5 else 0)

    def rotate_args():
        tightly = p.get("run_out") and last_third[0] and s.count[0] < s.count[1]
        return dict(limit=1 if tightly else int(rng.choice((0, 0, 0, p["limit"]))), new_cap=p["new_cap"],
                    align=int(rng.choice(p["align"])), flags=ck)

    def sparing():
        """Before the last third of a walk whose list is to run out there: keep a batch's worth of it."""
        return bool(p.get("run_out")) and not last_third[0] and s.count[1] - s.count[0] <= n

    def needs(a, b):
        """Per image: 0, what fits, or more than the room."""
        need = rng.integers(1, 2 * p["rec_len"], b - a).astype(np.uint64)
        need[rng.random(b - a) < 0.2] = 0
        return need

    def per_image(a, b, kind):
        """Record lengths of write / write_at: empty, one byte too many, exactly the room, ordinary."""
        lens = rng.integers(1, p["rec_len"] + 1, b - a).astype(np.uint64)
        at = np.zeros(b - a, np.uint64)
        cls = rng.random(b - a)
        for k, i in enumerate(range(a, b)):
            g = s.geo(i)
            if g is None:
                if cls[k] < 0.5:
                    lens[k] = 0               # a no-op with CIO_OK even there
                continue
            room = s.caps[i] - 24 - g[0] - g[1]
            if kind == "write_at":
                at[k] = g[1] + 1 if cls[k] < 0.07 else g[1] if cls[k] < 0.2 else int(rng.integers(0, g[1] + 1))
                room += g[1] - min(int(at[k]), g[1])
            if cls[k] > 0.9:
                lens[k] = 0
            elif cls[k] > 0.84 and room + 1 <= 4 * p["rec_len"] + 400:
                lens[k] = room + 1
            elif cls[k] > 0.8 and 0 < room <= 4 * p["rec_len"] + 400:
                lens[k] = room
            elif room > 0:
                lens[k] = min(int(lens[k]), max(1, room // 2 + 1)) if cls[k] < 0.7 else lens[k]
        return lens, at

    def rollback_flags(a, b, cond):
        """The four kinds in turn; CIOA_TX_RECOMPUTE where an image that the call
        takes saw write_at, a metadata rewrite, init or a rotate since its begin
        (without it: the documented hazard)."""
        zero, rec = min(rolled, key=rolled.get)          # the kind that has taken the fewest images so far
        for k, i in enumerate(range(a, b)):
            if s.tx[i][0] and s.taint[i] and (cond is None or cond[k] != OK):
                rec = TX_REC
        return zero | rec | (CK if rec else ck)

    def a_cond(a, b):
        return None if rng.random() < 0.5 else rng.choice(np.asarray([0, 0, -1, -3], np.int32), b - a)

    def build(kind, extra):
        a, b = (extra["a"], extra["b"]) if "a" in extra else a_slice()
        op = dict(kind=kind, a=a, b=b, flags=ck)
        if kind == "init":
            lens = rng.integers(0, p["meta"] + 1, b - a)
            for k, i in enumerate(range(a, b)):
                if s.bad.get(i) == "magic" or rng.random() < 0.1:
                    lens[k] = max(s.caps[i] - 23, 0)          # metadata that does not fit
            op.update(sources(lens))
        elif kind in ("write", "write_at"):
            lens, at = extra["lens"] if "lens" in extra else per_image(a, b, kind)
            op.update(sources(lens))
            if kind == "write_at":
                op["at"] = at
        elif kind == "meta":
            lens = rng.integers(0, p["meta"] + 1, b - a)
            for k, i in enumerate(range(a, b)):
                g = s.geo(i)
                if g is not None and rng.random() < 0.15:
                    lens[k] = s.caps[i] - 24 - g[1] + 1       # one byte too long
                    if lens[k] > 2000:
                        lens[k] = 65536
            op.update(sources(lens))
        elif kind in ("records", "ungrouped", "grow_records", "rotate_records"):
            rec = extra if "rec_img" in extra else record_list(a, b, kind in ("records", "ungrouped"), single=True)
            op.update({k: rec[k] for k in ("rec_img", "ro", "rl", "src")})
            if kind == "records":
                order = np.argsort(np.minimum(op["rec_img"], b - a), kind="stable")
                op.update(rec_img=op["rec_img"][order], ro=op["ro"][order], rl=op["rl"][order])
            if kind == "grow_records":
                op.update(grow_args())
            if kind == "rotate_records":
                op.update(rotate_args())
        elif kind == "grow":
            op.update(grow_args(), need=extra["need"] if "need" in extra else needs(a, b))
        elif kind == "rotate":
            op.update(rotate_args(), need=extra["need"] if "need" in extra else needs(a, b))
            if sparing():
                op.update(limit=0, need=np.zeros(b - a, np.uint64))       # a need of 0: not read
        elif kind == "tx_rollback":
            cond = s.last_cond if "cond" in extra else a_cond(a, b) if "a" not in extra or "given" in extra else None
            op.update(cond="last" if "cond" in extra else cond, flags=rollback_flags(a, b, cond))
        elif kind == "tx_commit":
            op["cond"] = "last" if "cond" in extra else a_cond(a, b)
        elif kind == "seal":
            op["flags"] = CK | SEAL_REC if not ck or rng.random() < 0.5 else CK
            if extra.get("final"):
                op["flags"] = CK if ck else CK | SEAL_REC
        elif kind in ("read", "read_packed"):
            op.update(what=int(rng.integers(0, 3)), flags=NUL if rng.random() < 0.5 else 0)
            sizes = [24 + sum(g) if g is not None else 0 for g in (s.geo(i) for i in range(a, b))]
            if kind == "read":
                caps = np.asarray(sizes, np.uint64) + np.uint64(1)
                short = rng.random(b - a) < 0.1
                caps[short] = np.asarray(sizes, np.uint64)[short] // np.uint64(3)     # a slot too small
                op["out_caps"] = caps
                op["out_offs"] = (np.cumsum(caps + np.uint64(3)) - caps).astype(np.uint64)
                op["out_size"] = int((caps + np.uint64(3)).sum()) + 8
            else:
                op["align"] = int(rng.choice((1, 4, 16)))
                full = sum(sizes) + (op["align"] + 1) * (b - a)
                op["out_size"] = full if rng.random() < 0.7 else full // 2            # the tail does not fit
        elif kind == "meta_cmp":
            metas = [s.meta[i] for i in range(a, b)]
            for k in np.flatnonzero(rng.random(b - a) < 0.3):
                metas[k] = metas[k] + b"x" if rng.random() < 0.5 else bytes(x ^ 1 for x in metas[k])
            so, src = packed([len(m) for m in metas], rng)
            for o, m in zip(so, metas):
                src[int(o):int(o) + len(m)] = np.frombuffer(m, np.uint8)
            op.update(src=src, so=so, sl=np.asarray([len(m) for m in metas], np.uint64))
        return op

    def chain_records():
        """[begin] [rotate_records] [grow_records] append cond rollback(cond) commit(cond), one list, one slice."""
        a, b = chain_slice()
        roomy = rng.random() < 0.6
        rec = record_list(a, b, tight=not roomy)
        out = [("tx_begin", dict(a=a, b=b))]
        if roomy and rng.random() < 0.7 and not sparing():
            out.append(("rotate_records", rec))
        if roomy:
            out.append(("grow_records", rec))
        out.append(("records" if rng.random() < 0.5 else "ungrouped", rec))
        out += [("tx_cond", dict(a=a, b=b)), ("tx_rollback", dict(a=a, b=b, cond="last")),
                ("tx_commit", dict(a=a, b=b, cond="last"))]
        return out

    def chain_write():
        """rotate grow write: the needs are the records' lengths."""
        a, b = chain_slice()
        lens = rng.integers(0, p["rec_len"] + 1, b - a).astype(np.uint64)
        for k, i in enumerate(range(a, b)):
            if i in s.bad and rng.random() < 0.5:
                lens[k] = 0
        x = dict(a=a, b=b, need=lens, lens=(lens, None))
        return [("rotate", x), ("grow", x), ("write", x)][sparing():]

    def chain_tx_write():
        """begin write rollback: what the write appended is dropped."""
        a, b = chain_slice()
        x = dict(a=a, b=b)
        return [("tx_begin", x), ("write", x), ("tx_rollback", x if rng.random() < 0.7 else dict(x, given=True))]

    chains = (chain_records, chain_write, chain_tx_write)
    # the deck: every kind `each` times, the chains, shuffled; the rest drawn as the walk goes
    deck = [[(k, {})] for k in SINGLES for _ in range(p["each"])]
    deck += [j for j in range(3) for _ in range(p["chains"][j])]
    deck = [deck[i] for i in rng.permutation(len(deck))]
    queue, done, cut_grow = [], 0, [False]
    while done < n_ops:
        last_third[0] = done >= 2 * n_ops // 3
        if p.get("run_out") and last_third[0]:
            full = s.count[0] >= s.count[1]
            if not trimmed[0] or (full and not trimmed[1]):
                end = min(s.arena[1], s.arena[0] + p["run_out"][0]) if trimmed[0] else s.arena[1]
                op = dict(kind="trim", arena_end=end, list_cap=min(s.count[1], s.count[0] + p["run_out"][1]), flags=0)
                trimmed[trimmed[0]] = True
                yield op, s.apply(op)
            elif not full and done >= 5 * n_ops // 6 and not queue:
                queue = [("rotate", dict(a=0, b=n, need=np.ones(n, np.uint64), force=True))]
            elif trimmed[1] and not cut_grow[0] and done >= n_ops - 8 and not queue:
                queue = [("grow", dict(a=0, b=n, need=np.full(n, 5000, np.uint64)))]
        if not queue:
            item = deck.pop(0) if deck else [(str(rng.choice(SINGLES)), {})] if rng.random() < 0.6 else \
                int(rng.integers(0, 3))
            queue = chains[item]() if isinstance(item, int) else list(item)
        kind, extra = queue.pop(0)
        if kind == "verify" and s.count[0] == 0:
            queue = [("verify", {})] + queue  # nothing finished yet: rotate first, verify after it
            kind, extra = "rotate", dict(a=0, b=n, need=np.ones(n, np.uint64), force=True)
        op = build(kind, extra)
        if extra.get("force"):
            op["limit"] = 1                   # every image with content is full
        want = s.apply(op)
        done += 1
        cut_grow[0] = cut_grow[0] or (kind in ("grow", "grow_records") and s.info["cut"])
        if kind in ("write", "write_at"):
            entries[0] += int((want["status"] == OK).sum())
            entries[1] += int((want["status"] != OK).sum())
        elif kind in ("records", "ungrouped"):
            entries[0] += s.info["accepted"]
            entries[1] += s.info["rejected"]
        if kind == "tx_rollback" and s.info["rolled"]:
            rolled[op["flags"] & TX_ZERO, op["flags"] & TX_REC] += 1
        yield op, want
    # the end of the walk: everything is sealed
    if not ck and s.count[0]:
        op = dict(kind="seal_list", flags=CK | SEAL_REC)
        yield op, s.apply(op)
    op = build("seal", dict(a=0, b=n, final=True))
    yield op, s.apply(op)


def describe(op):
    skip = ("src", "so", "sl", "ro", "rl", "rec_img", "at", "need", "out_offs", "out_caps", "cond")
    text = " ".join(f"{k}={v}" for k, v in op.items() if k not in skip)
    if "rec_img" in op:
        text += f" n_rec={len(op['rec_img'])}"
    if "cond" in op:
        text += " cond=" + ("none" if op["cond"] is None else "last" if isinstance(op["cond"], str) else "given")
    return text


# ------------------------------------------------------------------ the device

class Device:
    """The same state on the GPU: one DevWriter and one Crc32DevPlan for the
    whole walk.  call(op) queues one call with every output array pre-filled
    with a marker and returns the output tensors by the names of Store.apply's;
    nothing is read back."""

    def __init__(self, store, cuda):
        import torch

        import chunkio_amd as cio
        from chunkio_amd import chunkfile as cf
        self.torch, self.cf, self.cuda = torch, cf, cuda
        p = store.p
        self.w = cio.DevWriter(max(p["n_img"], p["max_rec"]), move=True)
        self.plan = cio.Crc32DevPlan(max(p["n_img"], p["max_rec"]))
        self.base = self.u8(store.buf)
        self.offs, self.caps, self.arena = self.i64(store.offs), self.i64(store.caps), self.i64(store.arena)
        self.crc = self.i32(np.asarray(store.crc, np.uint32))
        self.tx = cf.tx_state(store.n, cuda)
        self.lo, self.lc, self.li = self.i64(store.lo), self.i64(store.lc), self.i32(np.asarray(store.li, np.uint32))
        self.count = self.i64(store.count)
        self.append = self.cond = None
        self.keep = []                        # every argument tensor of the calls not yet compared

    def close(self):
        self.torch.cuda.synchronize()
        self.plan.close() if hasattr(self.plan, "close") else None
        self.w.close()

    def u8(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(self.cuda)

    def i64(self, a):
        return self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(self.cuda)

    def i32(self, a):
        a = np.ascontiguousarray(a)
        return self.torch.from_numpy(a.view(np.int32) if a.dtype.itemsize == 4 else a.astype(np.int32)).to(self.cuda)

    def full(self, n, value, dtype=None):
        return self.torch.full((n,), value, dtype=dtype or self.torch.int32, device=self.cuda)

    def call(self, op, want):
        cf, t = self.cf, self.torch
        kind, fl = op["kind"], op["flags"]
        if kind == "trim":
            self.arena[1:2].copy_(self.i64([op["arena_end"]]))
            self.count[1:2].copy_(self.i64([op["list_cap"]]))
            return {}
        if kind in ("verify", "seal_list"):
            cnt = len(want["status"])
            lo, lc = self.lo[:cnt], self.lc[:cnt]
            if kind == "verify":
                out = dict(zip(("status", "error", "crc", "meta_len", "content_len"),
                               cf.verify_batch_dev(self.plan, self.base, lo, lc, flags=fl)))
            else:
                crc = self.full(cnt, 0x5EED)
                out = {"status": cf.seal_batch_dev(self.w, self.base, lo, lc, crc, flags=fl, status=self.full(cnt, 99)),
                       "crc": crc}
            self.keep.append((lo, lc, out))
            return out
        a, b = op["a"], op["b"]
        m = b - a
        O, C, R, T = self.offs[a:b], self.caps[a:b], self.crc[a:b], self.tx[a:b]
        args = {k: (self.u8 if k == "src" else self.i32 if k == "rec_img" else self.i64)(op[k])
                for k in ("src", "so", "sl", "ro", "rl", "rec_img", "at", "need", "out_offs", "out_caps") if k in op}
        st = self.full(m, 99)
        out = {"status": st}
        if kind == "init":
            cf.init_batch_dev(self.w, self.base, O, C, args["src"], args["so"], args["sl"], flags=fl, crc_cur=R,
                              status=st)
        elif kind == "write":
            cf.write_batch_dev(self.w, self.base, O, C, args["src"], args["so"], args["sl"], R, flags=fl, status=st)
        elif kind == "write_at":
            cf.write_at_batch_dev(self.w, self.base, O, C, args["at"], args["src"], args["so"], args["sl"], R, flags=fl,
                                  status=st)
        elif kind == "meta":
            cf.write_metadata_batch_dev(self.w, self.base, O, C, args["src"], args["so"], args["sl"], R, flags=fl,
                                        status=st)
        elif kind == "seal":
            cf.seal_batch_dev(self.w, self.base, O, C, R, flags=fl, status=st)
        elif kind in ("records", "ungrouped"):
            call = cf.write_records_batch_dev if kind == "records" else cf.write_records_ungrouped_batch_dev
            rst = self.full(len(op["rec_img"]), 99)
            call(self.w, self.base, O, C, args["src"], args["rec_img"], args["ro"], args["rl"], R, flags=fl,
                 img_status=st, rec_status=rst)
            out = {"img_status": st, "rec_status": rst}
            self.append = (args["rec_img"], st, rst)
        elif kind in ("grow", "grow_records"):
            out.update(total=self.i64([0x55]), prev_offs=self.i64(np.full(m, 0x77, np.uint64)),
                       prev_caps=self.i64(np.full(m, 0x77, np.uint64)))
            kw = dict(realloc=op["realloc"], page=op["page"], align=op["align"], flags=fl, **out)
            if kind == "grow":
                cf.grow_batch_dev(self.w, self.base, O, C, args["need"], self.arena, **kw)
            else:
                cf.grow_records_batch_dev(self.w, self.base, O, C, args["rec_img"], args["rl"], self.arena, **kw)
        elif kind in ("rotate", "rotate_records"):
            out["total"] = self.i64([0x55, 0x55])
            kw = dict(limit=op["limit"], new_cap=op["new_cap"], align=op["align"], arena=self.arena, out_offs=self.lo,
                      out_caps=self.lc, out_img=self.li, out_count=self.count, flags=fl,
                      crc_cur=R if fl & CK else None, **out)
            if kind == "rotate":
                cf.rotate_batch_dev(self.w, self.base, O, C, args["need"], **kw)
            else:
                cf.rotate_records_batch_dev(self.w, self.base, O, C, args["rec_img"], args["rl"], **kw)
        elif kind == "tx_begin":
            cf.tx_begin_batch_dev(self.w, self.base, O, C, T, R if fl & CK else None, flags=fl, status=st)
        elif kind in ("tx_rollback", "tx_commit"):
            cond = self.cond if isinstance(op["cond"], str) else None if op["cond"] is None else self.i32(op["cond"])
            call = cf.tx_rollback_batch_dev if kind == "tx_rollback" else cf.tx_commit_batch_dev
            call(self.w, self.base, O, C, T, R if fl & CK else None, cond=cond, flags=fl, status=st)
            args["cond"] = cond
        elif kind == "tx_cond":
            rec_img, ist, rst = self.append   # the statuses of the append before it, as the device left them
            self.cond = cf.tx_cond_records_batch_dev(rec_img, rst, m, img_status=ist, cond=self.full(m, 77))
            out = {"cond": self.cond}
        elif kind == "read":
            out.update(out=self.full(op["out_size"], MARK, t.uint8), out_lens=self.i64(np.full(m, 0x77, np.uint64)))
            cf.read_batch_dev(self.w, self.base, O, C, op["what"], out["out"], args["out_offs"], args["out_caps"],
                              flags=fl, out_lens=out["out_lens"], status=st)
        elif kind == "read_packed":
            out.update(out=self.full(op["out_size"], MARK, t.uint8), out_lens=self.i64(np.full(m, 0x77, np.uint64)),
                       out_offs=self.i64(np.full(m, 0x77, np.uint64)), total=self.i64([0x55]))
            cf.read_packed_batch_dev(self.w, self.base, O, C, op["what"], out["out"], align=op["align"], flags=fl,
                                     out_offs=out["out_offs"], out_lens=out["out_lens"], total=out["total"], status=st)
        elif kind == "meta_cmp":
            out["result"] = self.full(m, 99)
            cf.meta_cmp_batch_dev(self.base, O, C, args["src"], args["so"], args["sl"], result=out["result"], status=st)
        else:
            raise ValueError(kind)
        self.keep.append((O, C, R, T, args, out))
        return out

    def compare_outputs(self, out, want, what):
        for name, w in want.items():
            if name == "list_new":
                continue
            g = out[name].cpu().numpy()
            w = np.asarray(w)
            g = g.view(w.dtype) if g.dtype != w.dtype and g.dtype.itemsize == w.dtype.itemsize else g
            if not np.array_equal(g, w):
                bad = np.flatnonzero(g != w) if g.shape == w.shape else []
                raise AssertionError(f"{what}: output {name} differs at {[int(x) for x in bad[:8]]} of {len(w)}: "
                                     f"{g[bad[:8]] if len(bad) else g.shape} for {w[bad[:8]] if len(bad) else w.shape}")

    def compare_state(self, s, what):
        """Everything a call may touch, against the Store."""
        def u(t, dt):
            return t.cpu().numpy().view(dt).reshape(-1).tolist()
        for name, t, dt, w in (("offsets", self.offs, np.uint64, s.offs), ("capacities", self.caps, np.uint64, s.caps),
                               ("crc_cur", self.crc, np.uint32, s.crc), ("arena", self.arena, np.uint64, s.arena),
                               ("count", self.count, np.uint64, s.count), ("list offsets", self.lo, np.uint64, s.lo),
                               ("list capacities", self.lc, np.uint64, s.lc), ("list images", self.li, np.uint32, s.li),
                               ("transaction state", self.tx, np.uint32, [x for t4 in s.tx for x in t4])):
            got = u(t, dt)
            if got != w:
                bad = [i for i in range(len(w)) if got[i] != w[i]][:8]
                raise AssertionError(f"{what}: {name} differ at {bad}: {[got[i] for i in bad]} for "
                                     f"{[w[i] for i in bad]}")
        got = self.base.cpu().numpy()
        if not np.array_equal(got, s.buf):
            bad = np.flatnonzero(got != s.buf)
            raise AssertionError(f"{what}: {len(bad)} bytes of the buffer differ, first at {bad[:6]} of {len(got)}")

    def checkpoint(self, s, ledger, what):
        """verify_batch_dev accepts every finished chunk, and read_packed_batch_dev
        of list + live gives the ledger's contents."""
        cf, t = self.cf, self.torch
        cnt = s.count[0]
        if cnt:
            vst = cf.verify_batch_dev(self.plan, self.base, self.lo[:cnt], self.lc[:cnt], flags=s.ck)[0]
            assert not vst.cpu().numpy().any(), (what, "verify-on-load of the finished chunks", vst.cpu().numpy())
        got = []
        for offs, caps, size in ((self.lo[:cnt], self.lc[:cnt], sum(s.lc[:cnt])), (self.offs, self.caps, sum(s.caps))):
            if offs.numel() == 0:
                continue
            out = self.full(int(size), 0, t.uint8)
            st, po, ln, _ = cf.read_packed_batch_dev(self.w, self.base, offs, caps, rmodel.CONTENT, out)
            st, po, ln, out = st.cpu().numpy(), po.cpu().numpy(), ln.cpu().numpy(), out.cpu().numpy()
            got += [out[int(o):int(o + k)].tobytes() if x == OK else None for x, o, k in zip(st, po, ln)]
        compare_ledger(got, ledger.expected(rmodel.CONTENT), cnt, what + " (device content)")


def compare_ledger(got, want, cnt, what):
    assert len(got) == len(want), (what, len(got), len(want))
    for k, (g, w) in enumerate(zip(got, want)):
        if g != w:
            where = f"finished chunk {k}" if k < cnt else f"open image {k - cnt}"
            first = "" if None in (g, w) else "; first difference at %d" % next(
                (i for i, (x, y) in enumerate(zip(g, w)) if x != y), min(len(g), len(w)))
            raise AssertionError(f"{what}: {where} holds {None if g is None else len(g)} bytes, the ledger "
                                 f"{None if w is None else len(w)}{first}")


# ------------------------------------------------------------------ the driver

def count(c, op, info, want, prev_n):
    """What one op adds to the counters of the floors; the op's n."""
    kind = op["kind"]
    if kind == "trim":
        return prev_n
    c["kind", kind] += 1
    c["calls"] += 1
    n_now = len(want["status"]) if kind in ("verify", "seal_list") else op["b"] - op["a"]
    c["smaller"] += prev_n is not None and n_now < prev_n
    c["a>0"] += op.get("a", 0) > 0
    c["whole"] += bool(info.get("whole"))
    if kind in ("write", "write_at"):
        c["accepted"] += int((want["status"] == OK).sum())
        c["rejected"] += int((want["status"] != OK).sum())
    elif kind in ("records", "ungrouped"):
        c["accepted"] += info["accepted"]
        c["rejected"] += info["rejected"]
    elif kind in ("grow", "grow_records"):
        c["grows"] += info["moved"]
        c["cut grow"] += info["cut"]
        c["first cut grow at"] = c["first cut grow at"] or info["cut"] * c["calls"]
    elif kind in ("rotate", "rotate_records"):
        c["rotations"] += info["rotated"]
        c["cut rotate"] += info["cut"]
        c["full list"] += info["full"]
        c["first cut rotate at"] = c["first cut rotate at"] or info["cut"] * c["calls"]
        c["rotated in tx"] += info["in_tx"]
    elif kind == "tx_rollback":
        c["dropped"] += info["dropped"] > 0
        if info["rolled"]:
            c["rb zero"] += bool(op["flags"] & TX_ZERO)
            c["rb recompute"] += bool(op["flags"] & TX_REC)
            c["rb neither"] += not op["flags"] & (TX_ZERO | TX_REC)
    return n_now


def floors(c, profile):
    """The conditions on the generator: every op kind >= 3 times (narrow) / once
    (wide); >= 60 % of the record entries accepted, >= 5 % rejected; 1 .. 10 % of
    the calls rejected whole; >= 3 rotations and >= 3 grows that moved an image;
    >= 3 rollbacks that dropped bytes; a rollback that took an image with ZERO,
    with RECOMPUTE and with neither; >= 5 calls of a smaller n than the call
    before; >= 5 slices with a > 0; (narrow) a rotate inside a transaction, and a
    cut grow, a cut rotate and a full list, none of them before the last third.
    Returns those that are not met."""
    narrow = profile == "narrow"
    entries = c["accepted"] + c["rejected"]
    want = {f"kind {k}": c["kind", k] >= (3 if narrow else 1) for k in KINDS}
    want.update({
        "60 % of the record entries accepted": c["accepted"] >= 0.6 * entries,
        "5 % of the record entries rejected": c["rejected"] >= 0.05 * entries,
        "a call rejected whole": c["whole"] >= 1,
        "at most 10 % of the calls rejected whole": c["whole"] <= 0.1 * c["calls"],
        "3 rotations": c["rotations"] >= 3, "3 grows that moved an image": c["grows"] >= 3,
        "3 rollbacks that dropped bytes": c["dropped"] >= 3,
        "rollback with ZERO": c["rb zero"] >= 1, "rollback with RECOMPUTE": c["rb recompute"] >= 1,
        "rollback with neither": c["rb neither"] >= 1,
        "5 calls of a smaller n": c["smaller"] >= 5, "5 slices with a > 0": c["a>0"] >= 5})
    if narrow:
        third = 2 * PROFILES[profile]["n_ops"] // 3
        want.update({"a cut grow": c["cut grow"] >= 1, "a cut rotate": c["cut rotate"] >= 1,
                     "a full list": c["full list"] >= 1, "a rotate inside a transaction": c["rotated in tx"] >= 1,
                     "arena and list last until the last third": min(c["first cut grow at"],
                                                                     c["first cut rotate at"]) > third})
    return [k for k, ok in want.items() if not ok]


def walk(profile, seed, cuda=None, sync_every=1, every=10):
    """One walk.  Without a device: the models and the ledger alone.  With one:
    the kernels in lock step, compared after every sync_every ops.  Returns
    (store, ledger, counters); the floors are asserted."""
    s = Store(profile, seed)
    ledger = Ledger(s)
    dev = Device(s, cuda) if cuda is not None else None
    c, prev_n, pending = Counter(), None, []
    offs_before, top_before = list(s.offs), s.arena[0]
    tag = f"walk {profile} seed {seed}"

    def sync(what):
        for k, op, out, want in pending:
            dev.compare_outputs(out, want, f"{tag} op {k}: {describe(op)}")
        dev.compare_state(s, what + (f" (ops {pending[0][0]}..{pending[-1][0]})" if len(pending) > 1 else ""))
        del pending[:], dev.keep[:]

    try:
        for k, (op, want) in enumerate(ops(profile, seed, s)):
            what = f"{tag} op {k}: {describe(op)}"
            prev_n = count(c, op, s.info, want, prev_n)
            if op["kind"] in ("grow", "grow_records", "rotate", "rotate_records"):
                placement(s, op, offs_before, top_before, what)
            offs_before, top_before = list(s.offs), s.arena[0]
            if dev is not None:
                pending.append((k, op, dev.call(op, want), want))
                if len(pending) >= sync_every:
                    sync(what)
            try:
                ledger.update(op, want)
            except AssertionError as e:
                raise AssertionError(f"{what}: the ledger: {e}") from e
            if (k + 1) % every == 0:
                if dev is not None:
                    if pending:
                        sync(what)
                    dev.checkpoint(s, ledger, what)
                checkpoint(s, ledger, what)
        if dev is not None:
            if pending:
                sync(what)
            dev.checkpoint(s, ledger, what + " (the end)")
        checkpoint(s, ledger, what + " (the end)")
    finally:
        if dev is not None:
            dev.close()
    missed = floors(c, profile)
    assert not missed, (tag, "coverage floors not met", missed, dict(c))
    return s, ledger, c


def placement(s, op, offs_before, top_before, what):
    """What grow and rotate promise about where they put an image, checked
    without their models: the slot starts at a multiple of align inside what
    was the arena's free part, and no two chunks -- finished or live -- share
    a byte."""
    moved = [i for i in range(s.n) if s.offs[i] != offs_before[i]]
    for i in moved:
        assert s.offs[i] % op["align"] == 0, (what, "image", i, "at", s.offs[i], "align", op["align"])
        assert top_before <= s.offs[i] and s.offs[i] + s.caps[i] <= s.arena[0] <= s.arena[1], \
            (what, "image", i, "arena")
    if moved:
        offs, caps = s.chunks()
        spans = sorted((o, o + c, k) for k, (o, c) in enumerate(zip(offs, caps))
                       if k < s.count[0] or k - s.count[0] not in s.bad)
        for (_, e0, k0), (o1, _, k1) in zip(spans, spans[1:]):
            assert e0 <= o1, (what, "chunks overlap", k0, k1)


def checkpoint(s, ledger, what):
    """Finished chunks in list order, then the open images: content and metadata equal the ledger's."""
    cnt = s.count[0]
    assert cnt == len(ledger.done), (what, "finished chunks", cnt, len(ledger.done))
    compare_ledger(s.contents(rmodel.CONTENT), ledger.expected(rmodel.CONTENT), cnt, what + " (content)")
    compare_ledger(s.contents(rmodel.META), ledger.expected(rmodel.META), cnt, what + " (metadata)")


def sealed_chunks(s, ledger):
    """After the walk's last op every chunk is sealed: (name, the image's used
    bytes, the ledger's metadata, the ledger's content) of list + live."""
    offs, caps = s.chunks()
    want = ledger.expected(rmodel.CONTENT)
    metas = ledger.expected(rmodel.META)
    out = []
    for k, (off, cap) in enumerate(zip(offs, caps)):
        if want[k] is None:
            continue
        m, c = image_check(s.buf, len(s.buf), off, cap)
        out.append((f"c{k:05d}", s.buf[off:off + 24 + m + c].tobytes(), metas[k], want[k]))
    return out


def crc_field_ok(image):
    """Bytes 2..9 of a sealed image against zlib over [22, 24 + meta + content)."""
    return image[2:10] == struct.pack(">I", zlib.crc32(image[22:])) + b"\0" * 4
