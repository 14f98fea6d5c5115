"""Replace-metadata and write_at on chunk images in device memory
(include/chunkio_amd/cio_write_dev_move.h): the reference-written fixtures that
need them, byte for byte; the in-place move over every shift, length class and
alignment against a numpy model that does the reference's memmove / memcpy;
this repo's host chunk layer; rejections, checksums off, graph replay.  Every
comparison is of the WHOLE device buffer, guard bytes included, and crc_cur."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

from write_dev_move_model import (EMPTY_RAW, M32, m_geometry, m_init, m_meta_write, m_region_crc, m_seal, m_write,
                                  m_write_at, pattern, raw_update)

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "chunks", "manifest.json")) as _f:
    MANIFEST = json.load(_f)

FILL = 0xA5
CK = cf.CIO_CHECKSUM


# ------------------------------------------------------------------ helpers

def dev_i64(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(cuda)


def dev_u8(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(cuda)


def dev_u32(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(cuda)


def u32(t):
    return t.cpu().numpy().view(np.uint32).copy()


def pack_records(records, rng, slack=64):
    """One source buffer of random filler holding the records in order, record
    i at an offset that is (7 i + 3) modulo 16.  (buffer, offs, lens)."""
    offs, pos = [], 3
    for i, r in enumerate(records):
        pos += ((7 * i + 3) - pos) % 16
        offs.append(pos)
        pos += len(r) + int(rng.integers(0, 9))
    buf = rng.integers(0, 256, pos + slack, dtype=np.uint8)
    for o, r in zip(offs, records):
        buf[o:o + len(r)] = np.frombuffer(bytes(r), np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray([len(r) for r in records], np.uint64)


def place(buf, off, meta, content, raw=None):
    """An image as init + writes would have left it, written straight into the
    model: header, metadata, content; the raw CRC state of its region."""
    m_init(buf, off, meta)
    buf[off + 10:off + 14] = np.frombuffer(struct.pack(">I", len(content)), np.uint8)
    pos = off + 24 + len(meta)
    buf[pos:pos + len(content)] = np.frombuffer(content, np.uint8) if isinstance(content, bytes) else content
    raw = m_region_crc(buf, off) if raw is None else raw
    buf[off + 2:off + 10] = np.frombuffer(struct.pack("<Q", raw), np.uint8)
    return raw


class Images:
    """n images in one device buffer with its numpy model side by side."""

    def __init__(self, cuda, offs, caps, total, fill=FILL):
        self.cuda, self.n = cuda, len(offs)
        self.offs, self.caps = np.asarray(offs, np.uint64), np.asarray(caps, np.uint64)
        self.model = np.full(total, fill, np.uint8)
        self.base = None
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.raw = [0] * self.n               # the model's crc_cur
        self.crc_cur = None
        self.rng = np.random.default_rng(17)

    def upload(self):
        """The model as it stands becomes the device buffer and crc_cur."""
        self.base = dev_u8(self.model, self.cuda)
        self.crc_cur = dev_u32(np.asarray(self.raw, np.uint32), self.cuda)

    def init(self, w):
        if self.base is None:
            self.base = dev_u8(self.model, self.cuda)
        st, self.crc_cur = cf.init_batch_dev(w, self.base, self.offs_t, self.caps_t, flags=CK)
        for i in range(self.n):
            self.raw[i] = m_init(self.model, int(self.offs[i]))
        return st.cpu().numpy()

    def write(self, w, records, flags=CK):
        src, so, sl = pack_records(records, self.rng)
        st = cf.write_batch_dev(w, self.base, self.offs_t, self.caps_t, dev_u8(src, self.cuda),
                                dev_i64(so, self.cuda), dev_i64(sl, self.cuda), self.crc_cur, flags=flags)
        for i in range(self.n):
            self.raw[i] = m_write(self.model, int(self.offs[i]), records[i], self.raw[i], bool(flags & CK))
        return st.cpu().numpy()

    def meta_write(self, w, metas, flags=CK, skip=()):
        """skip: entries the device is expected to refuse (the model leaves them alone)."""
        src, so, sl = pack_records(metas, self.rng)
        st = cf.write_metadata_batch_dev(w, self.base, self.offs_t, self.caps_t, dev_u8(src, self.cuda),
                                         dev_i64(so, self.cuda), dev_i64(sl, self.cuda), self.crc_cur, flags=flags)
        for i in range(self.n):
            if i not in skip:
                self.raw[i] = m_meta_write(self.model, int(self.offs[i]), metas[i], self.raw[i], bool(flags & CK))
        return st.cpu().numpy()

    def write_at(self, w, ats, records, flags=CK, skip=()):
        src, so, sl = pack_records(records, self.rng)
        st = cf.write_at_batch_dev(w, self.base, self.offs_t, self.caps_t, dev_i64(ats, self.cuda),
                                   dev_u8(src, self.cuda), dev_i64(so, self.cuda), dev_i64(sl, self.cuda),
                                   self.crc_cur, flags=flags)
        for i in range(self.n):
            if i not in skip:
                self.raw[i] = m_write_at(self.model, int(self.offs[i]), int(ats[i]), records[i], self.raw[i],
                                         bool(flags & CK))
        return st.cpu().numpy()

    def seal(self, w, flags=CK):
        st = cf.seal_batch_dev(w, self.base, self.offs_t, self.caps_t, self.crc_cur, flags=flags)
        if flags & CK:
            for i in range(self.n):
                if flags & cf.CIOA_SEAL_RECOMPUTE:
                    self.raw[i] = m_region_crc(self.model, int(self.offs[i]))
                m_seal(self.model, int(self.offs[i]), self.raw[i])
        return st.cpu().numpy()

    def current_meta(self, i):
        o = int(self.offs[i])
        return self.model[o + 24:o + 24 + m_geometry(self.model, o)[0]].tobytes()

    def device(self):
        return self.base.cpu().numpy()

    def check(self, what=""):
        """The WHOLE device buffer (data, headers, every guard byte) and crc_cur."""
        got = self.device()
        if not np.array_equal(got, self.model):
            bad = np.flatnonzero(got != self.model)
            owner = int(np.searchsorted(self.offs, bad[0], side="right")) - 1
            raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0]} (image {owner} at "
                                 f"{int(self.offs[owner])}, +{bad[0] - int(self.offs[owner])}): "
                                 f"{got[bad[0]]:#x} for {self.model[bad[0]]:#x}")
        np.testing.assert_array_equal(u32(self.crc_cur), np.asarray(self.raw, np.uint32), err_msg=what)


# ------------------------------------------------------------------ 1. fixtures

def build_fixtures(cuda, names):
    """The named fixtures built on the device in zeroed images of the files'
    sizes, in ONE batch: every op of the manifest in order, each device call
    serving the images whose next op is of its kind while the others idle (a
    zero-length record; a rewrite of the metadata they already have)."""
    specs = [s for s in MANIFEST["chunks"] if s["name"] in names]
    assert [s["name"] for s in specs] == list(names)
    n = len(specs)
    sizes = [s["size"] for s in specs]
    offs, pos = [], 0
    for i, size in enumerate(sizes):
        pos = ((pos + 4095) & ~4095) + 7 * i + 1
        offs.append(pos)
        pos += size
    im = Images(cuda, offs, sizes, pos + 100, fill=0)
    todo = [[o for o in s["ops"] if o["op"] not in ("sync", "close")] for s in specs]
    kinds = []
    with cio.DevWriter(n, move=True) as w:
        assert not im.init(w).any()
        while any(todo):
            kind = next(t[0]["op"] for t in todo if t)
            kinds.append(kind)
            ops = [t.pop(0) if t and t[0]["op"] == kind else None for t in todo]
            if kind == "write":
                st = im.write(w, [pattern(o["len"], o["seed"]) if o else b"" for o in ops])
            elif kind == "write_at":
                st = im.write_at(w, [o["offset"] if o else 0 for o in ops],
                                 [pattern(o["len"], o["seed"]) if o else b"" for o in ops])
            else:
                assert kind == "meta_write"
                st = im.meta_write(w, [o["meta"].encode() if o else im.current_meta(i) for i, o in enumerate(ops)])
            assert not st.any(), kind
            im.check(kind)
        assert not im.seal(w).any()
    got = im.device()
    for i, s in enumerate(specs):
        img = got[offs[i]:offs[i] + sizes[i]].tobytes()
        assert hashlib.sha256(img).hexdigest() == s["sha256"], s["name"]
        assert int(u32(im.crc_cur)[i]) == s["load"]["crc_cur"], s["name"]
    with cio.Crc32DevPlan(n) as plan:
        st, er, cr, ml, cl = cf.verify_batch_dev(plan, im.base, im.offs_t, im.caps_t, flags=CK)
        for i, s in enumerate(specs):
            ld = s["load"]
            assert ld["ok"] and int(st[i]) == cf.CIO_OK and int(er[i]) == ld["last_chunk_error"], s["name"]
            assert int(u32(cr)[i]) == ld["crc_cur"], s["name"]
            assert (int(ml[i]), int(cl[i])) == (ld["meta_size"], ld["content_size"]), s["name"]
    im.check("fixtures")                      # and nothing outside the images
    return kinds


def test_write_at_and_meta_after_content_fixtures_byte_for_byte(cuda):
    """c04_write_at and c05_meta_after_content: the reference's bytes (its
    stale bytes past a shrunk content included), its loader's crc_cur, sizes
    and verdict."""
    kinds = build_fixtures(cuda, ["c04_write_at", "c05_meta_after_content"])
    assert "write_at" in kinds and kinds.count("meta_write") == 2


def test_all_buildable_fixtures_in_one_batch(cuda):
    """All six fixtures that need no damage step in one batch: mixed batches
    keep their indexing."""
    build_fixtures(cuda, ["c01_empty", "c02_content", "c03_meta_content", "c04_write_at", "c05_meta_after_content",
                          "c06_close_no_sync"])


# ------------------------------------------------------------------ 2., 3. the shift sweeps

def shift_case(d):
    """(old, new) metadata lengths giving the shift d with the least metadata."""
    return (0, d) if d > 0 else (-d, 0)


def run_shift_batch(cuda, w, cases, seed):
    """cases: (content length, old, new).  Images laid out with guard bytes so
    that the destination 24 + new of image i is (5 i + 1) modulo 16; every
    second image fits its capacity exactly.  One write_metadata call; returns
    the Images after the whole-buffer check."""
    rng = np.random.default_rng(seed)
    offs, caps, pos = [], [], 2
    for i, (length, old, new) in enumerate(cases):
        pos += int(rng.integers(1, 30))
        pos += ((5 * i + 1) - (pos + 24 + new)) % 16
        offs.append(pos)
        caps.append(24 + max(old, new) + length + (i % 2) * int(rng.integers(1, 40)))
        pos += caps[-1]
    im = Images(cuda, offs, caps, pos + 61)
    im.model[:] = rng.integers(0, 256, im.model.size, dtype=np.uint8)    # stale bytes are not all alike
    for i, (length, old, new) in enumerate(cases):
        content = rng.integers(0, 256, length, dtype=np.uint8)
        place(im.model, offs[i], rng.integers(0, 256, old, dtype=np.uint8).tobytes(), content, raw=0x1000 + i)
        im.raw[i] = 0x1000 + i                # stale on purpose: the call recomputes it
    im.upload()
    metas = [rng.integers(0, 256, new, dtype=np.uint8).tobytes() for _, _, new in cases]
    st = im.meta_write(w, metas)
    assert not st.any()
    im.check("shift batch")
    return im


SWEEP_LENGTHS = [0, 1, 3, 4, 15, 16, 17, 4095, 4096, 4097, 65534, 65535, 65536, 131077, (1 << 20) + 5]
SWEEP_SHIFTS = [1, 15, 16, 17, 127, 4095, 4096, 4097, 65535]


def test_shift_sweep_short_pieces(cuda):
    """Every length of SWEEP_LENGTHS with every shift of +-SWEEP_SHIFTS, an
    unchanged length (d = 0, other bytes) and a removal (m = 0), in one batch of
    about 30 MB of content: fewer than 16 steps per segment, so most pieces are
    shorter than the larger shifts and a piece's source is overwritten by
    several other workgroups.  Shifts of +-2..14 on one length complete the 16
    relative misalignments of load and store; the image offsets give all 16
    destination misalignments."""
    cases = []
    for length in SWEEP_LENGTHS:
        for d in SWEEP_SHIFTS:
            cases += [(length,) + shift_case(d), (length,) + shift_case(-d)]
        cases += [(length, 9, 9), (length, 33, 0)]
    for d in range(2, 15):
        cases += [(4097, 3, 3 + d), (4097, 20, 20 - d)]
    order = np.random.default_rng(8).permutation(len(cases))
    cases = [cases[j] for j in order]
    with cio.DevWriter(len(cases), move=True) as w:
        steps = sum((length + 4095) // 4096 for length, _, _ in cases)
        assert w.move_segments > 0 and steps < 16 * w.move_segments
        im = run_shift_batch(cuda, w, cases, seed=2)
    assert {(int(o) + 24 + new) % 16 for o, (_, _, new) in zip(im.offs, cases)} == set(range(16))
    assert {(new - old) % 16 for _, old, new in cases} == set(range(16))


def test_shift_sweep_long_pieces(cuda):
    """A batch sized from move_segments so that every segment holds at least 2
    x 65535 bytes: six images of tens of MB, one for each of d = +-65535,
    +-4097, +-1, among 2048 images of 4 KiB that cycle through the same
    shifts.  Pieces are longer than any shift: the saved part is a fraction of
    a piece and the walk inside a segment does the rest."""
    shifts = [65535, -65535, 4097, -4097, 1, -1]
    with cio.DevWriter(4096, move=True) as w:
        G = w.move_segments
        big = -(-(G * 2 * 65536) // len(shifts)) + 4099
        assert 100e6 < big * len(shifts) < 200e6, "the batch is sized for a grid of about 1024 segments"
        cases = [(4096,) + shift_case(shifts[i % 6]) for i in range(2048)]
        for k, d in enumerate(shifts):
            cases.insert(300 * k + 11, (big + k,) + shift_case(d))
        run_shift_batch(cuda, w, cases, seed=3)


# ------------------------------------------------------------------ 4. multiple updates, the host chunk layer

def test_multiple_updates_against_the_host_chunk_layer(cuda, tmp_path):
    """The reference's metadata_multiple_updates (tests/metadata_update.c:
    187-277: content, then small -> medium -> long -> tiny -> medium) and
    metadata_unsigned_underflow (tests/fs.c:942-1103: small, content, large),
    with content appended between the updates and a write_at in the middle, on
    12 images whose strings and contents are scaled differently; cf.Context
    does the same calls on files.  After seal / sync the images equal the
    files byte for byte, stale bytes past the content included."""
    strs = [b"small", b"medium-sized-metadata", b"very-long-metadata-string-that-exceeds-previous-sizes", b"tiny",
            b"another-medium-metadata-string"]
    n = 12
    scale = [1, 1, 2, 7, 40, 300, 1200, 1, 3, 90, 650, 1100]      # 1200 x 53 = 63600 bytes of metadata
    clen = [36, 0, 1, 5000, 70000, 3, 300000, 4096, 17, 65536, 15, 150000]
    rng = np.random.default_rng(44)
    contents = [rng.integers(0, 256, c, dtype=np.uint8).tobytes() for c in clen]
    extra = [rng.integers(0, 256, 10 + 37 * i, dtype=np.uint8).tobytes() for i in range(n)]
    caps = [24 + 53 * scale[i] + clen[i] + 3 * len(extra[i]) + (i % 3) * 50 for i in range(n)]
    offs, pos = [], 5
    for i in range(n):
        offs.append(pos)
        pos += caps[i] + 3 + i
    im = Images(cuda, offs, caps, pos + 40, fill=0)
    with cf.Context(str(tmp_path / "root"), CK, max_chunks_up=n + 4) as ctx, cio.DevWriter(n, move=True) as w:
        stream = ctx.stream("s")
        chunks = []
        for i in range(n):
            c, err = stream.open(f"c{i:02d}", cf.CIO_OPEN, 0)
            assert c is not None, err
            chunks.append(c)

        def both_meta(k):
            metas = [strs[k] * scale[i] for i in range(n)]
            for c, m in zip(chunks, metas):
                assert c.meta_write(m) == 0
            assert not im.meta_write(w, metas).any()

        def both_write(records):
            for c, r in zip(chunks, records):
                if r:
                    assert c.write(r) == 0
            assert not im.write(w, records).any()

        def compare(what):
            np.testing.assert_array_equal(u32(im.crc_cur), [c.crc_cur for c in chunks], err_msg=what)
            im.check(what)

        assert not im.init(w).any()
        both_meta(0)                          # metadata on an empty chunk
        both_write(contents)
        compare("content")
        for k in (1, 2):
            both_meta(k)
            compare(f"update {k}")
        both_write(extra)
        both_meta(3)                          # long -> tiny: the content moves down
        compare("update 3")
        ats = [len(contents[i]) // 2 for i in range(n)]
        for c, a, r in zip(chunks, ats, extra):
            assert c.write_at(r[::-1], a) == 0
        assert not im.write_at(w, ats, [r[::-1] for r in extra]).any()
        compare("write_at")
        both_meta(4)
        both_write(extra)
        compare("update 4")
        for c in chunks:
            assert c.sync() == 0
        assert not im.seal(w).any()
        got = im.device()
        for i, c in enumerate(chunks):
            end = 24 + len(strs[4]) * scale[i] + ats[i] + 2 * len(extra[i])
            assert c.data_size == end - 24 - c.meta_len() and c.meta_len() == len(strs[4]) * scale[i], i
            k = min(caps[i], len(c.map))
            assert k >= end
            assert got[offs[i]:offs[i] + k].tobytes() == bytes(c.map[:k]), i
    im.check("host layer")


# ------------------------------------------------------------------ 5. rejections

def test_rejected_metadata_entries_change_nothing(cuda):
    """One bad entry of each kind among good ones: status CIO_ERROR, no byte of
    the image and not its crc_cur changes, the neighbours are replaced."""
    rng = np.random.default_rng(5)
    n, cap = 16, 70000
    bad = {1: "bad magic", 3: "cap < 24", 5: "m = 65536", 7: "24 + m + content = cap + 1",
           9: "metadata source out of range", 11: "image outside dev_bytes", 13: "metadata source offset wraps",
           14: "forged content length"}
    caps = [cap] * n
    caps[3] = 23
    offs, pos = [0] * n, 31
    for i in [i for i in range(n) if i != 11] + [11]:         # image 11 lies last ...
        offs[i] = pos + i % 5
        pos = offs[i] + cap + 19
    total = offs[11] + cap - 1                # ... and ends one byte past the buffer
    im = Images(cuda, offs, caps, total)
    old = [rng.integers(0, 256, 10 + i, dtype=np.uint8).tobytes() for i in range(n)]
    clen = [1000 + 100 * i for i in range(n)]
    clen[7] = cap - 24 - 500                  # the new metadata of 501 bytes is one too many
    clen[8] = cap - 24 - 500                  # ... and 500 fit exactly
    for i in range(n):
        if i not in (3, 11):
            im.raw[i] = place(im.model, offs[i], old[i], rng.integers(0, 256, clen[i], dtype=np.uint8))
        else:
            im.raw[i] = 0x12345678
    im.model[offs[1]] = 0xC0
    im.model[offs[14] + 10:offs[14] + 14] = np.frombuffer(struct.pack(">I", 0xFFFFFFF0), np.uint8)
    im.upload()
    lens = np.asarray([40 + 3 * i for i in range(n)], np.uint64)
    lens[0] = 0                               # removal
    lens[2] = len(old[2])                     # same length, other bytes
    lens[5] = 65536
    lens[6] = 65535
    lens[7] = 501
    lens[8] = 500
    src = rng.integers(0, 256, 70000, dtype=np.uint8)
    so = np.asarray([97 * i for i in range(n)], np.uint64)
    so[9] = 70000 - int(lens[9]) + 1          # ends one byte past the source
    so[13] = 2 ** 64 - 8
    with cio.DevWriter(n, move=True) as w:
        st = cf.write_metadata_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_u8(src, cuda), dev_i64(so, cuda),
                                         dev_i64(lens, cuda), im.crc_cur, flags=CK).cpu().numpy()
        for i in range(n):
            if i in bad:
                assert st[i] == cf.CIO_ERROR, bad[i]
            else:
                assert st[i] == cf.CIO_OK, i
                meta = src[int(so[i]):int(so[i]) + int(lens[i])].tobytes()
                im.raw[i] = m_meta_write(im.model, offs[i], meta, im.raw[i])
        im.check("bad batch")
        assert m_geometry(im.model, offs[8]) == (500, cap - 524) and m_geometry(im.model, offs[6])[0] == 65535


def test_rejected_write_at_entries_change_nothing(cuda):
    rng = np.random.default_rng(6)
    n, cap = 10, 5000
    bad = {1: "at = content + 1", 3: "at + count one past the capacity", 5: "source out of range", 7: "bad magic"}
    offs = [13 + i * (cap + 11) + i % 3 for i in range(n)]
    im = Images(cuda, offs, [cap] * n, offs[-1] + cap + 30)
    metas = [b"m" * (i % 4) for i in range(n)]
    clen = [1000] * n
    for i in range(n):
        im.raw[i] = place(im.model, offs[i], metas[i], rng.integers(0, 256, clen[i], dtype=np.uint8))
    im.model[offs[7] + 1] = 0x01
    im.upload()
    ats = np.asarray([500] * n, np.uint64)
    lens = np.asarray([50] * n, np.uint64)
    ats[0] = 1000                             # at = content: a plain append
    ats[1] = 1001
    ats[2], lens[2] = 100, cap - 24 - len(metas[2]) - 100        # fits exactly
    ats[3], lens[3] = 100, cap - 24 - len(metas[3]) - 100 + 1
    ats[4] = 0                                # everything replaced
    ats[6], lens[6] = 2000, 0                 # no record: a no-op, even with at past the content
    src = rng.integers(0, 256, 8192, dtype=np.uint8)
    so = np.asarray([300 * i + i for i in range(n)], np.uint64)
    so[5] = 8192 - 49
    with cio.DevWriter(n) as w:               # no move arena needed
        assert w.move_segments == 0
        before0, raw0 = im.model.copy(), im.raw[0]
        st = cf.write_at_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_i64(ats, cuda), dev_u8(src, cuda),
                                   dev_i64(so, cuda), dev_i64(lens, cuda), im.crc_cur, flags=CK).cpu().numpy()
        for i in range(n):
            if i in bad:
                assert st[i] == cf.CIO_ERROR, bad[i]
            else:
                assert st[i] == cf.CIO_OK, i
                rec = src[int(so[i]):int(so[i]) + int(lens[i])].tobytes()
                im.raw[i] = m_write_at(im.model, offs[i], int(ats[i]), rec, im.raw[i])
        im.check("bad batch")
        # at = content equals the plain append
        rec = src[int(so[0]):int(so[0]) + 50].tobytes()
        assert im.raw[0] == m_write(before0, offs[0], rec, raw0)
        assert np.array_equal(before0[offs[0]:offs[0] + cap], im.model[offs[0]:offs[0] + cap])
        assert m_geometry(im.model, offs[6])[1] == 1000 and m_geometry(im.model, offs[4])[1] == 50


# ------------------------------------------------------------------ 6. checksums off

def test_checksums_off(cuda):
    """Without CIO_CHECKSUM neither call launches a CRC: bytes 2..9 and crc_cur
    stay as they were; a recomputing seal afterwards gives the model's CRC."""
    rng = np.random.default_rng(7)
    n = 24
    clen = [int(x) for x in rng.integers(0, 40000, n)]
    clen[0], clen[1] = 0, 2
    old = [bytes(rng.integers(0, 256, (11 * i) % 200, dtype=np.uint8)) for i in range(n)]
    new = [bytes(rng.integers(0, 256, (37 * i + 5) % 300, dtype=np.uint8)) for i in range(n)]
    offs, caps, pos = [], [], 9
    for i in range(n):
        offs.append(pos)
        caps.append(24 + 300 + clen[i] + 200)
        pos += caps[-1] + i % 7
    im = Images(cuda, offs, caps, pos + 20)
    mark = np.frombuffer(b"\x01\x02\x03\x04\x05\x06\x07\x08", np.uint8)
    for i in range(n):
        place(im.model, offs[i], old[i], rng.integers(0, 256, clen[i], dtype=np.uint8))
        im.model[offs[i] + 2:offs[i] + 10] = mark
        im.raw[i] = 1000 + i
    im.upload()
    with cio.DevWriter(n, move=True) as w:
        assert not im.meta_write(w, new, flags=0).any()
        im.check("write_metadata without checksums")
        ats = [c // 3 for c in clen]
        recs = [rng.integers(0, 256, 150, dtype=np.uint8).tobytes() for _ in range(n)]
        assert not im.write_at(w, ats, recs, flags=0).any()
        im.check("write_at without checksums")
        assert all(m_geometry(im.model, o) == (len(m), a + 150) for o, m, a in zip(offs, new, ats))
        assert not im.seal(w, flags=CK | cf.CIOA_SEAL_RECOMPUTE).any()
        im.check("recomputing seal")


# ------------------------------------------------------------------ 7. graph replay

def test_graph_replay_is_idempotent(cuda):
    """One captured write_metadata and one captured write_at (each a single
    linear stream), each replayed twice: the lengths are read on the device at
    run time, so the second write_metadata finds d = 0 and the second write_at
    cuts at the same place -- two replays equal one application."""
    import torch
    rng = np.random.default_rng(9)
    n = 36
    clen = [int(x) for x in rng.integers(0, 60000, n)]
    clen[0], clen[1], clen[2] = 0, 3, 131077
    old = [bytes(rng.integers(0, 256, (29 * i) % 400, dtype=np.uint8)) for i in range(n)]
    new = [bytes(rng.integers(0, 256, (53 * i + 1) % 700, dtype=np.uint8)) for i in range(n)]
    new[2] = bytes(rng.integers(0, 256, 65535, dtype=np.uint8))
    offs, caps, pos = [], [], 4
    for i in range(n):
        offs.append(pos)
        caps.append(24 + max(len(old[i]), len(new[i])) + clen[i] + 400)
        pos += caps[-1] + i % 9
    im = Images(cuda, offs, caps, pos + 20)
    for i in range(n):
        im.raw[i] = place(im.model, offs[i], old[i], rng.integers(0, 256, clen[i], dtype=np.uint8))
    im.upload()
    msrc, mo, ml = pack_records(new, rng)
    recs = [rng.integers(0, 256, 100 + i, dtype=np.uint8).tobytes() for i in range(n)]
    rsrc, ro, rl = pack_records(recs, rng)
    ats = [c // 2 for c in clen]
    msrc_t, mo_t, ml_t = dev_u8(msrc, cuda), dev_i64(mo, cuda), dev_i64(ml, cuda)
    rsrc_t, ro_t, rl_t, at_t = dev_u8(rsrc, cuda), dev_i64(ro, cuda), dev_i64(rl, cuda), dev_i64(ats, cuda)
    status = torch.full((n,), 99, dtype=torch.int32, device=cuda)

    def call_meta():
        cf.write_metadata_batch_dev(w, im.base, im.offs_t, im.caps_t, msrc_t, mo_t, ml_t, im.crc_cur, flags=CK,
                                    status=status)

    def call_at():
        cf.write_at_batch_dev(w, im.base, im.offs_t, im.caps_t, at_t, rsrc_t, ro_t, rl_t, im.crc_cur, flags=CK,
                              status=status)

    with cio.DevWriter(n, move=True) as w:
        # warm-up outside the capture, on a scratch copy of the buffer
        keep, keep_crc = im.base.clone(), im.crc_cur.clone()
        call_meta()
        call_at()
        torch.cuda.synchronize()
        im.base.copy_(keep)
        im.crc_cur.copy_(keep_crc)
        for name, call in (("write_metadata", call_meta), ("write_at", call_at)):
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                call()
            im.check(f"capturing {name} runs nothing")
            for i in range(n):
                if name == "write_metadata":
                    im.raw[i] = m_meta_write(im.model, offs[i], new[i], im.raw[i])
                else:
                    im.raw[i] = m_write_at(im.model, offs[i], ats[i], recs[i], im.raw[i])
            for k in (1, 2):
                status.fill_(99)
                graph.replay()
                torch.cuda.synchronize()
                assert not status.cpu().numpy().any()
                im.check(f"{name}, replay {k}")
            del graph
        assert not im.seal(w).any()
        im.check("seal")
    with cio.Crc32DevPlan(n) as plan:
        st = cf.verify_batch_dev(plan, im.base, im.offs_t, im.caps_t, flags=CK)[0]
        assert not st.cpu().numpy().any()


# ------------------------------------------------------------------ 8. the move writer

def test_write_metadata_needs_a_move_writer(cuda):
    rng = np.random.default_rng(10)
    im = Images(cuda, [7], [500], 600)
    im.raw[0] = place(im.model, 7, b"old", rng.integers(0, 256, 100, dtype=np.uint8))
    assert im.raw[0] != EMPTY_RAW and im.raw[0] == raw_update(M32, im.model[7 + 22:7 + 24 + 3 + 100].tobytes())
    im.upload()
    with cio.DevWriter(1) as w:
        assert w.move_segments == 0
        with pytest.raises(cio.CioGpuError, match="created without CIOA_WRITER_MOVE"):
            im.meta_write(w, [b"a longer one"])
        im.check("refused call")
    with cio.DevWriter(1, move=True) as w:
        assert w.move_segments > 0
        assert not im.meta_write(w, [b"a longer one"]).any()
        im.check("move writer")
