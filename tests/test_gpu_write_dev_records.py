"""The grouped append to chunk images in device memory
(include/chunkio_amd/cio_write_dev_records.h): many records per image in one
call.  Every case compares with the Python model (write_dev_records_model.py):
the WHOLE image buffer including a sentinel pattern in the slack between and
after the images, crc_cur, both status arrays, and the untouched source."""
import hashlib
import json
import os
import struct

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import write_dev_records_model as model
from write_dev_move_model import INIT
from write_dev_records_model import m_init, m_seal, pattern

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


class Images:
    """Images in one device buffer with the model's copy side by side; the
    slack between and after them holds a position-dependent sentinel."""

    def __init__(self, cuda, rooms, metas=None, gap=37, fill=None):
        self.cuda, self.n = cuda, len(rooms)
        metas = metas or [b""] * self.n
        offs, caps, pos = [], [], 13
        for i, room in enumerate(rooms):
            offs.append(pos)
            caps.append(24 + len(metas[i]) + room)
            pos += caps[-1] + gap + i % 5
        total = pos + 50
        self.offs, self.caps = np.asarray(offs, np.uint64), np.asarray(caps, np.uint64)
        if fill is None:
            self.model = ((np.arange(total, dtype=np.uint64) * 7 + 3) % 251).astype(np.uint8)
        else:
            self.model = np.full(total, fill, np.uint8)
        self.raw = [m_init(self.model, offs[i], metas[i]) for i in range(self.n)]
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.upload()

    def upload(self):
        """The model as it stands becomes the device buffer and crc_cur."""
        self.base = dev_u8(self.model, self.cuda)
        self.crc_cur = dev_u32(np.asarray(self.raw, np.uint32), self.cuda)

    def check(self, what=""):
        got = self.base.cpu().numpy()
        if not np.array_equal(got, self.model):
            bad = np.flatnonzero(got != self.model)
            owner = int(np.searchsorted(self.offs, bad[0], side="right")) - 1
            raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0]} (image {owner} at "
                                 f"{int(self.offs[owner])}, +{bad[0] - int(self.offs[owner])}): "
                                 f"{got[bad[0]]:#x} for {self.model[bad[0]]:#x}")
        np.testing.assert_array_equal(u32(self.crc_cur), np.asarray(self.raw, np.uint32), err_msg=what)

    def append(self, w, src, rec_img, rec_offs, rec_lens, flags=CK, what=""):
        """One grouped call on the device and in the model; everything
        compared.  Returns the model's (img_status, rec_status)."""
        src = np.ascontiguousarray(src, dtype=np.uint8)
        src_t = dev_u8(src, self.cuda)
        ist, rst = cf.write_records_batch_dev(w, self.base, self.offs_t, self.caps_t, src_t,
                                              dev_u32(rec_img, self.cuda), dev_i64(rec_offs, self.cuda),
                                              dev_i64(rec_lens, self.cuda), self.crc_cur, flags=flags)
        mi, mr = model.m_write_records(self.model, self.offs.tolist(), self.caps.tolist(), src, rec_img, rec_offs,
                                       rec_lens, self.raw, checksum=bool(flags & CK))
        np.testing.assert_array_equal(ist.cpu().numpy(), mi, err_msg=what + ": img_status")
        np.testing.assert_array_equal(rst.cpu().numpy(), mr, err_msg=what + ": rec_status")
        self.check(what)
        assert np.array_equal(src_t.cpu().numpy(), src), what + ": the source changed"
        return mi, mr


def pack(lens, rng, gap=9):
    """A source buffer of random bytes holding records of the given lengths at
    random misalignment.  (buffer, offs)."""
    lens = np.asarray(lens, np.int64)
    gaps = rng.integers(0, gap, lens.size)
    offs = np.cumsum(lens + gaps) - lens + 1
    total = int(offs[-1] + lens[-1]) + 19 if lens.size else 19
    return rng.integers(0, 256, total, dtype=np.uint8), offs.astype(np.uint64)


def runs_to_img(runs):
    return np.repeat(np.arange(len(runs), dtype=np.uint32), runs)


# ------------------------------------------------------------------ 1. the reference's fixtures

def test_reference_fixtures_in_one_call(cuda):
    """c02, c03 and c06 in ONE call: three images, their writes as grouped
    records after an init_batch_dev with the 8-byte and the 1-byte metadata;
    then seal.  The bytes and crc_cur are the fixtures', and verify-on-load
    accepts all three."""
    names = ("c02_content", "c03_meta_content", "c06_close_no_sync")
    specs = [s for s in MANIFEST["chunks"] if s["name"] in names]
    assert [s["name"] for s in specs] == list(names)
    metas = [b"".join(o["meta"].encode() for o in s["ops"] if o["op"] == "meta_write") for s in specs]
    assert [len(m) for m in metas] == [0, 8, 1]
    im = Images(cuda, [s["size"] - 24 - len(m) for s, m in zip(specs, metas)], metas, fill=0)
    # the images start zeroed on the device: init_batch_dev writes what the model's m_init wrote
    dev = np.zeros_like(im.model)
    im.base = dev_u8(dev, cuda)
    recs, rec_img = [], []
    for i, s in enumerate(specs):
        for o in s["ops"]:
            if o["op"] == "write":
                recs.append(pattern(o["len"], o["seed"]))
                rec_img.append(i)
    rng = np.random.default_rng(1)
    src, offs = pack([len(r) for r in recs], rng)
    for o, r in zip(offs, recs):
        src[int(o):int(o) + len(r)] = np.frombuffer(r, np.uint8)
    msrc = np.frombuffer(b"?" + metas[1] + b"??" + metas[2], np.uint8).copy()
    with cio.DevWriter(8) as w:
        st, im.crc_cur = cf.init_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_u8(msrc, cuda),
                                           dev_i64([0, 1, 11], cuda), dev_i64([0, 8, 1], cuda), flags=CK)
        assert not st.cpu().numpy().any()
        im.check("init")
        mi, mr = im.append(w, src, rec_img, offs, [len(r) for r in recs], what="fixtures")
        assert not mi.any() and not mr.any() and len(mr) == 5
        st = cf.seal_batch_dev(w, im.base, im.offs_t, im.caps_t, im.crc_cur, flags=CK)
        assert not st.cpu().numpy().any()
    for i in range(3):
        m_seal(im.model, int(im.offs[i]), im.raw[i])
    im.check("seal")
    got = im.base.cpu().numpy()
    for i, s in enumerate(specs):
        o = int(im.offs[i])
        assert hashlib.sha256(got[o:o + s["size"]].tobytes()).hexdigest() == s["sha256"], s["name"]
        assert int(u32(im.crc_cur)[i]) == s["load"]["crc_cur"], s["name"]
    with cio.Crc32DevPlan(3) as plan:
        st, er, cr, ml, cl = cf.verify_batch_dev(plan, im.base, im.offs_t, im.caps_t, flags=CK)
        for i, s in enumerate(specs):
            assert int(st[i]) == cf.CIO_OK and int(u32(cr)[i]) == s["load"]["crc_cur"], s["name"]
            assert (int(ml[i]), int(cl[i])) == (s["load"]["meta_size"], s["load"]["content_size"]), s["name"]


# ------------------------------------------------------------------ 2. against the single-record path

def test_equals_the_rounds_of_write_batch_dev(cuda):
    """Equivalence rule 7.  9 images; the first, a middle one and the last have
    no run; one run of 1024 records ends where the next, of 2100, starts
    exactly at record 1024 and crosses two workgroup boundaries; records of
    0..40 bytes, a few of 4 KiB +- 1, one of 1 MiB; one run is cut by its
    capacity.  The same buffer through write_batch_dev, round k carrying the
    k-th record of every image and an image fed no further after its first
    CIO_ERROR, ends byte for byte the same."""
    import torch
    rng = np.random.default_rng(2)
    runs = [0, 1024, 2100, 6, 0, 40, 1, 30, 0]
    n_img, n_rec = len(runs), sum(runs)
    rec_img = runs_to_img(runs)
    lens = rng.integers(0, 41, n_rec)
    first = np.cumsum([0] + runs)
    lens[first[7] + np.asarray([2, 9, 17])] = [4095, 4096, 4097]
    lens[first[2] + 1030] = 4097
    lens[first[6]] = 1 << 20
    lens[first[3]:first[3] + 6] = [30, 0, 25, 40, 3, 0]       # the cut run: room for the first three
    rooms = [int(lens[first[i]:first[i + 1]].sum()) + 50 + 3 * i for i in range(n_img)]
    rooms[3] = 60                             # 30 + 0 + 25 fit, 40 does not; the 3 after it would
    src, offs = pack(lens, rng)
    metas = [b"m" * (i % 4) for i in range(n_img)]
    im = Images(cuda, rooms, metas)
    start = im.model.copy()
    seeds = list(im.raw)
    with cio.DevWriter(n_rec) as w:
        mi, mr = im.append(w, src, rec_img, offs, lens, what="grouped")
        assert not mi.any()
        assert mr[first[3]:first[4]].tolist() == [0, 0, 0, -1, -1, -1]
        assert not np.delete(mr, np.s_[first[3]:first[4]]).any()
        # the rounds on a copy of the buffer
        base2, crc2 = dev_u8(start, cuda), dev_u32(np.asarray(seeds, np.uint32), cuda)
        src_t = dev_u8(src, cuda)
        rounds = model.rounds(rec_img.tolist(), n_img)
        assert len(rounds) == 2100
        so, sl = np.zeros((len(rounds), n_img), np.uint64), np.zeros((len(rounds), n_img), np.uint64)
        for k, rd in enumerate(rounds):
            for i, r in rd.items():
                so[k, i], sl[k, i] = offs[r], lens[r]
        so_t, sl_t = dev_i64(so, cuda), dev_i64(sl, cuda)
        status = torch.zeros((len(rounds), n_img), dtype=torch.int32, device=cuda)
        stopped = set()
        for k in range(len(rounds)):
            if stopped:
                sl_t[k, sorted(stopped)] = 0
            cf.write_batch_dev(w, base2, im.offs_t, im.caps_t, src_t, so_t[k], sl_t[k], crc2, flags=CK,
                               status=status[k])
            if k < 8:                         # the short runs: the caller looks at every status
                stopped |= set(np.flatnonzero(status[k].cpu().numpy()).tolist())
        st = status.cpu().numpy()
        assert stopped == {3} and st[3, 3] == -1 and not np.delete(st, 3, axis=1).any()
    assert np.array_equal(base2.cpu().numpy(), im.model)
    np.testing.assert_array_equal(u32(crc2), np.asarray(im.raw, np.uint32))


# ------------------------------------------------------------------ 3., 4. the scan's edges

@pytest.mark.parametrize("n_rec", [1, 1023, 1024, 1025, 2049])
def test_record_counts_at_the_scans_edges(cuda, n_rec):
    rng = np.random.default_rng(n_rec)
    runs = [0, n_rec] if n_rec == 1 else [n_rec // 3, 0, n_rec - n_rec // 3 - 1, 1]
    lens = rng.integers(0, 21, n_rec)
    first = np.cumsum([0] + runs)
    rooms = [int(lens[first[i]:first[i + 1]].sum()) for i in range(len(runs))]
    rooms[0] = rooms[0] // 2                  # the first run is cut in its middle; the others fit exactly
    src, offs = pack(lens, rng)
    im = Images(cuda, rooms)
    with cio.DevWriter(max(n_rec, len(runs))) as w:
        mi, mr = im.append(w, src, runs_to_img(runs), offs, lens, what=f"n_rec = {n_rec}")
    assert not mi.any() and not mr[first[1]:].any()


def test_the_scan_workgroups_second_pass(cuda):
    """1024^2 + 1025 records of 0..8 bytes into 5 images: 1026 workgroup
    aggregates, so the scan workgroup makes a second pass; one run spans more
    than 1024 workgroups and is cut near its end."""
    n_rec = 1024 * 1024 + 1025
    rng = np.random.default_rng(4)
    runs = [10, 0, n_rec - 10 - 300 - 7, 300, 7]
    lens = rng.integers(0, 9, n_rec)
    first = np.cumsum([0] + runs)
    rooms = [int(lens[first[i]:first[i + 1]].sum()) + 5 for i in range(5)]
    rooms[2] -= 1000                          # cut inside workgroup 1024
    src, offs = pack(lens, rng, gap=3)
    im = Images(cuda, rooms)
    with cio.DevWriter(n_rec) as w:
        mi, mr = im.append(w, src, runs_to_img(runs), offs, lens, what="second pass")
    cut = int(np.argmax(mr[first[2]:first[3]] != 0))
    assert not mi.any() and first[2] + cut > 1024 * 1024 and mr[first[2] + cut:first[3]].all() and not mr[first[3]:].any()


# ------------------------------------------------------------------ 5. the cut

def test_the_cut(cuda):
    """Five runs of the same six records: cut at the first record, in the
    middle, at the last record; exactly at room (all fit); one byte past."""
    rng = np.random.default_rng(5)
    one = [17, 4, 0, 33, 9, 21]
    lens = np.asarray(one * 5)
    rooms = [16, 17 + 4 + 32, 70, sum(one), sum(one) - 1]
    src, offs = pack(lens, rng)
    im = Images(cuda, rooms, [b"", b"abc", b"", b"q", b""])
    with cio.DevWriter(64) as w:
        mi, mr = im.append(w, src, runs_to_img([6] * 5), offs, lens, what="cut")
    assert not mi.any()
    assert mr.reshape(5, 6).tolist() == [[-1] * 6, [0, 0, 0, -1, -1, -1], [0, 0, 0, 0, 0, -1], [0] * 6,
                                         [0, 0, 0, 0, 0, -1]]


# ------------------------------------------------------------------ 6. bad sources, the 32-bit bound

def test_bad_sources_mid_run(cuda):
    """A record whose source range leaves src_bytes, one whose range wraps, one
    longer than 2^32 - 1: each ends its run there; a zero-length record has no
    source range."""
    rng = np.random.default_rng(6)
    lens = rng.integers(1, 30, 24).astype(np.uint64)
    src, offs = pack(lens, rng)
    rooms = [int(lens[6 * i:6 * i + 6].sum()) + 4 for i in range(4)]
    offs[3] = src.size - 2                    # leaves src_bytes by one byte
    lens[3] = 3
    offs[6 + 2] = (1 << 64) - 4               # wraps
    lens[12 + 4] = 1 << 32                    # no content can hold it
    offs[18 + 1], lens[18 + 1] = (1 << 64) - 1, 0
    im = Images(cuda, rooms)
    with cio.DevWriter(64) as w:
        mi, mr = im.append(w, src, runs_to_img([6] * 4), offs, lens, what="bad sources")
    assert not mi.any()
    assert mr.reshape(4, 6).tolist() == [[0, 0, 0, -1, -1, -1], [0, 0, -1, -1, -1, -1], [0, 0, 0, 0, -1, -1],
                                         [0] * 6]


def test_content_plus_total_crossing_the_32_bit_bound(cuda):
    """An image whose header claims 2^32 - 11 bytes of content inside a
    capacity of 2^32 + 1000 has room for 10 bytes, not for the 987 its capacity
    would leave: the smallest allocation at which the 32-bit bound binds.  The
    buffer is compared on the device."""
    import torch
    content = (1 << 32) - 11
    cap = (1 << 32) + 1000
    base = torch.full((cap + 64,), FILL, dtype=torch.uint8, device=cuda)
    hdr = np.frombuffer(INIT, np.uint8).copy()
    hdr[10:14] = np.frombuffer(struct.pack(">I", content), np.uint8)
    base[:24] = dev_u8(hdr, cuda)
    want = base.clone()
    src = np.arange(1, 41, dtype=np.uint8)
    seed = 0x12345678
    crc = dev_u32([seed], cuda)
    with cio.DevWriter(16) as w:
        ist, rst = cf.write_records_batch_dev(w, base, dev_i64([0], cuda), dev_i64([cap], cuda), dev_u8(src, cuda),
                                              dev_u32([0, 0, 0, 0], cuda), dev_i64([0, 10, 20, 30], cuda),
                                              dev_i64([4, 6, 1, 0], cuda), crc, flags=CK)
        assert ist.cpu().tolist() == [0] and rst.cpu().tolist() == [0, 0, -1, -1]
    data = bytes(src[0:4]) + bytes(src[10:16])
    raw = model.raw_update(seed, data)
    pos = 24 + content
    want[pos:pos + 10] = dev_u8(np.frombuffer(data, np.uint8).copy(), cuda)
    want[2:10] = dev_u8(np.frombuffer(struct.pack("<Q", raw), np.uint8).copy(), cuda)
    want[10:14] = dev_u8(np.frombuffer(struct.pack(">I", content + 10), np.uint8).copy(), cuda)
    assert content + 10 == 0xFFFFFFFF and torch.equal(base, want) and int(u32(crc)[0]) == raw


# ------------------------------------------------------------------ 7. rejected runs

def test_rejected_images(cuda):
    """A bad-magic image, one that leaves the buffer and one whose header
    claims more than its capacity are untouched and their runs rejected, zero-
    length records included; later runs are unaffected; the same defects on
    images WITHOUT a run are not looked at."""
    rng = np.random.default_rng(7)
    runs = [3, 2, 0, 4, 3, 0, 2, 0, 5]
    n_rec = sum(runs)
    lens = rng.integers(0, 50, n_rec)
    lens[3] = 0                               # a zero-length record to the bad-magic image
    src, offs = pack(lens, rng)
    im = Images(cuda, [400] * 9)
    im.model[int(im.offs[1])] = 0xC2          # bad magic, with a run
    im.model[int(im.offs[2]) + 1] = 0x01      # bad magic, no run
    im.model[int(im.offs[4]) + 10] = 0x40     # content beyond the capacity, with a run
    im.model[int(im.offs[5]) + 10] = 0x40     # the same, no run
    im.upload()
    caps = im.caps.copy()
    caps[6] = im.model.size - int(im.offs[6]) + 1      # leaves the buffer by one byte, with a run
    caps[7] = 1 << 62                                  # far outside, no run
    im.caps, im.caps_t = caps, dev_i64(caps, cuda)
    with cio.DevWriter(32) as w:
        mi, mr = im.append(w, src, runs_to_img(runs), offs, lens, what="rejected images")
    assert mi.tolist() == [0, -1, 0, 0, -1, 0, -1, 0, 0]
    first = np.cumsum([0] + runs)
    assert [int(mr[first[i]:first[i + 1]].any()) for i in range(9)] == [0, 1, 0, 0, 1, 0, 1, 0, 0]


# ------------------------------------------------------------------ 8. malformed grouping

@pytest.mark.parametrize("case", ["descending pair at a workgroup boundary", "index == n_img"])
def test_malformed_grouping_rejects_the_batch(cuda, case):
    rng = np.random.default_rng(8)
    runs = [1023, 1, 500, 0, 30]
    rec_img = runs_to_img(runs)
    if case.startswith("descending"):
        rec_img[1023] = 3                     # record 1024, the next workgroup's first, is of image 2
        assert rec_img[1024] < rec_img[1023] and (np.diff(rec_img.astype(np.int64)) < 0).sum() == 1
    else:
        rec_img[-1] = len(runs)
    lens = rng.integers(0, 30, rec_img.size)
    src, offs = pack(lens, rng)
    im = Images(cuda, [40000] * len(runs))
    before = im.model.copy()
    with cio.DevWriter(4096) as w:
        mi, mr = im.append(w, src, rec_img, offs, lens, what=case)
    assert mi.all() and mr.all() and np.array_equal(im.model, before)


# ------------------------------------------------------------------ 9. checksums off

def test_checksums_off(cuda):
    """flags = 0: bytes 2..9 and crc_cur stay untouched; lengths and content as
    with checksums."""
    rng = np.random.default_rng(9)
    runs = [40, 0, 1100, 3]
    lens = rng.integers(0, 300, sum(runs))
    first = np.cumsum([0] + runs)
    rooms = [int(lens[first[i]:first[i + 1]].sum()) + 7 for i in range(4)]
    rooms[2] //= 2
    src, offs = pack(lens, rng)
    im, ck = Images(cuda, rooms), Images(cuda, rooms)
    marks = np.asarray([0xDEAD0000 + i for i in range(4)], np.uint32)
    im.raw, im.crc_cur = marks.tolist(), dev_u32(marks, cuda)
    with cio.DevWriter(2048) as w:
        mi, mr = im.append(w, src, runs_to_img(runs), offs, lens, flags=0, what="checksums off")
        ci, cr = ck.append(w, src, runs_to_img(runs), offs, lens, what="checksums on")
    assert np.array_equal(mi, ci) and np.array_equal(mr, cr)
    assert u32(im.crc_cur).tolist() == marks.tolist()
    a, b = im.base.cpu().numpy(), ck.base.cpu().numpy()
    for o in im.offs.tolist():
        assert a[o + 2:o + 10].tobytes() == bytes([0xFF, 0x12, 0xD9, 0x41, 0, 0, 0, 0])
        b[o + 2:o + 10] = a[o + 2:o + 10]
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ 10. graph capture

def test_graph_replay_appends_the_runs_again(cuda):
    """One captured call (a single linear stream) after a warm-up call,
    replayed twice: the lengths are read on the device at run time, so every
    call appends after the last.  Image 0 has room for all three calls; image 1
    for two and a half (the third run is cut by the prefix rule); image 2 for
    exactly two (the third is rejected from its first record); image 3 never
    has a run."""
    import torch
    rng = np.random.default_rng(10)
    runs = [50, 1200, 7, 0]
    lens = rng.integers(1, 60, sum(runs))
    first = np.cumsum([0] + runs)
    tot = [int(lens[first[i]:first[i + 1]].sum()) for i in range(4)]
    rooms = [3 * tot[0] + 9, 2 * tot[1] + tot[1] // 2, 2 * tot[2], 5]
    src, offs = pack(lens, rng)
    rec_img = runs_to_img(runs)
    im = Images(cuda, rooms)
    src_t, ri_t, ro_t, rl_t = dev_u8(src, cuda), dev_u32(rec_img, cuda), dev_i64(offs, cuda), dev_i64(lens, cuda)
    ist = torch.full((4,), 99, dtype=torch.int32, device=cuda)
    rst = torch.full((sum(runs),), 99, dtype=torch.int32, device=cuda)

    def call():
        cf.write_records_batch_dev(w, im.base, im.offs_t, im.caps_t, src_t, ri_t, ro_t, rl_t, im.crc_cur, flags=CK,
                                   img_status=ist, rec_status=rst)

    def step(what):
        mi, mr = model.m_write_records(im.model, im.offs.tolist(), im.caps.tolist(), src, rec_img, offs, lens, im.raw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ist.cpu().numpy(), mi, err_msg=what)
        np.testing.assert_array_equal(rst.cpu().numpy(), mr, err_msg=what)
        im.check(what)
        return mr

    with cio.DevWriter(2048) as w:
        call()                                # warm-up outside the capture (an append like the others)
        assert not step("warm-up").any()
        keep = im.model.copy()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        assert np.array_equal(im.base.cpu().numpy(), keep), "capture runs nothing"
        ist.fill_(99)
        rst.fill_(99)
        graph.replay()
        assert not step("replay 1").any()
        ist.fill_(99)
        rst.fill_(99)
        graph.replay()
        mr = step("replay 2")
        del graph
    assert not mr[:first[1]].any() and mr[first[2]:].all()
    cut = int(np.argmax(mr[first[1]:first[2]] != 0))
    assert 0 < cut < 1200 and mr[first[1] + cut:first[2]].all()


# ------------------------------------------------------------------ 11. round trip

def test_round_trip_through_seal_verify_and_packed_read(cuda):
    """Init -> grouped append -> grouped append -> seal -> verify-on-load ->
    read_packed_batch_dev(CIOA_READ_CONTENT): the concatenation of the accepted
    records in order."""
    import torch
    rng = np.random.default_rng(11)
    runs = [300, 0, 1500, 20]
    n = len(runs)
    first = np.cumsum([0] + runs)
    im = Images(cuda, [60_000, 10, 130_000, 700], [b"", b"meta", b"xy", b""], fill=0)
    im.base = dev_u8(np.zeros_like(im.model), cuda)
    msrc = np.frombuffer(b"metaxy", np.uint8).copy()
    expect = [b""] * n
    with cio.DevWriter(2048) as w:
        st, im.crc_cur = cf.init_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_u8(msrc, cuda),
                                           dev_i64([0, 0, 4, 0], cuda), dev_i64([0, 4, 2, 0], cuda), flags=CK)
        assert not st.cpu().numpy().any()
        im.check("init")
        for k in range(2):
            lens = rng.integers(0, 40, sum(runs))
            lens[first[3]:] = 20              # 400 bytes a call into room for 700: the second call is cut
            src, offs = pack(lens, rng)
            mi, mr = im.append(w, src, runs_to_img(runs), offs, lens, what=f"append {k}")
            assert not mi.any()
            for r in np.flatnonzero(mr == 0):
                i = int(np.searchsorted(first, r, side="right")) - 1
                expect[i] += src[int(offs[r]):int(offs[r]) + int(lens[r])].tobytes()
        assert mr[first[3]:].tolist() == [0] * 15 + [-1] * 5 and not mr[:first[3]].any()
        st = cf.seal_batch_dev(w, im.base, im.offs_t, im.caps_t, im.crc_cur, flags=CK)
        assert not st.cpu().numpy().any()
        with cio.Crc32DevPlan(n) as plan:
            vst = cf.verify_batch_dev(plan, im.base, im.offs_t, im.caps_t, flags=CK)
            assert not vst[0].cpu().numpy().any()
            assert [int(x) for x in vst[4]] == [len(e) for e in expect]
        out = torch.full((sum(len(e) for e in expect) + 8,), 0x5A, dtype=torch.uint8, device=cuda)
        st, po, pl, total = cf.read_packed_batch_dev(w, im.base, im.offs_t, im.caps_t, cf.CIOA_READ_CONTENT, out)
        assert not st.cpu().numpy().any()
    got = out.cpu().numpy().tobytes()
    assert got == b"".join(expect) + b"\x5a" * 8 and int(total[0]) == len(got) - 8
