"""The ungrouped append to chunk images in device memory
(include/chunkio_amd/cio_write_dev_ungrouped.h): many records per image in one
call, the record list in any order.  Every case compares with the Python model
(write_dev_ungrouped_model.py): the WHOLE image buffer including a sentinel
pattern in the slack between and after the images, crc_cur, both status arrays,
the order array, and the untouched source."""
import hashlib
import json
import os

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import write_dev_ungrouped_model as model
from write_dev_records_model import m_init, m_seal, pattern

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
with open(os.path.join(HERE, "golden", "chunks", "manifest.json")) as _f:
    MANIFEST = json.load(_f)

CK = cf.CIO_CHECKSUM
MARK = 0x7FFFFFFF        # what the order array holds before a call


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
    slack between and after them holds a position-dependent sentinel.

    With n_img and index, the len(rooms) images built are the images `index` of
    a batch of n_img; every other image of the batch is 24 zero bytes behind
    the sentinel (no magic: it would fail its check if it were ever read)."""

    def __init__(self, cuda, rooms, metas=None, gap=37, fill=None, n_img=None, index=None):
        self.cuda, self.n = cuda, len(rooms)
        metas = metas or [b""] * self.n
        offs, caps, pos = [], [], 13
        for i, room in enumerate(rooms):
            offs.append(pos)
            caps.append(24 + len(metas[i]) + room)
            pos += caps[-1] + gap + i % 5
        total = pos + 50
        self.built = np.asarray(offs, np.uint64)
        if fill is None:
            self.model = ((np.arange(total + 24, dtype=np.uint64) * 7 + 3) % 251).astype(np.uint8)
        else:
            self.model = np.full(total + 24, fill, np.uint8)
        self.model[total:] = 0
        self.raw = [m_init(self.model, offs[i], metas[i]) for i in range(self.n)]
        if n_img is None:
            self.offs, self.caps = np.asarray(offs, np.uint64), np.asarray(caps, np.uint64)
        else:
            self.offs, self.caps = np.full(n_img, total, np.uint64), np.full(n_img, 24, np.uint64)
            self.offs[index], self.caps[index] = offs, caps
            raw = [0] * n_img
            for k, i in enumerate(index):
                raw[int(i)] = self.raw[k]
            self.raw = raw
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
            owner = int(np.searchsorted(self.built, bad[0], side="right")) - 1
            raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0]} (built image {owner} at "
                                 f"{int(self.built[owner])}, +{bad[0] - int(self.built[owner])}): "
                                 f"{got[bad[0]]:#x} for {self.model[bad[0]]:#x}")
        np.testing.assert_array_equal(u32(self.crc_cur), np.asarray(self.raw, np.uint32), err_msg=what)

    def append(self, w, src, rec_img, rec_offs, rec_lens, flags=CK, what="", with_order=True):
        """One ungrouped call on the device and in the model; everything
        compared.  Returns the model's (img_status, rec_status, order)."""
        import torch
        src = np.ascontiguousarray(src, dtype=np.uint8)
        src_t = dev_u8(src, self.cuda)
        n_rec = len(rec_img)
        order = torch.full((max(n_rec, 1),), MARK, dtype=torch.int32, device=self.cuda) if with_order else None
        ist, rst = cf.write_records_ungrouped_batch_dev(w, self.base, self.offs_t, self.caps_t, src_t,
                                                        dev_u32(rec_img, self.cuda), dev_i64(rec_offs, self.cuda),
                                                        dev_i64(rec_lens, self.cuda), self.crc_cur, flags=flags,
                                                        order=order)
        mi, mr, mo = model.m_write_records_ungrouped(self.model, self.offs.tolist(), self.caps.tolist(), src, rec_img,
                                                     rec_offs, rec_lens, self.raw, checksum=bool(flags & CK))
        np.testing.assert_array_equal(ist.cpu().numpy(), mi, err_msg=what + ": img_status")
        np.testing.assert_array_equal(rst.cpu().numpy(), mr, err_msg=what + ": rec_status")
        if with_order:
            np.testing.assert_array_equal(u32(order)[:n_rec], mo, err_msg=what + ": order")
        self.check(what)
        assert np.array_equal(src_t.cpu().numpy(), src), what + ": the source changed"
        return mi, mr, mo


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


def rooms_of(rec_img, lens, n_img, slack=0):
    return np.bincount(np.asarray(rec_img, np.int64), weights=np.asarray(lens, np.float64),
                       minlength=n_img).astype(np.int64) + slack


# ------------------------------------------------------------------ 1. the reference's fixtures

def test_reference_fixtures_as_one_interleaved_list(cuda):
    """c02, c03 and c06 in ONE call: three images, their five writes dealt
    round-robin (image 2 first) after an init_batch_dev with the 8-byte and the
    1-byte metadata; then seal.  The bytes and crc_cur are the fixtures', and
    verify-on-load accepts all three."""
    names = ("c02_content", "c03_meta_content", "c06_close_no_sync")
    specs = [s for s in MANIFEST["chunks"] if s["name"] in names]
    assert [s["name"] for s in specs] == list(names)
    metas = [b"".join(o["meta"].encode() for o in s["ops"] if o["op"] == "meta_write") for s in specs]
    assert [len(m) for m in metas] == [0, 8, 1]
    im = Images(cuda, [s["size"] - 24 - len(m) for s, m in zip(specs, metas)], metas, fill=0)
    im.base = dev_u8(np.zeros_like(im.model), cuda)      # zeroed on the device: init_batch_dev writes m_init's bytes
    per = [[pattern(o["len"], o["seed"]) for o in s["ops"] if o["op"] == "write"] for s in specs]
    recs, rec_img, k = [], [], 0
    while any(k < len(p) for p in per):
        for i in (2, 0, 1):
            if k < len(per[i]):
                recs.append(per[i][k])
                rec_img.append(i)
        k += 1
    assert len(recs) == 5 and rec_img != sorted(rec_img)
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
        mi, mr, mo = im.append(w, src, rec_img, offs, [len(r) for r in recs], what="fixtures")
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


# ------------------------------------------------------------------ 2., 9. against the grouped call

def grouped_batch():
    """The batch of test_gpu_write_dev_records.test_equals_the_rounds_of_write_batch_dev:
    9 images, runs of 1024 and 2100 records, lengths 0..40 plus 4095 / 4096 /
    4097 and one of 1 MiB, one run cut by its room."""
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
    return rng, rec_img, offs, lens, rooms, src, metas, first


def test_equals_the_grouped_call_over_the_stable_sort(cuda):
    """The grouped batch randomly permuted through the new call, and its stable
    sort through write_records_batch_dev on a second copy of the buffer: the
    two copies end byte for byte the same, the statuses agree after
    un-permuting, and order is numpy's stable argsort.  The lengths differ
    between the records of a run, so an unstable sort shows in the bytes.
    Then, on the same writer, the grouped call still rejects a descending
    list."""
    rng, rec_img, offs, lens, rooms, src, metas, first = grouped_batch()
    n_rec = rec_img.size
    perm = rng.permutation(n_rec)
    p_img, p_offs, p_lens = rec_img[perm], offs[perm], lens[perm]
    assert (np.diff(p_img.astype(np.int64)) < 0).any()
    im = Images(cuda, rooms, metas)
    start, seeds = im.model.copy(), list(im.raw)
    with cio.DevWriter(n_rec) as w:
        mi, mr, mo = im.append(w, src, p_img, p_offs, p_lens, what="permuted")
        assert np.array_equal(mo, np.argsort(p_img, kind="stable"))
        assert not mi.any()
        # the cut run: its accepted records are its first three in LIST order
        cut = np.flatnonzero(p_img == 3)
        fits = np.cumsum(p_lens[cut]) <= 60
        n_acc = int(np.argmin(fits)) if not fits.all() else cut.size
        assert 0 < n_acc < 6 and not mr[cut[:n_acc]].any() and mr[cut[n_acc:]].all()
        assert not np.delete(mr, cut).any()
        # the stable sort through the grouped call, on a copy
        base2, crc2 = dev_u8(start, cuda), dev_u32(np.asarray(seeds, np.uint32), cuda)
        ist, rst = cf.write_records_batch_dev(w, base2, im.offs_t, im.caps_t, dev_u8(src, cuda),
                                              dev_u32(p_img[mo], cuda), dev_i64(p_offs[mo], cuda),
                                              dev_i64(p_lens[mo], cuda), crc2, flags=CK)
        assert np.array_equal(base2.cpu().numpy(), im.base.cpu().numpy())
        np.testing.assert_array_equal(u32(crc2), u32(im.crc_cur))
        np.testing.assert_array_equal(ist.cpu().numpy(), mi)
        back = np.empty(n_rec, np.int32)
        back[mo] = rst.cpu().numpy()
        np.testing.assert_array_equal(back, mr)
        # 9. the existing contract on the writer the new call has just used: a descending list is malformed
        desc = np.sort(p_img)[::-1].copy()
        keep = base2.cpu().numpy()
        ist, rst = cf.write_records_batch_dev(w, base2, im.offs_t, im.caps_t, dev_u8(src, cuda), dev_u32(desc, cuda),
                                              dev_i64(p_offs, cuda), dev_i64(np.zeros(n_rec), cuda), crc2, flags=CK)
        assert ist.cpu().numpy().all() and rst.cpu().numpy().all()
        assert np.array_equal(base2.cpu().numpy(), keep)
        np.testing.assert_array_equal(u32(crc2), np.asarray(im.raw, np.uint32))
        # ... which the new call accepts
        mi, mr, mo = im.append(w, src, desc, p_offs, np.zeros(n_rec, np.int64), what="descending, empty records")
        assert not mi.any() and not mr.any()


# ------------------------------------------------------------------ 3. pass counts

@pytest.mark.parametrize("n_img", [255, 256, 257, 65536, 65537])
def test_pass_counts(cuda, n_img):
    """One pass up to 255 images, two up to 65535, three beyond.  A few dozen
    images get records: 0, 255, 256 and n_img - 1 where they exist, and indices
    that differ only in their second or only in their third byte.  About 3000
    records of 1..16 bytes.  The other images are zero bytes that are never
    read."""
    rng = np.random.default_rng(n_img)
    want = {0, 1, 2, 7, 100, 254, 255, 256, 0x0101, 0x0201, 0x0301, 0xFF01, 0xFFFF, 0x10000, 0x010203, 0x020203,
            0x010303, n_img - 2, n_img - 1}
    index = np.asarray(sorted(i for i in want if 0 <= i < n_img), np.int64)
    extra = rng.choice(n_img, 12, replace=False)
    index = np.unique(np.concatenate([index, extra]))
    n_rec = 3000
    rec_img = index[rng.integers(0, index.size, n_rec)].astype(np.uint32)
    rec_img[:index.size] = index[::-1]                      # every one of them at least once, descending
    lens = rng.integers(1, 17, n_rec)
    src, offs = pack(lens, rng)
    rooms = rooms_of(rec_img, lens, n_img)[index]
    rooms[::4] //= 2                                        # every fourth run is cut
    im = Images(cuda, rooms.tolist(), n_img=n_img, index=index)
    with cio.DevWriter(max(n_img, n_rec)) as w:
        mi, mr, mo = im.append(w, src, rec_img, offs, lens, what=f"n_img = {n_img}")
    assert not mi.any() and mr.any() and not mr.all()


# ------------------------------------------------------------------ 4. boundaries

@pytest.mark.parametrize("n_rec", [1, 63, 64, 65, 1023, 1024, 1025, 2049])
def test_record_counts_at_the_wave_and_workgroup_edges(cuda, n_rec):
    """All records to one image; all to distinct images in reversed order; two
    alternating images."""
    rng = np.random.default_rng(n_rec)
    lens = rng.integers(0, 21, n_rec)
    src, offs = pack(lens, rng)
    lists = {
        "one image": (np.full(n_rec, 2, np.uint32), 4),
        "distinct, reversed": (np.arange(n_rec, dtype=np.uint32)[::-1].copy(), n_rec),
        "two alternating": ((np.arange(n_rec, dtype=np.uint32) % 2) * 2 + 1, 5),
    }
    with cio.DevWriter(max(n_rec, 8)) as w:
        for what, (rec_img, n_img) in lists.items():
            rooms = rooms_of(rec_img, lens, n_img)
            rooms[rec_img[0]] -= rooms[rec_img[0]] // 3     # the first record's image is cut; the others fit exactly
            im = Images(cuda, rooms.tolist())
            mi, mr, mo = im.append(w, src, rec_img, offs, lens, what=f"{what}, n_rec = {n_rec}")
            assert not mi.any()
            assert not mr[rec_img != rec_img[0]].any()


# ------------------------------------------------------------------ 5. already sorted

def test_already_sorted_input(cuda):
    """A grouped list gives the grouped call's result, and order is the
    identity."""
    rng, rec_img, offs, lens, rooms, src, metas, first = grouped_batch()
    im, gr = Images(cuda, rooms, metas), Images(cuda, rooms, metas)
    with cio.DevWriter(rec_img.size) as w:
        mi, mr, mo = im.append(w, src, rec_img, offs, lens, what="sorted")
        ist, rst = cf.write_records_batch_dev(w, gr.base, gr.offs_t, gr.caps_t, dev_u8(src, cuda),
                                              dev_u32(rec_img, cuda), dev_i64(offs, cuda), dev_i64(lens, cuda),
                                              gr.crc_cur, flags=CK)
    assert np.array_equal(mo, np.arange(rec_img.size))
    assert np.array_equal(gr.base.cpu().numpy(), im.base.cpu().numpy())
    np.testing.assert_array_equal(u32(gr.crc_cur), u32(im.crc_cur))
    np.testing.assert_array_equal(ist.cpu().numpy(), mi)
    np.testing.assert_array_equal(rst.cpu().numpy(), mr)
    assert mr[first[3]:first[4]].tolist() == [0, 0, 0, -1, -1, -1]


# ------------------------------------------------------------------ 6. malformed

def test_an_index_outside_the_batch_rejects_the_batch(cuda):
    """One index equal to n_img, and one 0xFFFFFFFF, each at the first record,
    in the middle and at the last record of 2100 records: every status is
    CIO_ERROR, no image byte and no crc_cur changes, and order is still the
    stable order of the clamped keys.  A descending list with valid indices is
    accepted."""
    rng = np.random.default_rng(6)
    n_img, n_rec = 5, 2100
    good = rng.integers(0, n_img, n_rec).astype(np.uint32)
    lens = rng.integers(0, 30, n_rec)
    src, offs = pack(lens, rng)
    im = Images(cuda, [40000] * n_img)
    before, seeds = im.model.copy(), list(im.raw)
    with cio.DevWriter(4096) as w:
        for bad in (n_img, 0xFFFFFFFF):
            for at in (0, 1024, n_rec - 1):
                rec_img = good.copy()
                rec_img[at] = bad
                mi, mr, mo = im.append(w, src, rec_img, offs, lens, what=f"{bad:#x} at {at}")
                assert mi.all() and mr.all() and mo[-1] == at
                assert np.array_equal(im.model, before) and im.raw == seeds
        desc = np.sort(good)[::-1].copy()
        mi, mr, mo = im.append(w, src, desc, offs, lens, what="descending")
        assert not mi.any() and not mr.any() and not np.array_equal(im.model, before)


# ------------------------------------------------------------------ 7. checksums off

def test_checksums_off(cuda):
    """flags = 0: bytes 2..9 and crc_cur stay untouched; lengths, content,
    statuses and order as with checksums.  No order array the second time."""
    rng = np.random.default_rng(9)
    runs = [40, 0, 1100, 3]
    rec_img = rng.permutation(runs_to_img(runs))
    lens = rng.integers(0, 300, sum(runs))
    rooms = rooms_of(rec_img, lens, 4, slack=7)
    rooms[2] //= 2
    src, offs = pack(lens, rng)
    im, ck = Images(cuda, rooms.tolist()), Images(cuda, rooms.tolist())
    marks = np.asarray([0xDEAD0000 + i for i in range(4)], np.uint32)
    im.raw, im.crc_cur = marks.tolist(), dev_u32(marks, cuda)
    with cio.DevWriter(2048) as w:
        mi, mr, mo = im.append(w, src, rec_img, offs, lens, flags=0, what="checksums off")
        ci, cr, co = ck.append(w, src, rec_img, offs, lens, what="checksums on", with_order=False)
    assert np.array_equal(mi, ci) and np.array_equal(mr, cr) and np.array_equal(mo, co)
    assert u32(im.crc_cur).tolist() == marks.tolist()
    a, b = im.base.cpu().numpy(), ck.base.cpu().numpy()
    for o in im.offs.tolist():
        assert a[o + 2:o + 10].tobytes() == bytes([0xFF, 0x12, 0xD9, 0x41, 0, 0, 0, 0])
        b[o + 2:o + 10] = a[o + 2:o + 10]
    assert np.array_equal(a, b)


# ------------------------------------------------------------------ 8. graph capture

def test_graph_replay_appends_again(cuda):
    """One captured call after a warm-up call, replayed twice: the sort and the
    lengths are read on the device at run time, so every call appends after the
    last.  Image 0 has room for all three calls; image 1 for two and a half (the
    third run is cut by the prefix rule); image 2 for exactly two; image 3 never
    gets a record."""
    import torch
    rng = np.random.default_rng(10)
    runs = [50, 1200, 7, 0]
    rec_img = rng.permutation(runs_to_img(runs))
    n_rec = rec_img.size
    lens = rng.integers(1, 60, n_rec)
    tot = rooms_of(rec_img, lens, 4)
    rooms = [3 * int(tot[0]) + 9, 2 * int(tot[1]) + int(tot[1]) // 2, 2 * int(tot[2]), 5]
    src, offs = pack(lens, rng)
    im = Images(cuda, rooms)
    src_t, ri_t, ro_t, rl_t = dev_u8(src, cuda), dev_u32(rec_img, cuda), dev_i64(offs, cuda), dev_i64(lens, cuda)
    ist = torch.full((4,), 99, dtype=torch.int32, device=cuda)
    rst = torch.full((n_rec,), 99, dtype=torch.int32, device=cuda)
    order = torch.full((n_rec,), MARK, dtype=torch.int32, device=cuda)

    def call():
        cf.write_records_ungrouped_batch_dev(w, im.base, im.offs_t, im.caps_t, src_t, ri_t, ro_t, rl_t, im.crc_cur,
                                             flags=CK, img_status=ist, rec_status=rst, order=order)

    def step(what):
        mi, mr, mo = model.m_write_records_ungrouped(im.model, im.offs.tolist(), im.caps.tolist(), src, rec_img, offs,
                                                     lens, im.raw)
        torch.cuda.synchronize()
        np.testing.assert_array_equal(ist.cpu().numpy(), mi, err_msg=what)
        np.testing.assert_array_equal(rst.cpu().numpy(), mr, err_msg=what)
        np.testing.assert_array_equal(u32(order), mo, err_msg=what)
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
        for k in (1, 2):
            ist.fill_(99)
            rst.fill_(99)
            order.fill_(MARK)
            graph.replay()
            mr = step(f"replay {k}")
            assert k == 2 or not mr.any()
        del graph
    assert not mr[rec_img == 0].any() and mr[rec_img == 2].all()
    of1 = mr[rec_img == 1]
    cut = int(np.argmax(of1 != 0))
    assert 0 < cut < 1200 and of1[cut:].all() and not of1[:cut].any()
