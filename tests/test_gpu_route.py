"""Routing records to chunk images in device memory by their metadata
(include/chunkio_amd/cio_route_dev.h): the directory word for word against the
model's, the routed indices, statuses, totals and miss list against the model
(route_model.py, direct comparison, no hash), against cio_meta_cmp_batch_dev as
the judge, on the reference-written fixtures, on tags that collide in the key,
through stale and damaged directories, and as the head of a captured chain
route -> rotate_records -> grow_records -> ungrouped append.  The image buffer
is compared whole after every case: no byte of it is written."""
import json
import os

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import grow_dev_model as gmodel
import rotate_dev_model as rmodel
import route_model as model
import write_dev_ungrouped_model as umodel
from read_dev_model import layout, make_image
from test_gpu_write_dev_ungrouped import dev_i64, dev_u8, dev_u32, u32
from write_dev_move_model import m_init, pattern

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "chunks")
with open(os.path.join(GDIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)

CK, OK, ERR, RETRY = cf.CIO_CHECKSUM, cf.CIO_OK, cf.CIO_ERROR, cf.CIO_RETRY
# the compare's 16-byte and 1 KiB-row edges, the CRC's 4 KiB step, the longest metadata
LENS = [0, 1, 15, 16, 17, 63, 64, 65, 1023, 1024, 1025, 4095, 4096, 4097, 65535]
MARK = 0x7FFFFFFF        # what the miss list holds before a call


# ------------------------------------------------------------------ helpers

def sentinel(nbytes):
    """What lies between and behind the images: depends on the position, never
    the magic."""
    return ((np.arange(nbytes, dtype=np.uint64) * 7 + 3) % 191).astype(np.uint8)


class Images:
    """Images of the given metadata in one sentinel-filled device buffer, the
    host copy beside it.  bad: images whose magic is destroyed afterwards."""

    def __init__(self, cuda, metas, bad=(), content=lambda i: pattern(i % 5, i), slack=lambda i: i % 7):
        self.cuda, self.n = cuda, len(metas)
        caps = np.asarray([24 + len(m) + len(content(i)) + slack(i) for i, m in enumerate(metas)], np.uint64)
        self.offs, end = layout(caps, [(5 * i + 3) % 16 + 1 for i in range(self.n)])
        self.caps = caps
        self.host = sentinel(end + 11)
        for i, m in enumerate(metas):
            make_image(self.host, int(self.offs[i]), m, content(i))
        for i in bad:
            self.host[int(self.offs[i])] = 0xC0
        self.upload()

    def upload(self):
        self.base = dev_u8(self.host, self.cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, self.cuda), dev_i64(self.caps, self.cuda)

    def unchanged(self, what=""):
        assert np.array_equal(self.base.cpu().numpy(), self.host), what + ": the image buffer changed"

    def build(self, w, check=True):
        d = cf.route_build_dev(w, self.base, self.offs_t, self.caps_t, cf.route_dir(self.n, self.cuda))
        if check:
            k, i, h = model.build(self.host, self.offs, self.caps)
            np.testing.assert_array_equal(u32(d[0])[:self.n], k, err_msg="dir_keys")
            np.testing.assert_array_equal(u32(d[1])[:self.n], i, err_msg="dir_imgs")
            np.testing.assert_array_equal(u32(d[2]), h, err_msg="dir_hdr")
        return d

    def route(self, w, d, tags, t_offs, t_lens, miss_img, gate=None, what="", compare=True, tag_bytes=None):
        """One route call on the device and in the model; everything compared.
        Returns the device's (rec_img, rec_status)."""
        import torch
        n_rec = len(t_offs)
        tags_t = None if tags is None else dev_u8(tags, self.cuda)
        if tags_t is not None and tag_bytes is not None:
            tags_t = tags_t[:tag_bytes]
        gate_t = None if gate is None else torch.from_numpy(np.ascontiguousarray(gate, np.int32)).to(self.cuda)
        ml = torch.full((max(n_rec, 1),), MARK, dtype=torch.int32, device=self.cuda)
        img, st, total, ml = cf.route_records_batch_dev(w, self.base, self.offs_t, self.caps_t, d, tags_t,
                                                        dev_i64(t_offs, self.cuda), dev_i64(t_lens, self.cuda),
                                                        miss_img, gate=gate_t, miss_list=ml)
        img, st, total, ml = u32(img), st.cpu().numpy(), total.cpu().numpy().view(np.uint64), u32(ml)
        if compare:
            mi, ms, mt, mm = model.route(self.host, self.offs, self.caps, tags, t_offs, t_lens, miss_img, gate=gate,
                                         tag_bytes=tag_bytes)
            np.testing.assert_array_equal(st, ms, err_msg=what + ": rec_status")
            np.testing.assert_array_equal(img, mi, err_msg=what + ": rec_img")
            np.testing.assert_array_equal(total, mt, err_msg=what + ": total")
            np.testing.assert_array_equal(ml[:len(mm)], mm, err_msg=what + ": miss_list")
            assert (ml[len(mm):] == MARK).all(), what + ": the rest of the miss list changed"
        if tags is not None:
            assert np.array_equal(tags_t.cpu().numpy(), np.asarray(tags)[:len(tags_t)]), what + ": the tags changed"
        self.unchanged(what)
        return img, st

    def judged(self, tags, t_offs, t_lens, img, st, gate=None, what=""):
        """R6 by the reference-pinned call, one-to-one: the image a record was
        routed to against the record's tag; and by the model on the host."""
        hit = np.flatnonzero(st == OK)
        model.judge(self.host, self.offs, self.caps, tags, t_offs, t_lens, img, st, gate=gate)
        if hit.size == 0:
            return 0
        assert (img[hit] < self.n).all(), what
        res, cst = cf.meta_cmp_batch_dev(self.base, dev_i64(self.offs[img[hit]], self.cuda),
                                         dev_i64(self.caps[img[hit]], self.cuda), dev_u8(tags, self.cuda),
                                         dev_i64(np.asarray(t_offs, np.uint64)[hit], self.cuda),
                                         dev_i64(np.asarray(t_lens, np.uint64)[hit], self.cuda))
        assert not res.cpu().numpy().any() and not cst.cpu().numpy().any(), what
        return hit.size


def mixed_metas(n_img):
    """Every length of LENS; the metadata of image i again at i + 120, the
    empty one every 15 images."""
    return [pattern(LENS[(4 * i + 1) % 15], i % 40) for i in range(n_img)]


def mixed_tags(metas, n_rec):
    """Hits on every kind of image, tags nobody has (the last byte differs, or
    one byte more), and the three malformed kinds.  (tags, offs, lens)."""
    n_img, tags = len(metas), []
    for r in range(n_rec):
        m = metas[(7 * r + 3) % n_img]
        if r % 11 == 5:
            m = m[:-1] + bytes([m[-1] ^ 0x40]) if m else b"\x00"
        elif r % 11 == 8:
            m = (m + b"+")[:65535] if len(m) < 65535 else m[:-1]
        tags.append(m)
    buf, offs, lens = model.pack_tags(tags)
    for r in range(n_rec):
        if r % 13 == 4:
            kind = (r // 13) % 3
            if kind == 0:
                offs[r], lens[r] = len(buf) - 2, 5            # ends behind tag_bytes
            elif kind == 1:
                offs[r], lens[r] = 0, 65536                   # too long for a metadata field
            else:
                offs[r], lens[r] = 2 ** 64 - 3, 5             # off + len wraps
    return buf, offs, lens


# ------------------------------------------------------------------ 1. small shapes, against the models

@pytest.mark.parametrize("n_img", [1, 2, 1023, 1024, 1025, 2049])
def test_against_the_models_at_the_workgroup_edges(cuda, n_img):
    """The sort's workgroup edges in n_img, the probe's and the scan's in
    n_rec; every seventh image without its magic, every ninth gated off in the
    second pass -- with duplicated metadata the next index wins."""
    metas = mixed_metas(n_img)
    bad = [i for i in range(n_img) if i % 7 == 6]
    im = Images(cuda, metas, bad=bad)
    gate = np.asarray([ERR if i % 9 == 0 else OK for i in range(n_img)], np.int32)
    seen = set()
    with cio.DevWriter(max(n_img, 1025)) as w:
        d = im.build(w)
        for n_rec in (1, 63, 64, 65, 255, 256, 257, 1025):
            tags, t_offs, t_lens = mixed_tags(metas, n_rec)
            assert all(int(o) % 2 == 1 for o, ln in zip(t_offs, t_lens) if ln <= 65535 and o < len(tags) - 2)
            img, st = im.route(w, d, tags, t_offs, t_lens, n_img, what=f"{n_img} x {n_rec}")
            seen |= set(st.tolist())
            if n_rec in (257, 1025):
                g_img, g_st = im.route(w, d, tags, t_offs, t_lens, 0xFFFFFFFF, gate=gate,
                                       what=f"{n_img} x {n_rec}, gated")
                if n_img >= 1023:                 # a later image of the same metadata took over from a gated one
                    moved = np.flatnonzero((st == OK) & (g_st == OK) & (g_img != img))
                    assert moved.size and (g_img[moved] > img[moved]).all() and (gate[img[moved]] != OK).all()
                    assert all(metas[int(g_img[r])] == metas[int(img[r])] for r in moved)
    assert seen == {OK, ERR, RETRY} or n_img <= 2


# ------------------------------------------------------------------ 2. against the reference-pinned call

def test_against_meta_cmp_as_the_judge(cuda):
    """33 images x 257 records: cio_meta_cmp_batch_dev once per image k, that
    image repeated and the tags as candidates.  The routed index is the lowest
    k with result 0; a record no k accepts is a miss."""
    n_img, n_rec = 33, 257
    metas = [pattern(LENS[(2 * i) % 15] % 5000, i % 9) for i in range(n_img)]
    metas[20], metas[31] = metas[2], metas[2]
    im = Images(cuda, metas, bad=[2, 13])
    tags, t_offs, t_lens = mixed_tags(metas, n_rec)
    well = np.asarray([model.tag_ok(o, ln, len(tags)) for o, ln in zip(t_offs, t_lens)])
    tags_t, to_t, tl_t = dev_u8(tags, cuda), dev_i64(t_offs, cuda), dev_i64(t_lens, cuda)
    verdict = np.full((n_img, n_rec), -1, np.int32)
    for k in range(n_img):
        res, cst = cf.meta_cmp_batch_dev(im.base, dev_i64(np.full(n_rec, im.offs[k]), cuda),
                                         dev_i64(np.full(n_rec, im.caps[k]), cuda), tags_t, to_t, tl_t)
        res, cst = res.cpu().numpy(), cst.cpu().numpy()
        assert ((cst == OK) == well).all() or k in (2, 13)
        verdict[k] = np.where(cst == OK, res, -1)
    with cio.DevWriter(512) as w:
        d = im.build(w)
        img, st = im.route(w, d, tags, t_offs, t_lens, n_img, what="judge")
    accepted = verdict == 0
    lowest = np.where(accepted.any(axis=0), accepted.argmax(axis=0), n_img)
    assert (lowest[~well] == n_img).all()
    np.testing.assert_array_equal(img, lowest.astype(np.uint32))
    np.testing.assert_array_equal(st == OK, lowest < n_img)
    np.testing.assert_array_equal(st == RETRY, (lowest == n_img) & well)
    assert (st == OK).sum() > 100 and (st == RETRY).sum() > 20 and (st == ERR).sum() > 10
    assert 20 in img and 2 not in img and 13 not in img          # the failing 2's duplicate took its records


# ------------------------------------------------------------------ 3. the reference's fixtures

def test_reference_fixtures(cuda):
    """The 14 reference-written files as images; the tags are each file's
    metadata as its header says, interleaved with tags no file has.  Every
    record lands on the lowest file with that metadata among those that pass
    the image check; a file that fails it is never matched."""
    files = []
    for s in MANIFEST["chunks"]:
        with open(os.path.join(GDIR, "files", s["name"]), "rb") as f:
            files.append(np.frombuffer(f.read(), np.uint8))
    assert len(files) == 14
    caps = np.asarray([len(b) for b in files], np.uint64)
    offs, end = layout(caps, [(5 * i + 3) % 16 + 1 for i in range(len(files))])
    im = Images.__new__(Images)
    im.cuda, im.n, im.offs, im.caps, im.host = cuda, len(files), offs, caps, sentinel(end + 9)
    for o, b in zip(offs, files):
        im.host[int(o):int(o) + len(b)] = b
    im.upload()
    passes = [model.metadata(im.host, len(im.host), offs[i], caps[i]) is not None for i in range(im.n)]
    by_name = {s["name"]: i for i, s in enumerate(MANIFEST["chunks"])}
    assert not passes[by_name["c12_bad_magic"]] and not passes[by_name["c13_short_header"]] and sum(passes) >= 8
    own, tags = [], []
    for i, b in enumerate(files):
        m = bytes(b[24:24 + ((int(b[22]) << 8) | int(b[23]))]) if len(b) >= 24 else b""
        tags += [m, b"no-such-tag-%d" % i]
        own += [i, None]
    assert {len(t) for t in tags[::2]} >= {0, 1, 2, 8}
    buf, t_offs, t_lens = model.pack_tags(tags)
    with cio.DevWriter(64) as w:
        d = im.build(w)
        assert int(u32(d[2])[1]) == sum(passes)
        img, st = im.route(w, d, buf, t_offs, t_lens, im.n, what="fixtures")
    for r, i in enumerate(own):
        if i is None:
            assert st[r] == RETRY and img[r] == im.n
            continue
        same = [k for k in range(im.n) if passes[k] and model.metadata(im.host, len(im.host), offs[k], caps[k]) == tags[r]]
        if passes[i]:
            assert st[r] == OK and img[r] == same[0] <= i, MANIFEST["chunks"][i]["name"]
        else:
            assert img[r] != i and (st[r], int(img[r])) == ((OK, same[0]) if same else (RETRY, im.n))
    assert all(passes[int(k)] for k in img[st == OK])
    assert im.judged(buf, t_offs, t_lens, img, st) >= 8


# ------------------------------------------------------------------ 4. collisions

def test_tags_that_collide_in_the_key(cuda):
    """Groups of two and of five images whose different metadata share one
    key, of equal and of different lengths, between other images.  Every tag
    routes to its own image; a sixth string of the key misses.  The keys 0 and
    0xffffffff are there: 0xffffffff on a string, on a valid image without
    metadata, and on an image that fails the check."""
    k2, k5 = model.key(b"pair"), 0
    pair = [b"pair", model.colliding([b"x" * 61], k2)[0]]
    five = model.colliding([b"", b"a", b"bb", b"c" * 12, b"d" * 12], k5)
    six = model.colliding([b"e" * 12], k5)[0]
    ones = model.colliding([b"ones", b"o" * 1021], 0xFFFFFFFF)
    assert len({model.key(x) for x in five + [six]}) == 1 and len(set(five + [six])) == 6
    other = [pattern(n, 3) for n in (5, 16, 33, 100)]
    #        0         1         2        3         4        5        6   7        8         9        10
    metas = [other[0], five[0], pair[0], other[1], five[1], ones[0], b"", five[2], other[2], pair[1], five[3],
             b"never seen", five[4], other[3], ones[1], b""]
    #        11 (fails) 12      13        14       15
    im = Images(cuda, metas, bad=[11])
    tags = list(metas) + [six, model.colliding([b"q"], 0xFFFFFFFF)[0], model.colliding([b"zz"], k2)[0], b"never seen"]
    want = [0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 16, 12, 13, 14, 6, 16, 16, 16, 16]
    buf, t_offs, t_lens = model.pack_tags(tags)
    with cio.DevWriter(64) as w:
        d = im.build(w)
        keys = u32(d[0])
        assert (keys == 0).sum() == 5 and (keys == k2).sum() == 2 and (keys == 0xFFFFFFFF).sum() == 5
        img, st = im.route(w, d, buf, t_offs, t_lens, 16, what="collisions")
        assert img.tolist() == want
        assert st.tolist() == [OK if x != 16 else RETRY for x in want]
        # with its own image gated off a colliding tag misses: its neighbours of the key are other strings
        gate = np.zeros(16, np.int32)
        gate[[4, 9, 6]] = ERR
        g_img, g_st = im.route(w, d, buf, t_offs, t_lens, 16, gate=gate, what="collisions, gated")
        assert [int(g_img[r]) for r in (4, 9, 6, 15)] == [16, 16, 15, 15]
        assert im.judged(buf, t_offs, t_lens, g_img, g_st, gate=gate) == 13


# ------------------------------------------------------------------ 5. R6: stale and damaged directories

def test_a_stale_or_damaged_directory_only_loses_matches(cuda):
    import torch
    n_img, n_rec = 300, 700
    metas = [pattern(LENS[i % 11], i % 50) for i in range(n_img)]
    im = Images(cuda, metas, bad=[9, 77], slack=lambda i: 40 + i % 7)
    tags, t_offs, t_lens = mixed_tags(metas, n_rec)
    rng = np.random.default_rng(6)
    with cio.DevWriter(1024, move=True) as w:
        d = im.build(w)
        full_img, full_st = im.route(w, d, tags, t_offs, t_lens, n_img, what="fresh")
        n_full = im.judged(tags, t_offs, t_lens, full_img, full_st)
        # shuffled: pairs kept together, the order gone
        perm = torch.from_numpy(rng.permutation(n_img)).to(cuda)
        shuffled = (d[0][perm].contiguous(), d[1][perm].contiguous(), d[2])
        img, st = im.route(w, shuffled, tags, t_offs, t_lens, n_img, what="shuffled", compare=False)
        n_shuf = im.judged(tags, t_offs, t_lens, img, st)
        assert n_shuf <= n_full and ((st == OK) <= (full_st == OK)).all()
        np.testing.assert_array_equal(st == ERR, full_st == ERR)
        # keys in order, every index 0xffffffff: nothing can match, nothing is loaded from outside
        void = (d[0], torch.full_like(d[1], -1), d[2])
        img, st = im.route(w, void, tags, t_offs, t_lens, n_img, what="void", compare=False)
        np.testing.assert_array_equal(st, np.where(full_st == ERR, ERR, RETRY))
        assert (img == n_img).all()
        # keys in order, the indices random: most beyond n_img, some a wrong image
        wild = rng.integers(0, 2 ** 32, n_img, dtype=np.uint64).astype(np.uint32)
        wild[::3] = rng.integers(0, n_img, len(wild[::3]))
        img, st = im.route(w, (d[0], dev_u32(wild, cuda), d[2]), tags, t_offs, t_lens, n_img, what="wild",
                           compare=False)
        im.judged(tags, t_offs, t_lens, img, st)
        # stale: a third of the images get new metadata behind the directory's back
        sel = np.arange(0, n_img, 3)
        new = [b"renamed-%d" % i + pattern(i % 30, 2) for i in sel]
        mbuf, m_offs, m_lens = model.pack_tags(new)
        mst = cf.write_metadata_batch_dev(w, im.base, dev_i64(im.offs[sel], cuda), dev_i64(im.caps[sel], cuda),
                                          dev_u8(mbuf, cuda), dev_i64(m_offs, cuda), dev_i64(m_lens, cuda), None,
                                          flags=0)
        ok = mst.cpu().numpy() == OK
        assert ok.sum() > 60                      # the two without a magic, and any that would not fit, are refused
        im.host = im.base.cpu().numpy().copy()
        for i, m, fine in zip(sel, new, ok):
            if fine:
                assert model.metadata(im.host, len(im.host), im.offs[i], im.caps[i]) == m
                metas[i] = m
        tags2, t_offs2, t_lens2 = mixed_tags(metas, n_rec)       # the tags follow the new names
        img, st = im.route(w, d, tags2, t_offs2, t_lens2, n_img, what="stale", compare=False)
        n_stale = im.judged(tags2, t_offs2, t_lens2, img, st)
        assert not np.isin(img[st == OK], sel[ok]).any(), "a renamed image was found through the old directory"
        d = im.build(w)
        img, st = im.route(w, d, tags2, t_offs2, t_lens2, n_img, what="rebuilt")
        assert np.isin(img[st == OK], sel[ok]).any() and (st == OK).sum() > n_stale


# ------------------------------------------------------------------ 6. R7, R8

def test_directory_of_another_size_and_empty_batches(cuda):
    import torch
    metas = [b"a", b"bb", b"", b"a"]
    im = Images(cuda, metas)
    tags, t_offs, t_lens = model.pack_tags([b"a", b"", b"zz", b"bb"])
    t_lens[2] = 70000
    with cio.DevWriter(16) as w:
        d = im.build(w)
        img, st = im.route(w, d, tags, t_offs, t_lens, 9, what="four images")
        assert img.tolist() == [0, 2, 9, 1] and st.tolist() == [OK, OK, ERR, OK]
        # R7: the directory of three of them, and an unbuilt one, for a batch of four
        small = Images(cuda, metas[:3])
        for other in (small.build(w), cf.route_dir(4, cuda)):
            tm = dev_u8(tags, cuda)
            out = cf.route_records_batch_dev(w, im.base, im.offs_t, im.caps_t, other, tm, dev_i64(t_offs, cuda),
                                             dev_i64(t_lens, cuda), 9, miss_list=True)
            assert u32(out[0]).tolist() == [9] * 4 and out[1].cpu().numpy().tolist() == [ERR] * 4
            assert out[2].cpu().numpy().tolist() == [0, 0, 4] and u32(out[3]).tolist() == [0] * 4
        # R8: no record -- nothing is written, the arrays may be anything
        keep = torch.full((3,), 5, dtype=torch.int64, device=cuda)
        rc = cio.lib().cio_file_route_records_batch_dev(w._handle, None, 0, None, None, 0, None, None, None,
                                                        d[2].data_ptr(), None, 0, None, None, 0, 9, 0, None, None,
                                                        None, keep.data_ptr(), None)
        torch.cuda.synchronize()
        assert rc == 0 and keep.cpu().numpy().tolist() == [5, 5, 5]
        # R8: no image -- the header alone; every well-formed record misses, whatever the image arrays hold
        empty = cf.route_build_dev(w, im.base, im.offs_t[:0], im.caps_t[:0], cf.route_dir(0, cuda))
        assert u32(empty[2]).tolist() == [0, 0, 0, 0] and u32(empty[0]).tolist() == [0]
        out = cf.route_records_batch_dev(w, im.base, im.offs_t[:0], im.caps_t[:0], empty, dev_u8(tags, cuda),
                                         dev_i64(t_offs, cuda), dev_i64(t_lens, cuda), 0, miss_list=True)
        assert u32(out[0]).tolist() == [0] * 4 and out[1].cpu().numpy().tolist() == [RETRY, RETRY, ERR, RETRY]
        assert out[2].cpu().numpy().tolist() == [0, 3, 1] and u32(out[3]).tolist()[:3] == [0, 1, 3]
        # no tag buffer: only empty tags are well-formed
        out = cf.route_records_batch_dev(w, im.base, im.offs_t, im.caps_t, d, None, dev_i64([0, 77, 0], cuda),
                                         dev_i64([0, 0, 1], cuda), 9)
        assert len(out) == 3 and u32(out[0]).tolist() == [2, 2, 9] and out[1].cpu().numpy().tolist() == [OK, OK, ERR]
        # a tag buffer cut short: tag_bytes decides, not what lies behind it
        img, st = im.route(w, d, tags, t_offs, t_lens, 9, what="cut", tag_bytes=int(t_offs[3]) + 1)
        assert st.tolist() == [OK, OK, ERR, ERR]
    im.unchanged("R7, R8")


# ------------------------------------------------------------------ 7. the chain, captured

def test_the_chain_captured_and_replayed(cuda):
    """route -> rotate_records -> grow_records -> write_records_ungrouped
    captured once behind a warm-up round and replayed twice, the tags, the
    record lengths and the source rewritten before every round.  Image 5 is the
    catch-all.  After each round the whole buffer, the arrays, crc_cur and the
    arena are what the numpy models of the four calls give for the model's
    rec_img."""
    import torch
    n_img, n_rec, slot, new_cap, align = 6, 300, 24, 24 + 16 + 900, 32
    names = [b"cpu", b"mem.used", b"disk-io-0123456789", b"net", b"k", b"*"]
    caps = [24 + len(m) + 300 + 50 * i for i, m in enumerate(names)]
    offs, pos = [], 13
    for c in caps:
        offs.append(pos)
        pos += c + 21
    total = 1 << 19
    buf = sentinel(total)
    crc = [m_init(buf, offs[i], names[i]) for i in range(n_img)]
    arena, first = [pos + 7, total], list(offs)
    l_offs, l_caps, l_img, count = [0] * 64, [0] * 64, [0] * 64, [0, 64]
    base_t, offs_t, caps_t = dev_u8(buf, cuda), dev_i64(offs, cuda), dev_i64(caps, cuda)
    crc_t, arena_t = dev_u32(np.asarray(crc, np.uint32), cuda), dev_i64(arena, cuda)
    lists = dict(out_offs=dev_i64(l_offs, cuda), out_caps=dev_i64(l_caps, cuda), out_img=dev_u32(l_img, cuda),
                 out_count=dev_i64(count, cuda))
    t_offs = np.arange(n_rec, dtype=np.uint64) * slot + 1          # a 24-byte slot per tag, odd offsets
    s_offs = np.arange(n_rec, dtype=np.uint64) * 41 + 3
    tags_t = dev_u8(np.zeros(n_rec * slot + 8, np.uint8), cuda)
    src_t = dev_u8(np.zeros(n_rec * 41 + 8, np.uint8), cuda)
    to_t, so_t = dev_i64(t_offs, cuda), dev_i64(s_offs, cuda)
    tl_t, sl_t = dev_i64(np.zeros(n_rec), cuda), dev_i64(np.zeros(n_rec), cuda)
    rst = torch.full((n_img,), 99, dtype=torch.int32, device=cuda)
    gst = torch.full((n_img,), 99, dtype=torch.int32, device=cuda)
    ist = torch.full((n_img,), 99, dtype=torch.int32, device=cuda)
    wst = torch.full((n_rec,), 99, dtype=torch.int32, device=cuda)
    rng = np.random.default_rng(27)
    out = {}

    def stage(k):
        """Round k's inputs on the device, and the models' outcome."""
        pick = rng.integers(0, 7, n_rec)                          # 5: the catch-all's own name, 6: an unknown tag
        tag_list = [names[p] if p < 6 else b"unknown-%d" % (r % 9) for r, p in enumerate(pick)]
        tags = rng.integers(0, 256, tags_t.numel(), dtype=np.uint8)
        for o, t in zip(t_offs, tag_list):
            tags[int(o):int(o) + len(t)] = np.frombuffer(t, np.uint8)
        t_lens = np.asarray([len(t) for t in tag_list], np.uint64)
        s_lens = rng.integers(0, 41, n_rec).astype(np.uint64)
        src = rng.integers(0, 256, src_t.numel(), dtype=np.uint8)
        tags_t.copy_(torch.from_numpy(tags))
        src_t.copy_(torch.from_numpy(src))
        tl_t.copy_(torch.from_numpy(t_lens.view(np.int64)))
        sl_t.copy_(torch.from_numpy(s_lens.view(np.int64)))
        m_img, m_st, m_total, _ = model.route(buf, offs, caps, tags, t_offs, t_lens, 5)
        assert m_img.tolist() == [p if p < 6 else 5 for p in pick] and m_total[1] == (pick == 6).sum() > 0
        need = gmodel.needs_of(m_img, s_lens, n_img)
        r_st, _, rotated = rmodel.m_rotate(buf, offs, caps, need, 0, new_cap, align, arena, l_offs, l_caps, l_img,
                                           count, flags=CK, crc_cur=crc)
        g_st = gmodel.m_grow(buf, offs, caps, need, arena, realloc=512, page=256, align=align)[0]
        mi, mr, _ = umodel.m_write_records_ungrouped(buf, offs, caps, src, m_img, s_offs, s_lens, crc)
        return m_img, m_st, m_total, r_st, g_st, mi, mr, rotated

    def call():
        out["route"] = cf.route_records_batch_dev(w, base_t, offs_t, caps_t, d, tags_t, to_t, tl_t, 5)
        rec_img = out["route"][0]
        cf.rotate_records_batch_dev(w, base_t, offs_t, caps_t, rec_img, sl_t, limit=0, new_cap=new_cap, align=align,
                                    arena=arena_t, flags=CK, crc_cur=crc_t, status=rst, **lists)
        cf.grow_records_batch_dev(w, base_t, offs_t, caps_t, rec_img, sl_t, arena_t, realloc=512, page=256,
                                  align=align, status=gst)
        cf.write_records_ungrouped_batch_dev(w, base_t, offs_t, caps_t, src_t, rec_img, so_t, sl_t, crc_t, flags=CK,
                                             img_status=ist, rec_status=wst)

    def compare(want, what):
        m_img, m_st, m_total, r_st, g_st, mi, mr, _ = want
        torch.cuda.synchronize()
        img, st, tot = out["route"]
        np.testing.assert_array_equal(u32(img), m_img, err_msg=what + ": rec_img")
        np.testing.assert_array_equal(st.cpu().numpy(), m_st, err_msg=what + ": route status")
        np.testing.assert_array_equal(tot.cpu().numpy().view(np.uint64), m_total, err_msg=what + ": route total")
        np.testing.assert_array_equal(rst.cpu().numpy(), r_st, err_msg=what + ": rotate status")
        np.testing.assert_array_equal(gst.cpu().numpy(), g_st, err_msg=what + ": grow status")
        np.testing.assert_array_equal(ist.cpu().numpy(), mi, err_msg=what + ": img_status")
        np.testing.assert_array_equal(wst.cpu().numpy(), mr, err_msg=what + ": rec_status")
        assert offs_t.cpu().numpy().tolist() == [int(x) for x in offs], what + ": img_offs"
        assert caps_t.cpu().numpy().tolist() == [int(x) for x in caps], what + ": img_caps"
        assert arena_t.cpu().numpy().tolist() == arena, what + ": arena"
        assert lists["out_count"].cpu().numpy().tolist() == count, what + ": out_count"
        np.testing.assert_array_equal(u32(crc_t), np.asarray(crc, np.uint32), err_msg=what + ": crc_cur")
        got = base_t.cpu().numpy()
        bad = np.flatnonzero(got != buf)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, the first at {bad[0]}"

    with cio.DevWriter(512) as w:
        d = cf.route_build_dev(w, base_t, offs_t, caps_t, cf.route_dir(n_img, cuda))
        want = stage(0)
        call()                                    # warm-up outside the capture (a round like the others)
        compare(want, "warm-up")
        keep = buf.copy()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        assert np.array_equal(base_t.cpu().numpy(), keep), "capture runs nothing"
        moved = []
        for k in (1, 2):
            want = stage(k)
            for t in (rst, gst, ist, wst):
                t.fill_(99)
            graph.replay()
            compare(want, f"replay {k}")
            assert not want[6].any() and not want[5].any()
            moved += want[7]
        del graph
    # the directory was built once: rotate and grow moved images under it, and every round still found them
    assert moved and count[0] == len(moved) and all(a != b for a, b in zip(offs, first))
