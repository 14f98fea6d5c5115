"""The write lifecycle of chunk images in device memory
(include/chunkio_amd/cio_write_dev.h): init -> append -> ... -> seal, against
the reference-written fixtures byte for byte, a numpy model of the same
appends over every source / destination alignment, this repo's host chunk
layer, and cio_file_verify_batch_dev / cio_file_verify_batch as the readers."""
import hashlib
import json
import os
import struct
import zlib

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "chunks")
with open(os.path.join(GDIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)

M32 = 0xFFFFFFFF
EMPTY_RAW = 0xBE26ED00
INIT = bytes([0xC1, 0x00, 0xFF, 0x12, 0xD9, 0x41] + [0] * 18)
FILL = 0xA5
CK = cf.CIO_CHECKSUM


# ------------------------------------------------------------------ the model

def raw_update(raw, data):
    """crc_update on the raw (not finalized) state."""
    return zlib.crc32(bytes(data), raw ^ M32) ^ M32


def m_init(buf, off, meta=b"", checksum=True):
    buf[off:off + 24] = np.frombuffer(INIT, np.uint8)
    if not checksum:
        buf[off + 2:off + 6] = 0
    buf[off + 22:off + 24] = np.frombuffer(struct.pack(">H", len(meta)), np.uint8)
    buf[off + 24:off + 24 + len(meta)] = np.frombuffer(bytes(meta), np.uint8)
    return raw_update(M32, buf[off + 22:off + 24 + len(meta)].tobytes())


def m_geometry(buf, off):
    meta = struct.unpack(">H", buf[off + 22:off + 24].tobytes())[0]
    content = struct.unpack(">I", buf[off + 10:off + 14].tobytes())[0]
    return meta, content


def m_write(buf, off, data, raw, checksum=True):
    """cio_file_write + update_checksum on the image at off; the new raw state."""
    if len(data) == 0:
        return raw
    meta, content = m_geometry(buf, off)
    pos = off + 24 + meta + content
    buf[pos:pos + len(data)] = np.frombuffer(bytes(data), np.uint8)
    if checksum:
        raw = raw_update(raw, data)
        buf[off + 2:off + 10] = np.frombuffer(struct.pack("<Q", raw), np.uint8)
    buf[off + 10:off + 14] = np.frombuffer(struct.pack(">I", content + len(data)), np.uint8)
    return raw


def m_seal(buf, off, raw):
    buf[off + 2:off + 10] = np.frombuffer(struct.pack(">I", raw ^ M32) + b"\0\0\0\0", np.uint8)


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


def pack_records(records, misalign, rng, slack=64):
    """One source buffer of random filler holding the records in order, record
    i at an offset that is misalign[i] modulo 16.  (buffer, offs, lens)."""
    offs, pos = [], 3
    for r, mis in zip(records, misalign):
        pos += (mis - pos) % 16
        offs.append(pos)
        pos += len(r) + int(rng.integers(0, 9))
    buf = rng.integers(0, 256, pos + slack, dtype=np.uint8)
    for o, r in zip(offs, records):
        buf[o:o + len(r)] = np.frombuffer(bytes(r), np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray([len(r) for r in records], np.uint64)


class Images:
    """n images in one device buffer with its numpy model side by side."""

    def __init__(self, cuda, offs, caps, total, fill=FILL):
        self.cuda, self.n = cuda, len(offs)
        self.offs, self.caps = np.asarray(offs, np.uint64), np.asarray(caps, np.uint64)
        self.model = np.full(total, fill, np.uint8)
        self.base = dev_u8(self.model, cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.raw = [0] * self.n               # the model's crc_cur
        self.crc_cur = None

    def init(self, w, metas=None, flags=CK, skip=()):
        """skip: entries the device is expected to refuse (the model leaves them alone)."""
        rng = np.random.default_rng(7)
        if metas is None:
            st, self.crc_cur = cf.init_batch_dev(w, self.base, self.offs_t, self.caps_t, flags=flags)
        else:
            src, so, sl = pack_records(metas, [(5 * i + 1) % 16 for i in range(self.n)], rng)
            st, self.crc_cur = cf.init_batch_dev(w, self.base, self.offs_t, self.caps_t, dev_u8(src, self.cuda),
                                                 dev_i64(so, self.cuda), dev_i64(sl, self.cuda), flags=flags)
        for i in range(self.n):
            if i in skip:
                continue
            raw = m_init(self.model, int(self.offs[i]), metas[i] if metas is not None else b"", bool(flags & CK))
            if flags & CK:
                self.raw[i] = raw
        return st.cpu().numpy()

    def write(self, w, records, misalign=None, flags=CK, seed=11):
        rng = np.random.default_rng(seed)
        src, so, sl = pack_records(records, misalign or [(3 * i) % 16 for i in range(self.n)], rng)
        st = cf.write_batch_dev(w, self.base, self.offs_t, self.caps_t, dev_u8(src, self.cuda),
                                dev_i64(so, self.cuda), dev_i64(sl, self.cuda), self.crc_cur, flags=flags)
        for i in range(self.n):
            self.raw[i] = m_write(self.model, int(self.offs[i]), records[i], self.raw[i], bool(flags & CK))
        return st.cpu().numpy()

    def seal(self, w, flags=CK):
        st = cf.seal_batch_dev(w, self.base, self.offs_t, self.caps_t, self.crc_cur, flags=flags)
        if flags & CK:
            for i in range(self.n):
                m_seal(self.model, int(self.offs[i]), self.raw[i])
        return st.cpu().numpy()

    def device(self):
        return self.base.cpu().numpy()

    def check(self, what=""):
        """The WHOLE device buffer (data, headers, every guard byte) and crc_cur."""
        got = self.device()
        if not np.array_equal(got, self.model):
            bad = np.flatnonzero(got != self.model)
            owner = int(np.searchsorted(self.offs, bad[0], side="right")) - 1
            raise AssertionError(f"{what}: {bad.size} bytes differ, the first at {bad[0]} (image {owner} at "
                                 f"{int(self.offs[owner])}): {got[bad[0]]:#x} for {self.model[bad[0]]:#x}")
        np.testing.assert_array_equal(u32(self.crc_cur), np.asarray(self.raw, np.uint32), err_msg=what)


def pattern(length, seed):
    i = np.arange(length, dtype=np.uint64)
    return (((i * 131 + seed * 7 + 17) % 251) + 1).astype(np.uint8).tobytes()


# ------------------------------------------------------------------ 1. fixtures

def buildable(spec):
    """ops = an optional leading meta_write, then writes, an optional sync,
    close -- and the file left as the ops wrote it (no "post" damage)."""
    if "post" in spec:
        return False
    ops = [o["op"] for o in spec["ops"]]
    if ops and ops[0] == "meta_write":
        ops = ops[1:]
    while ops and ops[0] == "write":
        ops = ops[1:]
    return ops in (["sync", "close"], ["close"])


def test_reference_fixtures_byte_for_byte(cuda):
    """c01_empty, c02_content, c03_meta_content and c06_close_no_sync (the
    reference's close syncs an unsynced chunk, so its closing state is init,
    writes, seal as well) built on the GPU in zeroed images of the files'
    sizes: the reference's bytes, its loader's crc_cur and its verdict."""
    specs = [s for s in MANIFEST["chunks"] if buildable(s)]
    assert [s["name"] for s in specs] == ["c01_empty", "c02_content", "c03_meta_content", "c06_close_no_sync"]
    n = len(specs)
    sizes = [s["size"] for s in specs]
    offs, pos = [], 0
    for i, size in enumerate(sizes):
        pos = ((pos + 4095) & ~4095) + 7 * i
        offs.append(pos)
        pos += size
    im = Images(cuda, offs, sizes, pos + 100, fill=0)
    metas = [(s["ops"][0]["meta"].encode() if s["ops"][0]["op"] == "meta_write" else b"") for s in specs]
    writes = [[pattern(o["len"], o["seed"]) for o in s["ops"] if o["op"] == "write"] for s in specs]
    with cio.DevWriter(n) as w:
        assert not im.init(w, metas).any()
        for k in range(max(len(x) for x in writes)):
            st = im.write(w, [x[k] if k < len(x) else b"" for x in writes], seed=k)
            assert not st.any()
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


# ------------------------------------------------------------------ 2. the sweep

SMALL = [0, 1, 2, 3, 4, 15, 16, 17, 63, 64, 65, 4095, 4096, 4097]
LARGE = [300_000, (1 << 20) + 5]


def test_alignment_and_length_sweep(cuda):
    """Every length of SMALL against all 16 x 16 source / destination
    misalignments, and each of LARGE against every source and every destination
    misalignment (32 pairs, relative shifts of both parities), in ONE batch;
    the destination misalignment comes from the image offset and a first
    append of 0..47 bytes.  The buffer is 0xA5 before; afterwards the whole of
    it equals the numpy model, and crc_cur is zlib's."""
    rng = np.random.default_rng(2)
    cases = [(length, s, d) for length in SMALL for s in range(16) for d in range(16)]
    for length in LARGE:
        cases += [(length, k, (7 * k + 3) % 16) for k in range(16)] + [(length, k, (5 * k) % 16) for k in range(16)]
    order = rng.permutation(len(cases))       # the large records anywhere among the small ones
    cases = [cases[j] for j in order]
    n = len(cases)
    offs, caps, pre, pos = [], [], [], 1
    for i, (length, s, d) in enumerate(cases):
        pos += int(rng.integers(1, 41))                       # guard bytes between the images
        pos += ((5 * i) % 16 - pos) % 16                      # the image's own misalignment
        c0 = (d - pos - 24) % 16 + 16 * (i % 3)               # the first append sets the second's alignment
        assert (pos + 24 + c0) % 16 == d
        offs.append(pos)
        pre.append(c0)
        caps.append(24 + c0 + length + (i % 2) * int(rng.integers(0, 30)))    # half of them fit exactly
        pos += caps[-1]
    im = Images(cuda, offs, caps, pos + 77)
    with cio.DevWriter(n) as w:
        assert not im.init(w).any()
        assert im.raw[0] == EMPTY_RAW
        st = im.write(w, [rng.integers(0, 256, c0, dtype=np.uint8).tobytes() for c0 in pre], seed=3)
        assert not st.any()
        im.check("first append")
        records = [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for length, _, _ in cases]
        st = im.write(w, records, misalign=[s for _, s, _ in cases], seed=4)
        assert not st.any()
        im.check("sweep")
        assert not im.seal(w).any()
        im.check("seal")
    for i in (0, n // 2, n - 1):              # the model's crc_cur is zlib's over the image's region
        o = offs[i] + 22
        assert im.raw[i] == zlib.crc32(im.model[o:o + 2 + pre[i] + cases[i][0]].tobytes()) ^ M32


# ------------------------------------------------------------------ 3. the host chunk layer

def host_verify(buf, offs, sizes, flags):
    lib = cf._bind()
    n = len(offs)
    items = (cf.VerifyItem * n)()
    for i in range(n):
        items[i].map = buf.ctypes.data + int(offs[i])
        items[i].fs_size = int(sizes[i])
        items[i].taint = 0
    assert lib.cio_file_verify_batch(items, n, flags) == 0
    return [it.status for it in items], [it.crc_raw for it in items]


def test_against_the_host_chunk_layer(cuda, tmp_path):
    """200 images, metadata 0..200 bytes, three rounds of appends of 0..100 KB
    (zero-length records among them, one record of 2 MB), then seal; cf.Context
    does the same meta_write / write / sync on files.  After each round bytes
    2..9 and 10..13 equal the host map's; at the end the images equal the
    host's up to the data end and the host verify accepts the D2H copy."""
    rng = np.random.default_rng(33)
    n, rounds = 200, 3
    metas = [rng.integers(0, 256, int(m), dtype=np.uint8).tobytes() for m in rng.integers(0, 201, n)]
    metas[0], metas[1] = b"", bytes(200)
    counts = rng.integers(0, 100_001, (rounds, n))
    counts[:, 5] = 0                                          # never written
    counts[0, ::17] = 0
    counts[1, 3::13] = 0
    counts[1, 40] = 2_000_000
    pool = rng.integers(0, 256, 2_000_000 + n, dtype=np.uint8).tobytes()
    offs, caps, pos = [], [], 0
    for i in range(n):
        pos += i % 53
        offs.append(pos)
        caps.append(24 + len(metas[i]) + int(counts[:, i].sum()) + (i % 5) * 100)
        pos += caps[-1]
    im = Images(cuda, offs, caps, pos + 64, fill=0)
    with cf.Context(str(tmp_path / "root"), CK, max_chunks_up=n + 8) as ctx, cio.DevWriter(n) as w:
        stream = ctx.stream("s")
        chunks = []
        for i in range(n):
            c, err = stream.open(f"c{i:03d}", cf.CIO_OPEN, 0)
            assert c is not None, err
            if metas[i]:
                assert c.meta_write(metas[i]) == 0
            chunks.append(c)
        assert not im.init(w, metas).any()
        np.testing.assert_array_equal(u32(im.crc_cur), [c.crc_cur for c in chunks])
        for r in range(rounds):
            records = [pool[i + r:i + r + int(counts[r, i])] for i in range(n)]
            for c, rec in zip(chunks, records):
                if rec:
                    assert c.write(rec) == 0
            assert not im.write(w, records, seed=r).any()
            got = im.device()
            for i, c in enumerate(chunks):
                m = c.map
                assert got[offs[i] + 2:offs[i] + 14].tobytes() == bytes(m[2:14]), (r, i)
            np.testing.assert_array_equal(u32(im.crc_cur), [c.crc_cur for c in chunks])
        for c in chunks:
            assert c.sync() == 0
        assert not im.seal(w).any()
        got = im.device()
        ends = []
        for i, c in enumerate(chunks):
            end = 24 + len(metas[i]) + int(counts[:, i].sum())
            assert c.data_size == int(counts[:, i].sum()) and c.meta_len() == len(metas[i]), i
            assert got[offs[i]:offs[i] + end].tobytes() == bytes(c.map[:end]), i
            ends.append(end)
    im.check("host layer")
    status, crc = host_verify(got, offs, caps, CK)
    assert status == [cf.CIO_OK] * n
    assert crc == im.raw
    status, _ = host_verify(got, offs, ends, CK)             # cut at the data end: a file of exactly that size
    assert status == [cf.CIO_OK] * n


# ------------------------------------------------------------------ 4. rejections

def test_rejected_entries_change_nothing(cuda):
    """One bad entry of each kind among good ones, in one batch.  Validation
    refuses them on the device: status CIO_ERROR, image bytes and crc_cur
    unchanged, the neighbours appended as usual."""
    rng = np.random.default_rng(4)
    n, cap = 14, 1000
    bad = {1: "capacity exceeded by one byte", 3: "bad magic", 5: "source out of range", 7: "cap < 24",
           9: "forged content length", 11: "source offset wraps", 13: "image out of dev_bytes"}
    offs = [40 + i * 1100 + i % 7 for i in range(n)]
    caps = [cap] * n
    caps[7] = 23
    total = offs[13] + cap - 1                # image 13 ends one byte past the buffer
    im = Images(cuda, offs, caps, total)
    metas = [b"m" * (i % 4) for i in range(n)]
    with cio.DevWriter(n) as w:
        good = np.ones(n, bool)
        good[[7, 13]] = False                 # init refuses these two already
        st = im.init(w, metas, skip={7, 13})
        assert (st == np.where(good, cf.CIO_OK, cf.CIO_ERROR)).all()
        sentinel = 0x12345678                 # crc_cur of the two that no call may ever accept
        cur = u32(im.crc_cur)
        assert not cur[~good].any()
        cur[~good] = sentinel
        im.crc_cur = dev_u32(cur, cuda)
        im.raw[7] = im.raw[13] = sentinel
        im.check("init")
        # first a good append of 100 bytes everywhere it can go
        first = [rng.integers(0, 256, 100, dtype=np.uint8).tobytes() if good[i] else b"" for i in range(n)]
        assert not im.write(w, first).any()
        im.check("first append")
        # the bad batch
        lens = np.full(n, 50, np.uint64)
        lens[1] = cap - 24 - len(metas[1]) - 100 + 1          # one byte too many
        im.model[offs[3]] = 0xC0                              # bad magic
        im.model[offs[9] + 10:offs[9] + 14] = np.frombuffer(struct.pack(">I", 0xFFFFFFF0), np.uint8)
        im.base.copy_(dev_u8(im.model, cuda))
        src = rng.integers(0, 256, 4096, dtype=np.uint8)
        so = np.asarray([16 * i + i for i in range(n)], np.uint64)
        so[1] = 1000
        so[5] = 4096 - 49                                     # ends one byte past the source
        so[11] = 2 ** 64 - 8
        st = cf.write_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_u8(src, cuda), dev_i64(so, cuda),
                                dev_i64(lens, cuda), im.crc_cur, flags=CK).cpu().numpy()
        for i in range(n):
            if i in bad:
                assert st[i] == cf.CIO_ERROR, bad[i]
            else:
                assert st[i] == cf.CIO_OK, i
                rec = src[int(so[i]):int(so[i]) + 50].tobytes()
                im.raw[i] = m_write(im.model, offs[i], rec, im.raw[i])
        im.check("bad batch")                 # the rejected images and crc_cur entries did not change
        # the same append with the one byte taken off fits exactly
        lens2 = np.zeros(n, np.uint64)
        lens2[1] = lens[1] - 1
        st = cf.write_batch_dev(w, im.base, im.offs_t, im.caps_t, dev_u8(src, cuda), dev_i64(so, cuda),
                                dev_i64(lens2, cuda), im.crc_cur, flags=CK).cpu().numpy()
        assert not st.any()
        im.raw[1] = m_write(im.model, offs[1], src[1000:1000 + int(lens2[1])].tobytes(), im.raw[1])
        im.check("exact fit")
        # seal refuses the same broken images
        st = cf.seal_batch_dev(w, im.base, im.offs_t, im.caps_t, im.crc_cur, flags=CK).cpu().numpy()
        for i in range(n):
            assert st[i] == (cf.CIO_ERROR if i in (3, 7, 9, 13) else cf.CIO_OK), i
            if st[i] == cf.CIO_OK:
                m_seal(im.model, offs[i], im.raw[i])
        im.check("seal")


# ------------------------------------------------------------------ 5. graph replay

def test_graph_replay_appends_again(cuda):
    """One captured write_batch_dev (a single linear stream), replayed twice
    with src_lens and the source bytes changed in between: the content length
    is read on the device at run time, so the second append lands after the
    first and the CRCs chain."""
    import torch
    rng = np.random.default_rng(5)
    n, room = 40, 90_100                      # three appends of at most 30 000 bytes each
    offs = [9 + i * (room + 24 + 13) for i in range(n)]
    im = Images(cuda, offs, [room + 24] * n, offs[-1] + room + 24 + 50)
    size = 30_000
    so = np.asarray([i * (size + 5) + i % 16 for i in range(n)], np.uint64)
    src_t = dev_u8(np.zeros(int(so[-1]) + size + 16, np.uint8), cuda)
    so_t = dev_i64(so, cuda)
    sl_t = dev_i64(np.zeros(n, np.uint64), cuda)
    status = torch.full((n,), 99, dtype=torch.int32, device=cuda)

    def stage(k):
        lens = rng.integers(0, size + 1, n).astype(np.uint64)
        lens[k] = 0
        lens[k + 1] = 3
        src = rng.integers(0, 256, src_t.numel(), dtype=np.uint8)
        src_t.copy_(torch.from_numpy(src))
        sl_t.copy_(torch.from_numpy(lens.view(np.int64)))
        for i in range(n):
            rec = src[int(so[i]):int(so[i]) + int(lens[i])].tobytes()
            im.raw[i] = m_write(im.model, offs[i], rec, im.raw[i])

    def call():
        cf.write_batch_dev(w, im.base, im.offs_t, im.caps_t, src_t, so_t, sl_t, im.crc_cur, flags=CK, status=status)

    with cio.DevWriter(n) as w:
        assert not im.init(w).any()
        stage(0)
        call()                                # warm-up outside the capture (an append like the others)
        torch.cuda.synchronize()
        im.check("warm-up")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        im.check("capture runs nothing")
        for k in (1, 2):
            stage(2 * k)
            status.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any()
            im.check(f"replay {k}")
        del graph
        assert not im.seal(w).any()
        im.check("seal")
    with cio.Crc32DevPlan(n) as plan:
        st = cf.verify_batch_dev(plan, im.base, im.offs_t, im.caps_t, flags=CK)[0]
        assert not st.cpu().numpy().any()


# ------------------------------------------------------------------ 6. recompute, checksums off

def test_seal_recompute_and_checksums_off(cuda):
    import torch
    rng = np.random.default_rng(6)
    n = 30
    lens = [int(x) for x in rng.integers(0, 50_000, n)]
    lens[0], lens[1] = 0, 1
    metas = [bytes(rng.integers(0, 256, i % 9, dtype=np.uint8)) for i in range(n)]
    offs, caps, pos = [], [], 5
    for i in range(n):
        offs.append(pos)
        caps.append(24 + len(metas[i]) + lens[i] + 10)
        pos += caps[-1] + i % 11
    records = [rng.integers(0, 256, length, dtype=np.uint8).tobytes() for length in lens]
    with cio.DevWriter(n) as w:
        # CIOA_SEAL_RECOMPUTE over a garbage crc_cur gives the plain seal's image and restores crc_cur
        im = Images(cuda, offs, caps, pos + 30)
        assert not im.init(w, metas).any()
        assert not im.write(w, records).any()
        im.crc_cur = torch.full((n,), 0x5EED, dtype=torch.int32, device=cuda)
        assert not im.seal(w, flags=CK | cf.CIOA_SEAL_RECOMPUTE).any()
        im.check("recompute")
        # without CIO_CHECKSUM: init zeroes bytes 2..5, write leaves 2..9 alone, seal writes nothing
        im = Images(cuda, offs, caps, pos + 30)
        assert not im.init(w, metas, flags=0).any()
        sentinel = np.arange(n, dtype=np.uint32) + 1000
        im.crc_cur = dev_u32(sentinel, cuda)
        im.raw = [int(x) for x in sentinel]
        im.check("init without checksums")
        mark = np.frombuffer(b"\x01\x02\x03\x04\x05\x06\x07\x08", np.uint8)
        for o in offs:
            im.model[o + 2:o + 10] = mark
        im.base.copy_(dev_u8(im.model, cuda))
        assert not im.write(w, records, flags=0).any()
        im.check("write without checksums")
        assert all(m_geometry(im.model, o)[1] == length for o, length in zip(offs, lens))
        assert not im.seal(w, flags=0).any()
        im.check("seal without checksums")
