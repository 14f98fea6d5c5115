"""Verify-on-load of chunk images that are already in device memory
(cio_file_verify_batch_dev): the reference loader's verdicts on the files the
reference wrote (tests/golden/chunks), and the host route's verdicts on a
synthetic batch written through this repo's chunk layer and then damaged."""
import ctypes
import hashlib
import json
import os
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
CHUNKS = MANIFEST["chunks"]
NAMES = [c["name"] for c in CHUNKS]


def _verdicts(st, er, cr, names, flags_of):
    """What the host call's test keeps of each file: status, error, and the
    raw CRC only where the chunk loaded with checksums on."""
    out = {}
    for i, n in enumerate(names):
        out[n] = (int(st[i]), int(er[i]), int(cr[i]) if int(st[i]) == cf.CIO_OK and flags_of(n) else None)
    return out


def _expected(names):
    by = {s["name"]: s for s in CHUNKS}
    out = {}
    for n in names:
        ld = by[n]["load"]
        status = cf.CIO_OK if ld["ok"] else ld["err"]
        crc = ld["crc_cur"] if ld["ok"] and by[n]["load_flags"] & cf.CIO_CHECKSUM else None
        out[n] = (status, ld["last_chunk_error"], crc)
    return out


def place(images, offset_of):
    """One host buffer holding every image at offset_of(i, previous end)."""
    offs, pos = [], 0
    for i, b in enumerate(images):
        pos = offset_of(i, pos)
        offs.append(pos)
        pos += len(b)
    buf = np.zeros(pos + 4096, np.uint8)
    for o, b in zip(offs, images):
        buf[o:o + len(b)] = np.frombuffer(b, np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray([len(b) for b in images], np.uint64)


def dev_i64(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(cuda)


def run_dev(plan, base_t, offs, sizes, flags, cuda):
    st, er, cr, ml, cl = cf.verify_batch_dev(plan, base_t, dev_i64(offs, cuda), dev_i64(sizes, cuda), flags=flags)
    return (st.cpu().numpy(), er.cpu().numpy(), cr.cpu().numpy().view(np.uint32), ml.cpu().numpy(),
            cl.cpu().numpy())


def test_reference_files_get_the_reference_loaders_verdicts(cuda):
    """The 14 reference-written files in one device buffer, file i at a 4 KiB
    boundary plus 7 i bytes (every region alignment), grouped by the manifest's
    load flags.  Covers the empty file, bad magic, short header, truncation,
    both legacy-inference cases, bad CRC and bad CRC with checksums off."""
    import torch
    by = {s["name"]: s for s in CHUNKS}
    images = [open(os.path.join(GDIR, "files", n), "rb").read() for n in NAMES]
    assert len(images) == 14
    buf, offs, sizes = place(images, lambda i, pos: ((pos + 4095) & ~4095) + 7 * i)
    before = hashlib.sha256(buf.tobytes()).hexdigest()
    base_t = torch.from_numpy(buf).to(cuda)
    expected = _expected(NAMES)
    with cio.Crc32DevPlan(len(NAMES)) as plan:
        for load_flags in sorted({s["load_flags"] for s in CHUNKS}):
            idx = [i for i, n in enumerate(NAMES) if by[n]["load_flags"] == load_flags]
            names = [NAMES[i] for i in idx]
            st, er, cr, ml, cl = run_dev(plan, base_t, offs[idx], sizes[idx], load_flags, cuda)
            got = _verdicts(st, er, cr, names, lambda n: by[n]["load_flags"] & cf.CIO_CHECKSUM)
            assert got == {n: expected[n] for n in names}
            for k, n in enumerate(names):
                if by[n]["load"]["ok"]:
                    assert (int(ml[k]), int(cl[k])) == (by[n]["load"]["meta_size"], by[n]["load"]["content_size"]), n
                if not (load_flags & cf.CIO_CHECKSUM):
                    assert int(cr[k]) == 0, n
    assert hashlib.sha256(base_t.cpu().numpy().tobytes()).hexdigest() == before     # nothing written back


@pytest.fixture
def host_route():
    cio.route(reset=True, cpu_max=1 << 62, threads=1)
    yield
    cio.route(reset=True)


def host_verify(buf, offs, sizes, flags):
    lib = cf._bind()
    n = len(offs)
    items = (cf.VerifyItem * n)()
    for i in range(n):
        items[i].map = buf.ctypes.data + int(offs[i])
        items[i].fs_size = int(sizes[i])
        items[i].taint = 0
    assert lib.cio_file_verify_batch(items, n, flags) == 0
    return ([it.status for it in items], [it.error for it in items], [it.crc_raw for it in items],
            [it.meta_len for it in items], [it.content_len for it in items])


def test_synthetic_batch_matches_the_host_route(cuda, host_route, tmp_path):
    """300 images written by the chunk layer (metadata 0..200 bytes, content
    0..300 KB), 10 with one flipped byte (header CRC, metadata, content,
    byte 7 in turn), 2 with a length field larger than the file: the device
    verdicts equal cio_file_verify_batch's on the host route over the same
    bytes, and every passing crc_raw is zlib's CRC of the region."""
    import torch
    rng = np.random.default_rng(300)
    n = 300
    metas = rng.integers(0, 201, n)
    contents = rng.integers(0, 300_001, n)
    metas[:16] = rng.integers(1, 201, 16)           # the damaged ones have metadata and content
    contents[:16] = rng.integers(1000, 300_001, 16)
    contents[20], metas[20] = 0, 0                   # an empty chunk among them
    pool = rng.integers(1, 256, 300_000 + 200, dtype=np.uint8).tobytes()
    with cf.Context(str(tmp_path / "root"), cf.CIO_CHECKSUM) as ctx:
        st = ctx.stream("s")
        for i in range(n):
            c, err = st.open(f"c{i:03d}", cf.CIO_OPEN, 0)
            assert c is not None, err
            if metas[i]:
                assert c.meta_write(pool[i:i + int(metas[i])]) == 0
            if contents[i]:
                assert c.write(pool[2 * i:2 * i + int(contents[i])]) == 0
            assert c.sync() == 0
            c.close()
    images = [bytearray(open(tmp_path / "root" / "s" / f"c{i:03d}", "rb").read()) for i in range(n)]
    for k in range(10):
        i, img = k, images[k]
        pos = (2 + k % 4, 24 + int(metas[i]) // 2, 24 + int(metas[i]) + int(contents[i]) // 2, 7)[k % 4]
        img[pos] ^= 0x40
    for i in (10, 11):
        images[i][10:14] = (len(images[i]) + 1000).to_bytes(4, "big")
    buf, offs, sizes = place([bytes(b) for b in images], lambda i, pos: ((pos + 63) & ~63) + i % 61)
    want = host_verify(buf, offs, sizes, cf.CIO_CHECKSUM)
    assert sum(1 for s in want[0] if s != cf.CIO_OK) == 12
    assert sorted({e for e in want[1] if e}) == [cf.CIO_ERR_BAD_FILE_SIZE, cf.CIO_ERR_BAD_CHECKSUM]
    base_t = torch.from_numpy(buf).to(cuda)
    with cio.Crc32DevPlan(n) as plan:
        st_, er, cr, ml, cl = run_dev(plan, base_t, offs, sizes, cf.CIO_CHECKSUM, cuda)
    assert [int(x) for x in st_] == want[0]
    assert [int(x) for x in er] == want[1]
    assert [int(x) for x in cr] == want[2]
    assert [int(x) for x in ml] == want[3]
    assert [int(x) for x in cl] == want[4]
    for i in range(n):
        if int(st_[i]) == cf.CIO_OK:
            o = int(offs[i]) + 22
            region = buf[o:o + 2 + int(ml[i]) + int(cl[i])].tobytes()
            assert int(cr[i]) == zlib.crc32(region) ^ 0xFFFFFFFF, i
