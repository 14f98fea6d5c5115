"""The grouped append to chunk images in device memory
(include/chunkio_amd/cio_write_dev_records.h), without a GPU: the symbol and the
Python export exist with the declared prototype, the argument checks run before
any device call, the Python model the GPU tests compare against reproduces the
reference-written fixtures and this repo's host chunk layer, and the host check
of the segmented scan and the acceptance rule (`make recordscheck`, a
stand-alone program under ASan + UBSan) passes."""
import ctypes
import inspect
import json
import os
import re
import subprocess

import numpy as np

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import write_dev_records_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cio_file_write_records_batch_dev"
GDIR = os.path.join(ROOT, "tests", "golden", "chunks")
with open(os.path.join(GDIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
FIXTURES = ("c02_content", "c03_meta_content", "c06_close_no_sync")

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_records.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (CTYPE[res], types)
    return out, raw


def call_args(writer, buf, n_img=1, n_rec=1, flags=cf.CIO_CHECKSUM):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n_img, buf, 64, buf, buf, buf, n_rec, flags, buf, buf, buf, None]


def test_symbol_is_exported_with_the_declared_prototype():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {NAME}
    res, args = decl[NAME]
    assert NAME in _lib.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is res
    bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
    assert bound == args and len(args) == 17
    assert '#include "cio_write_dev.h"' in raw
    # the prefix rule is pinned in the header
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "the accepted records of a run are exactly those before the first rejected one" in flat
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev.h")) as f:
        assert "cio_write_dev_records.h" in f.read()


def test_python_binding_export():
    assert chunkio_amd.write_records_batch_dev is cf.write_records_batch_dev
    p = inspect.signature(cf.write_records_batch_dev).parameters
    assert list(p) == ["writer", "base", "img_offs", "img_caps", "src", "rec_img", "rec_offs", "rec_lens", "crc_cur",
                       "flags", "img_status", "rec_status", "stream"]
    assert p["flags"].default == cf.CIO_CHECKSUM and p["img_status"].default is None


def test_null_writer_and_unknown_flags_are_refused_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)     # just a non-null address: refused before it is looked at
    for n_img, n_rec in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert fn(*call_args(None, buf, n_img, n_rec)) == -1
        assert b"null writer" in lib.cio_gpu_last_error()
    for flags in (1, 2, 8, 16, 64, 128, 256, 512, cf.CIO_CHECKSUM | 1, 1 << 30,
                  cf.CIOA_SEAL_RECOMPUTE | cf.CIO_CHECKSUM):
        assert fn(*call_args(writer, buf, flags=flags)) == -1, flags
        assert b"unknown flags" in lib.cio_gpu_last_error()


def test_null_buffers_and_oversized_batches_are_refused_without_a_gpu():
    """Null buffers are refused before the writer is looked at; then the
    writer's capacity, for images and for records (the block stands in for a
    writer: max_chunks, its first word, 4, everything else zero)."""
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    full = call_args(writer, buf, 5, 5)
    # dev_base, img_offs, img_caps, dev_src, rec_img, rec_offs, rec_lens, crc_cur (with CIO_CHECKSUM), both statuses
    for j in (1, 3, 4, 6, 8, 9, 10, 13, 14, 15):
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert b"null pointer" in lib.cio_gpu_last_error(), j
    assert fn(*call_args(writer, buf, 5, 4)) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()
    assert fn(*call_args(writer, buf, 4, 5)) == -1
    assert b"more records than the writer" in lib.cio_gpu_last_error()
    # without CIO_CHECKSUM crc_cur is not used and may be NULL: the capacity check is reached
    a = call_args(writer, buf, 5, 1, flags=0)
    a[13] = None
    assert fn(*a) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()


def test_both_empty_batches_are_accepted_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)     # max_chunks reads 0: an empty batch never gets that far
    assert fn(*call_args(writer, buf, 0, 7)) == 0
    assert fn(*call_args(writer, buf, 7, 0)) == 0
    assert fn(writer, None, 0, None, None, 0, None, 0, None, None, None, 0, cf.CIO_CHECKSUM, None, None, None,
              None) == 0


def fixture_batch():
    """The fixtures' images in one zeroed buffer, initialised with their
    metadata, and their writes as ONE grouped batch.  (buffer, offs, caps,
    crc_cur, src, rec_img, rec_offs, rec_lens, specs)."""
    specs = [s for s in MANIFEST["chunks"] if s["name"] in FIXTURES]
    assert [s["name"] for s in specs] == list(FIXTURES)
    offs, pos = [], 5
    for s in specs:
        offs.append(pos)
        pos += s["size"] + 11
    buf = bytearray(pos)
    raws, src, rec_img, rec_offs, rec_lens = [], bytearray(b"\x99" * 3), [], [], []
    view = np.frombuffer(buf, np.uint8)
    for i, s in enumerate(specs):
        metas = [o["meta"].encode() for o in s["ops"] if o["op"] == "meta_write"]
        assert s["ops"][0]["op"] in ("meta_write", "write") and len(metas) <= 1
        raws.append(model.m_init(view, offs[i], metas[0] if metas else b""))
        for o in s["ops"]:
            if o["op"] == "write":
                rec_img.append(i)
                rec_offs.append(len(src))
                rec_lens.append(o["len"])
                src += model.pattern(o["len"], o["seed"]) + b"\x77" * (i + 1)
    return buf, offs, [s["size"] for s in specs], raws, bytes(src), rec_img, rec_offs, rec_lens, specs


def test_model_reproduces_the_reference_fixtures():
    """c02, c03 and c06: init, their writes as one grouped call, seal.  The
    first 24 + meta + content bytes are the fixture's, and crc_cur its
    loader's."""
    buf, offs, caps, raws, src, rec_img, rec_offs, rec_lens, specs = fixture_batch()
    assert len(rec_img) == 5
    ist, rst = model.m_write_records(buf, offs, caps, src, rec_img, rec_offs, rec_lens, raws)
    assert not ist.any() and not rst.any()
    view = np.frombuffer(buf, np.uint8)
    for i, s in enumerate(specs):
        model.m_seal(view, offs[i], raws[i])
        used = 24 + s["load"]["meta_size"] + s["load"]["content_size"]
        with open(os.path.join(GDIR, "files", s["name"]), "rb") as f:
            want = f.read()
        assert bytes(buf[offs[i]:offs[i] + used]) == want[:used], s["name"]
        assert not any(buf[offs[i] + used:offs[i] + caps[i] + 11]), s["name"]
        assert raws[i] == s["load"]["crc_cur"], s["name"]
    assert not any(buf[:5])


def test_model_rules():
    """The prefix rule, the cut at room, rejected images, malformed grouping
    and checksums off, on a small batch in plain Python."""
    def fresh():
        buf = bytearray(b"\xa5" * 400)
        view = np.frombuffer(buf, np.uint8)
        raws = [model.m_init(view, 10), model.m_init(view, 110, b"mm"), 0, model.m_init(view, 310)]
        return buf, raws
    offs, caps = [10, 110, 210, 310], [24 + 20, 24 + 2 + 30, 50, 24 + 5]
    src = bytes(range(1, 101))
    rec_img = [0, 0, 0, 0, 1, 2, 3, 3]
    rec_offs = [0, 10, 20, 30, 40, 50, 60, 99]
    rec_lens = [8, 13, 2, 0, 30, 1, 5, 2]            # image 0: 8 fits, 13 does not, 2 would, 0 would
    buf, raws = fresh()
    ist, rst = model.m_write_records(buf, offs, caps, src, rec_img, rec_offs, rec_lens, raws)
    assert ist.tolist() == [0, 0, -1, 0]            # image 2 was never initialised: bad magic
    assert rst.tolist() == [0, -1, -1, -1, 0, -1, 0, -1]       # the last: source past the end
    assert bytes(buf[10 + 24:10 + 32]) == src[:8] and buf[10 + 32] == 0xA5
    assert model.image_check(buf, 10, 44) == (0, 8) and model.image_check(buf, 110, 56) == (2, 30)
    assert model.image_check(buf, 310, 29) == (0, 5)
    assert bytes(buf[210:260]) == b"\xa5" * 50
    assert raws[0] == model.raw_update(0xBE26ED00, src[:8]) and raws[2] == 0
    # malformed: nothing changes
    for bad in ([0, 0, 0, 0, 1, 2, 3, 4], [0, 0, 0, 0, 1, 2, 3, 2], [1, 0, 0, 0, 1, 2, 3, 3]):
        buf2, raws2 = fresh()
        before = bytes(buf2)
        ist, rst = model.m_write_records(buf2, offs, caps, src, bad, rec_offs, rec_lens, raws2)
        assert ist.tolist() == [-1] * 4 and rst.tolist() == [-1] * 8 and bytes(buf2) == before
    # checksums off: the same bytes but for 2..9, crc_cur untouched
    buf3, raws3 = fresh()
    keep = list(raws3)
    model.m_write_records(buf3, offs, caps, src, rec_img, rec_offs, rec_lens, raws3, checksum=False)
    assert raws3 == keep
    for o, c in zip(offs, caps):
        assert bytes(buf3[o + 10:o + c]) == bytes(buf[o + 10:o + c]) and bytes(buf3[o:o + 2]) == bytes(buf[o:o + 2])
    assert bytes(buf3[12:20]) == bytes([0xFF, 0x12, 0xD9, 0x41, 0, 0, 0, 0])
    assert model.rounds([0, 0, 2, 3, 3, 3], 4) == [{0: 0, 2: 2, 3: 3}, {0: 1, 3: 4}, {3: 5}]


def test_model_agrees_with_the_host_chunk_layer(tmp_path):
    """Chunk.write record by record on the host route leaves the same trimmed
    file as the model's grouped append into an initialised image."""
    rng = np.random.default_rng(3)
    records = [rng.integers(0, 256, int(n), dtype=np.uint8).tobytes() for n in (1, 0, 4097, 300, 7, 65536, 3)]
    path = tmp_path / "root" / "stream" / "chunk"
    os.makedirs(path.parent)
    c, err = cf.ChunkFile.open(str(path))
    assert err == cf.CIO_OK
    for r in records:
        assert c.write(r) == 0
    assert c.sync() == 0
    c.close()
    with open(path, "rb") as f:
        host = f.read()
    total = sum(len(r) for r in records)
    buf = bytearray(len(host) + 9)
    raws = [model.m_init(np.frombuffer(buf, np.uint8), 4)]
    src = b"".join(records)
    offs = np.cumsum([0] + [len(r) for r in records])[:-1]
    ist, rst = model.m_write_records(buf, [4], [len(host)], src, [0] * len(records), offs,
                                     [len(r) for r in records], raws)
    assert not ist.any() and not rst.any()
    model.m_seal(np.frombuffer(buf, np.uint8), 4, raws[0])
    assert bytes(buf[4:4 + 24 + total]) == host[:24 + total]


def test_recordscheck():
    """The segmented scan, the carry across workgroups and passes, and the
    acceptance rule on the host, every workgroup order, under ASan + UBSan (a
    stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "recordscheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "records_check: ok" in r.stdout
