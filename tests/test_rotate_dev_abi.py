"""Rotating full chunk images in device memory
(include/chunkio_amd/cio_write_dev_rotate.h), without a GPU: the two symbols
and the Python exports exist with the declared prototypes, every argument
check runs before any device call, the host check of the kernels' arithmetic
(`make rotatecheck`, a stand-alone program under ASan + UBSan) passes, and the
numpy model the GPU tests compare against is asserted by hand on a batch of
eight images, its fresh image against m_init and its seal against m_seal."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import rotate_dev_model as model
from write_dev_move_model import m_init, m_seal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ROT, RECS = "cio_file_rotate_batch_dev", "cio_file_rotate_records_batch_dev"

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_rotate.h")) as f:
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


def rot_args(writer, buf, n=1, limit=0, new_cap=24, align=16, flags=0):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n, buf, limit, new_cap, align, buf, buf, buf, buf, buf, flags, buf, buf, buf,
            None]


def recs_args(writer, buf, n=1, n_rec=1, limit=0, new_cap=24, align=16, flags=0):
    return [writer, buf, 64, buf, buf, n, buf, buf, n_rec, limit, new_cap, align, buf, buf, buf, buf, buf, flags, buf,
            buf, buf, None]


CALLS = ((ROT, rot_args), (RECS, recs_args))


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {ROT, RECS}
    for name, nargs in ((ROT, 20), (RECS, 22)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert '#include "cio_write_dev.h"' in raw and "#define" not in raw.split("#define CIO_WRITE_DEV_ROTATE_H")[1]
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "an empty image is never rotated" in flat and "preconditions, not checked" in flat
    # the measurement hook is exported, and not declared in any public header
    assert hasattr(lib, "cioa_debug_rotate_events")
    for h in os.listdir(os.path.join(ROOT, "include", "chunkio_amd")):
        with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
            assert "cioa_debug_rotate_events" not in f.read(), h


def test_python_binding_exports():
    assert chunkio_amd.rotate_batch_dev is cf.rotate_batch_dev
    assert chunkio_amd.rotate_records_batch_dev is cf.rotate_records_batch_dev
    p = inspect.signature(cf.rotate_batch_dev).parameters
    assert list(p) == ["writer", "base", "img_offs", "img_caps", "need", "limit", "new_cap", "align", "arena",
                       "out_offs", "out_caps", "out_img", "out_count", "flags", "crc_cur", "total", "status", "stream"]
    q = inspect.signature(cf.rotate_records_batch_dev).parameters
    assert list(q) == ["writer", "base", "img_offs", "img_caps", "rec_img", "rec_lens", "limit", "new_cap", "align",
                       "arena", "out_offs", "out_caps", "out_img", "out_count", "flags", "crc_cur", "total", "status",
                       "stream"]
    for sig in (p, q):
        assert (sig["limit"].default, sig["align"].default, sig["flags"].default) == (0, 16, cf.CIO_CHECKSUM)
        for name in ("out_offs", "out_caps", "out_img", "out_count", "total", "status"):
            assert sig[name].default is None


@pytest.mark.parametrize("name,make", CALLS)
def test_bad_values_are_refused_without_a_gpu(name, make):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # just a non-null address: refused before it is looked at
    err = lib.cio_gpu_last_error
    for flags in (1, 2, 8, 256, 5, 1 << 30, -1):
        assert fn(*make(writer, buf, flags=flags)) == -1, flags
        assert (name + ": unknown flags").encode() in err()
    for new_cap in (0, 1, 23):
        assert fn(*make(writer, buf, new_cap=new_cap)) == -1, new_cap
        assert (name + ": new_cap must be at least 24").encode() in err()
    for align in (0, 3, 24, 8192, 1 << 40):
        assert fn(*make(writer, buf, align=align)) == -1, align
        assert (name + ": align must be a power of two in 1 .. 4096").encode() in err()
    # the same with an empty batch: the values are checked first
    assert fn(*make(writer, buf, n=0, flags=2)) == -1
    assert fn(*make(writer, buf, n=0, new_cap=23)) == -1
    assert fn(*make(writer, buf, n=0, align=3)) == -1
    for n in (0, 1):
        assert fn(*make(None, buf, n=n)) == -1
        assert (name + ": null writer").encode() in err()


@pytest.mark.parametrize("name,make", CALLS)
def test_null_pointers_and_oversized_batches_are_refused_without_a_gpu(name, make):
    """Null buffers are refused before the writer is looked at; then the
    writer's capacity (the block stands in for a writer: max_chunks, its first
    word, 4, everything else zero).  dev_need may be NULL, and dev_crc_cur
    without CIO_CHECKSUM."""
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    for flags in (0, cf.CIO_CHECKSUM):
        full = make(writer, buf, n=5, flags=flags)
        if name == ROT:
            required, crc, optional = (1, 3, 4, 10, 11, 12, 13, 14, 17, 18), 16, (6,)
        else:
            required, crc, optional = (1, 3, 4, 6, 7, 12, 13, 14, 15, 16, 19, 20), 18, ()
        for j in required + ((crc,) if flags else ()):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (name + ": null pointer").encode() in lib.cio_gpu_last_error(), j
        for j in optional + (() if flags else (crc,)):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (name + ": more images than the writer").encode() in lib.cio_gpu_last_error(), j
        assert fn(*full) == -1
        assert (name + ": more images than the writer").encode() in lib.cio_gpu_last_error()
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=4, n_rec=5)) == -1
        assert (name + ": more records than the writer").encode() in lib.cio_gpu_last_error()


@pytest.mark.parametrize("name,make", CALLS)
def test_empty_batches_are_accepted_without_a_gpu(name, make):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # max_chunks reads 0: an empty batch never gets that far
    assert fn(*make(writer, buf, n=0)) == 0
    assert fn(*make(writer, buf, n=0, flags=cf.CIO_CHECKSUM, limit=7)) == 0
    assert fn(*[None if x is buf else x for x in make(writer, buf, n=0)]) == 0
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=7, n_rec=0)) == 0
        assert fn(*recs_args(writer, buf, n=0, n_rec=7)) == 0


def test_rotatecheck():
    """The header, scan, place and commit kernels on the host, every workgroup
    order, against a sequential loop in 128-bit arithmetic, and the sums'
    pre-reduction lane by lane, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "rotatecheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "rotate_check: ok" in r.stdout


# ------------------------------------------------------------------ the model, by hand

M32 = 0xFFFFFFFF
META = b"tag!"


def hand_batch():
    """Eight images of capacity 80 at 0, 100, .. 700, metadata "tag!" unless
    said: 0 not an image at all, need 0; 1 not full; 2 full by room; 3 full by
    the limit of 40 only; 4 empty and over its room; 5 bad magic; 6 full, 41
    bytes of metadata, which do not fit new_cap = 64; 7 full, and cut by the
    arena.  Returns (buf, offs, caps, need, crc_cur)."""
    buf = np.full(2048, 0xA5, np.uint8)
    offs, caps = [100 * i for i in range(8)], [80] * 8
    content = [None, 10, 40, 30, 0, 10, 10, 50]
    need = [0, 5, 13, 11, 100, 5, 100, 10]
    for i in range(1, 8):
        meta = bytes(range(1, 42)) if i == 6 else META
        m_init(buf, offs[i], meta)
        buf[offs[i] + 10:offs[i] + 14] = np.frombuffer(struct.pack(">I", content[i]), np.uint8)
        buf[offs[i] + 24 + len(meta):offs[i] + 24 + len(meta) + content[i]] = 0x30 + i
    buf[offs[5] + 1] = 0x01
    return buf, offs, caps, need, [0x1000 + i for i in range(8)]


def test_model_on_a_hand_written_batch():
    buf, offs, caps, need, crc = hand_batch()
    before = buf.copy()
    arena = [1001, 1008 + 2 * 64 + 63]            # room for two slots of 64 behind the gap of 7, and 63 bytes
    lo, lc, li, count = [7] * 8, [7] * 8, [7] * 8, [1, 8]
    st, total, rotated = model.m_rotate(buf, offs, caps, need, 40, 64, 8, arena, lo, lc, li, count, crc_cur=crc)
    # image 0 is read, because the limit is not 0, and is no image; 7 is cut
    assert st.tolist() == [-1, 0, 0, 0, 0, -1, -1, -1] and rotated == [2, 3]
    assert total == [7 + 3 * 64, 3]               # 2, 3 and 7 reach the placement; 6 has no slot
    assert offs == [0, 100, 1008, 1072, 400, 500, 600, 700] and caps == [80, 80, 64, 64, 80, 80, 80, 80]
    assert arena == [1136, 1199] and count == [3, 8]
    assert lo == [7, 200, 300, 7, 7, 7, 7, 7] and lc == [7, 80, 80, 7, 7, 7, 7, 7] and li == [7, 2, 3] + [7] * 5
    want = before.copy()
    for i, noff in ((2, 1008), (3, 1072)):
        # the seal: htonl(crc_finalize(crc_cur)) and four zero bytes; nothing else of the old image
        want[100 * i + 2:100 * i + 10] = np.frombuffer(struct.pack(">I", (0x1000 + i) ^ M32) + b"\0" * 4, np.uint8)
        # the fresh image: the init header, the length, the metadata; the slot's tail keeps its bytes
        want[noff:noff + 28] = np.frombuffer(bytes([0xC1, 0, 0xFF, 0x12, 0xD9, 0x41] + [0] * 16 + [0, 4]) + META,
                                             np.uint8)
    assert np.array_equal(buf, want)
    raw = model.m_init(np.zeros(64, np.uint8), 0, META)
    assert crc == [0x1000, 0x1001, raw, raw, 0x1004, 0x1005, 0x1006, 0x1007]
    # the same call again: 2 and 3 are empty now, 7 is cut again, nothing changes
    again = buf.copy()
    st, total, rotated = model.m_rotate(buf, offs, caps, need, 40, 64, 8, arena, lo, lc, li, count, crc_cur=crc)
    assert st.tolist() == [-1, 0, 0, 0, 0, -1, -1, -1] and rotated == [] and total == [1136 - 1136 + 64, 1]
    assert np.array_equal(buf, again) and arena == [1136, 1199] and count == [3, 8]


def test_model_without_a_limit_and_without_checksum():
    """limit = 0: image 0 has no need and is not read, image 3 is not full; 2
    and 7 both fit.  Without CIO_CHECKSUM bytes 2..9 of the old image and
    crc_cur stay, and the fresh header has no CRC."""
    buf, offs, caps, need, crc = hand_batch()
    before = buf.copy()
    arena = [1001, 1199]
    lo, lc, li, count = [7] * 2, [7] * 2, [7] * 2, [0, 2]
    st, total, rotated = model.m_rotate(buf, offs, caps, need, 0, 64, 8, arena, lo, lc, li, count, flags=0,
                                        crc_cur=crc)
    assert st.tolist() == [0, 0, 0, 0, 0, -1, -1, 0] and rotated == [2, 7] and total == [7 + 128, 2]
    assert offs == [0, 100, 1008, 300, 400, 500, 600, 1072] and arena == [1136, 1199] and count == [2, 2]
    assert (lo, lc, li) == ([200, 700], [80, 80], [2, 7]) and crc == [0x1000 + i for i in range(8)]
    want = before.copy()
    for noff in (1008, 1072):
        want[noff:noff + 28] = np.frombuffer(bytes([0xC1, 0] + [0] * 20 + [0, 4]) + META, np.uint8)
    assert np.array_equal(buf, want)
    # a list with room for one entry cuts image 7, whatever the arena holds
    buf, offs, caps, need, crc = hand_batch()
    count = [1, 2]
    st, total, rotated = model.m_rotate(buf, offs, caps, need, 0, 64, 8, [1001, 2048], lo, lc, li, count, crc_cur=crc)
    assert st.tolist() == [0, 0, 0, 0, 0, -1, -1, -1] and rotated == [2] and total == [7 + 128, 2] and count == [2, 2]
    # the records variant's malformed list
    st, total, rotated = model.m_rotate(buf, offs, caps, None, 0, 64, 8, [1001, 2048], lo, lc, li, count, crc_cur=crc)
    assert st.tolist() == [-1] * 8 and total == [0, 0] and rotated == []


@pytest.mark.parametrize("meta", [b"", b"x", bytes(range(200))])
def test_model_fresh_image_is_m_init_and_sealed_image_is_m_seal(meta):
    buf = np.full(1024, 0x5A, np.uint8)
    raw = m_init(buf, 3, meta)
    buf[3 + 13] = 9                               # 9 bytes of content
    old = buf.copy()
    offs, caps, crc, arena = [3], [24 + len(meta) + 9], [raw ^ 0x1234], [512, 1024]
    lo, lc, li, count = [0], [0], [0], [0, 1]
    st, total, rotated = model.m_rotate(buf, offs, caps, [1], 0, 300, 1, arena, lo, lc, li, count, crc_cur=crc)
    assert st.tolist() == [0] and rotated == [0] and offs == [512] and caps == [300] and arena == [812, 1024]
    m_seal(old, 3, raw ^ 0x1234)
    fresh = np.full(1024, 0x5A, np.uint8)
    assert crc == [m_init(fresh, 512, meta)]
    assert np.array_equal(buf[:512], old[:512]) and np.array_equal(buf[512:], fresh[512:])
