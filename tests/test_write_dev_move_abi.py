"""Replace-metadata and write_at on chunk images in device memory
(include/chunkio_amd/cio_write_dev_move.h), without a GPU: the symbols and
Python exports exist with the declared prototypes, the argument checks run
before any device call, the numpy model the GPU tests compare against
reproduces the reference-written fixtures, and the host check of the move's
arithmetic (`make movecheck`, a stand-alone program under ASan + UBSan)
passes."""
import ctypes
import hashlib
import json
import os
import re
import subprocess

import numpy as np

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import write_dev_move_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("cio_dev_writer_create_ex", "cio_dev_writer_move_segments", "cio_file_write_metadata_batch_dev",
       "cio_file_write_at_batch_dev")
META, AT = NEW[2], NEW[3]

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_move.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            if "*" in a:
                types.append(ctypes.c_void_p)
            else:
                types.append(CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (CTYPE[res], types)
    return out, text


def call_args(name, writer, buf, n=1, flags=cf.CIO_CHECKSUM):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    head = [writer, buf, 64, buf, buf, n]
    tail = [flags, buf, buf, None]
    if name == AT:
        return head + [buf, buf, 64, buf, buf] + tail
    return head + [buf, 64, buf, buf] + tail


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, text = declarations()
    assert set(decl) == set(NEW)
    for name, (res, args) in decl.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is res, name
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args, (name, bound, args)
    assert len(decl[META][1]) == 14 and len(decl[AT][1]) == 15
    assert "#define CIOA_WRITER_MOVE 1" in text and cf.CIOA_WRITER_MOVE == 1
    # cio_write_dev.h no longer says that these stay host operations
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev.h")) as f:
        old = f.read()
    assert "stays a host operation" not in old and "cio_write_dev_move.h" in old


def test_python_binding_exports():
    assert chunkio_amd.write_metadata_batch_dev is cf.write_metadata_batch_dev
    assert chunkio_amd.write_at_batch_dev is cf.write_at_batch_dev
    assert chunkio_amd.CIOA_WRITER_MOVE == cf.CIOA_WRITER_MOVE
    assert isinstance(cf.DevWriter.move_segments, property)
    import inspect
    assert inspect.signature(cf.DevWriter.__init__).parameters["move"].default is False


def test_writer_create_ex_rejects_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    h = ctypes.c_void_p()
    assert lib.cio_dev_writer_create_ex(None, 16, cf.CIOA_WRITER_MOVE) == -1
    assert b"null argument" in lib.cio_gpu_last_error()
    for bad in (0, (1 << 32) - 1, 1 << 32):
        assert lib.cio_dev_writer_create_ex(ctypes.byref(h), bad, cf.CIOA_WRITER_MOVE) == -1, bad
        assert b"max_chunks" in lib.cio_gpu_last_error()
    for flags in (2, 4, 256, cf.CIOA_WRITER_MOVE | 2, 1 << 30):
        assert lib.cio_dev_writer_create_ex(ctypes.byref(h), 16, flags) == -1, flags
        assert b"unknown flags" in lib.cio_gpu_last_error()
    assert not h.value
    assert lib.cio_dev_writer_move_segments(None) == 0


def test_entry_points_reject_null_writer_and_unknown_flags_without_a_gpu():
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)     # just a non-null address: refused before it is looked at
    for name in (META, AT):
        fn = getattr(lib, name)
        for n in (0, 1):
            assert fn(*call_args(name, None, buf, n=n)) == -1, (name, n)
            assert b"null writer" in lib.cio_gpu_last_error()
        for flags in (1, 2, 8, 16, 64, 128, 256, 512, cf.CIO_CHECKSUM | 1, 1 << 30,
                      cf.CIOA_SEAL_RECOMPUTE | cf.CIO_CHECKSUM):
            assert fn(*call_args(name, writer, buf, flags=flags)) == -1, (name, flags)
            assert b"unknown flags" in lib.cio_gpu_last_error()


def test_entry_points_reject_null_buffers_without_a_gpu():
    """Null buffers are refused before the writer is looked at; then the
    writer's capacity (`writer` is a zeroed block, whose max_chunks reads 0)."""
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)
    for name in (META, AT):
        fn = getattr(lib, name)
        full = call_args(name, writer, buf)
        k = 1 if name == AT else 0
        # dev_base, img_offs, img_caps; (at,) source, its offsets and lengths; crc_cur (with CIO_CHECKSUM), status
        must = [1, 3, 4, 6, 8 + k, 9 + k, 11 + k, 12 + k] + ([7] if name == AT else [])
        for j in must:
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, (name, j)
            assert b"null pointer" in lib.cio_gpu_last_error(), (name, j)
        assert fn(*full) == -1, name
        assert b"more images than the writer" in lib.cio_gpu_last_error()
        # without CIO_CHECKSUM crc_cur is not used and may be NULL: the capacity check is reached
        a = call_args(name, writer, buf, flags=0)
        a[11 + k] = None
        assert fn(*a) == -1
        assert b"more images than the writer" in lib.cio_gpu_last_error()


def test_write_metadata_needs_a_move_writer_without_a_gpu():
    """A writer created without CIOA_WRITER_MOVE is refused in the argument
    checks, after the capacity check.  The block stands in for such a writer:
    max_chunks (its first word) 4, everything else zero."""
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    assert lib.cio_file_write_metadata_batch_dev(*call_args(META, writer, buf, n=1)) == -1
    assert b"created without CIOA_WRITER_MOVE" in lib.cio_gpu_last_error()
    assert lib.cio_file_write_metadata_batch_dev(*call_args(META, writer, buf, n=5)) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()
    assert lib.cio_dev_writer_move_segments(writer) == 0


def test_entry_points_accept_an_empty_batch_without_a_gpu():
    lib = chunkio_amd.lib()
    writer = ctypes.create_string_buffer(256)
    none = [None, 0, None, None, 0]
    assert lib.cio_file_write_metadata_batch_dev(writer, *none, None, 0, None, None, cf.CIO_CHECKSUM, None, None,
                                                 None) == 0
    assert lib.cio_file_write_at_batch_dev(writer, *none, None, None, 0, None, None, cf.CIO_CHECKSUM, None, None,
                                           None) == 0


def test_model_reproduces_the_reference_fixtures():
    """The numpy model replays the ops of every fixture that needs no damage
    step -- c04_write_at and c05_meta_after_content among them -- in a zeroed
    image of the file's size and gets the reference's bytes and crc_cur."""
    with open(os.path.join(ROOT, "tests", "golden", "chunks", "manifest.json")) as f:
        specs = [s for s in json.load(f)["chunks"] if "post" not in s]
    assert [s["name"][:3] for s in specs] == ["c01", "c02", "c03", "c04", "c05", "c06"]
    for s in specs:
        buf = np.zeros(s["size"] + 32, np.uint8)
        raw = model.replay(buf, 16, s["ops"])
        assert hashlib.sha256(buf[16:16 + s["size"]].tobytes()).hexdigest() == s["sha256"], s["name"]
        assert raw == s["load"]["crc_cur"], s["name"]
        assert model.m_geometry(buf, 16) == (s["load"]["meta_size"], s["load"]["content_size"]), s["name"]
        assert not buf[:16].any() and not buf[16 + s["size"]:].any()


def test_movecheck():
    """The move's partition, save / shift split and tile arithmetic on the
    host, every segment order, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "movecheck"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "move_check: ok" in r.stdout
