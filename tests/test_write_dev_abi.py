"""The device-side write path (include/chunkio_amd/cio_write_dev.h): the
symbols and Python exports exist, and the argument checks of every entry point
run before any device call, so they hold without a GPU."""
import ctypes
import os
import re

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRY = ("cio_file_init_batch_dev", "cio_file_write_batch_dev", "cio_file_seal_batch_dev")


def call_args(name, writer, buf, n=1, flags=cf.CIO_CHECKSUM):
    """A full argument list of entry point `name` over one host buffer (never
    dereferenced: every call here is refused, or is a no-op, before that)."""
    head = [writer, buf, 64, buf, buf, n]
    tail = [flags, buf, buf, None]
    if name == "cio_file_seal_batch_dev":
        return head + tail
    return head + [buf, 64, buf, buf] + tail


def test_symbols_are_exported_and_declared():
    lib = chunkio_amd.lib()
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    decl = set(re.findall(r"\b(cio_[a-z_]+)\s*\(", text))
    assert decl == {"cio_dev_writer_create", "cio_dev_writer_destroy", *ENTRY}
    for name in decl:
        assert hasattr(lib, name), name
        assert name in _lib.EXPORTS, name
    assert "#define CIOA_SEAL_RECOMPUTE 256" in text and cf.CIOA_SEAL_RECOMPUTE == 256


def test_python_binding_exports():
    assert chunkio_amd.DevWriter is cf.DevWriter
    assert chunkio_amd.init_batch_dev is cf.init_batch_dev
    assert chunkio_amd.write_batch_dev is cf.write_batch_dev
    assert chunkio_amd.seal_batch_dev is cf.seal_batch_dev
    assert chunkio_amd.CIOA_SEAL_RECOMPUTE == cf.CIOA_SEAL_RECOMPUTE
    assert cf.DevWriter.__enter__ and cf.DevWriter.__exit__ and cf.DevWriter.close


def test_writer_create_rejects_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    h = ctypes.c_void_p()
    assert lib.cio_dev_writer_create(None, 16) == -1
    assert b"null argument" in lib.cio_gpu_last_error()
    for bad in (0, (1 << 32) - 1, 1 << 32):
        assert lib.cio_dev_writer_create(ctypes.byref(h), bad) == -1, bad
        assert b"max_chunks" in lib.cio_gpu_last_error()
        assert not h.value
    lib.cio_dev_writer_destroy(None)          # a no-op


def test_entry_points_reject_null_writer_and_unknown_flags_without_a_gpu():
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)     # just a non-null address: refused before it is looked at
    for name in ENTRY:
        fn = getattr(lib, name)
        for n in (0, 1):
            assert fn(*call_args(name, None, buf, n=n)) == -1, (name, n)
            assert b"null writer" in lib.cio_gpu_last_error()
        allowed = cf.CIO_CHECKSUM | (cf.CIOA_SEAL_RECOMPUTE if name == "cio_file_seal_batch_dev" else 0)
        for flags in (1, 2, 8, 16, 64, 128, 512, cf.CIO_CHECKSUM | 1, 1 << 30,
                      cf.CIOA_SEAL_RECOMPUTE | cf.CIO_CHECKSUM):
            if flags & ~allowed:
                assert fn(*call_args(name, writer, buf, flags=flags)) == -1, (name, flags)
                assert b"unknown flags" in lib.cio_gpu_last_error()
    # recomputing a CRC that is not kept makes no sense
    assert lib.cio_file_seal_batch_dev(*call_args(ENTRY[2], writer, buf, flags=cf.CIOA_SEAL_RECOMPUTE)) == -1
    assert b"needs CIO_CHECKSUM" in lib.cio_gpu_last_error()


def test_entry_points_reject_null_buffers_without_a_gpu():
    """Null buffers are refused before the writer is looked at (`writer` is a
    zeroed block, whose max_chunks reads 0)."""
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)
    for name in ENTRY:
        fn = getattr(lib, name)
        full = call_args(name, writer, buf)
        seal = name == "cio_file_seal_batch_dev"
        # dev_base, img_offs, img_caps, crc_cur (with CIO_CHECKSUM), status; the source and its geometry
        must = [1, 3, 4] + ([7, 8] if seal else [11, 12]) + ([] if seal else [8, 9])
        if name == "cio_file_write_batch_dev":
            must.append(6)
        for k in must:
            a = list(full)
            a[k] = None
            assert fn(*a) == -1, (name, k)
            assert b"null pointer" in lib.cio_gpu_last_error(), (name, k)
        # all there: the next check is the writer's capacity
        assert fn(*full) == -1, name
        assert b"more images than the writer" in lib.cio_gpu_last_error()
    # without CIO_CHECKSUM crc_cur is not used and may be NULL: the capacity check is reached
    a = call_args(ENTRY[1], writer, buf, flags=0)
    a[11] = None
    assert lib.cio_file_write_batch_dev(*a) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()
    # init without metadata takes no metadata geometry: the capacity check is reached
    a = call_args(ENTRY[0], writer, buf)
    a[6] = a[8] = a[9] = None
    assert lib.cio_file_init_batch_dev(*a) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()


def test_entry_points_accept_an_empty_batch_without_a_gpu():
    lib = chunkio_amd.lib()
    writer = ctypes.create_string_buffer(256)
    none = [None, 0, None, None, 0]
    assert lib.cio_file_init_batch_dev(writer, *none, None, 0, None, None, cf.CIO_CHECKSUM, None, None, None) == 0
    assert lib.cio_file_write_batch_dev(writer, *none, None, 0, None, None, cf.CIO_CHECKSUM, None, None, None) == 0
    assert lib.cio_file_seal_batch_dev(writer, *none, cf.CIO_CHECKSUM | cf.CIOA_SEAL_RECOMPUTE, None, None,
                                       None) == 0
