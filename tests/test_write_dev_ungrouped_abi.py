"""The ungrouped append to chunk images in device memory
(include/chunkio_amd/cio_write_dev_ungrouped.h), without a GPU: the symbol and
the Python export exist with the declared prototype, the argument checks run
before any device call, the Python model the GPU tests compare against behaves
as the header says on a hand-written batch, and the host check of the stable
radix sort (`make sortcheck`, a stand-alone program under ASan + UBSan)
passes."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import write_dev_records_model as grouped
import write_dev_ungrouped_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cio_file_write_records_ungrouped_batch_dev"

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_ungrouped.h")) as f:
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


def call_args(writer, buf, n_img=1, n_rec=1, flags=cf.CIO_CHECKSUM, order=None):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n_img, buf, 64, buf, buf, buf, n_rec, flags, buf, buf, buf, order, None]


def test_symbol_is_exported_with_the_declared_prototype():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {NAME}
    res, args = decl[NAME]
    assert NAME in _lib.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is res
    bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
    assert bound == args and len(args) == 18
    assert '#include "cio_write_dev_records.h"' in raw
    # the equivalence is stated in the header
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "the result is that of cio_file_write_records_batch_dev over the stably sorted list" in flat
    assert "cio_file_write_batch_dev called once per round" in flat
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_records.h")) as f:
        assert "cio_write_dev_ungrouped.h" in f.read()
    # the measurement hook is exported, and not declared in any public header
    assert hasattr(lib, "cioa_debug_sort_records_events")
    for h in os.listdir(os.path.join(ROOT, "include", "chunkio_amd")):
        with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
            assert "cioa_debug_sort_records_events" not in f.read(), h


def test_python_binding_export():
    assert chunkio_amd.write_records_ungrouped_batch_dev is cf.write_records_ungrouped_batch_dev
    p = inspect.signature(cf.write_records_ungrouped_batch_dev).parameters
    q = inspect.signature(cf.write_records_batch_dev).parameters
    assert list(p) == ["writer", "base", "img_offs", "img_caps", "src", "rec_img", "rec_offs", "rec_lens", "crc_cur",
                       "flags", "img_status", "rec_status", "order", "stream"]
    assert [k for k in p if k != "order"] == list(q)
    assert p["flags"].default == cf.CIO_CHECKSUM and p["img_status"].default is None and p["order"].default is None


def test_null_writer_and_unknown_flags_are_refused_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(512)     # just a non-null address: refused before it is looked at
    for n_img, n_rec in ((0, 0), (1, 0), (0, 1), (1, 1)):
        assert fn(*call_args(None, buf, n_img, n_rec)) == -1
        assert b"cio_file_write_records_ungrouped_batch_dev: null writer" in lib.cio_gpu_last_error()
    for flags in (1, 2, 8, 16, 64, 128, 256, 512, cf.CIO_CHECKSUM | 1, 1 << 30,
                  cf.CIOA_SEAL_RECOMPUTE | cf.CIO_CHECKSUM):
        assert fn(*call_args(writer, buf, flags=flags)) == -1, flags
        assert b"cio_file_write_records_ungrouped_batch_dev: unknown flags" in lib.cio_gpu_last_error()


def test_null_buffers_and_oversized_batches_are_refused_without_a_gpu():
    """Null buffers are refused before the writer is looked at; then the
    writer's capacity, for images and for records (the block stands in for a
    writer: max_chunks, its first word, 4, everything else zero).  The order
    array may be NULL or given: neither changes a verdict."""
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(512)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    for order in (None, buf):
        full = call_args(writer, buf, 5, 5, order=order)
        # dev_base, img_offs, img_caps, dev_src, rec_img, rec_offs, rec_lens, crc_cur (with CIO_CHECKSUM), statuses
        for j in (1, 3, 4, 6, 8, 9, 10, 13, 14, 15):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert b"cio_file_write_records_ungrouped_batch_dev: null pointer" in lib.cio_gpu_last_error(), j
        assert fn(*call_args(writer, buf, 5, 4, order=order)) == -1
        assert b"ungrouped_batch_dev: more images than the writer" in lib.cio_gpu_last_error()
        assert fn(*call_args(writer, buf, 4, 5, order=order)) == -1
        assert b"ungrouped_batch_dev: more records than the writer" in lib.cio_gpu_last_error()
        # without CIO_CHECKSUM crc_cur is not used and may be NULL: the capacity check is reached
        a = call_args(writer, buf, 5, 1, flags=0, order=order)
        a[13] = None
        assert fn(*a) == -1
        assert b"more images than the writer" in lib.cio_gpu_last_error()


def test_both_empty_batches_are_accepted_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(512)     # max_chunks reads 0: an empty batch never gets that far
    assert fn(*call_args(writer, buf, 0, 7)) == 0
    assert fn(*call_args(writer, buf, 7, 0)) == 0
    assert fn(*call_args(writer, buf, 7, 0, order=buf)) == 0
    assert fn(writer, None, 0, None, None, 0, None, 0, None, None, None, 0, cf.CIO_CHECKSUM, None, None, None,
              None, None) == 0


def fresh():
    buf = bytearray(b"\xa5" * 400)
    view = np.frombuffer(buf, np.uint8)
    raws = [grouped.m_init(view, 10), grouped.m_init(view, 110, b"mm"), 0, grouped.m_init(view, 310)]
    return buf, raws


OFFS, CAPS = [10, 110, 210, 310], [24 + 20, 24 + 2 + 30, 50, 24 + 5]
SRC = bytes(range(1, 101))


def test_model_on_a_hand_written_batch():
    """The records of image 0 (8, 13, 2 and 0 bytes into room for 20)
    interleaved with those of the others: 8 fits, 13 does not, and the 2 and the
    0 after it in LIST order are rejected by the prefix rule.  Image 2 was never
    initialised; the second record of image 3 reads past the source."""
    rec_img = [3, 0, 1, 0, 2, 0, 3, 0]
    rec_offs = [60, 0, 40, 10, 50, 20, 99, 30]
    rec_lens = [5, 8, 30, 13, 1, 2, 2, 0]
    buf, raws = fresh()
    ist, rst, order = model.m_write_records_ungrouped(buf, OFFS, CAPS, SRC, rec_img, rec_offs, rec_lens, raws)
    assert order.tolist() == [1, 3, 5, 7, 2, 4, 0, 6] and order.dtype == np.uint32
    assert ist.tolist() == [0, 0, -1, 0]
    assert rst.tolist() == [0, 0, 0, -1, -1, -1, -1, -1]
    assert bytes(buf[10 + 24:10 + 32]) == SRC[:8] and buf[10 + 32] == 0xA5
    assert grouped.image_check(buf, 10, 44) == (0, 8) and grouped.image_check(buf, 110, 56) == (2, 30)
    assert grouped.image_check(buf, 310, 29) == (0, 5) and bytes(buf[210:260]) == b"\xa5" * 50
    # the grouped model over the sorted list: the same buffer, the same states
    buf2, raws2 = fresh()
    gi, gr = grouped.m_write_records(buf2, OFFS, CAPS, SRC, [0, 0, 0, 0, 1, 2, 3, 3],
                                     [0, 10, 20, 30, 40, 50, 60, 99], [8, 13, 2, 0, 30, 1, 5, 2], raws2)
    assert bytes(buf2) == bytes(buf) and raws2 == raws and gi.tolist() == ist.tolist()
    assert gr.tolist() == rst[order].tolist()
    # the list reversed: image 0 now takes 0, 2 and 13 bytes, and the 8 no longer fit
    buf3, raws3 = fresh()
    ist, rst, order = model.m_write_records_ungrouped(buf3, OFFS, CAPS, SRC, rec_img[::-1], rec_offs[::-1],
                                                      rec_lens[::-1], raws3)
    assert order.tolist() == [0, 2, 4, 6, 5, 3, 1, 7]
    assert rst.tolist() == [0, -1, 0, -1, 0, 0, -1, -1]    # image 3: the bad source first, so its 5 bytes too
    assert bytes(buf3[10 + 24:10 + 24 + 15]) == SRC[20:22] + SRC[10:23] and buf3[10 + 24 + 15] == 0xA5
    # checksums off: crc_cur untouched
    buf4, raws4 = fresh()
    keep = list(raws4)
    model.m_write_records_ungrouped(buf4, OFFS, CAPS, SRC, rec_img, rec_offs, rec_lens, raws4, checksum=False)
    assert raws4 == keep and bytes(buf4[10 + 10:10 + 44]) == bytes(buf[10 + 10:10 + 44])


def test_model_an_index_outside_the_batch_changes_nothing():
    rec_offs = [60, 0, 40, 10, 50, 20, 99, 30]
    rec_lens = [5, 8, 30, 13, 1, 2, 2, 0]
    for at, bad in ((0, 4), (3, 0xFFFFFFFF), (7, 5)):
        rec_img = [3, 0, 1, 0, 2, 0, 3, 0]
        rec_img[at] = bad
        buf, raws = fresh()
        before, keep = bytes(buf), list(raws)
        ist, rst, order = model.m_write_records_ungrouped(buf, OFFS, CAPS, SRC, rec_img, rec_offs, rec_lens, raws)
        assert ist.tolist() == [-1] * 4 and rst.tolist() == [-1] * 8 and bytes(buf) == before and raws == keep
        key = np.minimum(np.asarray(rec_img, np.uint64), 4)
        assert order.tolist() == np.argsort(key, kind="stable").tolist() and order[-1] == at
    # a descending list of valid indices is no defect here
    buf, raws = fresh()
    ist, rst, order = model.m_write_records_ungrouped(buf, OFFS, CAPS, SRC, [3, 1, 0], [0, 10, 20], [1, 1, 1], raws)
    assert ist.tolist() == [0] * 4 and rst.tolist() == [0, 0, 0] and order.tolist() == [2, 1, 0]
    # the empty batches
    ist, rst, order = model.m_write_records_ungrouped(buf, OFFS, CAPS, SRC, [], [], [], raws)
    assert ist.tolist() == [0] * 4 and rst.size == 0 and order.size == 0


def test_sortcheck():
    """The histogram, scan and scatter kernels on the host: every workgroup
    order, wave by wave with an emulated ballot, one to four passes, against
    std::stable_sort, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "sortcheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "sort_check: ok" in r.stdout
