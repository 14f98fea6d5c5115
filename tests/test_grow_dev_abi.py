"""Growing chunk images in device memory out of an arena
(include/chunkio_amd/cio_write_dev_grow.h), without a GPU: the two symbols and
the Python exports exist with the declared prototypes, every argument check
runs before any device call, the host check of the kernels' arithmetic (`make
growcheck`, a stand-alone program under ASan + UBSan) passes, and the growth
rule of the numpy model the GPU tests compare against is pinned to the
reference's: to the sizes of a file the host chunk layer grows write by
write."""
import ctypes
import inspect
import os
import re
import subprocess

import numpy as np
import pytest

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import grow_dev_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GROW, RECS = "cio_file_grow_batch_dev", "cio_file_grow_records_batch_dev"
# cap + k * 32768 rounded up to 4096, by hand from the loop of cio_file_write (src/cio_file.c:1029-1035), for
# five writes of 409 600 bytes into a chunk opened with a 4096-byte size hint
SIZES = [430080, 823296, 1249280, 1642496, 2068480]

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_grow.h")) as f:
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


def grow_args(writer, buf, n=1, realloc=32768, page=4096, align=16, flags=0, prev=(None, None)):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n, buf, buf, realloc, page, align, flags, prev[0], prev[1], buf, buf, None]


def recs_args(writer, buf, n=1, n_rec=1, realloc=32768, page=4096, align=16, flags=0, prev=(None, None)):
    return [writer, buf, 64, buf, buf, n, buf, buf, n_rec, buf, realloc, page, align, flags, prev[0], prev[1], buf,
            buf, None]


CALLS = ((GROW, grow_args), (RECS, recs_args))


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {GROW, RECS}
    for name, nargs in ((GROW, 17), (RECS, 19)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert '#include "cio_write_dev.h"' in raw
    assert re.search(r"#define\s+CIOA_GROW_ZERO\s+1\b", raw) and cf.CIOA_GROW_ZERO == 1
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "no record of that image is rejected for room" in flat
    # the measurement hook is exported, and not declared in any public header
    assert hasattr(lib, "cioa_debug_grow_events")
    for h in os.listdir(os.path.join(ROOT, "include", "chunkio_amd")):
        with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
            assert "cioa_debug_grow_events" not in f.read(), h


def test_python_binding_exports():
    assert chunkio_amd.grow_batch_dev is cf.grow_batch_dev
    assert chunkio_amd.grow_records_batch_dev is cf.grow_records_batch_dev
    assert chunkio_amd.CIOA_GROW_ZERO == 1
    p = inspect.signature(cf.grow_batch_dev).parameters
    assert list(p) == ["writer", "base", "img_offs", "img_caps", "need", "arena", "realloc", "page", "align", "flags",
                       "prev_offs", "prev_caps", "total", "status", "stream"]
    q = inspect.signature(cf.grow_records_batch_dev).parameters
    assert list(q) == ["writer", "base", "img_offs", "img_caps", "rec_img", "rec_lens", "arena", "realloc", "page",
                       "align", "flags", "prev_offs", "prev_caps", "total", "status", "stream"]
    for sig in (p, q):
        assert (sig["realloc"].default, sig["page"].default, sig["align"].default, sig["flags"].default) == \
            (32768, 4096, 16, 0)


@pytest.mark.parametrize("name,make", CALLS)
def test_bad_values_are_refused_without_a_gpu(name, make):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # just a non-null address: refused before it is looked at
    err = lib.cio_gpu_last_error
    for flags in (2, 4, 8, 256, 3, 1 << 30, -1):
        assert fn(*make(writer, buf, flags=flags)) == -1, flags
        assert (name + ": unknown flags").encode() in err()
    assert fn(*make(writer, buf, realloc=0)) == -1
    assert (name + ": realloc_size must not be 0").encode() in err()
    for page in (0, 3, 4097, 6, (1 << 63) + 1):
        assert fn(*make(writer, buf, page=page)) == -1, page
        assert (name + ": page must be a power of two").encode() in err()
    for align in (0, 3, 24, 8192, 1 << 40):
        assert fn(*make(writer, buf, align=align)) == -1, align
        assert (name + ": align must be a power of two in 1 .. 4096").encode() in err()
    for prev in ((buf, None), (None, buf)):
        assert fn(*make(writer, buf, prev=prev)) == -1
        assert (name + ": dev_prev_offs and dev_prev_caps go together").encode() in err()
    # the same with an empty batch: the values are checked first
    assert fn(*make(writer, buf, n=0, realloc=0)) == -1
    assert fn(*make(writer, buf, n=0, align=3)) == -1
    for n in (0, 1):
        assert fn(*make(None, buf, n=n)) == -1
        assert (name + ": null writer").encode() in err()


@pytest.mark.parametrize("name,make", CALLS)
def test_null_pointers_and_oversized_batches_are_refused_without_a_gpu(name, make):
    """Null buffers are refused before the writer is looked at; then the
    writer's capacity (the block stands in for a writer: max_chunks, its first
    word, 4, everything else zero)."""
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    for prev in ((None, None), (buf, buf)):
        full = make(writer, buf, n=5, prev=prev)
        required = (1, 3, 4, 6, 7, 14, 15) if name == GROW else (1, 3, 4, 6, 7, 9, 16, 17)
        for j in required:
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (name + ": null pointer").encode() in lib.cio_gpu_last_error(), j
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
    assert fn(*make(writer, buf, n=0, flags=cf.CIOA_GROW_ZERO, prev=(buf, buf))) == 0
    assert fn(*[None if x is buf else x for x in make(writer, buf, n=0)]) == 0
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=7, n_rec=0)) == 0
        assert fn(*recs_args(writer, buf, n=0, n_rec=7)) == 0


def test_growcheck():
    """The header, scan, place and commit kernels on the host, every workgroup
    order, against a sequential loop in 128-bit arithmetic, and the zero walk
    lane by lane, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "growcheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "grow_check: ok" in r.stdout


def test_model_growth_rule_is_the_reference_s(tmp_path, data400):
    """A chunk opened with a 4096-byte size hint through the host chunk layer
    (which restates src/cio_file.c:1025-1035) gets five writes of 400kb.txt;
    the file's size after each write is the model's capacity for realloc_size
    32768 and page 4096, and both are the sizes derived by hand from the
    reference's loop.  The last is the per-file size of `cio -k -p`."""
    assert len(data400) == 409600
    sizes = []
    with cf.Context(str(tmp_path), cf.CIO_CHECKSUM) as ctx:
        c, err = ctx.stream("grow").open("perf", cf.CIO_OPEN, size=4096)
        assert c is not None, err
        path = os.path.join(str(tmp_path), "grow", "perf")
        assert os.stat(path).st_size == 4096
        for _ in range(5):
            assert c.write(data400) == 0
            sizes.append(os.stat(path).st_size)
        c.close()
    assert sizes == SIZES
    # the model: one image of capacity 4096 at byte 0, grown ahead of each append
    buf = np.full(8 << 20, 0xEE, np.uint8)
    offs, caps, arena = [0], [4096], [4096, len(buf)]
    buf[:24] = 0
    buf[0], buf[1] = 0xC1, 0x00
    got = []
    for k in range(5):
        st, total, po, pc = model.m_grow(buf, offs, caps, [len(data400)], arena, realloc=32768, page=4096, align=16)
        assert st.tolist() == [0] and total == caps[0] and (po[0], pc[0]) != (offs[0], caps[0])
        got.append(caps[0])
        content = (k + 1) * len(data400)
        buf[offs[0] + 10:offs[0] + 14] = np.frombuffer(content.to_bytes(4, "big"), np.uint8)
    assert got == SIZES
    assert model.new_capacity(4096, 24, 409600, 32768, 4096) == SIZES[0]


def test_model_on_a_hand_written_batch():
    """Six images: no need, room, exactly room, one byte over, bad magic,
    one that does not fit the arena any more."""
    buf = np.full(4096, 0xA5, np.uint8)
    offs, caps = [0, 100, 200, 300, 400, 500], [60, 60, 60, 60, 60, 60]
    for o in offs:
        buf[o:o + 24] = 0
        buf[o], buf[o + 1] = 0xC1, 0
        buf[o + 13] = 10                          # 10 bytes of content: used = 34
    buf[400] = 0
    before = buf.copy()
    arena = [1001, 1001 + 7 + 112 + 100]
    st, total, po, pc = model.m_grow(buf, offs, caps, [0, 5, 26, 27, 99, 27], arena, realloc=50, page=8, align=8,
                                     flags=model.GROW_ZERO)
    assert st.tolist() == [0, 0, 0, 0, -1, -1]
    assert offs == [0, 100, 200, 1008, 400, 500] and caps == [60, 60, 60, 112, 60, 60]
    assert total == 7 + 112 + 112 and arena == [1120, 1220]
    assert po.tolist() == [0, 100, 200, 300, 400, 500] and pc.tolist() == [60] * 6
    assert np.array_equal(buf[1008:1008 + 34], before[300:334]) and not buf[1008 + 34:1120].any()
    keep = np.ones(4096, bool)
    keep[1008:1120] = False
    assert np.array_equal(buf[keep], before[keep])
    # the records variant's needs
    assert model.needs_of([2, 0, 2, 1], [5, 1, 1 << 40, 0], 3) == [1, 0, 5 + (1 << 32)]
    assert model.needs_of([2, 3], [5, 1], 3) is None
