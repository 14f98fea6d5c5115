"""The device read path (include/chunkio_amd/cio_read_dev.h), without a GPU:
the symbols and Python exports exist with the declared prototypes, the argument
checks run before any device call, the numpy model the GPU tests compare
against reproduces the reference-written fixtures and agrees with the host
chunk layer, and the host check of the placement arithmetic (`make
placecheck`, a stand-alone program under ASan + UBSan) passes."""
import ctypes
import json
import os
import re
import shutil
import subprocess

import numpy as np

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import read_dev_model as model

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GDIR = os.path.join(ROOT, "tests", "golden", "chunks")
PLACED, PACKED, CMP = "cio_file_read_batch_dev", "cio_file_read_packed_batch_dev", "cio_meta_cmp_batch_dev"
CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}
LOADABLE = ["c01", "c02", "c03", "c04", "c05", "c06", "c14"]

with open(os.path.join(GDIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
SPECS = [s for s in MANIFEST["chunks"] if s["name"][:3] in LOADABLE]


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_read_dev.h")) as f:
        text = re.sub(r"/\*.*?\*/", "", f.read(), flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (CTYPE[res], types)
    return out, text


def placed_args(writer, buf, n=1, what=cf.CIOA_READ_CONTENT, flags=0):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n, what, None, buf, 64, buf, buf, flags, buf, buf, None]


def packed_args(writer, buf, n=1, what=cf.CIOA_READ_CONTENT, flags=0, align=16):
    return [writer, buf, 64, buf, buf, n, what, None, buf, 64, align, flags, buf, buf, buf, buf, None]


def fixture(name):
    with open(os.path.join(GDIR, "files", name), "rb") as f:
        return np.frombuffer(f.read(), np.uint8)


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, text = declarations()
    assert set(decl) == {PLACED, PACKED, CMP}
    for name, (res, args) in decl.items():
        assert name in _lib.EXPORTS, name
        fn = getattr(lib, name)
        assert fn.restype is res, name
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args, (name, bound, args)
    assert (len(decl[PLACED][1]), len(decl[PACKED][1]), len(decl[CMP][1])) == (16, 17, 12)
    for define, value in (("CIOA_READ_META", 0), ("CIOA_READ_CONTENT", 1), ("CIOA_READ_IMAGE", 2),
                          ("CIOA_READ_NUL", 1)):
        assert re.search(r"#define %s\s+%d\b" % (define, value), text), define
        assert getattr(cf, define) == value
    assert '#include "cio_write_dev.h"' in text
    # the headers it extends keep their declarations and point here
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev.h")) as f:
        assert "cio_read_dev.h" in f.read()


def test_python_binding_exports():
    for name in ("read_batch_dev", "read_packed_batch_dev", "meta_cmp_batch_dev", "CIOA_READ_META",
                 "CIOA_READ_CONTENT", "CIOA_READ_IMAGE", "CIOA_READ_NUL"):
        assert getattr(chunkio_amd, name) is getattr(cf, name), name
    assert (model.META, model.CONTENT, model.IMAGE, model.NUL) == (
        cf.CIOA_READ_META, cf.CIOA_READ_CONTENT, cf.CIOA_READ_IMAGE, cf.CIOA_READ_NUL)


def test_read_calls_reject_bad_arguments_without_a_gpu():
    """Unknown what / flags / align, a null writer and null pointers are
    refused before the writer is looked at; then the writer's capacity
    (`writer` is a zeroed block, whose max_chunks reads 0)."""
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(256)     # just a non-null address
    for fn, args in ((lib.cio_file_read_batch_dev, placed_args), (lib.cio_file_read_packed_batch_dev, packed_args)):
        for n in (0, 1):
            assert fn(*args(None, buf, n=n)) == -1
            assert b"null writer" in lib.cio_gpu_last_error()
        for what in (-1, 3, 4, 256):
            assert fn(*args(writer, buf, what=what)) == -1, what
            assert b"unknown what" in lib.cio_gpu_last_error()
        for flags in (2, 3, 4, 256, 1 << 30):
            assert fn(*args(writer, buf, flags=flags)) == -1, flags
            assert b"unknown flags" in lib.cio_gpu_last_error()
        assert fn(*args(writer, buf, flags=cf.CIOA_READ_NUL)) == -1
        assert b"more images than the writer" in lib.cio_gpu_last_error()
        ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)       # a writer for 4 images
        assert fn(*args(writer, buf, n=5)) == -1
        assert b"more images than the writer" in lib.cio_gpu_last_error()
        ctypes.memset(writer, 0, 4)
    for align in (0, 3, 8192, 4097, 1 << 40):
        for n in (0, 1):
            assert lib.cio_file_read_packed_batch_dev(*packed_args(writer, buf, n=n, align=align)) == -1, align
            assert b"align" in lib.cio_gpu_last_error()
    # dev_base, img_offs, img_caps, out_lens, status; with an output, its offsets and capacities
    for j in (1, 3, 4, 13, 14, 10, 11):
        a = placed_args(writer, buf)
        a[j] = None
        assert lib.cio_file_read_batch_dev(*a) == -1, j
        assert b"null pointer" in lib.cio_gpu_last_error(), j
    # dev_base, img_offs, img_caps, out_offs, out_lens, total, status
    for j in (1, 3, 4, 12, 13, 14, 15):
        a = packed_args(writer, buf)
        a[j] = None
        assert lib.cio_file_read_packed_batch_dev(*a) == -1, j
        assert b"null pointer" in lib.cio_gpu_last_error(), j
    # a size query (dev_out NULL) needs no slots: the capacity check is reached
    a = placed_args(writer, buf)
    a[8] = a[10] = a[11] = None
    assert lib.cio_file_read_batch_dev(*a) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()
    a = packed_args(writer, buf)
    a[8] = None
    assert lib.cio_file_read_packed_batch_dev(*a) == -1
    assert b"more images than the writer" in lib.cio_gpu_last_error()


def test_meta_cmp_rejects_null_pointers_without_a_gpu():
    lib = chunkio_amd.lib()
    buf = ctypes.create_string_buffer(64)
    full = [buf, 64, buf, buf, 1, buf, 64, buf, buf, buf, buf, None]
    for j in (0, 2, 3, 5, 7, 8, 9, 10):
        a = list(full)
        a[j] = None
        assert lib.cio_meta_cmp_batch_dev(*a) == -1, j
        assert b"null pointer" in lib.cio_gpu_last_error(), j


def test_entry_points_accept_an_empty_batch_without_a_gpu():
    lib = chunkio_amd.lib()
    writer = ctypes.create_string_buffer(256)
    assert lib.cio_file_read_batch_dev(writer, None, 0, None, None, 0, cf.CIOA_READ_META, None, None, 0, None, None,
                                       0, None, None, None) == 0
    assert lib.cio_file_read_packed_batch_dev(writer, None, 0, None, None, 0, cf.CIOA_READ_IMAGE, None, None, 0, 1,
                                              cf.CIOA_READ_NUL, None, None, None, None, None) == 0
    assert lib.cio_meta_cmp_batch_dev(None, 0, None, None, 0, None, 0, None, None, None, None, None) == 0


def one_buffer(files, slack=37):
    """The files at misaligned offsets of one buffer, each in a slot with slack."""
    caps = np.asarray([len(b) + slack for b in files], np.uint64)
    offs, end = model.layout(caps, [(5 * i + 3) % 16 + 1 for i in range(len(files))])
    base = np.full(end + 9, 0xEE, np.uint8)
    for o, b in zip(offs, files):
        base[int(o):int(o) + len(b)] = b
    return base, offs, caps


def test_model_reproduces_the_reference_fixtures():
    """CIOA_READ_IMAGE of each loadable fixture is the file trimmed to 24 +
    meta + content, and the sizes are the ones the reference reports on load."""
    assert [s["name"][:3] for s in SPECS] == LOADABLE
    files = [fixture(s["name"]) for s in SPECS]
    base, offs, caps = one_buffer(files)
    used = [24 + s["load"]["meta_size"] + s["load"]["content_size"] for s in SPECS]
    for what, sizes in ((model.META, [s["load"]["meta_size"] for s in SPECS]),
                        (model.CONTENT, [s["load"]["content_size"] for s in SPECS]), (model.IMAGE, used)):
        st, lens, _ = model.read_placed(base, offs, caps, what, None)
        assert not st.any() and lens.tolist() == sizes, what
    out = np.full(sum(used) + 7 * 64, 0x5A, np.uint8)
    st, po, lens, total, want = model.read_packed(base, offs, caps, model.IMAGE, out, align=64)
    assert not st.any() and int(total[0]) == sum((u + 63) // 64 * 64 for u in used)
    for i, f in enumerate(files):
        o = int(po[i])
        assert o % 64 == 0 and want[o:o + used[i]].tobytes() == f[:used[i]].tobytes(), SPECS[i]["name"]
        pad = want[o + used[i]:o + (used[i] + 63) // 64 * 64]
        assert (pad == 0x5A).all()
    assert (want[int(total[0]):] == 0x5A).all()


def test_model_agrees_with_the_host_chunk_layer(tmp_path):
    """ChunkFile.content, cioa_chunk_get_content_copy, cioa_meta_read and
    cioa_meta_cmp of this repo's host chunk layer on the same files."""
    lib = cf._bind()
    V, I = ctypes.c_void_p, ctypes.c_int
    lib.cioa_meta_read.restype, lib.cioa_meta_read.argtypes = I, [V, ctypes.POINTER(V), ctypes.POINTER(I)]
    lib.cioa_meta_cmp.restype, lib.cioa_meta_cmp.argtypes = I, [V, ctypes.c_char_p, I]
    lib.cioa_chunk_get_content_copy.restype = I
    lib.cioa_chunk_get_content_copy.argtypes = [V, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [V]
    files = [fixture(s["name"]) for s in SPECS]
    base, offs, caps = one_buffer(files)
    for i, s in enumerate(SPECS):
        d = tmp_path / s["name"] / MANIFEST["stream"]
        d.mkdir(parents=True)
        shutil.copyfile(os.path.join(GDIR, "files", s["name"]), d / s["name"])
        one = (offs[i:i + 1], caps[i:i + 1])
        with cf.Context(str(tmp_path / s["name"]), s["load_flags"]) as ctx:
            c, err = ctx.stream(MANIFEST["stream"]).open(s["name"], cf.CIO_OPEN)
            assert c is not None, (s["name"], err)
            # content, with cio_file_content_copy's terminator
            p, size = V(), ctypes.c_size_t()
            assert lib.cioa_chunk_get_content_copy(c._c(), ctypes.byref(p), ctypes.byref(size)) == 0
            host = ctypes.string_at(p.value, size.value + 1)
            libc.free(p)
            assert host[:-1] == c.content() and host[-1] == 0
            out = np.full(len(host) + 5, 0x77, np.uint8)
            st, lens, want = model.read_placed(base, *one, model.CONTENT, out, [2], [len(host)], flags=model.NUL)
            assert st[0] == 0 and int(lens[0]) == size.value == c.data_size
            assert want[2:2 + len(host)].tobytes() == host and (want[:2] == 0x77).all() and (want[-3:] == 0x77).all()
            # metadata
            st, lens, want = model.read_placed(base, *one, model.META, np.zeros(70000, np.uint8), [0], [70000])
            mp, ml = V(), I(-5)
            rc = lib.cioa_meta_read(c._c(), ctypes.byref(mp), ctypes.byref(ml))
            meta = want[:int(lens[0])].tobytes()
            assert int(lens[0]) == c.meta_len() == s["load"]["meta_size"]
            if meta:
                assert rc == 0 and ctypes.string_at(mp.value, ml.value) == meta
            else:
                assert rc == -1                   # cio_meta_read on empty metadata; the batch says OK, length 0
            # compare: equal, a changed byte, shorter, longer, empty
            cands = [meta, meta[:-1] + b"\xff" if meta else b"x", meta[:-1] if meta else b"xy", meta + b"z", b""]
            cbuf = np.frombuffer(b"".join(cands) + b"\0", np.uint8)
            co, _ = model.layout([len(x) for x in cands], [0] * len(cands))
            res, st = model.meta_cmp(base, np.repeat(one[0], 5), np.repeat(one[1], 5), cbuf, co,
                                     [len(x) for x in cands])
            assert not st.any()
            assert res.tolist() == [lib.cioa_meta_cmp(c._c(), x, len(x)) for x in cands], s["name"]
            assert res[0] == 0 and res[3] == -1
            c.close()


def test_placecheck():
    """The placement arithmetic on the host, every workgroup order, under
    ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "placecheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "place_check: ok" in r.stdout
