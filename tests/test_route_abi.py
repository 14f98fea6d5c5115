"""Routing records to chunk images by their metadata
(include/chunkio_amd/cio_route_dev.h), without a GPU: the two symbols and the
Python exports exist with the declared prototypes, every argument check runs
before any device call and names its reason, the header states its rules, the
host check of the kernels' arithmetic (`make routecheck`, a stand-alone program
under ASan + UBSan) passes, the numpy model the GPU tests compare against is
asserted by hand, and the helper that makes colliding tags is checked against
zlib."""
import ctypes
import inspect
import os
import re
import subprocess
import zlib

import numpy as np

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import route_model as model
from read_dev_model import layout, make_image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BUILD, ROUTE = "cio_file_route_build_dev", "cio_file_route_records_batch_dev"
CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def header():
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_route_dev.h")) as f:
        return f.read()


def build_args(writer, buf, n_img=1):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused before that)."""
    return [writer, buf, 64, buf, buf, n_img, buf, buf, buf, None]


def route_args(writer, buf, n_img=1, n_rec=1, flags=0, tag_bytes=64):
    return [writer, buf, 64, buf, buf, n_img, None, buf, buf, buf, buf, tag_bytes, buf, buf, n_rec, 7, flags, buf, buf,
            None, buf, None]


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    raw = header()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    found = re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M)
    assert [name for _, name, _ in found] == [BUILD, ROUTE]
    for (res, name, arglist), count in zip(found, (10, 22)):
        types = []
        for a in arglist.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is CTYPE[res]
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == types and len(types) == count, name
    assert '#include "cio_write_dev_ungrouped.h"' in raw
    assert re.search(r"#ifndef CIO_RETRY\s+#define\s+CIO_RETRY\s+-2\b", raw)
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cioa_chunk.h")) as f:
        assert re.search(r"#define\s+CIO_RETRY\s+-2\b", f.read())
    assert cf.CIO_RETRY == model.RETRY == -2 and cf.CIO_ERROR == model.ERROR == -1 and cf.CIO_OK == model.OK == 0
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_ungrouped.h")) as f:
        assert "cio_route_dev.h" in f.read()      # the header whose dev_rec_img this produces points here
    # the measurement hooks are exported, and not declared in any public header
    for hook in ("cioa_debug_route_build_events", "cioa_debug_route_records_events"):
        assert hasattr(lib, hook)
        for h in os.listdir(os.path.join(ROOT, "include", "chunkio_amd")):
            with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
                assert hook not in f.read(), h


def test_header_states_the_rules_and_what_is_not_here():
    flat = " ".join(header().replace("*", " ").split()).lower()
    for rule in ("r0. key.", "r1. build.", "r2. a well-formed tag.", "r3. candidates.", "r4. match.", "r5. outputs.",
                 "r6. a stale or damaged directory can only lose matches.", "r7. a directory of another size.",
                 "r8. empty batches."):
        assert rule in flat, rule
    assert "raw crc-32 state" in flat and "dev_seeds == null" in flat and "stable sort of (key_i, i)" in flat
    assert "no load leaves the arrays" in flat and "an entry >= n_img is skipped" in flat
    assert "neither call writes a byte of the image buffer" in flat
    for gap in ("not here: opening chunks for the missed tags", "de-duplicated first",
                "a per-image count of the routed records", "prefix or wildcard matching",
                "incremental updates of a directory", "multi-gpu"):
        assert gap in flat, gap


def test_python_binding_exports():
    for name in ("route_dir", "route_build_dev", "route_records_batch_dev"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)
    assert list(inspect.signature(cf.route_dir).parameters) == ["n_img", "device"]
    assert list(inspect.signature(cf.route_build_dev).parameters) == ["writer", "base", "offs", "caps", "dir",
                                                                     "stream"]
    p = inspect.signature(cf.route_records_batch_dev).parameters
    assert list(p) == ["writer", "base", "offs", "caps", "dir", "tags", "tag_offs", "tag_lens", "miss_img", "gate",
                       "miss_list", "flags", "stream"]
    assert p["gate"].default is None and p["miss_list"].default is False and p["flags"].default == 0
    assert p["stream"].default is None


def test_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    build, route = getattr(lib, BUILD), getattr(lib, ROUTE)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # a non-null address; max_chunks, its first word, is set below
    err = lib.cio_gpu_last_error
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(32)), 4)

    def refused(fn, name, a, why):
        assert fn(*a) == -1, (name, why)
        assert (name + ": " + why).encode() in err(), (name, why, err())

    for flags in (1, 2, 4, 256, 1 << 30, -1):
        refused(route, ROUTE, route_args(writer, buf, flags=flags), "unknown flags")
        refused(route, ROUTE, route_args(None, None, flags=flags), "unknown flags")     # before anything else
    refused(build, BUILD, build_args(None, buf), "null writer")
    refused(route, ROUTE, route_args(None, buf), "null writer")
    refused(route, ROUTE, route_args(None, buf, n_rec=0), "null writer")
    for n_img in (2 ** 32 - 1, 2 ** 32, 2 ** 40, 2 ** 64 - 1):
        refused(build, BUILD, build_args(writer, buf, n_img), "n_img must be below 2^32 - 1")
        refused(route, ROUTE, route_args(writer, buf, n_img), "n_img must be below 2^32 - 1")
    for n_img in (33, 1000, 2 ** 32 - 2):         # the scratch is sized by the writer's max_chunks (32 here)
        refused(build, BUILD, build_args(writer, buf, n_img), "more images than the writer was created for")
        refused(route, ROUTE, route_args(writer, buf, n_img), "more images than the writer was created for")
    for n_rec in (33, 2 ** 32, 2 ** 64 - 1):
        refused(route, ROUTE, route_args(writer, buf, n_rec=n_rec), "more records than the writer was created for")
    for at in (1, 3, 4, 6, 7, 8):                 # dev_base, the image arrays, the three directory arrays
        a = build_args(writer, buf)
        a[at] = None
        refused(build, BUILD, a, "null pointer")
    for at in (1, 3, 4, 7, 8, 9, 10, 12, 13, 17, 18, 20):
        a = route_args(writer, buf)               # ... the tags and their geometry, rec_img, rec_status, dev_total
        a[at] = None
        refused(route, ROUTE, a, "null pointer")
    # the header is wanted even without an image; the image and directory arrays are not
    a = build_args(writer, None, n_img=0)
    refused(build, BUILD, a, "null pointer")
    a = route_args(writer, buf, n_img=0)
    a[9] = None
    refused(route, ROUTE, a, "null pointer")
    # an empty batch is a no-op once the writer, the counts and the directory's pointers are accepted
    a = route_args(writer, buf, n_rec=0)
    for at in (10, 12, 13, 17, 18, 19, 20):
        a[at] = None
    assert route(*a) == 0
    a = route_args(writer, buf, n_img=0, n_rec=0)
    for at in (1, 3, 4, 7, 8):
        a[at] = None
    assert route(*a) == 0


def test_host_check_of_the_kernels_arithmetic_passes():
    r = subprocess.run(["make", "-C", ROOT, "routecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "route_check: ok" in r.stdout


def test_model_by_hand():
    """Seven images: 0 and 3 share the metadata b"alpha", 1 and 5 have none, 2
    fails the image check (its magic is gone) over the bytes b"alpha", 4 holds
    b"beta" and is gated off in the second call, 6 holds b"alphabet".  Nine
    tags: one per case, a tag nobody has, and three malformed ones."""
    metas = [b"alpha", b"", b"alpha", b"alpha", b"beta", b"", b"alphabet"]
    caps = np.asarray([24 + len(m) + 5 + i for i, m in enumerate(metas)], np.uint64)
    offs, end = layout(caps, [3] * len(metas))
    base = np.full(end + 7, 0xEE, np.uint8)
    for o, m in zip(offs, metas):
        make_image(base, int(o), m, b"xyz")
    base[int(offs[2])] = 0xC0
    tags = np.frombuffer(b"?alpha?beta?alphabet?gamma", np.uint8)
    #        alpha  ""   beta alphabet gamma  alph  len 65536  beyond  wraps
    t_offs = [1,    999, 7,   12,      21,    1,    0,         22,     2 ** 64 - 2]
    t_lens = [5,    0,   4,   8,       5,     4,    65536,     5,      5]
    k, d, hdr = model.build(base, offs, caps)
    e, a, b, ab = 0xFFFFFFFF, model.key(b"alpha"), model.key(b"beta"), model.key(b"alphabet")
    assert a == ~zlib.crc32(b"alpha") & 0xFFFFFFFF and model.key(b"") == e == model.EMPTY_KEY
    want = sorted([(a, 0), (e, 1), (e, 2), (a, 3), (b, 4), (e, 5), (ab, 6)])
    assert list(zip(k.tolist(), d.tolist())) == want and hdr.tolist() == [7, 6, 0, 0]
    img, st, total, miss = model.route(base, offs, caps, tags, t_offs, t_lens, 77)
    assert img.tolist() == [0, 1, 4, 6, 77, 77, 77, 77, 77]
    assert st.tolist() == [0, 0, 0, 0, -2, -2, -1, -1, -1] and total.tolist() == [4, 2, 3] and miss.tolist() == [4, 5]
    model.judge(base, offs, caps, tags, t_offs, t_lens, img, st)
    # gates: with 0 gated off the duplicate 3 wins, never the failing 2; with 1 off the other empty one; 4 has no second
    gate = np.asarray([-1, -1, 0, 0, -3, 0, 0], np.int32)
    img, st, total, miss = model.route(base, offs, caps, tags, t_offs, t_lens, 7, gate=gate)
    assert img.tolist() == [3, 5, 7, 6, 7, 7, 7, 7, 7]
    assert st.tolist() == [0, 0, -2, 0, -2, -2, -1, -1, -1] and total.tolist() == [3, 3, 3]
    assert miss.tolist() == [2, 4, 5]
    model.judge(base, offs, caps, tags, t_offs, t_lens, img, st, gate=gate)
    # R7: a directory of another size; R8: no image, every well-formed record misses
    img, st, total, miss = model.route(base, offs, caps, tags, t_offs, t_lens, 9, dir_n=6)
    assert set(img.tolist()) == {9} and set(st.tolist()) == {-1} and total.tolist() == [0, 0, 9] and len(miss) == 0
    img, st, total, miss = model.route(base, offs[:0], caps[:0], tags, t_offs, t_lens, 0)
    assert set(img.tolist()) == {0} and st.tolist() == [-2] * 6 + [-1] * 3 and total.tolist() == [0, 6, 3]
    # a tag buffer of no bytes: only empty tags are well-formed
    img, st, total, _ = model.route(base, offs, caps, None, [0, 5, 0], [0, 0, 1], 9)
    assert img.tolist() == [1, 1, 9] and st.tolist() == [0, 0, -1]


def test_collision_helper_against_zlib():
    rng = np.random.default_rng(5)
    for target in (0, 0xFFFFFFFF, 1, 0x80000000, 0xDEADBEEF, model.key(b"some metadata")):
        # equal lengths, different lengths, the empty prefix
        prefixes = [b"", b"a", b"b", b"ab", b"stream-7/tag", bytes(rng.integers(0, 256, 61, dtype=np.uint8)),
                    bytes(rng.integers(0, 256, 61, dtype=np.uint8)), bytes(1021)]
        made = model.colliding(prefixes, target)
        assert len(set(made)) == len(made)
        for p, s in zip(prefixes, made):
            assert s[:len(p)] == p and len(s) == len(p) + 4
            assert ~zlib.crc32(s) & 0xFFFFFFFF == target == model.key(s), (p, target)
    # a pair of equal length and a pair of different length under the key of a string that exists
    k = model.key(b"tag.one")
    x, y, z = model.colliding([b"aaa", b"bbb", b"a-longer-prefix"], k)
    assert len(x) == len(y) == 7 != len(z) and len({x, y, z, b"tag.one"}) == 4
    assert model.key(x) == model.key(y) == model.key(z) == k
    # pack_tags: odd offsets, the bytes where it says
    buf, offs, lens = model.pack_tags([x, b"", z, y])
    assert all(int(o) % 2 == 1 for o in offs) and lens.tolist() == [7, 0, 19, 7]
    assert bytes(buf[int(offs[2]):int(offs[2]) + 19]) == z
