"""Chunk images in device memory down to chunk files and up again
(include/chunkio_amd/cio_persist_dev.h), without a GPU: the five symbols and
the Python exports exist with the declared prototypes, every argument check of
the three calls runs before any device call, the round planner agrees with the
Python model on seeded size lists (a file of exactly the maximum and one of a
byte more among them), the two host checks of the arithmetic (`make alloccheck
persistcheck`, stand-alone programs under ASan + UBSan) pass, and the alloc
model is held to pool_set_model.m_grow_set: "alloc with need = c" places as
"grow to new_cap = c" does."""
import ctypes
import os
import re
import subprocess

import numpy as np
import pytest

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import alloc_set_model as amodel
import persist_model as pmodel
from test_rotate_dev_abi import CTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALLOC, LOAD, STORE = "cio_file_alloc_set_batch_dev", "cio_file_load_paths_dev", "cio_file_store_paths_dev"
RMAX, ROUNDS, TRIM = "cio_file_persist_round_max", "cio_file_persist_rounds", "cio_file_persist_trim"


def declarations():
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_persist_dev.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M):
        types = []
        for a in ([] if args.strip() == "void" else args.split(",")):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (None if res == "void" else CTYPE[res], types)
    return out, raw


def alloc_args(writer, buf, n=1, n_cls=2, stride=4, align=16, flags=0):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n, buf, buf, buf, buf, n_cls, stride, align, flags, buf, buf, buf, buf, None]


def path_list(n, null_at=None):
    arr = (ctypes.c_char_p * max(n, 1))(*[b"/nonexistent/chunk%d" % i for i in range(n)])
    if null_at is not None:
        arr[null_at] = None
    return arr


def load_args(writer, buf, paths, n=1, flags=4, stage_bytes=4096, n_cls=2, stride=4, align=16):
    return [writer, buf, 64, ctypes.cast(paths, ctypes.c_void_p) if paths is not None else None, n, flags, buf,
            stage_bytes, buf, buf, buf, buf, n_cls, stride, align, buf, buf, buf, buf, buf, buf, buf, None]


def store_args(writer, buf, paths, n=1, flags=0, page=4096, stage_bytes=4096):
    return [writer, buf, 64, buf, buf, n, buf, ctypes.cast(paths, ctypes.c_void_p) if paths is not None else None,
            flags, page, buf, stage_bytes, buf, buf, buf, None]


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {ALLOC, LOAD, STORE, RMAX, ROUNDS, TRIM}
    for name, nargs in ((ALLOC, 19), (LOAD, 23), (STORE, 16), (RMAX, 1), (ROUNDS, 4), (TRIM, 0)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert '#include "cio_write_dev_pool_set.h"' in raw and '#include "cio_read_dev.h"' in raw
    for name, value in (("CIOA_ALLOC_ZERO", 1), ("CIOA_LOAD_ZERO", 512), ("CIOA_STORE_TRIM", 1), ("CIOA_STORE_SYNC", 2)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), raw) and getattr(cf, name) == value
    flat = " ".join(raw.replace("*", " ").split()).lower()
    for phrase in ("a fused verify + copy kernel", "peer-to-peer file i/o", "multi-gpu variants",
                   "device-side directory", "max_chunks_up budget", "lifecycle walk"):
        assert phrase in flat, phrase                 # what is out of scope is said in the header too


def test_python_binding_exports():
    for name in ("alloc_set_batch_dev", "load_paths_dev", "store_paths_dev", "persist_round_max", "persist_rounds",
                 "persist_trim",
                 "CIOA_ALLOC_ZERO", "CIOA_LOAD_ZERO", "CIOA_STORE_TRIM", "CIOA_STORE_SYNC"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)


def test_alloc_set_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, ALLOC)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # just a non-null address: refused before it is looked at
    err = lib.cio_gpu_last_error
    for n in (0, 1):                              # the values are checked first, an empty batch included
        for flags in (2, 4, 256, 3, 1 << 30, -1):
            assert fn(*alloc_args(writer, buf, n=n, flags=flags)) == -1, flags
            assert (ALLOC + ": unknown flags").encode() in err()
        for align in (0, 3, 48, 8192):
            assert fn(*alloc_args(writer, buf, n=n, align=align)) == -1
            assert (ALLOC + ": align must be a power of two in 1 .. 4096").encode() in err()
        for n_cls in (9, 1 << 40):
            assert fn(*alloc_args(writer, buf, n=n, n_cls=n_cls)) == -1
            assert (ALLOC + ": n_cls must be in 0 .. 8").encode() in err()
        assert fn(*alloc_args(writer, buf, n=n, stride=0)) == -1
        assert (ALLOC + ": stride must not be 0").encode() in err()
        assert fn(*alloc_args(None, buf, n=n)) == -1
        assert (ALLOC + ": null writer").encode() in err()
    # an empty batch is a no-op, whatever the pointers, with a set and without
    assert fn(*alloc_args(writer, buf, n=0)) == 0 and fn(*alloc_args(writer, buf, n=0, flags=1)) == 0
    assert fn(*[None if x is buf else x for x in alloc_args(writer, buf, n=0)]) == 0
    assert fn(*alloc_args(writer, buf, n=0, n_cls=0, stride=0)) == 0
    # null buffers are refused before the writer's capacity is looked at (the block stands in for a writer:
    # max_chunks, its first word, 4)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    full = alloc_args(writer, buf, n=5)
    for j in (1, 3, 6, 7, 8, 9, 14, 15, 16, 17):  # the set's three pointers among them
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert (ALLOC + ": null pointer").encode() in err(), j
    a = list(full)
    a[4] = None                                   # dev_gate may be null
    assert fn(*a) == -1 and (ALLOC + ": more entries than the writer").encode() in err()
    a = alloc_args(writer, buf, n=5, n_cls=0, stride=0)
    a[7] = a[8] = a[9] = None                     # no classes: the set's pointers may be null
    assert fn(*a) == -1 and (ALLOC + ": more entries than the writer").encode() in err()


def test_load_paths_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, LOAD)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    err = lib.cio_gpu_last_error
    paths = path_list(5)
    for n in (0, 1):
        for flags in (1, 2, 8, 64, 16, 256, 1024, -1):      # 1 is chunkio's CIO_OPEN: no flag of this call
            assert fn(*load_args(writer, buf, paths, n=n, flags=flags)) == -1, flags
            assert (LOAD + ": unknown flags").encode() in err()
        for align in (0, 3, 8192):
            assert fn(*load_args(writer, buf, paths, n=n, align=align)) == -1
            assert (LOAD + ": align must be a power of two in 1 .. 4096").encode() in err()
        for n_cls in (9, 1 << 40):
            assert fn(*load_args(writer, buf, paths, n=n, n_cls=n_cls)) == -1
            assert (LOAD + ": n_cls must be in 0 .. 8").encode() in err()
        assert fn(*load_args(writer, buf, paths, n=n, stride=0)) == -1
        assert (LOAD + ": stride must not be 0").encode() in err()
        assert fn(*load_args(None, buf, paths, n=n)) == -1
        assert (LOAD + ": null writer").encode() in err()
    for flags in (0, 512, 4, 516):
        assert fn(*load_args(writer, buf, paths, n=0, flags=flags)) == 0
    assert fn(*[None if x is buf else x for x in load_args(writer, buf, None, n=0)]) == 0
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    assert fn(*load_args(writer, buf, paths, n=5, stage_bytes=0)) == -1
    assert (LOAD + ": stage_bytes must not be 0").encode() in err()
    full = load_args(writer, buf, paths, n=5)
    for j in (1, 3, 6, 8, 9, 10, 11, 15, 16, 17, 18, 19, 20):
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert (LOAD + ": null pointer").encode() in err(), j
    a = list(full)
    a[21] = None                                  # fs_sizes may be null
    assert fn(*a) == -1 and (LOAD + ": more files than the writer").encode() in err()
    assert fn(*load_args(writer, buf, path_list(3, null_at=2), n=3)) == -1
    assert (LOAD + ": null path").encode() in err()


def test_store_paths_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, STORE)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    err = lib.cio_gpu_last_error
    paths = path_list(5)
    for n in (0, 1):
        for flags in (4, 8, 256, 7, -1):
            assert fn(*store_args(writer, buf, paths, n=n, flags=flags)) == -1, flags
            assert (STORE + ": unknown flags").encode() in err()
        for page in (0, 3, 96, 1 << 31, 1 << 63):
            assert fn(*store_args(writer, buf, paths, n=n, page=page)) == -1
            assert (STORE + ": page must be a power of two in 1 .. 2^30").encode() in err()
        assert fn(*store_args(None, buf, paths, n=n)) == -1
        assert (STORE + ": null writer").encode() in err()
    for flags in (0, 1, 2, 3):
        assert fn(*store_args(writer, buf, paths, n=0, flags=flags, page=1)) == 0
    assert fn(*[None if x is buf else x for x in store_args(writer, buf, None, n=0)]) == 0
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    assert fn(*store_args(writer, buf, paths, n=5, stage_bytes=0)) == -1
    assert (STORE + ": stage_bytes must not be 0").encode() in err()
    full = store_args(writer, buf, paths, n=5)
    for j in (1, 3, 4, 7, 10, 12, 14):
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert (STORE + ": null pointer").encode() in err(), j
    for j in (6, 13):                             # dev_gate and file_sizes may be null
        a = list(full)
        a[j] = None
        assert fn(*a) == -1 and (STORE + ": more images than the writer").encode() in err()
    assert fn(*store_args(writer, buf, path_list(3, null_at=0), n=3)) == -1
    assert (STORE + ": null path").encode() in err()


@pytest.mark.parametrize("seed", range(6))
def test_round_planner_agrees_with_the_model(seed):
    rng = np.random.default_rng(seed)
    for stage in (0, 1, 127, 128, 4096, 4100, 70000, int(rng.integers(1, 1 << 20))):
        mx = cf.persist_round_max(stage)
        assert mx == pmodel.m_round_max(stage) and mx <= stage < mx + 128
        for n in (0, 1, 7, 200):
            sizes = rng.integers(0, max(stage // 2, 2) + 300, n).astype(np.uint64)
            if n >= 7:
                sizes[2], sizes[4], sizes[5] = mx, mx + 1, 0      # exactly the maximum, and a byte more
            rounds, round_of = cf.persist_rounds(sizes, stage)
            want_rounds, want = pmodel.m_rounds(sizes, stage)
            assert rounds == want_rounds and np.array_equal(round_of, want), (stage, n)
            if n >= 7:
                assert round_of[4] == pmodel.NO_ROUND and (mx == 0 or round_of[2] != pmodel.NO_ROUND)
    lib = chunkio_amd.lib()
    assert lib.cio_file_persist_rounds(None, 0, 4096, None) == 0
    assert lib.cio_file_persist_rounds(None, 3, 4096, None) == -1
    assert b"cio_file_persist_rounds: null pointer" in lib.cio_gpu_last_error()


@pytest.mark.parametrize("target", ["alloccheck", "persistcheck"])
def test_host_checks(target):
    """alloc_set.h and persist_plan.h at every boundary of their rules against
    restatements in 128-bit arithmetic, under ASan + UBSan (stand-alone
    programs)."""
    r = subprocess.run(["make", "-C", ROOT, target], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "cases passed" in r.stdout


# ------------------------------------------------------------------ the model

def test_alloc_model_on_a_hand_written_batch():
    """Two classes, (64, 16) with two entries and (256, 16) with one, stride 2;
    arena [1024, 1400), align 16.  Needs: 23 no; 24 -> class 0, its top entry
    (304, cap 70); 64 -> class 0, entry (208, cap 64); 64 -> class 0 is dry:
    arena slot of 64 at 1024; 65 -> class 1, its entry lies outside the buffer:
    consumed, rejected; 200 -> class 1 dry: arena, 256 at 1088; gated off; 300
    -> no class: arena, 304 bytes at 1344 do not fit 1400: cut; 30 -> class 0
    dry: arena 64 at 1648 -- behind the cut, rejected too."""
    buf = np.full(2048, 0xA5, np.uint8)
    so, sc, words = [208, 304, 5000, 0], [64, 70, 256, 0], [2, 2, 64, 16, 1, 2, 256, 16]
    arena = [1024, 1400]
    need, gate = [23, 24, 64, 64, 65, 200, 64, 300, 30], [0, 0, 0, 0, 0, 0, -1, 0, 0]
    st, total, offs, caps = amodel.m_alloc_set(buf, need, gate, arena, so, sc, words, 2, 2, align=16)
    N = amodel.NONE
    assert st.tolist() == [-1, 0, 0, 0, -1, 0, -1, -1, -1]
    assert offs == [N, 304, 208, 1024, N, 1088, N, N, N] and caps == [0, 70, 64, 64, 0, 256, 0, 0, 0]
    assert total == [64 + 256 + 304 + 64, 3, 4, 2] and arena == [1344, 1400] and words[0] == 0 and words[4] == 0
    assert (buf == 0xA5).all()
    arena, words = [1024, 2048], [2, 2, 64, 16, 1, 2, 256, 16]
    st, total, offs, caps = amodel.m_alloc_set(buf, need, gate, arena, so, sc, words, 2, 2, align=16,
                                               flags=amodel.ALLOC_ZERO)
    assert st.tolist() == [-1, 0, 0, 0, -1, 0, -1, 0, 0] and offs[7:] == [1344, 1648] and arena[0] == 1712
    want = np.full(2048, 0xA5, np.uint8)
    for o, c in ((304, 70), (208, 64), (1024, 64), (1088, 256), (1344, 300), (1648, 64)):
        want[o:o + c] = 0
    assert np.array_equal(buf, want)


@pytest.mark.parametrize("seed", range(40))
def test_alloc_with_need_c_places_as_grow_to_new_cap_c(seed):
    """m_alloc_set against pool_set_model.m_grow_set over 24-byte images that
    grow to the same capacities: statuses, slots, totals, set words, the top."""
    rng = np.random.default_rng(100 + seed)
    n_cls = int(rng.integers(0, 5))
    stride, align = int(rng.integers(1, 5)), int(rng.choice([1, 16, 64]))
    classes = sorted(set(int(x) for x in rng.integers(25, 3000, n_cls)))
    n_cls = len(classes)
    dev_bytes = 1 << 17
    so, sc, words, at = [], [], [], 0
    for c in classes:
        have = int(rng.integers(0, stride + 1))
        words += [have, stride, c, int(rng.choice([16, 64, 128]))]
        for e in range(stride):
            bad = rng.integers(0, 9) == 0
            so.append(at + (1 if bad and e % 2 else 0))
            sc.append(c - 1 if bad and not e % 2 else c + int(rng.integers(0, 3)))
            at += (c + 2 + 127) // 128 * 128
    if n_cls and rng.integers(0, 8) == 0:
        words[1] = stride + 1                     # unsound: the plain grow, the arena alone
    top = at + int(rng.integers(0, 100))
    end = dev_bytes if rng.integers(0, 2) else top + int(rng.integers(0, 20000))
    n = int(rng.integers(0, 40))
    need = [int(rng.choice([0, 23, 25, int(rng.integers(25, 4000))] + [c + d for c in classes for d in (0, 1)]))
            for _ in range(n)]
    gate = None if rng.integers(0, 2) else [0 if rng.integers(0, 4) else -1 for _ in range(n)]
    a_arena, a_words = [top, end], list(words)
    got = amodel.m_alloc_set(np.zeros(dev_bytes, np.uint8), need, gate, a_arena, so, sc, a_words, n_cls, stride,
                             align=align)
    g_arena, g_words = [top, end], list(words)
    want = amodel.m_alloc_via_grow(need, gate, g_arena, list(so), list(sc), g_words, n_cls, stride, align, dev_bytes)
    assert got[0].tolist() == want[0].tolist() and got[2] == want[2] and got[3] == want[3]
    assert got[1] == want[1] and a_arena == g_arena and a_words == g_words
