"""Recycling drained chunk slots in device memory
(include/chunkio_amd/cio_write_dev_pool.h), without a GPU: the three symbols
and the Python exports exist with the declared prototypes, every argument
check runs before any device call, the host check of the kernels' arithmetic
(`make poolcheck`, a stand-alone program under ASan + UBSan) passes, the numpy
model the GPU tests compare against is asserted by hand on a batch of eight
entries, and with an empty or unusable pool its rotate is the rotate model's
output for output."""
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

import pool_dev_model as model
import rotate_dev_model as rmodel
from test_rotate_dev_abi import CTYPE, hand_batch
from write_dev_move_model import m_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, ROT, RECS = ("cio_file_release_batch_dev", "cio_file_rotate_pool_batch_dev",
                  "cio_file_rotate_pool_records_batch_dev")


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_pool.h")) as f:
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


def rel_args(writer, buf, n=1, flags=0, count=True, live=False):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, buf, n, buf if count else None, buf, buf if live else None, flags, buf, buf,
            buf, buf, buf, None]


def rot_args(writer, buf, n=1, limit=0, new_cap=24, align=16, flags=0):
    return [writer, buf, 64, buf, buf, n, buf, limit, new_cap, align, buf, buf, buf, buf, buf, buf, buf, buf, flags,
            buf, buf, buf, None]


def recs_args(writer, buf, n=1, n_rec=1, limit=0, new_cap=24, align=16, flags=0):
    return [writer, buf, 64, buf, buf, n, buf, buf, n_rec, limit, new_cap, align, buf, buf, buf, buf, buf, buf, buf,
            buf, flags, buf, buf, buf, None]


ROTS = ((ROT, rot_args), (RECS, recs_args))


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {REL, ROT, RECS}
    for name, nargs in ((REL, 17), (ROT, 23), (RECS, 25)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert '#include "cio_write_dev.h"' in raw
    assert re.search(r"#define\s+CIOA_RELEASE_ZERO\s+1\b", raw) and re.search(r"#define\s+CIOA_RELEASE_COMPACT\s+2\b", raw)
    assert (cf.CIOA_RELEASE_ZERO, cf.CIOA_RELEASE_COMPACT) == (1, 2)
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "preconditions, not checked" in flat and "the pool's entries are trusted" in flat
    assert "grow keeps taking from the arena" in flat and "not here: grow taking from the pool" in flat
    # the pool variant differs from rotate's prototypes by the three pool pointers behind dev_arena
    for name, plain in ((ROT, "cio_file_rotate_batch_dev"), (RECS, "cio_file_rotate_records_batch_dev")):
        args = list(getattr(lib, name).argtypes)
        at = 11 if name == ROT else 13
        assert args[:at] + args[at + 3:] == list(getattr(lib, plain).argtypes), name


def test_python_binding_exports():
    for name in ("pool_state", "release_batch_dev", "rotate_pool_batch_dev", "rotate_pool_records_batch_dev"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)
    p = inspect.signature(cf.release_batch_dev).parameters
    assert list(p) == ["writer", "base", "offs", "caps", "pool_offs", "pool_caps", "pool", "img", "count", "gate",
                       "live_offs", "flags", "total", "status", "stream"]
    assert p["flags"].default == 0 and all(p[k].default is None for k in ("img", "count", "gate", "live_offs"))
    q = inspect.signature(cf.rotate_pool_batch_dev).parameters
    r = inspect.signature(cf.rotate_batch_dev).parameters
    assert [k for k in q if not k.startswith("pool")] == list(r)
    assert list(q)[list(q).index("arena") + 1:][:3] == ["pool_offs", "pool_caps", "pool"]
    q = inspect.signature(cf.rotate_pool_records_batch_dev).parameters
    r = inspect.signature(cf.rotate_records_batch_dev).parameters
    assert [k for k in q if not k.startswith("pool")] == list(r)
    assert list(inspect.signature(cf.pool_state).parameters) == ["capacity", "cls", "align", "device"]


def test_release_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, REL)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # just a non-null address: refused before it is looked at
    err = lib.cio_gpu_last_error
    for flags in (4, 8, 256, 7, 1 << 30, -1):
        assert fn(*rel_args(writer, buf, flags=flags)) == -1, flags
        assert (REL + ": unknown flags").encode() in err()
    for flags in (2, 3):
        for n in (0, 1):                          # the values are checked first, an empty batch included
            assert fn(*rel_args(writer, buf, n=n, flags=flags, count=False)) == -1
            assert b"CIOA_RELEASE_COMPACT needs dev_count" in err()
            assert fn(*rel_args(writer, buf, n=n, flags=flags, live=True)) == -1
            assert b"CIOA_RELEASE_COMPACT does not go with dev_live_offs" in err()
    for n in (0, 1):
        assert fn(*rel_args(None, buf, n=n)) == -1
        assert (REL + ": null writer").encode() in err()
    # null buffers are refused before the writer is looked at; then the writer's capacity (the block stands in
    # for a writer: max_chunks, its first word, 4, everything else zero)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    for flags in (0, 1, 2, 3):
        full = rel_args(writer, buf, n=5, flags=flags)
        for j in (1, 3, 4, 11, 12, 13, 14, 15):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (REL + ": null pointer").encode() in err(), j
        for j in (5, 8, 9) + (() if flags & 2 else (7,)):      # dev_img, dev_gate, dev_live_offs, dev_count
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (REL + ": more entries than the writer").encode() in err(), j
        assert fn(*full) == -1
        assert (REL + ": more entries than the writer").encode() in err()
    # an empty batch is a no-op, whatever the pointers
    writer = ctypes.create_string_buffer(1024)
    assert fn(*rel_args(writer, buf, n=0)) == 0 and fn(*rel_args(writer, buf, n=0, flags=3)) == 0
    assert fn(*[None if x is buf else x for x in rel_args(writer, buf, n=0)]) == 0


@pytest.mark.parametrize("name,make", ROTS)
def test_rotate_pool_refuses_bad_arguments_without_a_gpu(name, make):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    err = lib.cio_gpu_last_error
    for flags in (1, 2, 8, 256, 5, -1):
        assert fn(*make(writer, buf, flags=flags)) == -1, flags
        assert (name + ": unknown flags").encode() in err()
    for new_cap in (0, 23):
        assert fn(*make(writer, buf, new_cap=new_cap)) == -1
        assert (name + ": new_cap must be at least 24").encode() in err()
    for align in (0, 3, 8192):
        assert fn(*make(writer, buf, align=align)) == -1
        assert (name + ": align must be a power of two in 1 .. 4096").encode() in err()
    assert fn(*make(writer, buf, n=0, flags=2)) == -1 and fn(*make(writer, buf, n=0, new_cap=23)) == -1
    for n in (0, 1):
        assert fn(*make(None, buf, n=n)) == -1
        assert (name + ": null writer").encode() in err()
    assert fn(*make(writer, buf, n=0)) == 0
    assert fn(*[None if x is buf else x for x in make(writer, buf, n=0)]) == 0
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=7, n_rec=0)) == 0
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(8)), 4)
    pool_at = (11, 12, 13) if name == ROT else (13, 14, 15)
    required = ((1, 3, 4, 10, 14, 15, 16, 17, 20, 21) if name == ROT else (1, 3, 4, 6, 7, 12, 16, 17, 18, 19, 22, 23))
    full = make(writer, buf, n=5, flags=0)
    for j in required + pool_at:
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert (name + ": null pointer").encode() in err(), j
    full = make(writer, buf, n=9)
    assert fn(*full) == -1
    assert (name + ": more images than the writer").encode() in err()


def test_poolcheck():
    """Both chains on the host, every workgroup order, against a sequential
    loop in 128-bit arithmetic, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "poolcheck"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pool_check: ok" in r.stdout


# ------------------------------------------------------------------ the model, by hand

def release_batch():
    """Eight slots of 64 bytes at 0, 64, .. 448 in a pool of class 48 and
    alignment 32: 0 releasable; 1 gate-failed; 2 still live; 3 bad magic; 4
    capacity 47; 5 at an odd multiple of 16; 6 and 7 releasable.  Returns (buf,
    offs, caps, img, gate, live)."""
    buf = np.full(600, 0xA5, np.uint8)
    offs, caps = [64 * i for i in range(8)], [64] * 8
    caps[4] = 47
    offs[5] += 16
    for i in range(8):
        m_init(buf, offs[i], b"xy")
        buf[offs[i] + 13] = 5
    buf[offs[3] + 1] = 0x01
    gate = [0, -3, 0, 0, 0, 0, 0, 0]
    live = [7, 7, 128, 7, 7, 7, 7, 7]
    return buf, offs, caps, list(range(20, 28)), gate, live


def test_release_model_on_a_hand_written_batch():
    buf, offs, caps, img, gate, live = release_batch()
    before = buf.copy()
    po, pc, pool = [9] * 4, [9] * 4, [1, 3, 48, 32]           # room for two entries
    st, total, acc = model.m_release(buf, offs, caps, img, None, gate, live, 0, po, pc, pool)
    # 0, 6 and 7 reach the placement; the pool takes two of them
    assert st.tolist() == [0, -1, 0, -1, -1, -1, 0, -1] and acc == [0, 6] and total == [3, 6]
    assert po == [9, 0, 384, 9] and pc == [9, 64, 64, 9] and pool == [3, 3, 48, 32]
    want = before.copy()
    want[0:2] = 0
    want[384:386] = 0
    assert np.array_equal(buf, want) and offs[5] == 336 and img == list(range(20, 28))
    # again: 0 and 6 have no magic any more, 7 is cut again by the full pool; nothing changes
    st, total, acc = model.m_release(buf, offs, caps, img, None, gate, live, 0, po, pc, pool)
    assert st.tolist() == [-1, -1, 0, -1, -1, -1, -1, -1] and acc == [] and total == [1, 8]
    assert np.array_equal(buf, want) and pool == [3, 3, 48, 32]


def test_release_model_zero_and_compact():
    buf, offs, caps, img, gate, live = release_batch()
    before = buf.copy()
    po, pc, pool, count = [9] * 8, [9] * 8, [0, 8, 48, 32], [7, 8]
    st, total, acc = model.m_release(buf, offs, caps, img, count, gate, None, 3, po, pc, pool)
    # without dev_live_offs entry 2 is releasable; entry 7 lies beyond the count and is not looked at
    assert st.tolist() == [0, -1, 0, -1, -1, -1, 0, 0] and acc == [0, 2, 6] and total == [3, 4]
    assert offs == [64, 192, 256, 336, 0, 0, 0, 448] and caps == [64, 64, 47, 64, 0, 0, 0, 64]
    assert img == [21, 23, 24, 25] + [model.NO_IMAGE] * 3 + [27] and count == [4, 8]
    assert po[:3] == [0, 128, 384] and pool == [3, 8, 48, 32]
    want = before.copy()
    for o in (0, 128, 384):
        want[o:o + 64] = 0
    assert np.array_equal(buf, want)
    # an unsound pool: every entry that gets as far as the pool is refused, and nothing is written
    buf, offs, caps, img, gate, live = release_batch()
    for words in ([4, 3, 48, 32], [0, 8, 23, 32], [0, 8, 48, 48], [0, 8, 48, 8192]):
        st, total, acc = model.m_release(buf, offs, caps, img, None, gate, live, 1, po, pc, list(words))
        assert st.tolist() == [-1, -1, 0, -1, -1, -1, -1, -1] and acc == [] and total == [0, 8]
    assert np.array_equal(buf, before)


def test_rotate_pool_model_on_the_hand_written_batch():
    """test_rotate_dev_abi's batch: 2, 3 and 7 reach the placement.  With two
    pool entries 2 and 3 take them, last pushed first, with the entries' whole
    capacities, and 7 takes the arena's first slot."""
    buf, offs, caps, need, crc = hand_batch()
    buf = np.concatenate([buf, np.full(512, 0xA5, np.uint8)])
    arena = [1001, 1008 + 64]
    lo, lc, li, count = [7] * 8, [7] * 8, [7] * 8, [1, 8]
    po, pc, pool = [2048, 2176, 9], [100, 72, 9], [2, 3, 64, 8]
    st, total, rot, fp = model.m_rotate_pool(buf, offs, caps, need, 40, 64, 8, arena, lo, lc, li, count, po, pc, pool,
                                             crc_cur=crc)
    assert st.tolist() == [-1, 0, 0, 0, 0, -1, -1, 0] and rot == [2, 3, 7] and fp == 2 and total == [7 + 64, 3]
    assert offs == [0, 100, 2176, 2048, 400, 500, 600, 1008] and caps == [80, 80, 72, 100, 80, 80, 80, 64]
    assert arena == [1072, 1072] and count == [4, 8] and pool == [0, 3, 64, 8] and li[1:4] == [2, 3, 7]
    assert lo[1:4] == [200, 300, 700] and po == [2048, 2176, 9]
    raw = m_init(np.zeros(64, np.uint8), 0, b"tag!")
    assert crc[2] == crc[3] == crc[7] == raw and bytes(buf[2176:2176 + 28]) == bytes(buf[1008:1008 + 28])


@pytest.mark.parametrize("words", [[0, 3, 64, 8], [2, 3, 63, 8], [2, 3, 64, 4], [4, 3, 64, 8], [2, 3, 64, 24],
                                   [2, 3, 20, 8]])
@pytest.mark.parametrize("flags,limit", [(4, 40), (0, 40), (4, 0)])
def test_rotate_pool_model_with_an_unusable_pool_is_the_rotate_model(words, flags, limit):
    """An empty pool, a class below new_cap, an alignment that is no multiple of
    align, and unsound words: m_rotate_pool equals m_rotate output for output,
    and the pool is not written."""
    a, b = hand_batch(), hand_batch()
    arena_a, arena_b = [1001, 1199], [1001, 1199]
    la, lb = ([7] * 8, [7] * 8, [7] * 8, [1, 3]), ([7] * 8, [7] * 8, [7] * 8, [1, 3])
    po, pc, pool = [1500, 1600, 9], [64, 64, 9], list(words)
    got = model.m_rotate_pool(a[0], a[1], a[2], a[3], limit, 64, 8, arena_a, *la, po, pc, pool, flags=flags,
                              crc_cur=a[4])
    want = rmodel.m_rotate(b[0], b[1], b[2], b[3], limit, 64, 8, arena_b, *lb, flags=flags, crc_cur=b[4])
    assert np.array_equal(got[0], want[0]) and got[1] == want[1] and got[2] == want[2] and got[3] == 0
    assert len(want[2]) > 0 and want[0].any()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and a[4] == b[4] and arena_a == arena_b
    assert la == lb and (po, pc, pool) == ([1500, 1600, 9], [64, 64, 9], list(words))
    # the malformed list of the records variant
    got = model.m_rotate_pool(a[0], a[1], a[2], None, limit, 64, 8, arena_a, *la, po, pc, pool, crc_cur=a[4])
    assert got[0].tolist() == [-1] * 8 and got[1:] == ([0, 0], [], 0)
