"""The size-classed pool set in device memory
(include/chunkio_amd/cio_write_dev_pool_set.h), without a GPU: the three
symbols and the Python exports exist with the declared prototypes, every
argument check runs before any device call, the host check of the kernels'
arithmetic (`make poolsetcheck`, a stand-alone program under ASan + UBSan)
passes, the numpy model the GPU tests compare against is asserted by hand on
one release batch and one grow batch, with one class its release is
pool_dev_model.m_release and without a usable class its grow is
grow_dev_model.m_grow, and the steady-state shape the GPU test replays is fixed
here on the model alone."""
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

import grow_dev_model as gmodel
import pool_dev_model as pmodel
import pool_set_model as model
from test_rotate_dev_abi import CTYPE
from write_dev_move_model import m_init

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REL, GROW, RECS = ("cio_file_release_set_batch_dev", "cio_file_grow_set_batch_dev",
                   "cio_file_grow_set_records_batch_dev")


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_pool_set.h")) as f:
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


def rel_args(writer, buf, n=1, flags=0, count=True, live=False, n_cls=2, stride=4):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, buf, n, buf if count else None, buf, buf if live else None, flags, buf, buf,
            buf, n_cls, stride, buf, buf, None]


def grow_args(writer, buf, n=1, realloc=64, page=64, align=16, flags=0, n_cls=2, stride=4):
    return [writer, buf, 64, buf, buf, n, buf, buf, buf, buf, buf, n_cls, stride, realloc, page, align, flags, buf,
            buf, buf, buf, None]


def recs_args(writer, buf, n=1, n_rec=1, realloc=64, page=64, align=16, flags=0, n_cls=2, stride=4):
    return [writer, buf, 64, buf, buf, n, buf, buf, n_rec, buf, buf, buf, buf, n_cls, stride, realloc, page, align,
            flags, buf, buf, buf, buf, None]


GROWS = ((GROW, grow_args), (RECS, recs_args))


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {REL, GROW, RECS}
    for name, nargs in ((REL, 19), (GROW, 22), (RECS, 24)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert '#include "cio_write_dev_pool.h"' in raw and '#include "cio_write_dev_grow.h"' in raw
    assert re.search(r"#define\s+CIOA_POOL_SET_MAX\s+8\b", raw) and cf.CIOA_POOL_SET_MAX == model.SET_MAX == 8
    flat = " ".join(raw.replace("*", " ").split()).lower()
    assert "it needs no set variant" in flat and "with its whole capacity" in flat
    assert "not here: spilling to the next class" in flat and "coalescing adjacent free slots" in flat
    assert "duplicate entries within one release" in flat
    # the set stands where the pool stood (release) and behind dev_arena (grow): five arguments for three, or inserted
    args = list(getattr(lib, REL).argtypes)
    plain = list(lib.cio_file_release_batch_dev.argtypes)
    assert args[:11] == plain[:11] and args[16:] == plain[14:]
    for name, other, at in ((GROW, "cio_file_grow_batch_dev", 8), (RECS, "cio_file_grow_records_batch_dev", 10)):
        args = list(getattr(lib, name).argtypes)
        assert args[:at] + args[at + 5:] == list(getattr(lib, other).argtypes), name
    # the two older headers point here, in comments only
    for h in ("cio_write_dev_pool.h", "cio_write_dev_grow.h"):
        with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
            assert "cio_write_dev_pool_set.h" in f.read()


def test_python_binding_exports():
    for name in ("pool_set_state", "pool_set_class", "release_set_batch_dev", "grow_set_batch_dev",
                 "grow_set_records_batch_dev", "CIOA_POOL_SET_MAX"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)
    assert list(inspect.signature(cf.pool_set_state).parameters) == ["classes", "stride", "device"]
    assert list(inspect.signature(cf.pool_set_class).parameters) == ["set", "k"]
    p = inspect.signature(cf.release_set_batch_dev).parameters
    q = inspect.signature(cf.release_batch_dev).parameters
    assert [k for k in p if k != "set"] == [k for k in q if not k.startswith("pool")]
    assert list(p)[4] == "set"
    for one, other in ((cf.grow_set_batch_dev, cf.grow_batch_dev), (cf.grow_set_records_batch_dev,
                                                                    cf.grow_records_batch_dev)):
        p, q = inspect.signature(one).parameters, inspect.signature(other).parameters
        assert [k for k in p if k != "set"] == list(q)
        assert list(p)[list(p).index("arena") + 1] == "set"
    with pytest.raises(ValueError):
        cf.pool_set_state([], 4, "cpu")
    with pytest.raises(ValueError):
        cf.pool_set_state([(64, 16)] * 9, 4, "cpu")


def test_release_set_refuses_bad_arguments_without_a_gpu():
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
        for n_cls in (0, 9, 1 << 40):
            assert fn(*rel_args(writer, buf, n=n, n_cls=n_cls)) == -1
            assert (REL + ": n_cls must be in 1 .. 8").encode() in err()
        assert fn(*rel_args(writer, buf, n=n, stride=0)) == -1
        assert (REL + ": stride must not be 0").encode() in err()
        assert fn(*rel_args(None, buf, n=n)) == -1
        assert (REL + ": null writer").encode() in err()
    # null buffers are refused before the writer is looked at; then the writer's capacity (the block stands in
    # for a writer: max_chunks, its first word, 4, everything else zero)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    for flags in (0, 1, 2, 3):
        full = rel_args(writer, buf, n=5, flags=flags)
        for j in (1, 3, 4, 11, 12, 13, 16, 17):   # the set's three pointers among them
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (REL + ": null pointer").encode() in err(), j
        for j in (5, 8, 9) + (() if flags & 2 else (7,)):      # dev_img, dev_gate, dev_live_offs, dev_count
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (REL + ": more entries than the writer").encode() in err(), j
    for n_cls in (1, 8):
        assert fn(*rel_args(writer, buf, n=5, n_cls=n_cls)) == -1
        assert (REL + ": more entries than the writer").encode() in err()
    # an empty batch is a no-op, whatever the pointers
    writer = ctypes.create_string_buffer(1024)
    assert fn(*rel_args(writer, buf, n=0)) == 0 and fn(*rel_args(writer, buf, n=0, flags=3)) == 0
    assert fn(*[None if x is buf else x for x in rel_args(writer, buf, n=0)]) == 0


@pytest.mark.parametrize("name,make", GROWS)
def test_grow_set_refuses_bad_arguments_without_a_gpu(name, make):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)
    err = lib.cio_gpu_last_error
    for flags in (2, 8, 256, 3, -1):
        assert fn(*make(writer, buf, flags=flags)) == -1, flags
        assert (name + ": unknown flags").encode() in err()
    assert fn(*make(writer, buf, realloc=0)) == -1 and (name + ": realloc_size must not be 0").encode() in err()
    for page in (0, 3, 96):
        assert fn(*make(writer, buf, page=page)) == -1 and (name + ": page must be a power of two").encode() in err()
    for align in (0, 3, 8192):
        assert fn(*make(writer, buf, align=align)) == -1
        assert (name + ": align must be a power of two in 1 .. 4096").encode() in err()
    prev = 17 if name == GROW else 19
    a = make(writer, buf)
    a[prev] = None
    assert fn(*a) == -1 and (name + ": dev_prev_offs and dev_prev_caps go together").encode() in err()
    for n in (0, 1):                              # the values are checked first, an empty batch included
        for n_cls in (0, 9, 1 << 40):
            assert fn(*make(writer, buf, n=n, n_cls=n_cls)) == -1
            assert (name + ": n_cls must be in 1 .. 8").encode() in err()
        assert fn(*make(writer, buf, n=n, stride=0)) == -1
        assert (name + ": stride must not be 0").encode() in err()
        assert fn(*make(None, buf, n=n)) == -1
        assert (name + ": null writer").encode() in err()
    assert fn(*make(writer, buf, n=0)) == 0
    assert fn(*[None if x is buf else x for x in make(writer, buf, n=0)]) == 0
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=7, n_rec=0)) == 0
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(8)), 4)
    required = (1, 3, 4, 6, 7, 19, 20) if name == GROW else (1, 3, 4, 6, 7, 9, 21, 22)
    set_at = (8, 9, 10) if name == GROW else (10, 11, 12)
    full = make(writer, buf, n=5)
    for j in required + set_at:
        a = list(full)
        a[j] = None
        assert fn(*a) == -1, j
        assert (name + ": null pointer").encode() in err(), j
    assert fn(*make(writer, buf, n=9)) == -1
    assert (name + ": more images than the writer").encode() in err()
    if name == RECS:
        assert fn(*recs_args(writer, buf, n=5, n_rec=9)) == -1
        assert (name + ": more records than the writer").encode() in err()


def test_poolsetcheck():
    """Both chains on the host, every workgroup order, the ballots over 64
    explicit lanes, against a sequential loop in 128-bit arithmetic, under ASan
    + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "poolsetcheck"], capture_output=True, text=True, timeout=1800)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "pool_set_check: ok" in r.stdout


# ------------------------------------------------------------------ the model, by hand

def image(buf, off, content=5):
    m_init(buf, off, b"xy")
    buf[off + 13] = content


def test_release_set_model_on_a_hand_written_batch():
    """Two classes, (48, 32) with one entry and room for one more, (96, 64)
    empty with room for two.  Slots at multiples of 128: 0 cap 64 -> class 0;
    1 cap 100 -> class 1; 2 at 288 cap 96 (32 modulo 64) -> class 0, cut; 3 cap
    47 -> no class; 4 cap 128 -> class 1; 5 cap 96 -> class 1, cut; 6
    gate-failed; 7 at 16 modulo 32 -> no class."""
    buf = np.full(1100, 0xA5, np.uint8)
    offs, caps = [0, 128, 288, 384, 512, 640, 768, 912], [64, 100, 96, 47, 128, 96, 50, 64]
    for o in offs:
        image(buf, o)
    before = buf.copy()
    gate = [0, 0, 0, 0, 0, 0, -3, 0]
    so, sc, words = [7000, 9, 9, 9], [70, 9, 9, 9], [1, 2, 48, 32, 0, 2, 96, 64]
    img = list(range(20, 28))
    st, total, acc = model.m_release_set(buf, offs, caps, img, None, gate, None, 0, so, sc, words, 2, 2)
    assert st.tolist() == [0, 0, -1, -1, 0, -1, -1, -1] and acc == [0, 1, 4] and total == [5, 5, 2, 3]
    assert so == [7000, 0, 128, 512] and sc == [70, 64, 100, 128] and words == [2, 2, 48, 32, 2, 2, 96, 64]
    want = before.copy()
    for o in (0, 128, 512):
        want[o:o + 2] = 0
    assert np.array_equal(buf, want) and offs[2] == 288 and img == list(range(20, 28))
    # ZERO | COMPACT over the first seven, both classes with room: the cut entries go now, the kept ones move up
    words[0], words[4], count = 0, 0, [7, 8]
    st, total, acc = model.m_release_set(buf, offs, caps, img, count, gate, None, 3, so, sc, words, 2, 2)
    assert st.tolist() == [-1, -1, 0, -1, -1, 0, -1, 0] and acc == [2, 5] and total == [2, 5, 1, 1]
    assert offs == [0, 128, 384, 512, 768, 0, 0, 912] and caps == [64, 100, 47, 128, 50, 0, 0, 64]
    assert img == [20, 21, 23, 24, 26, model.NO_IMAGE, model.NO_IMAGE, 27] and count == [5, 8]
    assert so == [288, 0, 640, 512] and words == [1, 2, 48, 32, 1, 2, 96, 64]
    assert not buf[288:288 + 96].any() and not buf[640:640 + 96].any() and buf[640 + 96] == 0xA5


@pytest.mark.parametrize("words", [[3, 2, 48, 32, 0, 2, 96, 64], [0, 2, 23, 32, 0, 2, 96, 64],
                                   [0, 2, 48, 48, 0, 2, 96, 64], [0, 3, 48, 32, 0, 2, 96, 64],
                                   [0, 2, 96, 32, 0, 2, 96, 64], [0, 2, 100, 32, 0, 2, 96, 64]])
def test_release_set_model_unsound_set_changes_nothing(words):
    """Count above capacity, cls below 24, pal no power of two, a capacity above
    the stride, cls not increasing (equal, falling)."""
    buf = np.full(300, 0xA5, np.uint8)
    image(buf, 0)
    image(buf, 128)
    before, so, sc, w = buf.copy(), [9] * 4, [9] * 4, list(words)
    st, total, acc = model.m_release_set(buf, [0, 128], [64, 100], None, None, None, [7, 128], 1, so, sc, w, 2, 2)
    assert st.tolist() == [-1, 0] and acc == [] and total == [0, 2, 0, 0]
    assert np.array_equal(buf, before) and so == [9] * 4 and w == list(words)
    assert not model.set_sound(words, 2, 2) and model.set_sound([0, 2, 48, 32, 0, 2, 96, 64], 2, 2)


@pytest.mark.parametrize("flags", [0, 1, 2, 3])
def test_release_set_model_with_one_class_is_the_pool_model(flags):
    """test_pool_dev_abi's batch of eight, through both models: output for
    output, with a cut by the capacity."""
    def batch():
        buf = np.full(600, 0xA5, np.uint8)
        offs, caps = [64 * i for i in range(8)], [64] * 8
        caps[4] = 47
        offs[5] += 16
        for o in offs:
            image(buf, o)
        buf[offs[3] + 1] = 0x01
        return buf, offs, caps, list(range(20, 28)), [0, -3, 0, 0, 0, 0, 0, 0], [7, 7, 128, 7, 7, 7, 7, 7]
    a, b = batch(), batch()
    live = None if flags & 2 else a[5]
    ca, cb = ([7, 8], [7, 8]) if flags & 2 else (None, None)
    so, sc, words = [9] * 4, [9] * 4, [1, 3, 48, 32]
    po, pc, pool = [9] * 4, [9] * 4, [1, 3, 48, 32]
    got = model.m_release_set(a[0], a[1], a[2], a[3], ca, a[4], live, flags, so, sc, words, 1, 4)
    want = pmodel.m_release(b[0], b[1], b[2], b[3], cb, b[4], live, flags, po, pc, pool)
    assert np.array_equal(got[0], want[0]) and got[1][:2] == want[1] and got[1][2] == want[1][0]
    assert got[2] == want[2] and len(want[2]) == 2 and want[0].any()
    assert np.array_equal(a[0], b[0]) and a[1:4] == b[1:4] and ca == cb and (so, sc, words) == (po, pc, pool)


def grow_batch():
    """Seven images of 2 bytes of metadata and 30 of content (used 56), realloc
    64, page 64, align 16; the arena is [1001, 1600).  Returns (buf, offs, caps,
    need)."""
    buf = np.full(3000, 0xA5, np.uint8)
    offs, caps = [0, 100, 200, 320, 400, 500, 720], [64, 64, 100, 64, 64, 200, 64]
    for o in offs:
        image(buf, o, 30)
    return buf, offs, caps, [20, 5, 100, 60, 70, 300, 0]


def test_grow_set_model_on_a_hand_written_batch():
    """Classes (128, 16) with two entries and (256, 16) with one whose capacity,
    250, is below its class.  0 -> 128, class 0, the top entry with its whole
    144 bytes; 1 has room; 2 -> 192, class 1: the bad entry is consumed and the
    image stays; 3 -> 128, class 0, the other entry; 4 -> 128, class 0, which is
    empty by now: an arena slot of the CLASS's size; 5 -> 448, no class: an
    arena slot of 448; 6 needs nothing."""
    buf, offs, caps, need = grow_batch()
    before = buf.copy()
    arena = [1001, 1600]
    so, sc, words = [2048, 2176, 2560, 9], [128, 144, 250, 9], [2, 2, 128, 16, 1, 2, 256, 16]
    st, total, po, pc, served = model.m_grow_set(buf, offs, caps, need, arena, so, sc, words, 2, 2, realloc=64,
                                                 page=64, align=16, flags=1)
    assert st.tolist() == [0, 0, -1, 0, 0, 0, 0] and served == [0, 3] and total == [7 + 128 + 448, 3, 3, 1]
    assert offs == [2176, 100, 200, 2048, 1008, 1136, 720] and caps == [144, 64, 100, 128, 128, 448, 64]
    assert arena == [1584, 1600] and words == [0, 2, 128, 16, 0, 2, 256, 16]
    assert po.tolist() == [0, 100, 200, 320, 400, 500, 720] and pc.tolist() == [64, 64, 100, 64, 64, 200, 64]
    assert so == [2048, 2176, 2560, 9] and sc == [128, 144, 250, 9]
    want = before.copy()
    for old, new, cap in ((0, 2176, 144), (320, 2048, 128), (400, 1008, 128), (500, 1136, 448)):
        want[new:new + 56] = before[old:old + 56]
        want[new + 56:new + cap] = 0              # CIOA_GROW_ZERO: up to the WHOLE capacity of the slot taken
    assert np.array_equal(buf, want)
    # without the flag the tails keep their bytes; an arena that ends inside the second slot cuts image 5 alone
    buf, offs, caps, need = grow_batch()
    arena, words = [1001, 1583], [2, 2, 128, 16, 0, 2, 256, 16]
    st, total, po, pc, served = model.m_grow_set(buf, offs, caps, need, arena, so, sc, words, 2, 2, realloc=64,
                                                 page=64, align=16)
    assert st.tolist() == [0, 0, 0, 0, 0, -1, 0] and total == [7 + 256 + 128 + 448, 2, 3, 1] and arena == [1392, 1583]
    assert offs[2] == 1008 and caps[2] == 256 and offs[4] == 1264 and offs[5] == 500 and buf[2176 + 56] == 0xA5


@pytest.mark.parametrize("words,align", [([2, 2, 128, 8, 1, 2, 256, 8], 16), ([3, 2, 128, 16, 1, 2, 256, 16], 16),
                                         ([2, 2, 128, 16, 1, 2, 128, 16], 16), ([2, 2, 128, 16, 1, 3, 256, 16], 16)])
@pytest.mark.parametrize("flags", [0, 1])
def test_grow_set_model_without_a_usable_class_is_the_grow_model(words, align, flags):
    a, b = grow_batch(), grow_batch()
    arena_a, arena_b = [1001, 1700], [1001, 1700]
    so, sc, w = [2048, 2176, 2560, 9], [128, 144, 256, 9], list(words)
    got = model.m_grow_set(a[0], a[1], a[2], a[3], arena_a, so, sc, w, 2, 2, realloc=64, page=64, align=align,
                           flags=flags)
    want = gmodel.m_grow(b[0], b[1], b[2], b[3], arena_b, realloc=64, page=64, align=align, flags=flags)
    assert np.array_equal(got[0], want[0]) and got[1] == [want[1], 0, 0, 0] and got[4] == []
    assert np.array_equal(got[2], want[2]) and np.array_equal(got[3], want[3]) and want[0].any()
    assert np.array_equal(a[0], b[0]) and a[1] == b[1] and a[2] == b[2] and arena_a == arena_b and w == list(words)
    got = model.m_grow_set(a[0], a[1], a[2], None, arena_a, so, sc, [2, 2, 128, 16, 1, 2, 256, 16], 2, 2)
    assert got[0].tolist() == [-1] * 7 and got[1] == [0, 0, 0, 0]


def test_grow_set_model_with_one_unusable_class():
    """align 32 against a pal of 16 in class 0: its images go to the arena with
    their own new capacity when no higher class holds them... here 256 does."""
    buf, offs, caps, need = grow_batch()
    arena = [1001, 2000]
    so, sc, words = [2048, 2176, 2304, 2688], [128, 128, 256, 256], [2, 2, 128, 16, 2, 2, 256, 32]
    st, total, po, pc, served = model.m_grow_set(buf, offs, caps, need, arena, so, sc, words, 2, 2, realloc=64,
                                                 page=64, align=32)
    # 0, 2, 3, 4 all ask class 1; it serves two, the others get arena slots of 256; 5 has no class
    assert served == [0, 2] and total == [23 + 256 + 256 + 448, 2, 0, 4] and not st.any()
    assert offs[0] == 2688 and offs[2] == 2304 and caps[3] == caps[4] == 256 and words[0] == 2 and words[4] == 0


# ------------------------------------------------------------------ the steady-state shape

def test_steady_state_shape_on_the_model():
    """The shape test_gpu_pool_set.py replays: 12 images of 527 bytes at
    multiples of 32 with 3 bytes of metadata, 1 .. 300 bytes appended per image
    and round (one image per round appends nothing), limit 2000, rotation into
    class 0 (527), realloc 512, page 256, align = pal = 32, classes 527, 1280,
    1792, 2304 -- the capacities the growth rule yields from 527.  The rotation
    gets no needs (dev_need NULL): with them rotate counts an image that lacks
    room as full, and nothing ever grows.  Seed 1, 40 rounds, stride 16, an
    arena of 81920 bytes: no status but CIO_OK, no capacity beside the four
    classes, every class 1 .. 3 serves images from the pool, and the top stops
    after round 11 at 53504 bytes of the arena; the same rounds with m_grow in
    place of the set grow run the arena out in round 22."""
    s = model.Steady()
    tops = []
    for k in range(s.p["rounds"]):
        out = s.round(k)
        assert out["ok"], (k, [x for x in ("rotate", "grow", "release_prev", "release_list")
                               if x in out and out[x][0].any()])
        tops.append(s.arena[0])
    half = s.p["rounds"] // 2
    assert s.odd == 0 and all(x >= 1 for x in s.served[1:]) and s.served[0] == 0, (s.odd, s.served)
    assert len(set(tops[half:])) == 1 and tops[-1] < s.arena[1]
    stop = next(k for k in range(len(tops)) if tops[k] == tops[-1])
    assert (stop, tops[-1] - (s.arena[1] - s.p["arena_room"])) == (11, 53504)
    # what was written is what was drained followed by what is live
    for i in range(s.p["n"]):
        meta, content = model.image_check(s.buf, len(s.buf), s.offs[i], s.caps[i])
        live = s.buf[s.offs[i] + 24 + meta:s.offs[i] + 24 + meta + content].tobytes()
        assert s.drained[i] + live == s.wrote[i], i
    plain = model.Steady(plain=True)
    failed = None
    for k in range(plain.p["rounds"]):
        out = plain.round(k)
        if not out["ok"]:
            failed = (k, bool(out["grow"][0].any()), out["grow"][1][0] > plain.arena[1] - plain.arena[0])
            break
    assert failed == (22, True, True)
