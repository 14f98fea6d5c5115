"""Coalescing a pool set's free slots
(include/chunkio_amd/cio_write_dev_coalesce.h), without a GPU: the symbol and
the Python exports exist with the declared prototype, every argument check
runs before any device call and names its reason, the host check of the
kernels' arithmetic (`make coalescecheck`, a stand-alone program under ASan +
UBSan) passes, the numpy model the GPU tests compare against is asserted by
hand and keeps its invariants on random sets, and Drift -- the scenario the
call exists for -- is fixed here on the models alone."""
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

import coalesce_model as model
from test_rotate_dev_abi import CTYPE

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAME = "cio_file_coalesce_set_dev"


def args(writer, buf, dev_bytes=1 << 20, n_cls=4, stride=8, target=1, align=16, flags=0, total=True):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused before that)."""
    return [writer, dev_bytes, buf, buf, buf, n_cls, stride, target, align, flags, buf if total else None, None]


def test_symbol_is_exported_with_the_declared_prototype():
    lib = chunkio_amd.lib()
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_coalesce.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    found = re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M)
    assert [name for _, name, _ in found] == [NAME]
    res, _, arglist = found[0]
    types = []
    for a in arglist.split(","):
        a = a.strip()
        types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
    assert NAME in _lib.EXPORTS
    fn = getattr(lib, NAME)
    assert fn.restype is CTYPE[res]
    bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
    assert bound == types and len(types) == 12
    assert '#include "cio_write_dev_pool_set.h"' in raw
    assert re.search(r"#define\s+CIOA_COALESCE_DRY\s+1\b", raw) and cf.COALESCE_DRY == model.DRY == 1
    flat = " ".join(raw.replace("*", " ").split()).lower()
    for rule in ("c0.", "c1.", "c2.", "c3.", "c4.", "c5.", "c6.", "c7.", "c8.", "c9."):
        assert rule in flat, rule
    assert "it takes no dev_base" in flat and "all or nothing" in flat
    assert "not here: spilling to another class" in flat and "splitting large slots" in flat
    assert "more than one target per call" in flat and "moving live images" in flat
    for h in ("cio_write_dev_pool_set.h", "cio_write_dev_pool.h"):      # the older headers point here
        with open(os.path.join(ROOT, "include", "chunkio_amd", h)) as f:
            assert "cio_write_dev_coalesce.h" in f.read(), h


def test_python_binding_exports():
    for name in ("coalesce_set_dev", "COALESCE_DRY"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)
    p = inspect.signature(cf.coalesce_set_dev).parameters
    assert list(p) == ["writer", "dev_bytes", "set", "target", "align", "flags", "total", "stream"]
    assert p["align"].default == 16 and p["flags"].default == 0


def test_refuses_bad_arguments_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, NAME)
    buf = ctypes.create_string_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # a non-null address; max_chunks, its first word, is set below
    err = lib.cio_gpu_last_error
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(32)), 4)

    def refused(why, **kw):
        assert fn(*args(kw.pop("writer", writer), buf, **kw)) == -1, (why, kw)
        assert (NAME + ": " + why).encode() in err(), (why, err())

    for flags in (2, 3, 4, 256, 1 << 30, -1):
        refused("unknown flags", flags=flags)
    for n_cls in (0, 1, 9, 1 << 40):
        refused("n_cls must be in 2 .. 8", n_cls=n_cls)
    for n_cls, target in ((4, 0), (4, 4), (2, 2), (8, 8), (4, 1 << 40)):
        refused("target must be in 1 .. n_cls - 1", n_cls=n_cls, target=target)
    refused("stride must not be 0", stride=0)
    for align in (0, 3, 48, 8192, 1 << 40):
        refused("align must be a power of two in 1 .. 4096", align=align)
    refused("dev_bytes must not be 0", dev_bytes=0)
    for align in (1, 16, 4096):                   # (dev_bytes - 1) / align >= 2^32 - 1
        refused("dev_bytes / align does not fit the 32-bit sort key", dev_bytes=(2 ** 32 - 1) * align + 1,
                align=align)
        refused("dev_bytes / align does not fit the 32-bit sort key", dev_bytes=2 ** 64 - 1, align=align)
    refused("null writer", writer=None)
    for at in (2, 3, 4, 10):                      # the set's three pointers and dev_total
        a = args(writer, buf)
        a[at] = None
        assert fn(*a) == -1 and (NAME + ": null pointer").encode() in err(), at
    # the scratch is sized by the writer's max_chunks (32 here): n_cls * stride must not exceed it
    for n_cls, stride in ((4, 9), (2, 17), (8, 5), (4, 1 << 62), (8, 2 ** 64 - 1)):
        refused("more set entries than the writer was created for", n_cls=n_cls, stride=stride)
    # the values are checked before the pointers, the pointers before the writer is looked at
    a = args(None, None, flags=2)
    assert fn(*a) == -1 and b"unknown flags" in err()
    a = args(None, buf, stride=0)
    assert fn(*a) == -1 and b"stride must not be 0" in err()


def test_host_check_of_the_kernels_arithmetic_passes():
    r = subprocess.run(["make", "-C", ROOT, "coalescecheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "coalesce_check: ok" in r.stdout


def test_model_by_hand():
    """T = 520, P = 128, align 32, fourteen 96-byte slots from 4096 on, filed
    in descending order; a duplicate, a nested overlap, an unaligned entry, one
    beyond the buffer, and a non-candidate in the middle of nothing."""
    classes, stride = [(40, 32), (96, 32), (200, 32), (520, 128)], 32
    words = [w for c, p in classes for w in (0, stride, c, p)]
    so, sc = [0] * (4 * stride), [0] * (4 * stride)
    ents = [(4096 + 96 * (13 - j), 96) for j in range(14)]
    ents += [(4096, 96), (4096 + 96, 40), (4097, 96), ((1 << 20) - 32, 64), (65536, 600)]
    for j, (o, c) in enumerate(ents):
        so[stride + j], sc[stride + j] = o, c
    words[4] = len(ents)
    total = model.m_coalesce_set(so, sc, words, 4, stride, 1 << 20, 3, 32)
    # g_0 = 4096; off >= 4616 from the seventh slot, a multiple of 128 at the ninth: eight slots, 768 bytes; the rest
    # of the run covers 576 >= 520: six slots
    assert total == [0, 2, 2, 2, 14, 0, 0, 0, 3]
    assert (so[3 * stride:3 * stride + 3], sc[3 * stride:3 * stride + 3]) == ([4096, 4864, 65536], [768, 576, 600])
    assert words[0::4] == [0, 0, 0, 3]
    assert model.m_coalesce_set(so, sc, words, 4, stride, 1 << 20, 3, 32) == [0, 0, 0, 0, 0, 0, 0, 0, 3]
    # an interior group that ends short of T stays what it is and is met again without being counted: slots of 527
    # bytes (544 with padding), T = 1088
    words = [w for c, p in [(527, 32), (1088, 32)] for w in (0, 8, c, p)]
    so, sc = [0, 544, 1088, 1632] + [0] * 12, [527] * 4 + [0] * 12
    words[0] = 4
    # group 0 = the slots at 0 and 544, 1071 bytes < T; from 1088 the run's end leaves 1071 < T: two singles
    assert model.m_coalesce_set(so, sc, words, 2, 8, 4096, 1, 32) == [0, 0, 0, 1, 2, 3, 0]
    assert (so[:3], sc[:3], words[0::4]) == ([0, 1088, 1632], [1071, 527, 527], [3, 0])
    # again: the three are one run, its group 0 the 1071-byte slot alone -- that entry, unchanged, counted nowhere
    assert model.m_coalesce_set(so, sc, words, 2, 8, 4096, 1, 32) == [0, 0, 0, 0, 0, 3, 0]
    assert (so[:3], sc[:3], words[0::4]) == ([0, 1088, 1632], [1071, 527, 527], [3, 0])


@pytest.mark.parametrize("seed", range(12))
def test_model_invariants_on_random_sets(seed):
    """Outputs pairwise disjoint, every output in the class rule 4' gives it
    and in ascending offset, the bytes covered = the survivors' bytes plus the
    padding inside groups, nothing else in the arrays changed, and a second
    call changes nothing (C9)."""
    rng = np.random.default_rng(seed)
    n_cls = int(rng.integers(2, 9))
    target = int(rng.integers(1, n_cls))
    align = int(2 ** rng.integers(0, 8))
    pal = align * int(2 ** rng.integers(0, 3))
    cls = sorted(int(x) for x in rng.choice(np.arange(24, 6000), n_cls, replace=False))
    classes = [(c, pal if k == target else align) for k, c in enumerate(cls)]
    stride, dev_bytes = 256, 1 << 30
    so, sc, words = model.make_set(seed, classes, stride, int(rng.integers(0, 160)) * n_cls, dev_bytes, align,
                                   adjacent=float(rng.choice([0.0, 0.5, 0.9, 1.0])), bad=0.1)
    surv, ill, hit = model.survivors_of(so, sc, words, n_cls, stride, dev_bytes, align)
    outs, groups, absorbed = model.outputs_of(surv, cls[target], pal, align)
    before = (list(so), list(sc), list(words))
    total = model.m_coalesce_set(so, sc, words, n_cls, stride, dev_bytes, target, align)
    assert total[0] in (0, 2) and total[2] == hit and total[3] == groups and total[4] == absorbed
    assert sum(before[2][0::4]) == len(surv) + hit + ill
    if total[0] == 2:
        assert (so, sc, words) == before
        return
    got = [(so[k * stride + j], sc[k * stride + j], k) for k in range(n_cls) for j in range(words[4 * k])]
    assert len(got) == len(outs) - (total[1] - ill) == len(surv) - absorbed + groups - (total[1] - ill)
    for k in range(n_cls):                        # ascending inside a class, the rest of the arrays as they were
        mine = [o for o, _, c in got if c == k]
        assert mine == sorted(mine) and words[4 * k] == total[5 + k]
        assert so[k * stride + words[4 * k]:(k + 1) * stride] == before[0][k * stride + words[4 * k]:(k + 1) * stride]
        assert sc[k * stride + words[4 * k]:(k + 1) * stride] == before[1][k * stride + words[4 * k]:(k + 1) * stride]
    flat = sorted(got)
    for (o, c, k), nxt in zip(flat, flat[1:] + [(dev_bytes, 0, 0)]):
        assert o + c <= nxt[0], "outputs overlap"
        assert k == model.file_class(words, n_cls, o, c) and o % align == 0 and c >= 1
    # the bytes: every output is a survivor or spans survivors that follow one another slot by slot
    covered = sum(c for _, c in outs)
    padding = 0
    starts = {o: c for o, c in surv}
    for o, c in outs:
        if o in starts and starts[o] == c:
            continue
        at = o
        while at < o + c:
            assert at in starts, "a group spans a byte no survivor holds"
            nxt = model.round_up(at + starts[at], align)
            padding += min(nxt, o + c) - (at + starts[at])
            at = nxt
    assert covered == sum(c for _, c in surv) + padding
    again = (list(so), list(sc), list(words))
    assert model.m_coalesce_set(so, sc, words, n_cls, stride, dev_bytes, target, align)[:5] == [0, 0, 0, 0, 0]
    assert (so, sc, words) == again


def test_drift_on_the_models():
    """The arena size at which the arm without the call fails while the arm with
    it finishes with CIO_OK alone, and both high-water marks."""
    p = model.DRIFT
    assert p["arena_room"] == 24 * 1280 + 6 * 2304 == 44544
    with_call, without = model.Drift(coalesce=True), model.Drift(coalesce=False)
    a, b = with_call.run(), without.run()
    assert a["phase1_bad"] == b["phase1_bad"] == 0 and a["top1"] == b["top1"] == 6592 + 24 * 1280 == 37312
    # with the call: 24 entries of 1280 bytes become 12 slots of 2560, every image is served from the set with the
    # slot's whole capacity, and the top stands still
    assert a["coalesce"] == [0, 0, 0, 12, 24, 0, 0, 0, 12]
    assert not a["grow_status"].any() and a["served"] == list(range(12)) and a["grow_total"] == [0, 12, 0, 0, 0, 12]
    assert a["top2"] == a["top1"] and with_call.caps == [2560] * 12
    # without it the same grow asks the arena for twelve class-3 slots, gets six and cuts six
    assert b["grow_total"] == [12 * 2304, 0, 0, 0, 0, 12] and b["grow_status"].tolist() == [0] * 6 + [-1] * 6
    assert b["top2"] == b["top1"] + 6 * 2304 == without.arena[1] == 51136
    assert without.words[4] == 24, "the 24 class-1 entries idle"
    # one class-3 slot less of arena and the arm with the call is all it takes: the top never moves in phase 2
    tight = model.Drift(coalesce=True, arena_room=24 * 1280).run()
    assert not tight["grow_status"].any() and tight["top2"] == tight["top1"]
