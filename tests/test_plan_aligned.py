"""The wave-aligned class of uniform batches (crc_plan.cpp plan_choose:
cio_crc32_plan.aligned), on the host: no GPU.

A batch is in the class when it takes the issue-ahead stream kernel on the
full one-workgroup-per-CU grid, its S steps split into exactly q per wave and
every chunk is exactly p = 2, 4, 8 or 16 consecutive waves.  Each neighbour
just outside stays on the existing path.  cioa_debug_plan_aligned runs
plan_init and plan_choose for a device of a given CU count, like
cioa_debug_plan_choice in test_plan_choice.py.
"""
import ctypes
import os
import subprocess

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import workloads as wl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CUS = 256
W = 16 * CUS
SWITCHES = ("CIO_GPU_DIAG", "CIO_GPU_GRID", "CIO_GPU_SMALL", "CIO_GPU_L64", "CIO_GPU_AHEAD", "CIO_GPU_UNIFORM",
            "CIO_GPU_ANTICAMP", "CIO_GPU_ANTICAMP_MAX", "CIO_GPU_PRIO", "CIO_GPU_ALIGNED")
PQ = [(p, q) for p in (2, 4, 8, 16) for q in (1, 2, 3, 5, 25)]


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def _call(name, offs, lens, cus, nwords):
    f = getattr(cio.lib(), name)
    u64p = ctypes.POINTER(ctypes.c_uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    f.argtypes = [u64p, u64p, ctypes.c_size_t, ctypes.c_int, u32p]
    f.restype = ctypes.c_int
    o = np.ascontiguousarray(offs, np.uint64)
    n_ = np.ascontiguousarray(lens, np.uint64)
    w = np.zeros(nwords, np.uint32)
    assert f(o.ctypes.data_as(u64p), n_.ctypes.data_as(u64p), len(o), cus, w.ctypes.data_as(u32p)) == 0
    return [int(x) for x in w]


def aligned(offs, lens, cus=CUS):
    """(aligned, q, p) of the plan for this batch."""
    return tuple(_call("cioa_debug_plan_aligned", offs, lens, cus, 3))


def grid(offs, lens, cus=CUS):
    return _call("cioa_debug_plan_choice", offs, lens, cus, 11)[0]


def uniform(n, steps, stride=None, off0=0, length=None):
    length = steps * 4096 if length is None else length
    stride = length if stride is None else stride
    lens = np.full(n, length, np.uint64)
    offs = np.uint64(off0) + np.arange(n, dtype=np.uint64) * np.uint64(stride)
    return offs, lens


def test_cfg2_is_aligned():
    lens = wl.cfg2_lens()
    assert aligned(wl.packed_offsets(lens, align=16), lens) == (1, 25, 4)


@pytest.mark.parametrize("p,q", PQ)
def test_class_members(p, q):
    assert aligned(*uniform(W // p, p * q)) == (1, q, p)
    # padding between the chunks (a stride larger than the length) stays in the class
    assert aligned(*uniform(W // p, p * q, stride=p * q * 4096 + 4096 + 128)) == (1, q, p)
    assert aligned(*uniform(W // p, p * q, stride=p * q * 4096 + 128, off0=256)) == (1, q, p)


@pytest.mark.parametrize("p,q", PQ)
def test_neighbours_stay_out(p, q):
    n, steps = W // p, p * q
    for dn in (-1, 1):
        assert aligned(*uniform(n + dn, steps))[0] == 0, ("n", dn)
    for ds in (-1, 1):
        if steps + ds >= 1:
            assert aligned(*uniform(n, steps + ds))[0] == 0, ("steps", ds)
    # a 16-byte head: every chunk starts 16 bytes into its 128-byte line
    assert aligned(*uniform(n, steps, off0=16, stride=steps * 4096 + 128))[0] == 0
    assert aligned(*uniform(n, steps, off0=8, stride=steps * 4096 + 16))[0] == 0
    # a length that is not a multiple of 4096 (same step count, and one byte more)
    assert aligned(*uniform(n, steps, length=steps * 4096 - 16, stride=steps * 4096))[0] == 0
    assert aligned(*uniform(n, steps, length=steps * 4096 - 4095, stride=steps * 4096))[0] == 0
    # a tiny chunk appended
    offs, lens = uniform(n, steps)
    offs = np.append(offs, offs[-1] + lens[-1])
    lens = np.append(lens, np.uint64(3))
    assert aligned(offs, lens)[0] == 0


@pytest.mark.parametrize("q", (1, 2, 3, 5, 25))
def test_other_piece_counts_stay_out(q):
    """p = 32 and p = 3 (and p = 1: whole chunks per wave keep today's path)."""
    assert aligned(*uniform(W // 32, 32 * q))[0] == 0
    assert aligned(*uniform(W // 1, 1 * q))[0] == 0
    # p = 3 needs a wave count divisible by 3: a 240-CU device (W = 3840)
    assert aligned(*uniform(3840 // 3, 3 * q), cus=240)[0] == 0
    assert aligned(*uniform(3840 // 4, 4 * q), cus=240) == (1, q, 4)


def test_long_ranges_stay_out(monkeypatch):
    """Ranges over 64 steps per wave do not take the issue-ahead kernel, and
    forcing it (CIO_GPU_AHEAD=1) does not put them in the class."""
    for q in (64, 65, 66, 100):
        want = (1, q, 4) if q <= 64 and q % 16 else (0, 0, 0)
        assert aligned(*uniform(W // 4, 4 * q)) == want, q
    assert aligned(*uniform(W // 4, 4 * 63)) == (1, 63, 4)
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    monkeypatch.setenv("CIO_GPU_AHEAD", "1")
    assert aligned(*uniform(W // 4, 4 * 65))[0] == 0
    assert aligned(*uniform(W // 4, 4 * 63)) == (1, 63, 4)


def test_other_grids_stay_out(monkeypatch):
    """The anti-camping grid (31 of 32 workgroups, ranges a multiple of 16
    steps) and the 4x grid (>= 1024 steps per wave) are not in the class; with
    the anti-camping grid switched off the same batch is."""
    for q in (16, 32, 48, 64):
        o, l = uniform(W // 4, 4 * q)
        assert grid(o, l) == CUS // 32 * 31 and aligned(o, l)[0] == 0
    o, l = uniform(W // 4, 4 * 1024)
    assert grid(o, l) == 4 * CUS and aligned(o, l)[0] == 0
    o, l = uniform(W // 4, 4 * 16)
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    monkeypatch.setenv("CIO_GPU_ANTICAMP", "0")
    assert grid(o, l) == CUS and aligned(o, l) == (1, 16, 4)
    # a grid override is not the full grid
    monkeypatch.setenv("CIO_GPU_GRID", "128")
    assert aligned(*uniform(128 * 16 // 4, 4 * 5))[0] == 0


def test_switch_needs_the_gate(monkeypatch):
    """CIO_GPU_ALIGNED=0 keeps the issue-ahead kernel under CIO_GPU_DIAG=1 and
    is ignored without it; the kernel and grid of the plan do not move."""
    lens = wl.cfg2_lens()
    offs = wl.packed_offsets(lens, align=16)
    before = _call("cioa_debug_plan_choice", offs, lens, CUS, 11)
    monkeypatch.setenv("CIO_GPU_ALIGNED", "0")
    assert aligned(offs, lens)[0] == 1
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    assert aligned(offs, lens)[0] == 0
    assert _call("cioa_debug_plan_choice", offs, lens, CUS, 11) == before


def test_plancheck():
    """The planner's stand-alone ASan/UBSan program stays green."""
    r = subprocess.run(["make", "-C", ROOT, "plancheck"], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    assert "FAIL" not in r.stdout
