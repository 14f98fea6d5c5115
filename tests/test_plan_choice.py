"""Which kernel and which grid a batch gets (crc_plan.cpp plan_choose), on the
host: no GPU.

cio_crc32_plan_create takes these decisions for the device it runs on, and
test_gpu_crc.py pins them there (test_plan_workgroups, test_anticamp_grid,
test_stray_switches_without_the_gate_change_nothing).  The same expectations
are repeated here through cioa_debug_plan_choice, which runs plan_init and
plan_choose for a device of a given CU count and touches no device.
"""
import ctypes

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import workloads as wl

CUS = 256
SWITCHES = ("CIO_GPU_DIAG", "CIO_GPU_GRID", "CIO_GPU_SMALL", "CIO_GPU_L64", "CIO_GPU_AHEAD", "CIO_GPU_UNIFORM",
            "CIO_GPU_ANTICAMP", "CIO_GPU_ANTICAMP_MAX", "CIO_GPU_PRIO")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    """Every case starts from the shipped plans; the switches are read from the
    environment at each call, so a case sets what it needs."""
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def choice(offs, lens, cus=CUS):
    """cioa_debug_plan_choice's words, by name."""
    f = cio.lib().cioa_debug_plan_choice
    u64p = ctypes.POINTER(ctypes.c_uint64)
    u32p = ctypes.POINTER(ctypes.c_uint32)
    f.argtypes = [u64p, u64p, ctypes.c_size_t, ctypes.c_int, u32p]
    f.restype = ctypes.c_int
    o = np.ascontiguousarray(offs, np.uint64)
    n_ = np.ascontiguousarray(lens, np.uint64)
    w = np.zeros(11, np.uint32)
    assert f(o.ctypes.data_as(u64p), n_.ctypes.data_as(u64p), len(o), cus, w.ctypes.data_as(u32p)) == 0
    c = dict(zip(("grid", "W", "small", "ahead", "unsteps", "l64", "l64_small"), map(int, w[:7])))
    c["S"] = int(w[7]) | int(w[8]) << 32
    c["ntiny"] = int(w[9]) | int(w[10]) << 32
    assert c["W"] == 16 * c["grid"]
    return c


@pytest.fixture(scope="module")
def cfg3():
    lens = wl.cfg3_lens()
    return wl.packed_offsets(lens), lens


def test_grid_per_batch_length(cfg3):
    """test_plan_workgroups on the host: long batches (>= 4 MiB per wave)
    plan 4 workgroups per CU, shorter ones one."""
    assert choice(*cfg3)["grid"] == 4 * CUS
    l2 = wl.cfg2_lens()
    c2 = choice(wl.packed_offsets(l2, align=16), l2)
    assert c2["grid"] == CUS and c2["ahead"] == 1 and c2["small"] == 0
    assert c2["S"] == 1024 * 100 and c2["unsteps"] == 100 and c2["ntiny"] == 0
    l4 = np.full(1024, 4 << 20, np.uint64)      # uniform, 1 MiB per wave: one per CU
    assert choice(wl.packed_offsets(l4), l4)["grid"] == CUS
    l4 = np.full(8192, 4 << 20, np.uint64)      # cfg4 at one GPU, 8 MiB per wave: four
    assert choice(wl.packed_offsets(l4), l4)["grid"] == 4 * CUS


def test_small_chunk_batch():
    lens = np.full(4096, 4096, np.uint64)
    c = choice(wl.packed_offsets(lens, align=16), lens)
    assert c["small"] == 1 and c["S"] == 4096
    lens[7] = 2                                  # tiny chunks do not change the kernel
    c = choice(wl.packed_offsets(lens, align=16), lens)
    assert c["small"] == 1 and c["S"] == 4095 and c["ntiny"] == 1
    lens[9] = 4097                               # one chunk of two steps does
    assert choice(wl.packed_offsets(lens, align=16), lens)["small"] == 0


def test_grid_switch_needs_the_gate(cfg3, monkeypatch):
    """CIO_GPU_GRID=17 moves the grid under CIO_GPU_DIAG=1 and is ignored
    without it (a stray variable in a deployment: the shipped grid)."""
    monkeypatch.setenv("CIO_GPU_GRID", "17")
    assert choice(*cfg3)["grid"] == 4 * CUS
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    assert choice(*cfg3)["grid"] == 17


@pytest.mark.parametrize("clen,per_wave,reduced", [(4096, 16, True), (4096, 128, True), (4096, 25, False),
                                                   (4096, 256, False), (65536, 16, True), (65536, 64, True),
                                                   (65536, 25, False), (65536, 128, False)])
def test_anticamp_grid(monkeypatch, clen, per_wave, reduced):
    """test_anticamp_grid's rows on the host: every wave's range the same
    multiple of 16 steps (small-chunk batches up to 128 chunks per wave,
    stream batches up to 64 steps) plans 31 of every 32 workgroups;
    CIO_GPU_ANTICAMP=0 keeps the full grid, and so does a grid that is not a
    multiple of 32."""
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    for cus in (256, 304):
        lens = np.full(cus * 16 * per_wave // (clen // 4096), clen, np.uint64)
        offs = wl.packed_offsets(lens, align=16)
        for env in ("1", "0"):
            monkeypatch.setenv("CIO_GPU_ANTICAMP", env)
            want = cus // 32 * 31 if reduced and env == "1" and cus % 32 == 0 else cus
            assert choice(offs, lens, cus)["grid"] == want, (cus, env)
