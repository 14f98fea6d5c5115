"""Device-planned CRC-32 batches (cio_crc32_devplan_*): the planner kernels
write the host plan_build's image byte for byte, the CRC launch over it is
bit-exact against the oracle, one plan follows changing geometry (also in a
replayed graph), and bad geometry is refused on the device.

The planner's wave count W is the device's (16 per CU) or, under
CIO_GPU_DIAG=1 CIO_GPU_GRID=3 / 17, 48 / 272 (not powers of two)."""
import ctypes

import numpy as np
import pytest

import chunkio_amd as cio
from oracle import pyoracle as po

pytestmark = pytest.mark.gpu

STEP = 4096
MAX_CHUNKS = 10000
DESC = np.dtype([("a", "<u8"), ("vlen", "<u8"), ("g", "<u8"), ("nsteps", "<u4"), ("h", "<u4"),
                 ("npieces", "<u4"), ("w0", "<u4"), ("w1", "<u4"), ("pad", "<u4")])
WSTART = np.dtype([("d", DESC), ("c", "<u4"), ("pad", "<u4", 3)])
assert DESC.itemsize == 48 and WSTART.itemsize == 64
HDR_S, HDR_NTINY, HDR_BYTES, HDR_STATUS = 0, 1, 2, 3


def hooks():
    lib = cio.lib()
    V, U64 = ctypes.c_void_p, ctypes.c_uint64
    lib.cioa_debug_devplan_image.restype = ctypes.c_int
    lib.cioa_debug_devplan_image.argtypes = [V, U64, V, V, ctypes.c_size_t, V, V, V, V, V, V]
    lib.cioa_debug_plan_image.restype = ctypes.c_int
    lib.cioa_debug_plan_image.argtypes = [V, V, ctypes.c_size_t, ctypes.c_uint32, V, V, V, V, V]
    return lib


def dev_u64(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(cuda)


def pack(lens, rng, first_off=0):
    """Offsets for `lens` packed in order with gaps of 0..200 bytes."""
    gaps = rng.integers(0, 201, len(lens)).astype(np.uint64)
    ends = np.cumsum(lens.astype(np.uint64) + gaps)
    offs = np.concatenate([[0], ends[:-1]]).astype(np.uint64) + np.uint64(first_off)
    return offs


def log_uniform(rng, n, top):
    return (np.exp(rng.uniform(0.0, np.log(top), n)).astype(np.uint64) - np.uint64(1)).astype(np.uint64)


def batch2000(seed):
    """2000 log-uniform lengths in [0, 2 MiB), runs of tiny (< 4 byte) chunks at
    the start, at the end and between two multi-wave chunks."""
    rng = np.random.default_rng(seed)
    lens = log_uniform(rng, 2000, 2 << 20)
    lens[0:5] = [0, 1, 2, 3, 0]
    lens[-4:] = [3, 0, 2, 1]
    lens[1000] = (2 << 20) - 1
    lens[1001:1006] = [0, 3, 1, 0, 2]
    lens[1006] = (2 << 20) - 7
    return pack(lens, rng, first_off=int(rng.integers(0, 16))), lens


def geometries(W):
    """name -> (offs, lens), as the planner's traps want them for W waves."""
    g = {}
    for ln in (0, 3, 4, 4096, 4097):
        g[f"one_{ln}"] = (np.asarray([5], np.uint64), np.asarray([ln], np.uint64))
    # S < W: empty waves between a chunk's pieces
    lens = np.full(5, 3 * STEP - 400, np.uint64)       # head (< 128) + gap (<= 200) keep each at 3 steps
    g["five_of_3_steps"] = (pack(lens, np.random.default_rng(1), 16), lens)
    # S == W and S == W + 1: W - 7 one-step chunks, then one chunk of 7 (8) steps
    assert W - 6 <= MAX_CHUNKS
    for extra in (0, 1):
        lens = np.concatenate([np.full(W - 7, STEP, np.uint64), [np.uint64((7 + extra) * STEP - 9)]])
        g[f"S_eq_W_plus_{extra}"] = (np.arange(len(lens), dtype=np.uint64) * np.uint64(STEP), lens)
    g["one_spanning_every_wave"] = (np.asarray([22], np.uint64), np.asarray([3 * STEP * W + 5], np.uint64))
    g["mixed_2000"] = batch2000(2000)
    g["aligned_4k_x10000"] = (np.arange(10000, dtype=np.uint64) * np.uint64(STEP), np.full(10000, STEP, np.uint64))
    return g


def extent(offs, lens):
    return int((offs + lens).max()) if len(offs) else 0


@pytest.fixture(scope="module")
def data(cuda):
    """One random host buffer and its device copy, shared by every test."""
    import torch
    size = 0
    with cio.Crc32DevPlan(1) as plan:
        own = 16 * plan.workgroups
    for W in (48, 272, own):
        size = max(size, max(extent(o, l) for o, l in geometries(W).values()))
    size = max(size, extent(*batch2000(2001)))
    host = np.random.default_rng(0xD47A).integers(0, 256, size + 256, dtype=np.uint8)
    return host, torch.from_numpy(host).to(cuda)


_oracle_cache = {}


def oracle(key, host, offs, lens, seeds=None):
    if key not in _oracle_cache:
        _oracle_cache[key] = po.crc_batch(host, offs, lens, seeds=seeds)
    return _oracle_cache[key]


def set_grid(monkeypatch, grid):
    if grid is not None:
        monkeypatch.setenv("CIO_GPU_DIAG", "1")
        monkeypatch.setenv("CIO_GPU_GRID", str(grid))


def plan_waves(plan):
    W = ctypes.c_uint32(0)
    assert hooks().cioa_debug_devplan_image(plan._handle, 0, None, None, 0, None, None, None, None, None,
                                            ctypes.byref(W)) == 0
    return int(W.value)


def device_image(plan, offs_t, lens_t, n, W, dev_bytes):
    desc = np.zeros(n, DESC)
    ws = np.zeros(W, WSTART)
    tiny = np.zeros(n, np.uint32)
    pfac = np.zeros(W + n + 1 + 2 * W, np.uint32)
    hdr = np.zeros(4, np.uint64)
    rc = hooks().cioa_debug_devplan_image(plan._handle, dev_bytes, offs_t.data_ptr(), lens_t.data_ptr(), n,
                                          desc.ctypes.data, ws.ctypes.data, tiny.ctypes.data, pfac.ctypes.data,
                                          hdr.ctypes.data, None)
    assert rc == 0, cio.lib().cio_gpu_last_error()
    return desc, ws, tiny, pfac, hdr


def host_image(offs, lens, W):
    n = len(offs)
    desc = np.zeros(n, DESC)
    ws = np.zeros(W, WSTART)
    tiny = np.zeros(n, np.uint32)
    pfac = np.zeros(W + n + 1 + 2 * W, np.uint32)
    hdr = np.zeros(4, np.uint64)
    offs = np.ascontiguousarray(offs, np.uint64)
    lens = np.ascontiguousarray(lens, np.uint64)
    assert hooks().cioa_debug_plan_image(offs.ctypes.data, lens.ctypes.data, n, W, desc.ctypes.data, ws.ctypes.data,
                                         tiny.ctypes.data, pfac.ctypes.data, hdr.ctypes.data) == 0
    return desc, ws, tiny, pfac, hdr


@pytest.mark.parametrize("grid", [None, 3, 17])
def test_plan_image_equals_host_plan(cuda, data, monkeypatch, grid):
    """desc, wave starts, tiny list, all of pfac, S, ntiny and bytes, byte for
    byte, for every geometry -- on ONE reused plan, so each image also has to
    overwrite whatever the previous geometry left in the arenas."""
    set_grid(monkeypatch, grid)
    with cio.Crc32DevPlan(MAX_CHUNKS) as plan:
        W = plan_waves(plan)
        assert W == (16 * grid if grid else 16 * plan.workgroups)
        for name, (offs, lens) in geometries(W).items():
            n = len(offs)
            got = device_image(plan, dev_u64(offs, cuda), dev_u64(lens, cuda), n, W, data[1].numel())
            want = host_image(offs, lens, W)
            assert [int(x) for x in got[4]] == [int(x) for x in want[4]], (name, "header S/ntiny/bytes/status")
            ntiny = int(want[4][HDR_NTINY])
            for f in DESC.names:
                bad = np.nonzero(got[0][f] != want[0][f])[0]
                assert bad.size == 0, (name, "desc." + f, bad[:5], got[0][f][bad[:5]], want[0][f][bad[:5]])
            assert got[0].tobytes() == want[0].tobytes(), (name, "desc")
            bad = np.nonzero(got[1]["c"] != want[1]["c"])[0]
            assert bad.size == 0, (name, "wstart.c", bad[:5], got[1]["c"][bad[:5]], want[1]["c"][bad[:5]])
            assert got[1].tobytes() == want[1].tobytes(), (name, "wstart")
            np.testing.assert_array_equal(got[2][:ntiny], want[2][:ntiny], err_msg=name + " tiny")
            bad = np.nonzero(got[3] != want[3])[0]
            assert bad.size == 0, (name, "pfac", W, n, bad[:8], got[3][bad[:8]], want[3][bad[:8]])


def run_exec(plan, base_t, offs, lens, cuda, seeds=None):
    import torch
    n = len(offs)
    out = torch.full((n,), 0x5A5A5A5A, dtype=torch.int32, device=cuda)
    seeds_t = None if seeds is None else torch.from_numpy(seeds.view(np.int32)).to(cuda)
    plan.exec(base_t, dev_u64(offs, cuda), dev_u64(lens, cuda), out, seeds=seeds_t)
    got = out.cpu().numpy().view(np.uint32)
    assert plan.status() == 0
    return got


@pytest.mark.parametrize("l64", ["1", "0"])
@pytest.mark.parametrize("grid", [None, 3, 17])
def test_crc_parity_on_the_same_geometries(cuda, data, monkeypatch, grid, l64):
    """Bit-exact raw CRCs through cio_crc32_devplan_exec, default seeds and a
    seed array, both lane layouts of the stream kernel."""
    monkeypatch.setenv("CIO_GPU_DIAG", "1")
    monkeypatch.setenv("CIO_GPU_L64", l64)
    set_grid(monkeypatch, grid)
    host, base_t = data
    with cio.Crc32DevPlan(MAX_CHUNKS) as plan:
        W = plan_waves(plan)
        for name, (offs, lens) in geometries(W).items():
            want = oracle((name, W, None), host, offs, lens)
            np.testing.assert_array_equal(run_exec(plan, base_t, offs, lens, cuda), want, err_msg=name)
            seeds = np.random.default_rng(len(name) * 1000 + len(lens)).integers(
                0, 2 ** 32, len(lens), dtype=np.uint64).astype(np.uint32)
            want = oracle((name, W, "seeds"), host, offs, lens, seeds)
            np.testing.assert_array_equal(run_exec(plan, base_t, offs, lens, cuda, seeds=seeds), want,
                                          err_msg=name + " seeds")


def test_one_plan_changing_geometry(cuda, data):
    """2000 chunks, then ONE 3-byte chunk, then 2000 chunks of other lengths on
    the same plan: stale piece factors, partial slots and wave words of the
    earlier geometry must not reach the later results."""
    host, base_t = data
    with cio.Crc32DevPlan(2000) as plan:
        for key, (offs, lens) in (("a", batch2000(2000)),
                                  ("b", (np.asarray([9], np.uint64), np.asarray([3], np.uint64))),
                                  ("c", batch2000(2001)),
                                  ("a2", batch2000(2000))):
            want = oracle(("chg", key[0]), host, offs, lens)
            np.testing.assert_array_equal(run_exec(plan, base_t, offs, lens, cuda), want, err_msg=key)


def test_graph_replay_follows_device_geometry(cuda, data):
    """One captured devplan_exec (a serial chain of kernels), replayed over
    two geometries of the same n written into the same device arrays."""
    import torch
    host, _ = data
    n = 500
    geo = []
    for seed in (11, 12):
        rng = np.random.default_rng(seed)
        lens = log_uniform(rng, n, 256 << 10)
        lens[:3] = [0, 2, (200 << 10) + seed]
        offs = pack(lens, rng, first_off=seed)
        geo.append((offs, lens))
    size = max(extent(o, l) for o, l in geo) + 64
    bufs = [host[k * 4096 + k:k * 4096 + k + size] for k in (0, 1)]      # two different contents
    base_t = torch.from_numpy(np.ascontiguousarray(bufs[0])).to(cuda)
    offs_t, lens_t = dev_u64(geo[0][0], cuda), dev_u64(geo[0][1], cuda)
    out = torch.zeros(n, dtype=torch.int32, device=cuda)
    with cio.Crc32DevPlan(n) as plan:
        plan.exec(base_t, offs_t, lens_t, out)            # warm-up outside the capture
        torch.cuda.synchronize()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            plan.exec(base_t, offs_t, lens_t, out)
        for k in (0, 1, 0):
            base_t.copy_(torch.from_numpy(np.ascontiguousarray(bufs[k])))
            offs_t.copy_(torch.from_numpy(geo[k][0].view(np.int64)))
            lens_t.copy_(torch.from_numpy(geo[k][1].view(np.int64)))
            out.fill_(0)
            graph.replay()
            torch.cuda.synchronize()
            want = po.crc_batch(np.ascontiguousarray(bufs[k]), geo[k][0], geo[k][1])
            np.testing.assert_array_equal(out.cpu().numpy().view(np.uint32), want, err_msg=str(k))
            assert plan.status() == 0
        del graph


def test_device_side_validation_planner_only(cuda):
    """Bad geometry gives a non-zero status and an EMPTY plan (S = 0, ntiny =
    0).  Only the planner runs here (the debug hook): no CRC kernel is
    launched over any of these."""
    cases = {
        "past_dev_bytes": ([0, 4096, 100], [100, 4097, 2], 8192, cio.DEVPLAN_E_BOUNDS),
        "wraps_2_64": ([0, 2 ** 64 - 8, 64], [16, 16, 1], 1 << 20, cio.DEVPLAN_E_BOUNDS),
        "chunk_of_2_44": ([0, 4096, 0], [5, 2 ** 44, 2], 1 << 60, cio.DEVPLAN_E_CHUNK_TOO_LARGE),
    }
    with cio.Crc32DevPlan(16) as plan:
        W = plan_waves(plan)
        for name, (offs, lens, dev_bytes, code) in cases.items():
            offs, lens = np.asarray(offs, np.uint64), np.asarray(lens, np.uint64)
            hdr = device_image(plan, dev_u64(offs, cuda), dev_u64(lens, cuda), len(offs), W, dev_bytes)[4]
            assert int(hdr[HDR_STATUS]) & code, (name, hdr)
            assert int(hdr[HDR_S]) == 0 and int(hdr[HDR_NTINY]) == 0, (name, hdr)
        # and a good geometry on the same plan afterwards is accepted again
        offs, lens = np.asarray([0, 64], np.uint64), np.asarray([50, 2], np.uint64)
        got = device_image(plan, dev_u64(offs, cuda), dev_u64(lens, cuda), 2, W, 4096)
        want = host_image(offs, lens, W)
        assert [int(x) for x in got[4]] == [int(x) for x in want[4]] == [1, 1, 52, 0]
        assert got[3].tobytes() == want[3].tobytes()


def test_exec_argument_checks_with_a_real_plan(cuda):
    import torch
    t = torch.zeros(64, dtype=torch.int64, device=cuda)
    with cio.Crc32DevPlan(4) as plan:
        with pytest.raises(cio.CioGpuError, match="more chunks"):
            plan.exec(t.view(torch.uint8), t, t, t.view(torch.int32), n=5)
        plan.exec(t.view(torch.uint8), t, t, t.view(torch.int32), n=0)     # a no-op
