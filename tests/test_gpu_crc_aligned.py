"""GPU parity of the wave-aligned stream kernel (crc32_aligned_kernel).

Shapes: W = 16 x the plan's workgroups; batches of W / p chunks of p * q
steps, p in {2, 4, 8, 16}, q in {1..5} (q = 1, 2: no steady loop; odd and even
q: both peeled tails), 16-80 MiB each.  Bar: every chunk's raw CRC equals
zlib.crc32 of the host copy of its bytes -- plain, with seeds, with a chunk-id
map, with a padded stride -- and equals what the issue-ahead kernel gives for
the same batch (CIO_GPU_DIAG=1 CIO_GPU_ALIGNED=0, in one child process for all
shapes).  Each neighbour shape just outside the class still matches zlib on
the old path.

One device buffer of deterministic bytes (and its host copy) serves every
case; a case's batch is a prefix of it.
"""
import ctypes
import os
import subprocess
import sys
import zlib

import numpy as np
import pytest

import chunkio_amd as cio

pytestmark = pytest.mark.gpu
STEP = 4096
QMAX = 5
PQ = [(p, q) for p in (2, 4, 8, 16) for q in (1, 2, 3, 4, 5)]
PAD = 128           # padded stride: one 128-byte line between chunks (every chunk keeps head 0)
FILL_SEED = 0xA11C
SWITCHES = ("CIO_GPU_DIAG", "CIO_GPU_GRID", "CIO_GPU_SMALL", "CIO_GPU_L64", "CIO_GPU_AHEAD", "CIO_GPU_UNIFORM",
            "CIO_GPU_ANTICAMP", "CIO_GPU_ANTICAMP_MAX", "CIO_GPU_PRIO", "CIO_GPU_ALIGNED", "CIO_GPU_STAMPS")


@pytest.fixture(autouse=True)
def no_switches(monkeypatch):
    for k in SWITCHES:
        monkeypatch.delenv(k, raising=False)


def grid_waves():
    """W of the one-workgroup-per-CU grid, read from a plan (2 steps: no
    other grid applies)."""
    with cio.Crc32Plan([0], [2 * STEP]) as plan:
        return 16 * plan.workgroups


def buffer_bytes(W):
    """The end of the farthest chunk of any case: one chunk more, one step more
    per chunk, the padded stride; the ring test's shifted bases on top."""
    end = 0
    for p, q in PQ:
        n, steps = W // p, p * q
        end = max(end, (n + 1) * steps * STEP, n * (steps + 1) * STEP, n * (steps * STEP + PAD))
    return end + 4 * STEP


def make_data(dev, W):
    """The shared device buffer: 64 KiB blocks of the synthetic generator."""
    import torch
    size = buffer_bytes(W)
    nblk = (size + 65535) // 65536
    t = torch.empty(nblk * 65536, dtype=torch.uint8, device=dev)
    cio.fill_synthetic(t, np.arange(nblk, dtype=np.uint64) * np.uint64(65536), np.full(nblk, 65536, np.uint64),
                       FILL_SEED)
    torch.cuda.synchronize()
    return t


def batch(n, steps, stride=None):
    lens = np.full(n, steps * STEP, np.uint64)
    stride = steps * STEP if stride is None else stride
    return np.arange(n, dtype=np.uint64) * np.uint64(stride), lens


def seeds_for(n, tag):
    return np.random.default_rng(tag).integers(0, 2 ** 32, n, dtype=np.uint64).astype(np.uint32)


def run(plan, data, n, seeds=None, cid=None):
    """One launch; the outputs as uint32.  cid: a chunk-id map (chunk i's seed
    and output at index cid[i]), as the host pipeline launches its groups."""
    import torch
    out = torch.full((n,), 0x5EED5EED, dtype=torch.int32, device=data.device)
    st = None if seeds is None else torch.from_numpy(seeds.view(np.int32)).to(data.device)
    if cid is None:
        plan.exec(data, out, seeds=st)
    else:
        ct = torch.from_numpy(cid.view(np.int32)).to(data.device)
        f = cio.lib().cioa_debug_plan_exec_cid
        f.argtypes = [ctypes.c_void_p] * 6
        f.restype = ctypes.c_int
        stream = torch.cuda.current_stream().cuda_stream
        assert f(plan._handle, data.data_ptr(), None if st is None else st.data_ptr(), out.data_ptr(),
                 ct.data_ptr(), stream) == 0
    torch.cuda.synchronize()
    return out.cpu().numpy().view(np.uint32).copy()


def zref(host, offs, lens, seeds=None):
    """Raw crc_update(seed, chunk) of every chunk, by zlib."""
    mv = memoryview(host)
    out = np.empty(len(offs), np.uint32)
    for i, (o, l) in enumerate(zip(offs.tolist(), lens.tolist())):
        s = 0xFFFFFFFF if seeds is None else int(seeds[i])
        out[i] = zlib.crc32(mv[o:o + l], s ^ 0xFFFFFFFF) ^ 0xFFFFFFFF
    return out


def child_main(path):
    """In the child process (CIO_GPU_DIAG=1 CIO_GPU_ALIGNED=0): every shape on
    the issue-ahead kernel, plain and with seeds."""
    import torch
    dev = torch.device("cuda:0")
    W = grid_waves()
    data = make_data(dev, W)
    res = {}
    for p, q in PQ:
        n = W // p
        offs, lens = batch(n, p * q)
        with cio.Crc32Plan(offs, lens) as plan:
            assert not plan.aligned and plan.kernel_name() == "crc32_stream_kernel"
            res[f"plain_{p}_{q}"] = run(plan, data, n)
            res[f"seeds_{p}_{q}"] = run(plan, data, n, seeds=seeds_for(n, 100 * p + q))
    np.savez(path, **res)


@pytest.fixture(scope="module")
def waves(cuda):
    return grid_waves()


@pytest.fixture(scope="module")
def data(cuda, waves):
    t = make_data(cuda, waves)
    return t, t.cpu().numpy()


@pytest.fixture(scope="module")
def old_path(cuda, tmp_path_factory):
    """Outputs of the same batches with the aligned path switched off, from a
    fresh process (the switch is read at plan creation, under the gate)."""
    path = str(tmp_path_factory.mktemp("aligned") / "old.npz")
    env = {k: v for k, v in os.environ.items() if k not in SWITCHES}
    env.update(CIO_GPU_DIAG="1", CIO_GPU_ALIGNED="0")
    here = os.path.dirname(os.path.abspath(__file__))
    code = (f"import sys; sys.path.insert(0, {os.path.dirname(here)!r}); sys.path.insert(0, {here!r}); "
            f"import test_gpu_crc_aligned as t; t.child_main({path!r})")
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    return np.load(path)


@pytest.mark.parametrize("p,q", PQ)
def test_aligned_shapes(cuda, waves, data, old_path, p, q):
    dev, host = data
    n = waves // p
    offs, lens = batch(n, p * q)
    seeds = seeds_for(n, 100 * p + q)
    with cio.Crc32Plan(offs, lens) as plan:
        assert plan.aligned and plan.kernel_name() == "crc32_stream_kernel" and plan.workgroups * 16 == waves
        want = zref(host, offs, lens)
        got = run(plan, dev, n)
        assert np.array_equal(got, want)
        assert np.array_equal(got, old_path[f"plain_{p}_{q}"])
        want_s = zref(host, offs, lens, seeds)
        got_s = run(plan, dev, n, seeds=seeds)
        assert np.array_equal(got_s, want_s)
        assert np.array_equal(got_s, old_path[f"seeds_{p}_{q}"])
        # a chunk-id map: chunk i's seed and output live at index cid[i]
        cid = np.random.default_rng(7 * p + q).permutation(n).astype(np.uint32)
        got_c = run(plan, dev, n, cid=cid)
        assert np.array_equal(got_c[cid], want)
        by_id = np.empty(n, np.uint32)
        by_id[cid] = want_s                 # seeds[cid[i]] seeds chunk i
        sc = np.empty(n, np.uint32)
        sc[cid] = seeds
        got_cs = run(plan, dev, n, seeds=sc, cid=cid)
        assert np.array_equal(got_cs, by_id)
    # padded stride: 128 bytes between chunks
    offs_p, lens_p = batch(n, p * q, stride=p * q * STEP + PAD)
    with cio.Crc32Plan(offs_p, lens_p) as plan:
        assert plan.aligned
        assert np.array_equal(run(plan, dev, n), zref(host, offs_p, lens_p))
        assert np.array_equal(run(plan, dev, n, seeds=seeds), zref(host, offs_p, lens_p, seeds))


@pytest.mark.parametrize("p,q", PQ)
def test_neighbours_take_the_old_path(cuda, waves, data, p, q):
    """One chunk more or fewer, one step more or fewer per chunk: not in the
    class, same answers."""
    dev, host = data
    n, steps = waves // p, p * q
    for nn, ss in ((n + 1, steps), (n - 1, steps), (n, steps + 1), (n, steps - 1)):
        if ss < 1:
            continue
        offs, lens = batch(nn, ss)
        with cio.Crc32Plan(offs, lens) as plan:
            assert not plan.aligned, (nn, ss)
            assert np.array_equal(run(plan, dev, nn), zref(host, offs, lens)), (nn, ss)


@pytest.mark.parametrize("p,q", [(2, 1), (4, 2), (8, 3), (16, 4), (4, 5)])
def test_repeated_launches(cuda, waves, data, p, q):
    """Two back-to-back launches of one plan into different outputs, then the
    same again: the kernel leaves no state behind."""
    import torch
    dev, host = data
    n = waves // p
    offs, lens = batch(n, p * q)
    want = zref(host, offs, lens)
    with cio.Crc32Plan(offs, lens) as plan:
        assert plan.aligned
        for _ in range(2):
            o1 = torch.zeros(n, dtype=torch.int32, device=cuda)
            o2 = torch.full((n,), -1, dtype=torch.int32, device=cuda)
            plan.exec(dev, o1)
            plan.exec(dev, o2)
            torch.cuda.synchronize()
            assert np.array_equal(o1.cpu().numpy().view(np.uint32), want)
            assert np.array_equal(o2.cpu().numpy().view(np.uint32), want)


def test_ring_over_an_aligned_plan(cuda, waves, data):
    """Crc32Ring (depth 2) over an aligned geometry: four batches at different
    bases of the buffer, equal to the batch-by-batch results."""
    import torch
    dev, host = data
    p, q = 4, 3
    n = waves // p
    offs, lens = batch(n, p * q)
    shifts = [0, 128, 4096, 2 * STEP + 256]
    with cio.Crc32Plan(offs, lens) as plan:
        assert plan.aligned
        single = [run(plan, dev[s:], n) for s in shifts]
    for s, got in zip(shifts, single):
        assert np.array_equal(got, zref(host[s:], offs, lens))
    with cio.Crc32Ring(offs, lens, depth=2) as ring:
        outs = [torch.zeros(n, dtype=torch.int32, device=cuda) for _ in shifts]
        for s, o in zip(shifts, outs):
            ring.exec(dev[s:], o)
        ring.join()
        torch.cuda.synchronize()
        for o, want in zip(outs, single):
            assert np.array_equal(o.cpu().numpy().view(np.uint32), want)
