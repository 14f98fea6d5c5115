"""cio_file_alloc_set_batch_dev (include/chunkio_amd/cio_persist_dev.h)
against the numpy model (alloc_set_model.py).  Every call is compared bit for
bit in ALL it may touch: the WHOLE buffer (a position-dependent sentinel fills
it, so a stray store shows, and without CIOA_ALLOC_ZERO no byte may change),
every output array, the set's arrays (two sentinel entries behind them) and
words, the arena, every word of dev_total and the statuses.  No tolerance
anywhere.  The workgroup is 1024 entries, so the widths are both sides of it
and of two of them."""
import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import alloc_set_model as model
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, u64
from test_gpu_pool_dev import same_bytes
from test_gpu_pool_set import PoolSet
from write_dev_move_model import m_init

pytestmark = pytest.mark.gpu

ZERO = cf.CIOA_ALLOC_ZERO
CLS = (100, 300, 700, 1500, 2000, 2500, 3000, 4000)        # needs run from 24 to a few KiB
WIDTHS = [1, 1023, 1024, 1025, 2049]
NONE = model.NONE


def make_set(cuda, n_cls, align, stride, have, bad=(), words=None):
    """n_cls classes of CLS with `have` entries each (a list), the entries at
    multiples of max(align, 128) from the buffer's start, capacity cls + e % 3.
    bad: (class, entry, kind) entries that fail S3's check.  Returns (set or
    None, the first byte behind the entries)."""
    step = max(align, 128)
    at, entries = 0, []
    for k in range(n_cls):
        ent = []
        for e in range(stride):
            ent.append((at, CLS[k] + e % 3))
            at += -(-(CLS[k] + 3) // step) * step
        entries.append(ent[:have[k]])
    for k, e, kind in bad:
        o, c = entries[k][e]
        entries[k][e] = {"outside": ((1 << 40) + 4096 * e, c), "small": (o, CLS[k] - 1),
                         "misaligned": (o + 1, c - 1), "wraps": ((1 << 64) - 8, c)}[kind]
    if n_cls == 0:
        return None, at
    return PoolSet(cuda, [(CLS[k], 4096) for k in range(n_cls)], stride, entries=entries, words=words), at


def needs_for(rng, n, n_cls):
    edge = [24] + [c + d for c in CLS[:n_cls] for d in (-1, 0, 1)]
    pick = rng.integers(0, 10, n)
    need = np.where(pick == 0, rng.choice([0, 23], n),
                    np.where(pick < 4, rng.choice(edge, n), rng.integers(24, 4200, n))).astype(np.uint64)
    return need


def run(cuda, w, buf, base_t, need, gate, arena, arena_t, pset, align, flags, what):
    """One device call and the model's, compared in everything."""
    import torch
    n = len(need)
    n_cls = 0 if pset is None else pset.n_cls
    total = dev_i64([0x55] * (2 + n_cls), cuda)
    status = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    out_offs, out_caps = dev_i64([0x77] * n, cuda), dev_i64([0x77] * n, cuda)
    cf.alloc_set_batch_dev(w, base_t, dev_i64(need, cuda), arena_t, set=None if pset is None else pset.arg(),
                           gate=None if gate is None else dev_i32(np.asarray(gate, np.int32).view(np.uint32), cuda),
                           align=align, flags=flags, out_offs=out_offs, out_caps=out_caps, total=total,
                           status=status)
    margs = ([], [], [], 0, 0) if pset is None else pset.model_args()
    want = model.m_alloc_set(buf, need, gate, arena, *margs, align=align, flags=flags)
    assert np.array_equal(status.cpu().numpy(), want[0]), (what, "status")
    assert u64(total).tolist() == want[1], (what, "total", u64(total).tolist(), want[1])
    assert u64(out_offs).tolist() == want[2], (what, "out_offs")
    assert u64(out_caps).tolist() == want[3], (what, "out_caps")
    assert u64(arena_t).tolist() == arena, (what, "arena", u64(arena_t).tolist(), arena)
    if pset is not None:
        pset.check(what)
    same_bytes(base_t, buf, what)
    return want


@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("n_cls", [0, 1, 3, 8])
@pytest.mark.parametrize("n", WIDTHS)
def test_mixed_batches_equal_the_model(cuda, n, n_cls, align):
    """Needs of 0, 23, 24, both sides of every class and up to a few KiB,
    mixed gates in every other case, classes that run dry in mid-batch (class k
    has 3 + 5 k entries), three entries that fail S3's check and are consumed,
    and in every third case an arena that ends in mid-batch -- the pool-served
    entries behind the cut are still accepted.  Every other case zeroes."""
    case = WIDTHS.index(n) + 5 * [0, 1, 3, 8].index(n_cls) + 20 * [1, 16, 4096].index(align)
    rng = np.random.default_rng(1000 + case)
    need = needs_for(rng, n, n_cls)
    gate = None if case % 2 else rng.choice([0, 0, 0, -1, -3, 1], n).astype(np.int32)
    have = [3 + 5 * k for k in range(n_cls)]
    bad = [(k, 1, kind) for k, kind in zip(range(n_cls), ("outside", "small", "misaligned", "wraps"))]
    pset, top = make_set(cuda, n_cls, align, 40, have, bad=bad)
    reach = [int(x) for i, x in enumerate(need) if x >= 24 and (gate is None or gate[i] == 0)]
    room = len(reach) * (-(-4200 // align) * align) + 2 * 4096
    top += 5                                      # an unaligned top: the gap is part of dev_total[0]
    end = top + (6 * (-(-4200 // align) * align) if case % 3 == 0 else room)    # the cut: while the classes serve
    buf = fill(top + room + 64)
    arena = [top, end]
    base_t, arena_t = dev_u8(buf, cuda), dev_i64(arena, cuda)
    with cio.DevWriter(n) as w:
        want = run(cuda, w, buf, base_t, need, gate, arena, arena_t, pset, align, ZERO if case % 2 == 0 else 0,
                   f"case {case}")
    st = want[0]
    if case % 3 == 0 and n >= 1023:
        cut = int(np.flatnonzero((st != 0) & (need >= 24) & (True if gate is None else gate == 0))[0])
        assert st[:cut].tolist().count(0) > 0
        if n_cls:                                 # a pool-served entry behind the arena's cut
            assert any(st[i] == 0 and want[2][i] < top - 5 for i in range(cut, n))
    if n_cls and n >= 1023:
        assert want[1][1] == sum(have)            # every class ran dry
        assert sum(1 for i in range(n) if st[i] != 0 and need[i] >= 24 and (gate is None or gate[i] == 0)) >= 1


def test_an_unsound_set_is_the_arena_alone(cuda):
    n, align = 1025, 16
    rng = np.random.default_rng(7)
    need = needs_for(rng, n, 3)
    for words_of in (lambda w: w[:6] + [w[2]] + w[7:],      # cls not rising
                     lambda w: [41] + w[1:],                 # more entries than the capacity
                     lambda w: w[:5] + [41] + w[6:]):        # a capacity above the stride
        pset, top = make_set(cuda, 3, align, 40, [3, 8, 13])
        pset.words = words_of(pset.words)
        pset.words_t.copy_(dev_i64(pset.words, cuda))
        buf = fill(top + n * 4208 + 64)
        arena = [top, len(buf) - 64]
        base_t, arena_t = dev_u8(buf, cuda), dev_i64(arena, cuda)
        before = list(pset.words)
        with cio.DevWriter(n) as w:
            want = run(cuda, w, buf, base_t, need, None, arena, arena_t, pset, align, 0, "unsound")
        assert pset.words == before and want[1][1:] == [0, 0, 0, 0]
        assert all(want[3][i] == int(need[i]) for i in range(n) if want[0][i] == 0)


def test_without_zero_no_byte_changes_and_with_it_only_the_slots(cuda):
    """The same batch twice over a sentinel-filled buffer.  Without
    CIOA_ALLOC_ZERO the buffer is bit for bit what it was (run() compares the
    whole buffer with the model, which does not touch it); with it exactly the
    slots handed out are zero, the pool entries with their whole capacity."""
    n, align = 1025, 16
    rng = np.random.default_rng(11)
    need = needs_for(rng, n, 3)
    for flags in (0, ZERO):
        pset, top = make_set(cuda, 3, align, 40, [30, 30, 30])
        buf = fill(top + n * 4208 + 64)
        untouched = buf.copy()
        arena = [top + 3, len(buf) - 64]
        base_t, arena_t = dev_u8(buf, cuda), dev_i64(arena, cuda)
        with cio.DevWriter(n) as w:
            want = run(cuda, w, buf, base_t, need, None, arena, arena_t, pset, align, flags, f"flags {flags}")
        if not flags:
            assert np.array_equal(buf, untouched)
        else:
            mask = np.zeros(len(buf), bool)
            for i in range(n):
                if want[0][i] == 0:
                    assert not mask[want[2][i]:want[2][i] + want[3][i]].any()     # disjoint slots
                    mask[want[2][i]:want[2][i] + want[3][i]] = True
            assert not buf[mask].any() and np.array_equal(buf[~mask], untouched[~mask])
            assert sum(1 for i in range(n) if want[0][i] == 0 and want[2][i] < top) == 90


def test_capture_alloc_then_init_replayed_twice(cuda):
    """alloc_set -> init on one stream, captured once and replayed twice: the
    two replays yield disjoint slots, every slot holds a fresh image, and the
    arena top advances twice."""
    import torch
    n, align = 1025, 16
    rng = np.random.default_rng(13)
    need = rng.integers(24, 600, n).astype(np.uint64)
    pset, top = make_set(cuda, 3, align, 40, [40, 40, 40])
    buf = fill(top + 3 * n * 720 + 64)
    arena = [top, len(buf) - 64]
    base_t, arena_t, need_t = dev_u8(buf, cuda), dev_i64(arena, cuda), dev_i64(need, cuda)
    total = dev_i64([0] * 5, cuda)
    status = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    ist = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    crc = torch.zeros(n, dtype=torch.int32, device=cuda)
    out_offs, out_caps = dev_i64([0] * n, cuda), dev_i64([0] * n, cuda)

    def call():
        cf.alloc_set_batch_dev(w, base_t, need_t, arena_t, set=pset.arg(), align=align, out_offs=out_offs,
                               out_caps=out_caps, total=total, status=status)
        cf.init_batch_dev(w, base_t, out_offs, out_caps, status=ist, crc_cur=crc)

    def model_round():
        want = model.m_alloc_set(buf, need, None, arena, *pset.model_args(), align=align)
        for i in range(n):
            assert want[0][i] == 0
            m_init(buf, want[2][i])
        return want

    seen, tops = [], [arena[0]]
    with cio.DevWriter(n) as w:
        want = model_round()
        call()                                    # warm-up outside the capture (a round like the others)
        torch.cuda.synchronize()
        seen.append(want)
        tops.append(arena[0])
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        same_bytes(base_t, buf, "capture runs nothing")
        for k in (1, 2):
            want = model_round()
            status.fill_(99)
            ist.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any() and not ist.cpu().numpy().any(), k
            assert u64(out_offs).tolist() == want[2] and u64(out_caps).tolist() == want[3], k
            assert u64(arena_t).tolist() == arena and u64(total).tolist() == want[1], k
            pset.check(f"replay {k}")
            same_bytes(base_t, buf, f"replay {k}")
            seen.append(want)
            tops.append(arena[0])
        del graph
    assert tops[0] < tops[1] < tops[2] < tops[3]
    taken = sorted((o, o + c) for want in seen for o, c in zip(want[2], want[3]))
    assert all(a[1] <= b[0] for a, b in zip(taken, taken[1:]))            # disjoint across the replays
