"""Coalescing a pool set's free slots in device memory
(include/chunkio_amd/cio_write_dev_coalesce.h) against the numpy model
(coalesce_model.py).  Every call is compared bit for bit in ALL it may touch:
the set words, both arrays whole (two sentinel entries behind them, so a store
beyond them shows) and dev_total (a sentinel word behind it).  No tolerance
anywhere.  The call touches no slot byte, so dev_bytes is nominal -- 2^36 ..
2^44 -- and nothing large is allocated; only Drift runs on real images, in
lock step with the models of the whole chain."""
import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import coalesce_model as model
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, u64
from test_gpu_pool_dev import same_bytes
from test_gpu_rotate_dev import CK, S64, u32

pytestmark = pytest.mark.gpu

DRY = cf.COALESCE_DRY
CLASSES = [(527, 32), (1280, 32), (1792, 32), (2304, 32), (3000, 32), (5000, 32), (9000, 32), (20000, 32)]
WRITER = 4096                                 # n_cls * stride of most tests, and their writer


@pytest.fixture(scope="module")
def writer(cuda):
    with cio.DevWriter(WRITER) as w:
        yield w


def dev_u64(a, cuda):
    """dev_i64 for values up to 2^64 - 1 (an ill-formed entry's offset)."""
    return dev_i64(np.array([int(x) for x in a], dtype=object).astype(np.uint64), cuda)


class DevSet:
    """A pool set on the device and the host copy beside it, two sentinel
    entries behind the arrays."""

    def __init__(self, cuda, so, sc, words, n_cls, stride):
        self.cuda, self.n_cls, self.stride = cuda, n_cls, stride
        self.so, self.sc, self.words = list(so), list(sc), list(words)
        self.so_t, self.sc_t = dev_u64(self.so + [S64] * 2, cuda), dev_u64(self.sc + [S64] * 2, cuda)
        self.words_t = dev_i64(self.words, cuda)

    def arg(self):
        return (self.so_t, self.sc_t, self.words_t, self.n_cls, self.stride)

    def coalesce(self, w, dev_bytes, target, align, flags=0, what=""):
        """One device call and the model's, compared in everything.  Returns
        the model's dev_total."""
        total = dev_i64([0x55] * (5 + self.n_cls + 1), self.cuda)
        cf.coalesce_set_dev(w, dev_bytes, self.arg(), target, align=align, flags=flags, total=total)
        want = model.m_coalesce_set(self.so, self.sc, self.words, self.n_cls, self.stride, dev_bytes, target, align,
                                    flags)
        got = u64(total).tolist()
        assert got == want + [0x55], (what, "dev_total", got, want)
        self.check(what)
        return want

    def check(self, what=""):
        assert u64(self.words_t).tolist() == self.words, (what, "set words", u64(self.words_t).tolist(), self.words)
        got_o, got_c = u64(self.so_t).tolist(), u64(self.sc_t).tolist()
        if got_o != self.so + [S64] * 2 or got_c != self.sc + [S64] * 2:
            bad = [i for i in range(len(self.so)) if got_o[i] != self.so[i] or got_c[i] != self.sc[i]]
            raise AssertionError((what, "set arrays", len(bad), bad[:4],
                                  [(got_o[i], got_c[i], self.so[i], self.sc[i]) for i in bad[:4]]))


def coalesce_twice(cuda, w, made, n_cls, stride, dev_bytes, target, align, what):
    """The call, and the call again on its result (C9)."""
    s = DevSet(cuda, *made, n_cls, stride)
    first = s.coalesce(w, dev_bytes, target, align, what=what)
    if first[0] == 0:
        before = (list(s.so), list(s.sc), list(s.words))
        again = s.coalesce(w, dev_bytes, target, align, what=what + ", again")
        assert again[:5] == [0, 0, 0, 0, 0] and again[5:] == first[5:], (what, again)
        assert (s.so, s.sc, s.words) == before, what
    return first


# ------------------------------------------------------------------ 1. sizes

@pytest.mark.parametrize("entries", [0, 1, 63, 64, 65, 1023, 1024, 1025, 2049, 3077])
def test_entry_counts_on_both_sides_of_a_wave_and_a_workgroup(cuda, writer, entries):
    """n_cls * stride = 4096 = the writer's max_chunks; the entries straddle
    every boundary of the sorted order: the well-formed ones are a prefix of
    it, the survivors a subset, the outputs fewer again."""
    for seed, (align, adjacent) in enumerate([(32, 0.7), (4096, 0.9)]):
        dev_bytes = (1 << 36) if align == 32 else (1 << 43)
        classes = [(c * (align // 32), align) for c, _ in CLASSES[:4]]        # slots of a few `align` each
        made = model.make_set(1000 * entries + seed, classes, 1024, entries, dev_bytes, align, adjacent=adjacent)
        assert sum(made[2][0::4]) == entries
        total = coalesce_twice(cuda, writer, made, 4, 1024, dev_bytes, 3, align, f"{entries} entries, align {align}")
        assert total[0] == 0
        if entries >= 63:
            assert total[3] > 0 and total[1] + total[2] > 0, total      # groups formed, bad entries dropped


# ------------------------------------------------------------------ 2. key widths

@pytest.mark.parametrize("units", [255, 257, 65535, 65537, (1 << 24) - 1, (1 << 24) + 1, (1 << 32) - 1])
def test_key_bound_on_both_sides_of_every_sort_pass(cuda, writer, units):
    """dev_bytes / align just below and above 2^8, 2^16 and 2^24 and at the
    largest value the call accepts: one to four passes of the sort, the
    sentinel one above the largest key, and an entry that has that key."""
    classes = [(24, 1), (40, 1), (96, 1), (200, 1)]
    for align in (1, 64, 4096):
        dev_bytes = units * align
        classes = [(c, min(align, 32)) for c, _ in classes]
        made = model.make_set(units % 1000 + align, classes, 1024, 900, dev_bytes, align, adjacent=0.6,
                              caps=[24, 29, 40, 51, 96, 3 * align, 1])
        so, sc, words = made
        ents = [(so[k * 1024 + j], sc[k * 1024 + j]) for k in range(4) for j in range(words[4 * k])]
        if units > 300:                       # the smallest spaces cannot hold 900 slots
            assert len(ents) == 900
        assert any(o + c <= dev_bytes and o % align == 0 and o // align == units - 1 for o, c in ents if c), \
            "no well-formed entry has the last key"
        total = coalesce_twice(cuda, writer, made, 4, 1024, dev_bytes, 2, align, f"{units} units of {align}")
        assert total[0] in (0, 2)


# ------------------------------------------------------------------ 3. classes and targets

@pytest.mark.parametrize("n_cls", [2, 4, 8])
def test_every_class_count_and_every_legal_target(cuda, writer, n_cls):
    stride = WRITER // n_cls
    for target in range(1, n_cls):
        for pal in (32, 256):                 # the target's alignment above align: groups end on it
            classes = [(c, pal if k == target else 32) for k, (c, _) in enumerate(CLASSES[:n_cls])]
            made = model.make_set(n_cls * 100 + target * 10 + pal, classes, stride, 120 * n_cls, 1 << 36, 32,
                                  adjacent=0.85, bad=0.05, caps=[527, 532, 600, 96, 1, classes[-1][0]])
            total = coalesce_twice(cuda, writer, made, n_cls, stride, 1 << 36, target, 32,
                                   f"{n_cls} classes, target {target}, pal {pal}")
            assert total[0] == 0 and (total[3] > 0 or CLASSES[target][0] > 2304), total   # runs are ~2700 bytes


# ------------------------------------------------------------------ 4. structure

@pytest.mark.parametrize("entries", [63, 65, 1023, 1025, 2049])
@pytest.mark.parametrize("shape", ["one run", "none adjacent", "short tail", "aligned ends"])
def test_runs_and_groups_across_wave_and_workgroup_boundaries(cuda, writer, shape, entries):
    """One run holding every entry (its groups cross every wave and workgroup
    boundary of the sorted order); no two entries adjacent; runs whose tail
    lacks T bytes; groups ended by the target's alignment rather than by T."""
    align, dev_bytes = 32, 1 << 36
    classes = [(c, 32) for c, _ in CLASSES[:4]]
    if shape == "one run":
        made = model.make_set(entries, classes, 1024, entries, dev_bytes, align, adjacent=1.0, bad=0.0,
                              caps=[527, 600, 1280, 1792])
    elif shape == "none adjacent":
        made = model.make_set(entries, classes, 1024, entries, dev_bytes, align, adjacent=0.0, bad=0.0)
    elif shape == "short tail":               # runs of three 527-byte slots: 1615 bytes, T = 1792 at target 2
        made = model.make_set(entries, classes, 1024, entries, dev_bytes, align, adjacent=0.66, bad=0.0, caps=[527])
    else:
        classes[3] = (2304, 256)
        made = model.make_set(entries, classes, 1024, entries, dev_bytes, align, adjacent=0.97, bad=0.0,
                              caps=[527, 1280])
    target = 2 if shape == "short tail" else 3
    total = coalesce_twice(cuda, writer, made, 4, 1024, dev_bytes, target, align, f"{shape}, {entries}")
    assert total[0] == 0
    if shape == "one run":
        assert total[3] > 0 and total[4] >= entries - 8, total       # all but the run's tail and the top-key slot
    if shape == "none adjacent":
        assert total[3] == 0 and total[4] == 0, total
    if shape in ("short tail", "aligned ends"):
        assert total[3] > 0 and total[4] < entries, total


# ------------------------------------------------------------------ 5. all or nothing

@pytest.mark.parametrize("k", [0, 1, 2, 3])
def test_overflow_of_any_class_leaves_everything_untouched(cuda, writer, k):
    """Class k's capacity word is one below what the outputs need: verdict 2,
    the counts are reported, and no word of the set or its arrays changes."""
    classes = [(c, 32) for c, _ in CLASSES[:4]]
    # no overlaps here: which of two overlapping entries survives depends on where they are filed
    so, sc, words = model.make_set(50 + k, classes, 1024, 1500, 1 << 36, 32, adjacent=0.8, bad=0.0)
    dry = model.m_coalesce_set(list(so), list(sc), list(words), 4, 1024, 1 << 36, 3, 32, model.DRY)
    assert dry[0] == 0 and dry[5 + k] >= 2
    room = [1024] * 4
    room[k] = dry[5 + k] - 1                  # the same slots, class k's surplus filed elsewhere
    so, sc, words = model.make_set(50 + k, classes, 1024, 1500, 1 << 36, 32, adjacent=0.8, bad=0.0, room=room)
    assert sum(words[0::4]) == 1500 and words[4 * k + 1] == room[k]
    s = DevSet(cuda, so, sc, words, 4, 1024)
    total = s.coalesce(writer, 1 << 36, 3, 32, what=f"class {k} overflows")
    assert total[0] == 2 and total[5:] == dry[5:] and (s.so, s.sc, s.words) == (so, sc, words)


def test_dry_run_reports_and_changes_nothing(cuda, writer):
    classes = [(c, 32) for c, _ in CLASSES[:4]]
    made = model.make_set(77, classes, 1024, 2500, 1 << 36, 32, adjacent=0.8)
    s = DevSet(cuda, *made, 4, 1024)
    dry = s.coalesce(writer, 1 << 36, 3, 32, flags=DRY, what="dry")
    assert dry[0] == 0 and dry[3] > 0 and (s.so, s.sc, s.words) == tuple(list(x) for x in made)
    assert s.coalesce(writer, 1 << 36, 3, 32, what="then for real") == dry


@pytest.mark.parametrize("why", ["count", "cls", "pal", "capacity", "order"])
def test_unsound_set_changes_nothing(cuda, writer, why):
    classes = [(c, 32) for c, _ in CLASSES[:4]]
    so, sc, words = model.make_set(88, classes, 1024, 1200, 1 << 36, 32)
    at, value = {"count": (4 * 1, 1025), "cls": (2, 23), "pal": (4 * 2 + 3, 48), "capacity": (4 * 3 + 1, 1025),
                 "order": (4 * 2 + 2, 1280)}[why]
    words[at] = value
    s = DevSet(cuda, so, sc, words, 4, 1024)
    assert s.coalesce(writer, 1 << 36, 3, 32, what=why) == [1] + [0] * 8
    assert s.coalesce(writer, 1 << 36, 3, 32, flags=DRY, what=why + ", dry") == [1] + [0] * 8


# ------------------------------------------------------------------ 6. the drift

def test_drift_to_a_larger_class_is_served_from_coalesced_slots(cuda):
    """coalesce_model.Drift on the device, call by call in lock step with the
    models, on real images.  Phase 1 leaves 24 adjacent 1280-byte entries in
    class 1.  Phase 2 -- release_set of the list, coalesce, grow_set -- is
    CAPTURED ONCE as a graph and replayed twice: the first replay turns the 24
    entries into 12 class-3 slots and grows every image into one, the arena's
    top standing still; the second finds nothing to do.  The arm without the
    call, from the same state, runs out of arena: statuses other than CIO_OK."""
    import torch
    ZERO, COMPACT = cf.CIOA_RELEASE_ZERO, cf.CIOA_RELEASE_COMPACT
    for arm in (True, False):
        m = model.Drift(coalesce=arm)
        p = m.p
        n, align, list_cap = p["n"], p["align"], p["list_cap"]
        s = DevSet(cuda, m.so, m.sc, m.words, m.n_cls, m.stride)
        base_t, offs_t, caps_t = dev_u8(m.buf, cuda), dev_i64(m.offs, cuda), dev_i64(m.caps, cuda)
        arena_t, crc_t, count_t = dev_i64(m.arena, cuda), dev_i32(m.crc, cuda), dev_i64(m.count, cuda)
        lo_t, lc_t, li_t = dev_i64(m.lo, cuda), dev_i64(m.lc, cuda), dev_i32(m.li, cuda)
        src_t, so_t = dev_u8(m.src, cuda), dev_i64(m.src_offs, cuda)
        sl_t = dev_i64(np.full(n, p["size"], np.uint64), cuda)
        need_t = dev_i64([p["need1"]] * n, cuda)
        cls0 = cf.pool_set_class(s.arg(), 0)

        def st(k):
            return torch.full((k,), 99, dtype=torch.int32, device=cuda)
        go = dict(total=dev_i64([0] * 6, cuda), status=st(n), prev_offs=dev_i64([0] * n, cuda),
                  prev_caps=dev_i64([0] * n, cuda))
        rp = dict(total=dev_i64([0] * 6, cuda), status=st(n))
        ro = dict(total=dev_i64([0, 0], cuda), status=st(n))
        rl = dict(total=dev_i64([0] * 6, cuda), status=st(list_cap))
        ct = dev_i64([0x55] * 9, cuda)
        wst = st(n)

        def settle(what):
            torch.cuda.synchronize()
            s.so, s.sc, s.words = m.so, m.sc, m.words
            s.check(what)
            for t, v, name in ((offs_t, m.offs, "offsets"), (caps_t, m.caps, "capacities"), (arena_t, m.arena, "arena"),
                               (count_t, m.count, "count"), (lo_t, m.lo, "list offsets"), (lc_t, m.lc, "list caps")):
                assert u64(t).tolist() == v, (what, name, u64(t).tolist(), v)
            assert u32(crc_t).tolist() == m.crc and u32(li_t).tolist() == m.li, (what, "crc, list images")
            same_bytes(base_t, m.buf, what)

        def same(o, want, what):
            assert np.array_equal(o["status"].cpu().numpy(), want[0]), (what, "status", o["status"].cpu().numpy())
            assert u64(o["total"]).tolist() == want[1], (what, "total", u64(o["total"]).tolist(), want[1])

        def grow():
            cf.grow_set_batch_dev(w, base_t, offs_t, caps_t, need_t, arena_t, s.arg(), realloc=p["realloc"],
                                  page=p["page"], align=align, **go)

        with cio.DevWriter(m.n_cls * m.stride) as w:
            for r in range(2):                    # phase 1
                grow()
                want = m.grow(p["need1"])
                same(go, want, f"phase 1.{r} grow")
                assert not want[0].any() and want[1][0] == 12 * 1280 and want[4] == []
                cf.release_set_batch_dev(w, base_t, go["prev_offs"], go["prev_caps"], s.arg(), live_offs=offs_t, **rp)
                same(rp, m.release_prev(), f"phase 1.{r} release")
                cf.write_batch_dev(w, base_t, offs_t, caps_t, src_t, so_t, sl_t, crc_t, flags=CK, status=wst)
                m.write()
                cf.rotate_pool_batch_dev(w, base_t, offs_t, caps_t, None, limit=p["limit"], new_cap=p["new_cap"],
                                         align=align, arena=arena_t, pool_offs=cls0[0], pool_caps=cls0[1],
                                         pool=cls0[2], out_offs=lo_t, out_caps=lc_t, out_img=li_t,
                                         out_count=count_t, flags=CK, crc_cur=crc_t, **ro)
                want = m.rotate()
                same(ro, want, f"phase 1.{r} rotate")
                assert not want[0].any() and not wst.cpu().numpy().any()
                settle(f"phase 1.{r}")
            assert m.count[0] == 24
            top1 = m.arena[0]
            need_t.fill_(p["need2"])

            def phase2():
                cf.release_set_batch_dev(w, base_t, lo_t, lc_t, s.arg(), img=li_t, count=count_t,
                                         flags=ZERO | COMPACT, **rl)
                if arm:
                    cf.coalesce_set_dev(w, len(m.buf), s.arg(), p["target"], align=align, total=ct)
                grow()

            if arm:                               # every kernel has run once before the capture
                cf.coalesce_set_dev(w, len(m.buf), s.arg(), p["target"], align=align, flags=DRY, total=ct)
                assert u64(ct).tolist() == m.coalesce_set(model.DRY)
            torch.cuda.synchronize()
            graph = torch.cuda.CUDAGraph()
            with torch.cuda.graph(graph):
                phase2()
            torch.cuda.synchronize()
            settle("capture runs nothing")
            for replay in range(2):
                for t in (rl["status"], go["status"]):
                    t.fill_(99)
                graph.replay()
                what = f"phase 2, replay {replay}, coalesce {arm}"
                want = m.release_list()
                same(rl, want, what + ": release")
                assert not want[0].any()
                if arm:
                    total = m.coalesce_set()
                    assert u64(ct).tolist() == total, (what, u64(ct).tolist(), total)
                    assert total == ([0, 0, 0, 12, 24, 0, 0, 0, 12] if replay == 0 else [0] * 9), total
                want = m.grow(p["need2"])
                same(go, want, what + ": grow")
                settle(what)
                if replay == 0 and arm:
                    assert not want[0].any() and want[4] == list(range(n)) and m.caps == [2560] * n
                    assert m.arena[0] == top1, "the arena's top moved"
                if replay == 0 and not arm:
                    assert want[0].tolist() == [0] * 6 + [-1] * 6 and want[1][0] == 12 * 2304
                    assert m.arena[0] == top1 + 6 * 2304 == m.arena[1]
            del graph
