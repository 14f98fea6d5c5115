"""Growing chunk images in device memory out of an arena
(include/chunkio_amd/cio_write_dev_grow.h) against the numpy model
(grow_dev_model.py).  Every grow call is compared in ALL it may touch: the
WHOLE buffer (a position-dependent sentinel fills every slack and the arena, so
a stray or missing store shows), both arrays, the arena's top, dev_total, the
statuses and prev_*."""
import os

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import grow_dev_model as model
from write_dev_move_model import m_init, m_seal, m_write

pytestmark = pytest.mark.gpu

CK, ZERO = cf.CIO_CHECKSUM, cf.CIOA_GROW_ZERO
BLOCK = 1024                                  # kGrowBlock: images per workgroup of the header kernel
SIZES = [430080, 823296, 1249280, 1642496, 2068480]


# ------------------------------------------------------------------ helpers

def dev_i64(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(cuda)


def dev_u8(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(cuda)


def dev_i32(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(cuda)


def u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def fill(nbytes):
    """The sentinel: depends on the position, no long run of one value, no zero."""
    i = np.arange(nbytes, dtype=np.uint64)
    return ((i * 37 + (i >> 8) * 11) % 253 + 1).astype(np.uint8)


def put_image(buf, off, meta, content):
    """A valid image header (zero CRC field) with meta / content BYTES of a pattern."""
    buf[off:off + 24] = 0
    buf[off], buf[off + 1] = 0xC1, 0x00
    buf[off + 10:off + 14] = np.frombuffer(int(content).to_bytes(4, "big"), np.uint8)
    buf[off + 22:off + 24] = np.frombuffer(int(meta).to_bytes(2, "big"), np.uint8)
    k = np.arange(meta + content, dtype=np.uint64)
    buf[off + 24:off + 24 + meta + content] = ((k * 131 + off * 7 + 17) % 251 + 1).astype(np.uint8)
    return 24 + meta + content


class State:
    """Images and an arena in one device buffer, the host copy beside it; both
    are carried from call to call."""

    def __init__(self, cuda, buf, offs, caps, arena):
        self.cuda = cuda
        self.buf = buf
        self.offs, self.caps = [int(x) for x in offs], [int(x) for x in caps]
        self.arena = [int(arena[0]), int(arena[1])]
        self.n = len(self.offs)
        self.base_t = dev_u8(buf, cuda)
        self.offs_t, self.caps_t = dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)
        self.arena_t = dev_i64(self.arena, cuda)

    def outs(self):
        import torch
        return dict(prev_offs=dev_i64(np.full(self.n, 0x77, np.uint64), self.cuda),
                    prev_caps=dev_i64(np.full(self.n, 0x77, np.uint64), self.cuda),
                    total=dev_i64([0x55], self.cuda),
                    status=torch.full((self.n,), 99, dtype=torch.int32, device=self.cuda))

    def grow(self, w, need=None, recs=None, what="", **kw):
        """One device call (the records variant with recs = (rec_img,
        rec_lens)) and the model's, compared in everything."""
        o = self.outs()
        if recs is None:
            st, total = cf.grow_batch_dev(w, self.base_t, self.offs_t, self.caps_t, dev_i64(need, self.cuda),
                                          self.arena_t, **kw, **o)
        else:
            st, total = cf.grow_records_batch_dev(w, self.base_t, self.offs_t, self.caps_t,
                                                  dev_i32(recs[0], self.cuda), dev_i64(recs[1], self.cuda),
                                                  self.arena_t, **kw, **o)
            need = model.needs_of(recs[0], recs[1], self.n)
        want = model.m_grow(self.buf, self.offs, self.caps, need, self.arena, **kw)
        self.compare(st, total, o, want, what)
        return want

    def compare(self, st, total, o, want, what):
        got = (st.cpu().numpy(), int(u64(total)[0]), u64(o["prev_offs"]), u64(o["prev_caps"]))
        for g, m, name in zip(got, want, ("status", "total", "prev_offs", "prev_caps")):
            assert np.array_equal(g, m), (what, name, g, m)
        self.check(what)

    def check(self, what=""):
        assert u64(self.offs_t).tolist() == self.offs, (what, "offsets")
        assert u64(self.caps_t).tolist() == self.caps, (what, "capacities")
        assert u64(self.arena_t).tolist() == self.arena, (what, "arena", u64(self.arena_t).tolist(), self.arena)
        got = self.base_t.cpu().numpy()
        if not np.array_equal(got, self.buf):
            bad = np.flatnonzero(got != self.buf)
            raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:6]} of {len(got)}")


def layout(items, arena_room, gap=lambda i: (5 * i + 3) % 16 + 1, residue=None, resident=()):
    """One sentinel buffer: image i = (meta, content, room) after gap(i) bytes
    (or at the next offset that is residue(i) modulo 16), then the arena of
    arena_room bytes, the images `resident` placed INSIDE it at its far end.
    Returns (buf, offs, caps, arena)."""
    offs, caps, pos = [None] * len(items), [], 0
    for i, (meta, content, room) in enumerate(items):
        caps.append(24 + meta + content + room)
        if i in resident:
            continue
        pos += gap(i) if residue is None else (residue(i) - pos) % 16
        offs[i] = pos
        pos += caps[i]
    top = pos + 29
    pos = top + arena_room
    for i in resident:
        offs[i] = pos + 3
        pos += caps[i] + 9
    end = pos
    buf = fill(end + 41)
    for i, (meta, content, room) in enumerate(items):
        put_image(buf, offs[i], meta, content)
    return buf, offs, caps, [top, end]


# ------------------------------------------------------------------ 1. mixed batches

KINDS = ("over", "none", "fits", "exact", "magic", "used", "arena")


def mixed(n, realloc, page, align):
    """Image i of kind KINDS[i % 7]: grows by one byte too many; no need; need
    below the room; need of exactly the room; bad magic; used > cap; an image
    inside the arena's free part."""
    rng = np.random.default_rng(n)
    items, need, bound = [], [], 0
    for i in range(n):
        kind = KINDS[i % 7]
        meta, content, room = int(rng.integers(0, 40)) * (i % 3 == 0), int(rng.integers(0, 200)), int(
            rng.integers(2, 90))
        items.append((meta, content, room))
        need.append({"over": room + 1 + (i % 5) * 40, "none": 0, "fits": room - 1, "exact": room}.get(kind, room + 7))
        bound += model.round_up(model.round_up(24 + meta + content + room + need[-1] + realloc, page), align) + align
    resident = [i for i in range(n) if KINDS[i % 7] == "arena"]
    buf, offs, caps, arena = layout(items, bound, resident=resident)
    for i in range(n):
        if KINDS[i % 7] == "magic":
            buf[offs[i] + 1] = 0x01
        elif KINDS[i % 7] == "used":
            caps[i] = 24 + items[i][0] + items[i][1] - 1
    return buf, offs, caps, arena, need


@pytest.mark.parametrize("page", [1, 4096])
@pytest.mark.parametrize("align", [1, 16, 4096])
@pytest.mark.parametrize("n", [1, 2, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1])
def test_mixed_batches(cuda, n, align, page):
    realloc = (1, 100, 4096)[n % 3]
    buf, offs, caps, arena, need = mixed(n, realloc, page, align)
    s = State(cuda, buf, offs, caps, arena)
    with cio.DevWriter(n) as w:
        st, total, po, pc = s.grow(w, need, realloc=realloc, page=page, align=align, flags=ZERO * (n % 2),
                                   what=f"mixed {n} {align} {page}")
        want = [0 if KINDS[i % 7] in ("over", "none", "fits", "exact") else -1 for i in range(n)]
        assert st.tolist() == want
        grown = [i for i in range(n) if s.offs[i] != int(po[i])]
        assert grown == [i for i in range(n) if i % 7 == 0] and s.arena[0] > arena[0]
        # the same call again: everything now has room (or is still invalid), nothing moves
        top = s.arena[0]
        st2 = s.grow(w, need, realloc=realloc, page=page, align=align, what="again")[0]
        assert st2.tolist() == want and s.arena[0] == top


# ------------------------------------------------------------------ 2. the arena cut

@pytest.mark.parametrize("fit", range(8))
def test_arena_cut_and_retry(cuda, fit):
    """7 growing images and an arena that ends exactly behind the first `fit`
    slots (and one byte short of the next): the cut images stay byte for byte
    where they were, still valid, and a retry with a second arena of
    dev_total[0] bytes grows all of them."""
    align, page, realloc = 64, 1, 100
    items = [(i, 50 + 30 * i, 5) for i in range(7)] + [(0, 10, 50)]
    need = [6 + 100 * i for i in range(7)] + [3]
    slots = [model.round_up(model.new_capacity(24 + m + c + r, 24 + m + c, nd, realloc, page), align)
             for (m, c, r), nd in zip(items[:7], need)]
    buf, offs, caps, arena = layout(items, 3 * sum(slots) + 4 * align)
    top = arena[0]
    base = model.round_up(top, align)
    end = base + sum(slots[:fit]) + (slots[fit] - 1 if fit < 7 else 0)
    s = State(cuda, buf, offs, caps, [top, end])
    before = buf.copy()
    with cio.DevWriter(8) as w:
        st, total, po, pc = s.grow(w, need, realloc=realloc, page=page, align=align, flags=ZERO, what=f"cut {fit}")
        assert st.tolist() == [0] * fit + [-1] * (7 - fit) + [0]
        assert total == base - top + sum(slots) and s.arena[0] == (base + sum(slots[:fit]) if fit else top)
        for i in range(fit, 7):
            assert (s.offs[i], s.caps[i]) == (offs[i], caps[i])
            assert np.array_equal(s.buf[offs[i]:offs[i] + caps[i]], before[offs[i]:offs[i] + caps[i]])
            assert model.image_check(s.buf, len(s.buf), offs[i], caps[i]) is not None
        # the retry: a fresh arena of dev_total[0] bytes behind the first, at the same residue
        top2 = end + (top - end) % align + align
        s.arena = [top2, top2 + total]
        s.arena_t = dev_i64(s.arena, cuda)
        st = s.grow(w, need, realloc=realloc, page=page, align=align, flags=ZERO, what=f"retry {fit}")[0]
        assert not st.any() and all(c >= 24 + m + k + nd for c, (m, k, r), nd in zip(s.caps, items, need))


# ------------------------------------------------------------------ 3. copy alignment

@pytest.mark.parametrize("used", [24, 25, 39, 40, 24 + 4095, 24 + 4096, 24 + 4097])
def test_copy_alignment(cuda, used):
    """256 images of `used` bytes, image i at old offset residue i // 16 and,
    with align = page = realloc_size = 1 (the new capacity is used + need, the
    slots are packed), at new offset residue top + i modulo 16: every pair."""
    n = 256
    items = [(min(used - 24, i % 3), used - 24 - min(used - 24, i % 3), i % 2) for i in range(n)]
    need = [room + 1 + (1 - (used + room + 1)) % 16 for _, _, room in items]      # new_cap = 1 modulo 16
    buf, offs, caps, arena = layout(items, n * (used + 40), residue=lambda i: i // 16)
    s = State(cuda, buf, offs, caps, arena)
    with cio.DevWriter(n) as w:
        st, total, po, pc = s.grow(w, need, realloc=1, page=1, align=1, what=f"alignment {used}")
    assert not st.any()
    assert sorted((int(a) % 16, b % 16) for a, b in zip(po, s.offs)) == [(a, b) for a in range(16) for b in range(16)]


def test_one_large_image_among_small_ones(cuda):
    n = 301
    items = [(i % 5, i % 37, 0) for i in range(n)]
    items[137] = (300, (1 << 20) - 324, 0)                   # 1 MiB used
    need = [1 + i % 9 for i in range(n)]
    buf, offs, caps, arena = layout(items, (1 << 20) + 40000 + n * 4200)
    s = State(cuda, buf, offs, caps, arena)
    with cio.DevWriter(n) as w:
        st = s.grow(w, need, realloc=4096, page=1, align=4, what="one large image")[0]
    assert not st.any() and s.caps[137] == (1 << 20) + 4096


# ------------------------------------------------------------------ 4. CIOA_GROW_ZERO

TAILS = [1, 15, 16, 17, 4095, 4096, 4097]


@pytest.mark.parametrize("flags", [ZERO, 0])
def test_zeroed_tails(cuda, flags):
    """With align = page = realloc_size = 1 the tail [used, new_cap) is the
    need: the tails of growcheck's list (and tiny ones) behind every used-size
    residue modulo 16, then one long tail among many short ones."""
    tails = [t for t in TAILS + [2, 3] for _ in range(16)]
    items = [(0, 7 * i % 61, 0) for i in range(len(tails))]
    buf, offs, caps, arena = layout(items, sum(tails) + sum(24 + c for _, c, _ in items) + 64)
    s = State(cuda, buf, offs, caps, arena)
    top = arena[0]
    with cio.DevWriter(400) as w:
        st = s.grow(w, tails, realloc=1, page=1, align=1, flags=flags, what=f"tails {flags}")[0]
        assert not st.any()
        residues = {(o + 24 + c) % 16 for o, (_, c, _) in zip(s.offs[:16], items)}
        assert len(residues) > 8
        sentinel = fill(len(s.buf))
        for o, c, (_, k, _), t in zip(s.offs, s.caps, items, tails):
            tail = s.buf[o + 24 + k:o + c]
            assert len(tail) == t
            assert not tail.any() if flags else np.array_equal(tail, sentinel[o + 24 + k:o + c])
        assert np.array_equal(s.buf[s.arena[0]:], sentinel[s.arena[0]:]) and s.arena[0] > top
        # one long tail among many short ones
        items = [(0, i % 23, 0) for i in range(400)]
        need = [1 + i % 30 for i in range(400)]
        need[211] = (1 << 20) + 5
        buf, offs, caps, arena = layout(items, sum(need) + 400 * 50)
        s = State(cuda, buf, offs, caps, arena)
        st = s.grow(w, need, realloc=1, page=1, align=1, flags=flags, what="a long tail")[0]
        assert not st.any() and s.caps[211] == 24 + 211 % 23 + (1 << 20) + 5


# ------------------------------------------------------------------ 5. lifecycle

def lifecycle(cuda, rec_img, n_img, roomy):
    """Init n_img images (zero room unless roomy), grow for the records, append
    them ungrouped, seal, verify.  Returns the trimmed images and crc_cur."""
    import torch
    rng = np.random.default_rng(12)
    n_rec = len(rec_img)
    metas = [bytes(rng.integers(1, 255, i % 11, dtype=np.uint8)) for i in range(n_img)]
    rec_lens = rng.integers(0, 180, n_rec).astype(np.uint64)
    rec_offs = np.concatenate(([0], np.cumsum(rec_lens)[:-1])).astype(np.uint64)
    src = rng.integers(0, 256, int(rec_lens.sum()) + 16, dtype=np.uint8)
    need = model.needs_of(rec_img, rec_lens, n_img)
    items = [(0, len(m), need[i] + 100 if roomy else 0) for i, m in enumerate(metas)]     # metadata as "content"
    buf, offs, caps, arena = layout(items, 0 if roomy else sum(model.round_up(24 + len(m) + nd + 4096, 4096)
                                                                for m, nd in zip(metas, need)) + 4096)
    buf = fill(len(buf))
    s = State(cuda, buf, offs, caps, arena)
    msrc = np.frombuffer(b"".join(metas) + b"\0", np.uint8).copy()
    mlens = np.asarray([len(m) for m in metas], np.uint64)
    moffs = np.concatenate(([0], np.cumsum(mlens)[:-1])).astype(np.uint64)
    with cio.DevWriter(max(n_img, n_rec)) as w:
        st, crc = cf.init_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(msrc, cuda), dev_i64(moffs, cuda),
                                    dev_i64(mlens, cuda), flags=CK)
        assert not st.cpu().numpy().any()
        for i, m in enumerate(metas):
            m_init(s.buf, offs[i], m)
        s.check("init")
        img_t, lens_t = dev_i32(rec_img, cuda), dev_i64(rec_lens, cuda)
        if not roomy:
            gst = s.grow(w, recs=(rec_img, rec_lens), realloc=4096, page=4096, align=16, what="lifecycle grow")[0]
            assert not gst.any()
            assert all(c == 24 + len(m) or c % 4096 == 0 for c, m in zip(s.caps, metas))
        ist, rst = cf.write_records_ungrouped_batch_dev(w, s.base_t, s.offs_t, s.caps_t, dev_u8(src, cuda), img_t,
                                                        dev_i64(rec_offs, cuda), lens_t, crc, flags=CK)
        assert not rst.cpu().numpy().any() and not ist.cpu().numpy().any()
        assert not cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, crc, flags=CK).cpu().numpy().any()
    with cio.Crc32DevPlan(n_img) as plan:
        # the trimmed images: an empty content in front of sentinel slack would read as a legacy chunk
        used_t = dev_i64([24 + len(m) + nd for m, nd in zip(metas, need)], cuda)
        vst, er, cr, ml, cl = cf.verify_batch_dev(plan, s.base_t, s.offs_t, used_t, flags=CK)
        assert not vst.cpu().numpy().any()
        assert cl.cpu().numpy().tolist() == need
    torch.cuda.synchronize()
    got = s.base_t.cpu().numpy()
    offs_now = u64(s.offs_t).tolist()
    return [got[o:o + 24 + len(m) + nd].tobytes() for o, m, nd in zip(offs_now, metas, need)], \
        crc.cpu().numpy().view(np.uint32).tolist()


@pytest.mark.parametrize("one", [False, True])
def test_lifecycle_grow_then_ungrouped_append(cuda, one):
    """257 images without any room, 3000 records in a permuted list (the sort
    runs two passes, the need kernel sees repeated keys) -- or all 3000 to one
    image: grow, append, seal, verify; the trimmed images and crc_cur equal
    those of the same appends into slots that were large from the start."""
    n_img, n_rec = 257, 3000
    rng = np.random.default_rng(3)
    rec_img = np.full(n_rec, 131, np.uint32) if one else rng.permutation(np.arange(n_rec) % n_img).astype(np.uint32)
    grown, crc = lifecycle(cuda, rec_img, n_img, roomy=False)
    roomy, crc2 = lifecycle(cuda, rec_img, n_img, roomy=True)
    assert grown == roomy and crc == crc2


# ------------------------------------------------------------------ 6. the perf file, replayed

def test_perf_file_replay(cuda, tmp_path, data400):
    """One image of capacity 4096; five rounds of grow (CIOA_GROW_ZERO, realloc
    32768, page 4096) -> append of 400kb.txt, then seal.  The capacities are
    the reference's, and the final image's whole 2 068 480 bytes are the file
    the host chunk layer writes for the same five writes without trimming."""
    with cf.Context(str(tmp_path), CK) as ctx:
        c, err = ctx.stream("grow").open("perf", cf.CIO_OPEN, size=4096)
        assert c is not None, err
        for _ in range(5):
            assert c.write(data400) == 0
        assert c.sync() == 0
        c.close()
    with open(os.path.join(str(tmp_path), "grow", "perf"), "rb") as f:
        host = np.frombuffer(f.read(), np.uint8)
    assert len(host) == SIZES[-1]

    buf = fill(8 << 20)
    s = State(cuda, buf, [5], [4096], [4096 + 16, len(buf) - 7])
    src = np.frombuffer(data400, np.uint8).copy()
    src_t, so_t, sl_t = dev_u8(src, cuda), dev_i64([0], cuda), dev_i64([len(src)], cuda)
    with cio.DevWriter(1) as w:
        st, crc = cf.init_batch_dev(w, s.base_t, s.offs_t, s.caps_t, flags=CK)
        raw = m_init(s.buf, 5)
        for k in range(5):
            gst = s.grow(w, [len(src)], realloc=32768, page=4096, align=16, flags=ZERO, what=f"round {k}")[0]
            assert not gst.any() and s.caps[0] == SIZES[k]
            st = cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, so_t, sl_t, crc, flags=CK)
            assert not st.cpu().numpy().any()
            raw = m_write(s.buf, s.offs[0], data400, raw)
            s.check(f"append {k}")
        assert not cf.seal_batch_dev(w, s.base_t, s.offs_t, s.caps_t, crc, flags=CK).cpu().numpy().any()
        m_seal(s.buf, s.offs[0], raw)
        s.check("seal")
    image = s.base_t.cpu().numpy()[s.offs[0]:s.offs[0] + s.caps[0]]
    assert np.array_equal(image, host)


# ------------------------------------------------------------------ 7. graph

def test_graph_replay_grows_again(cuda):
    """grow_batch_dev -> write_batch_dev captured once, dev_need = the source
    lengths array, replayed three times: three sequential rounds of the model,
    the top advancing each time an image outgrows its slot."""
    import torch
    n, size = 40, 700
    rng = np.random.default_rng(7)
    items = [(i % 4, 0, 300 + 40 * i) for i in range(n)]
    buf, offs, caps, arena = layout(items, 5 * n * 4096)
    s = State(cuda, buf, offs, caps, arena)
    so = np.arange(n, dtype=np.uint64) * (size + 3)
    src_t = dev_u8(np.zeros(n * (size + 3) + 16, np.uint8), cuda)
    so_t, sl_t = dev_i64(so, cuda), dev_i64(np.zeros(n, np.uint64), cuda)
    o = s.outs()
    wst = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    raws = [0] * n

    def stage(k):
        lens = rng.integers(0, size + 1, n).astype(np.uint64)
        lens[k] = 0
        src = rng.integers(0, 256, src_t.numel(), dtype=np.uint8)
        src_t.copy_(torch.from_numpy(src))
        sl_t.copy_(torch.from_numpy(lens.view(np.int64)))
        want = model.m_grow(s.buf, s.offs, s.caps, lens, s.arena, realloc=512, page=256, align=32, flags=ZERO)
        for i in range(n):
            m_write(s.buf, s.offs[i], src[int(so[i]):int(so[i]) + int(lens[i])].tobytes(), raws[i], checksum=False)
        return want

    def call():
        cf.grow_batch_dev(w, s.base_t, s.offs_t, s.caps_t, sl_t, s.arena_t, realloc=512, page=256, align=32,
                          flags=ZERO, **o)
        cf.write_batch_dev(w, s.base_t, s.offs_t, s.caps_t, src_t, so_t, sl_t, None, flags=0, status=wst)

    with cio.DevWriter(n) as w:
        want = stage(0)
        call()                                # warm-up outside the capture (a round like the others)
        torch.cuda.synchronize()
        s.compare(o["status"], o["total"], o, want, "warm-up")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        torch.cuda.synchronize()
        s.check("capture runs nothing")
        tops = [s.arena[0]]
        for k in (1, 2, 3):
            want = stage(k)
            o["status"].fill_(99)
            wst.fill_(99)
            graph.replay()
            torch.cuda.synchronize()
            s.compare(o["status"], o["total"], o, want, f"replay {k}")
            assert not wst.cpu().numpy().any() and not want[0].any()
            tops.append(s.arena[0])
        del graph
    assert tops[0] < tops[1] < tops[2] < tops[3]


# ------------------------------------------------------------------ 8., 9. rejected input

@pytest.mark.parametrize("at", [0, 255, 256, 2999])
def test_malformed_records_list_changes_nothing(cuda, at):
    n_img, n_rec = 257, 3000
    rng = np.random.default_rng(at)
    items = [(0, i % 50, 0) for i in range(n_img)]
    buf, offs, caps, arena = layout(items, 1 << 20)
    s = State(cuda, buf, offs, caps, arena)
    rec_img = rng.integers(0, n_img, n_rec).astype(np.uint32)
    rec_img[at] = n_img + (at % 2) * 0xFFFFFEFE
    rec_lens = rng.integers(1, 100, n_rec).astype(np.uint64)
    with cio.DevWriter(n_rec) as w:
        st, total, po, pc = s.grow(w, recs=(rec_img, rec_lens), realloc=64, page=1, align=1, flags=ZERO,
                                   what=f"malformed at {at}")
        assert st.tolist() == [-1] * n_img and total == 0 and s.arena == arena and s.offs == offs
        # the writer is not left marked: the same list, mended, grows
        rec_img[at] = 0
        st = s.grow(w, recs=(rec_img, rec_lens), realloc=64, page=1, align=1, flags=ZERO, what="mended")[0]
        assert not st.any() and s.arena[0] > arena[0]


def test_a_need_of_all_ones_is_rejected(cuda):
    items = [(0, 10, 5), (3, 20, 5), (0, 0, 5)]
    buf, offs, caps, arena = layout(items, 1 << 16)
    s = State(cuda, buf, offs, caps, arena)
    with cio.DevWriter(3) as w:
        st, total, po, pc = s.grow(w, [(1 << 64) - 1, 6, 5], realloc=32768, page=4096, align=16,
                                   flags=ZERO, what="need 2^64 - 1")
    assert st.tolist() == [-1, 0, 0] and s.offs[0] == offs[0] and s.offs[1] != offs[1] and s.offs[2] == offs[2]
