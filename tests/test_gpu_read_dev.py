"""The device read path on chunk images in device memory (include/chunkio_amd/
cio_read_dev.h): metadata, content and trimmed images gathered into an output
buffer at caller-given and at device-computed places, and the metadata
compare, byte for byte against the numpy model (read_dev_model.py).  The
output buffer is pre-filled with a pattern and compared WHOLE, so a stray
store shows; the image buffer is compared with what was uploaded."""
import ctypes
import json
import os
import shutil

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import read_dev_model as model
from write_dev_move_model import m_init, m_seal, m_write

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
GDIR = os.path.join(HERE, "golden", "chunks")
with open(os.path.join(GDIR, "manifest.json")) as _f:
    MANIFEST = json.load(_f)
LOADABLE = ["c01", "c02", "c03", "c04", "c05", "c06", "c14"]
SPECS = [s for s in MANIFEST["chunks"] if s["name"][:3] in LOADABLE]

CK = cf.CIO_CHECKSUM
META, CONTENT, IMAGE, NUL = cf.CIOA_READ_META, cf.CIOA_READ_CONTENT, cf.CIOA_READ_IMAGE, cf.CIOA_READ_NUL
BLOCK = 1024                                  # kReadBlock: images per workgroup of the header kernel


# ------------------------------------------------------------------ helpers

def dev_i64(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(cuda)


def dev_u8(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint8)).to(cuda)


def dev_i32(a, cuda):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32)).to(cuda)


def u64(t):
    return t.cpu().numpy().view(np.uint64).copy()


def fill(nbytes):
    """The output buffer's pattern: no long run of one value, no zero."""
    i = np.arange(nbytes, dtype=np.uint64)
    return ((i * 37 + (i >> 8) * 11) % 253 + 1).astype(np.uint8)


def pattern(length, seed):
    i = np.arange(length, dtype=np.uint64)
    return (((i * 131 + seed * 7 + 17) % 251) + 1).astype(np.uint8)


class Batch:
    """Images in one device buffer, the host copy beside it."""

    def __init__(self, cuda, base, offs, caps):
        self.cuda, self.base = cuda, base
        self.offs, self.caps = np.asarray(offs, np.uint64), np.asarray(caps, np.uint64)
        self.n = len(self.offs)
        self.base_t, self.offs_t, self.caps_t = dev_u8(base, cuda), dev_i64(self.offs, cuda), dev_i64(self.caps, cuda)

    def gate_t(self, gate):
        return None if gate is None else dev_i32(gate, self.cuda)

    def packed(self, w, what, out_bytes, align=1, flags=0, gate=None, query=False):
        """One packed read, compared with the model in every output."""
        out = None if query else fill(out_bytes)
        out_t = None if query else dev_u8(out, self.cuda)
        st, po, ln, total = cf.read_packed_batch_dev(w, self.base_t, self.offs_t, self.caps_t, what, out_t,
                                                     align=align, gate=self.gate_t(gate), flags=flags)
        want = model.read_packed(self.base, self.offs, self.caps, what, out, align=align, gate=gate, flags=flags)
        got = (st.cpu().numpy(), u64(po), u64(ln), u64(total))
        for g, m, name in zip(got, want, ("status", "offsets", "lengths", "total")):
            assert np.array_equal(g, m), (name, what, align, flags, np.flatnonzero(g != m)[:8])
        if not query:
            same(out_t, want[4], (what, align, flags))
        self.unchanged()
        return want

    def placed(self, w, what, out_bytes, out_offs, out_caps, flags=0, gate=None, query=False):
        out = None if query else fill(out_bytes)
        out_t = None if query else dev_u8(out, self.cuda)
        st, ln = cf.read_batch_dev(w, self.base_t, self.offs_t, self.caps_t, what, out_t,
                                   None if query else dev_i64(out_offs, self.cuda),
                                   None if query else dev_i64(out_caps, self.cuda), gate=self.gate_t(gate),
                                   flags=flags)
        want = model.read_placed(self.base, self.offs, self.caps, what, out, out_offs, out_caps, gate=gate,
                                 flags=flags)
        for g, m, name in zip((st.cpu().numpy(), u64(ln)), want, ("status", "lengths")):
            assert np.array_equal(g, m), (name, what, flags, np.flatnonzero(g != m)[:8])
        if not query:
            same(out_t, want[2], (what, flags))
        self.unchanged()
        return want

    def unchanged(self):
        """The images are never written."""
        assert np.array_equal(self.base_t.cpu().numpy(), self.base), "the image buffer changed"


def same(out_t, want, what):
    got = out_t.cpu().numpy()
    if not np.array_equal(got, want):
        bad = np.flatnonzero(got != want)
        raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {bad[:6]} of {len(want)}")


def images_of(items, gap=lambda i: (5 * i + 3) % 16 + 1, slack=lambda i: (3 * i) % 29, seed=1, residue=None):
    """One random buffer holding an image per (meta, content) item, image i
    after gap(i) bytes (or at the next offset that is residue(i) modulo 16) in
    a slot of its used bytes + slack(i)."""
    used = [24 + len(m) + len(c) for m, c in items]
    caps = np.asarray([u + slack(i) for i, u in enumerate(used)], np.uint64)
    offs, end = [], 0
    for i, c in enumerate(caps):
        end += gap(i) if residue is None else (residue(i) - end) % 16
        offs.append(end)
        end += int(c)
    offs = np.asarray(offs, np.uint64)
    base = np.random.default_rng(seed).integers(0, 256, end + 11, dtype=np.uint8)
    for o, (m, c) in zip(offs, items):
        model.make_image(base, int(o), m, c)
    return base, offs, caps


def placed_slots(lens, residue, extra=lambda i: i % 5):
    """Distinct output slots of lens[i] + extra(i) bytes, slot i starting at
    residue(i) modulo 16; (offsets, caps, bytes)."""
    offs, pos = [], 0
    caps = [int(ln) + extra(i) for i, ln in enumerate(lens)]
    for i, c in enumerate(caps):
        pos += (residue(i) - pos) % 16
        offs.append(pos)
        pos += c
    return np.asarray(offs, np.uint64), np.asarray(caps, np.uint64), pos + 19


# ------------------------------------------------------------------ 1. reference fixtures

def host_content_copy(path_root, spec):
    """cioa_chunk_get_content_copy of the fixture, with its terminator."""
    lib = cf._bind()
    V = ctypes.c_void_p
    lib.cioa_chunk_get_content_copy.restype = ctypes.c_int
    lib.cioa_chunk_get_content_copy.argtypes = [V, ctypes.POINTER(V), ctypes.POINTER(ctypes.c_size_t)]
    libc = ctypes.CDLL(None)
    libc.free.argtypes = [V]
    d = path_root / spec["name"] / MANIFEST["stream"]
    d.mkdir(parents=True)
    shutil.copyfile(os.path.join(GDIR, "files", spec["name"]), d / spec["name"])
    with cf.Context(str(path_root / spec["name"]), spec["load_flags"]) as ctx:
        c, err = ctx.stream(MANIFEST["stream"]).open(spec["name"], cf.CIO_OPEN)
        assert c is not None, (spec["name"], err)
        p, size = V(), ctypes.c_size_t()
        assert lib.cioa_chunk_get_content_copy(c._c(), ctypes.byref(p), ctypes.byref(size)) == 0
        host = ctypes.string_at(p.value, size.value + 1)
        libc.free(p)
        c.close()
    return host


def test_reference_fixtures(cuda, tmp_path):
    files = []
    for s in SPECS:
        with open(os.path.join(GDIR, "files", s["name"]), "rb") as f:
            files.append(np.frombuffer(f.read(), np.uint8))
    caps = np.asarray([len(b) + 37 + i for i, b in enumerate(files)], np.uint64)
    offs, end = model.layout(caps, [(5 * i + 3) % 16 + 1 for i in range(len(files))])
    base = np.full(end + 9, 0xEE, np.uint8)
    for o, b in zip(offs, files):
        base[int(o):int(o) + len(b)] = b
    b = Batch(cuda, base, offs, caps)
    used = [24 + s["load"]["meta_size"] + s["load"]["content_size"] for s in SPECS]
    sizes = {META: [s["load"]["meta_size"] for s in SPECS], CONTENT: [s["load"]["content_size"] for s in SPECS],
             IMAGE: used}
    with cio.DevWriter(len(files)) as w:
        for what in (META, CONTENT, IMAGE):
            for flags in (0, NUL):
                st, po, ln, total, out = b.packed(w, what, sum(used) + 8 * 64, align=16, flags=flags)
                assert not st.any() and ln.tolist() == sizes[what]
                so, sc, sb = placed_slots(sizes[what], lambda i: (7 * i + 5) % 16, extra=lambda i: i % 3 + 1)
                st, ln, pout = b.placed(w, what, sb, so, sc, flags=flags)
                assert not st.any() and ln.tolist() == sizes[what]
                if what == IMAGE:
                    for i, f in enumerate(files):
                        assert out[int(po[i]):int(po[i]) + used[i]].tobytes() == f[:used[i]].tobytes()
                        assert pout[int(so[i]):int(so[i]) + used[i]].tobytes() == f[:used[i]].tobytes()
                if what == CONTENT and flags == NUL:
                    for i, s in enumerate(SPECS):
                        host = host_content_copy(tmp_path, s)
                        assert out[int(po[i]):int(po[i]) + len(host)].tobytes() == host, s["name"]


# ------------------------------------------------------------------ 2. alignments and lengths

SWEEP_CONTENT = [0, 1, 3, 4, 15, 16, 17, 4095, 4096, 4097, 8191, 12289]


def sweep_images():
    items = []
    for k, c in enumerate(SWEEP_CONTENT):
        for m in range(18):                   # the content start takes every residue modulo 16
            items.append((pattern(m, 3 * k + m).tobytes(), pattern(c, 100 + k * 18 + m).tobytes()))
    return images_of(items, residue=lambda i: (i + 1) % 16, seed=2)


def test_alignment_and_length_sweep(cuda):
    base, offs, caps = sweep_images()
    assert {int(o) % 16 for o in offs} == set(range(16))
    b = Batch(cuda, base, offs, caps)
    with cio.DevWriter(b.n) as w:
        for flags in (0, NUL):
            for align in (1, 2, 16, 128, 4096):
                room = b.n * 4096 + int(caps.sum()) + 4096
                st, *_ = b.packed(w, CONTENT, room, align=align, flags=flags)
                assert not st.any()
            for what in (META, IMAGE):
                st, *_ = b.packed(w, what, int(caps.sum()) + b.n * 16, align=1 if what == META else 16, flags=flags)
                assert not st.any()
            lens = model.read_placed(base, offs, caps, CONTENT, None)[1]
            for shift in (0, 5):              # destination residues, against every source residue
                so, sc, sb = placed_slots(lens, lambda i: (3 * i + i // 16 + shift) % 16,
                                          extra=lambda i: 1 + i % 5)
                st, *_ = b.placed(w, CONTENT, sb, so, sc, flags=flags)
                assert not st.any()


# ------------------------------------------------------------------ 3. both partition regimes

def test_both_partition_regimes(cuda):
    """Fewer steps than the copy grid has waves, and more than one 4 KiB step
    per wave with one record that many waves share."""
    import torch
    cus = torch.cuda.get_device_properties(cuda).multi_processor_count
    waves = cus * 8 * 4                       # the copy grid: 8 workgroups of 4 waves per CU
    rng = np.random.default_rng(3)
    few = [(b"", pattern(int(c), i).tobytes()) for i, c in enumerate(rng.integers(1, 3000, 50))]
    big = waves * 4096 + (8 << 20) + 12345    # about 40 MiB on 256 CUs
    many = [(pattern(i % 9, i).tobytes(), rng.integers(0, 256, int(c), dtype=np.uint8))
            for i, c in enumerate(rng.integers(1024, 8193, 300))]
    many[137] = (b"big", rng.integers(0, 256, big, dtype=np.uint8))
    for items in (few, many):
        base, offs, caps = images_of(items, seed=4)
        steps = sum((len(c) + 4095) // 4096 for _, c in items)
        assert steps < waves if items is few else steps > waves
        b = Batch(cuda, base, offs, caps)
        with cio.DevWriter(b.n) as w:
            st, *_ = b.packed(w, CONTENT, int(caps.sum()) + 64 * b.n, align=64, flags=NUL)
            assert not st.any()


# ------------------------------------------------------------------ 4. scan boundaries

def tiny_batch(n):
    """n images of cap 24..40 and content 0..16 (no metadata), every 97th with
    a bad magic, built without a Python loop; (base, offs, caps, content)."""
    i = np.arange(n, dtype=np.uint64)
    caps = 24 + (i * 7) % 17
    content = (i * 5 + i // 17) % (caps - 23)
    gaps = (i * 3) % 5
    offs = np.cumsum(caps + gaps) - caps
    base = np.random.default_rng(5).integers(0, 256, int(offs[-1] + caps[-1]) + 3, dtype=np.uint8)
    for k in range(24):
        base[offs + k] = 0
    base[offs] = 0xC1
    base[offs + 13] = content.astype(np.uint8)
    base[offs[::97]] = 0xC0
    return base, offs, caps, content


def tiny_expected(base, offs, content, align, nul, out):
    """read_packed's outputs for a tiny batch, vectorised."""
    ok = base[offs] == 0xC1
    lens = np.where(ok, content, 0).astype(np.uint64)
    slots = np.where(ok, (lens + nul + align - 1) // align * align, 0).astype(np.uint64)
    po = np.cumsum(slots) - slots
    total = int(slots.sum())
    assert total <= len(out)
    want = out.copy()
    for k in range(16):
        m = ok & (lens > k)
        want[po[m] + k] = base[offs[m] + 24 + k]
    if nul:
        want[(po + lens)[ok]] = 0
    return np.where(ok, 0, -1).astype(np.int32), po, lens, np.asarray([total], np.uint64), want


@pytest.mark.parametrize("n", [1, BLOCK // 4 - 1, BLOCK // 4, BLOCK // 4 + 1, BLOCK - 1, BLOCK, BLOCK + 1,
                               BLOCK * BLOCK + 3])
def test_scan_boundaries(cuda, n):
    """n around one workgroup of the header kernel and around one pass of the
    scan workgroup; offsets, total and every byte."""
    base, offs, caps, content = tiny_batch(n)
    b = Batch(cuda, base, offs, caps)
    with cio.DevWriter(n) as w:
        for align, flags in ((1, 0), (8, NUL)):
            out = fill(n * 24 + 64)
            want = tiny_expected(base, offs, content, align, flags & NUL, out)
            if n <= BLOCK + 1:                # the vectorised expectation is the model's
                ref = model.read_packed(base, offs, caps, CONTENT, out, align=align, flags=flags)
                assert all(np.array_equal(a, r) for a, r in zip(want, ref))
            out_t = dev_u8(out, cuda)
            st, po, ln, total = cf.read_packed_batch_dev(w, b.base_t, b.offs_t, b.caps_t, CONTENT, out_t,
                                                         align=align, flags=flags)
            got = (st.cpu().numpy(), u64(po), u64(ln), u64(total))
            for g, m, name in zip(got, want, ("status", "offsets", "lengths", "total")):
                assert np.array_equal(g, m), (name, n, align, np.flatnonzero(g != m)[:8])
            same(out_t, want[4], (n, align, flags))
    b.unchanged()


# ------------------------------------------------------------------ 5. rejections

def test_rejections_change_nothing(cuda):
    """An entry for every rejection rule among valid ones; at most half are
    rejected.  The packed cut is pinned as built: offsets and total are the
    prefix sums of ALL slots and do not depend on out_bytes, so once an entry
    is cut no later entry can start inside out_bytes ("a later entry that
    still fits" cannot exist under that rule)."""
    rng = np.random.default_rng(6)
    items = [(pattern(i % 7, i).tobytes(), pattern(int(c), 50 + i).tobytes())
             for i, c in enumerate(rng.integers(0, 6000, 20))]
    base, offs, caps = images_of(items, seed=7)
    offs, caps = offs.copy(), caps.copy()
    gate = np.zeros(20, np.int32)
    base[int(offs[1])] = 0xC0                                     # bad magic
    caps[3] = 23                                                  # cap < 24
    offs[5] = len(base) - 10                                      # image outside dev_bytes
    caps[7] = 24 + len(items[7][0]) + len(items[7][1]) - 1        # lengths beyond cap
    gate[9] = cf.CIO_CORRUPTED                                    # gated off
    bad_common = {1, 3, 5, 7, 9}
    b = Batch(cuda, base, offs, caps)
    lens = model.read_placed(base, offs, caps, CONTENT, None, gate=gate)[1]
    with cio.DevWriter(20) as w:
        # placed: also a slot too small and a slot outside out_bytes
        so, sc, sb = placed_slots(lens, lambda i: (5 * i) % 16, extra=lambda i: 1 + i % 4)
        sc[11] = lens[11]                                         # no room for the terminator
        so[13] = sb - 3                                           # runs past out_bytes
        st, ln, _ = b.placed(w, CONTENT, sb, so, sc, flags=NUL, gate=gate)
        assert set(np.flatnonzero(st)) == bad_common | {11, 13} and not ln[st != 0].any()
        # packed: out_bytes ends one byte short of entry 15's slot.  The offsets do not depend on out_bytes
        # (a rejected entry keeps its slot in the sums, and the total sizes the retry), so no later entry
        # can start inside out_bytes either: exactly the entries from 15 on are cut, none before.
        st, po, ln, total, _ = b.packed(w, CONTENT, 1 << 20, align=32, gate=gate)
        assert set(np.flatnonzero(st)) == bad_common
        cut = int(po[15]) + (int(ln[15]) + 31) // 32 * 32 - 1
        st2, po2, ln2, total2, _ = b.packed(w, CONTENT, cut, align=32, gate=gate)
        assert set(np.flatnonzero(st2)) == bad_common | set(range(15, 20))
        assert np.array_equal(po2, po) and total2[0] == total[0] > cut
        st2, *_ = b.packed(w, CONTENT, cut + 1, align=32, gate=gate)      # entry 15 fits exactly
        assert set(np.flatnonzero(st2)) == bad_common | set(range(16, 20))
        # the size query: the unbounded placement, nothing written
        q = b.packed(w, CONTENT, 0, align=32, gate=gate, query=True)
        assert np.array_equal(q[1], po) and q[3][0] == total[0] and np.array_equal(q[0], st)
        q = b.placed(w, IMAGE, 0, None, None, gate=gate, query=True)
        assert set(np.flatnonzero(q[0])) == bad_common


# ------------------------------------------------------------------ 6. verified drain

def pack_source(records, cuda):
    lens = [len(r) for r in records]
    so, end = model.layout(lens, [(7 * i + 3) % 16 for i in range(len(records))])
    src = np.zeros(end + 16, np.uint8)
    for o, r in zip(so, records):
        src[int(o):int(o) + len(r)] = np.frombuffer(bytes(r), np.uint8)
    return dev_u8(src, cuda), dev_i64(so, cuda), dev_i64(np.asarray(lens, np.uint64), cuda)


def test_verified_drain(cuda):
    """verify_batch_dev and a packed CONTENT read gated by its status, queued
    on one stream with no host synchronisation between them."""
    n = 64
    rng = np.random.default_rng(9)
    records = [pattern(int(c), i).tobytes() for i, c in enumerate(rng.integers(1, 20000, n))]
    caps = np.asarray([24 + len(r) + i % 40 for i, r in enumerate(records)], np.uint64)
    offs, end = model.layout(caps, [(5 * i + 1) % 16 for i in range(n)])
    base_t = dev_u8(np.full(end + 5, 0x33, np.uint8), cuda)
    offs_t, caps_t = dev_i64(offs, cuda), dev_i64(caps, cuda)
    flipped = (4, 31, 63)
    with cio.DevWriter(n) as w, cio.Crc32DevPlan(n) as plan:
        st, crc_cur = cf.init_batch_dev(w, base_t, offs_t, caps_t, flags=CK)
        assert not st.cpu().numpy().any()
        src_t, so_t, sl_t = pack_source(records, cuda)
        st = cf.write_batch_dev(w, base_t, offs_t, caps_t, src_t, so_t, sl_t, crc_cur, flags=CK)
        assert not st.cpu().numpy().any()
        assert not cf.seal_batch_dev(w, base_t, offs_t, caps_t, crc_cur, flags=CK).cpu().numpy().any()
        for i in flipped:
            base_t[int(offs[i]) + 24 + len(records[i]) // 2] ^= 0x10
        out = fill(sum(len(r) for r in records) + 8)
        out_t = dev_u8(out, cuda)
        vst = cf.verify_batch_dev(plan, base_t, offs_t, caps_t, flags=CK)[0]
        st, po, ln, total = cf.read_packed_batch_dev(w, base_t, offs_t, caps_t, CONTENT, out_t, gate=vst)
        st, po, ln, vst = st.cpu().numpy(), u64(po), u64(ln), vst.cpu().numpy()
    assert set(np.flatnonzero(vst)) == set(flipped) == set(np.flatnonzero(st))
    want, pos = out.copy(), 0
    for i, r in enumerate(records):
        assert int(po[i]) == pos
        if i in flipped:
            assert ln[i] == 0
            continue
        assert int(ln[i]) == len(r)
        want[pos:pos + len(r)] = np.frombuffer(r, np.uint8)
        pos += len(r)
    assert int(u64(total)[0]) == pos
    same(out_t, want, "verified drain")
    m = model.read_packed(base_t.cpu().numpy(), offs, caps, CONTENT, out, gate=vst)
    assert np.array_equal(m[4], want) and np.array_equal(m[0], st)


# ------------------------------------------------------------------ 7. relocate

def test_relocate_into_larger_slots(cuda):
    """Full images refuse an append; their CIOA_READ_IMAGE copies in slots of
    twice the capacity take it, seal and verify."""
    n = 24
    rng = np.random.default_rng(10)
    metas = [pattern(i % 6, i).tobytes() for i in range(n)]
    first = [pattern(int(c), 20 + i).tobytes() for i, c in enumerate(rng.integers(1, 9000, n))]
    more = [pattern(int(c), 60 + i).tobytes() for i, c in enumerate(rng.integers(1, 3000, n))]
    caps = np.asarray([24 + len(m) + len(c) for m, c in zip(metas, first)], np.uint64)     # exactly full
    offs, end = model.layout(caps, [(3 * i + 2) % 16 for i in range(n)])
    new_caps = caps * np.uint64(2) + np.uint64(3000)
    new_offs, new_end = model.layout(new_caps, [(7 * i + 5) % 16 for i in range(n)])
    old = np.full(end + 7, 0x44, np.uint8)
    new = np.full(new_end + 7, 0x55, np.uint8)
    raw = []
    for i in range(n):
        r = m_init(old, int(offs[i]), metas[i])
        raw.append(m_write(old, int(offs[i]), first[i], r))
    old_t, new_t = dev_u8(np.full(end + 7, 0x44, np.uint8), cuda), dev_u8(new, cuda)
    offs_t, caps_t = dev_i64(offs, cuda), dev_i64(caps, cuda)
    new_offs_t, new_caps_t = dev_i64(new_offs, cuda), dev_i64(new_caps, cuda)
    with cio.DevWriter(n) as w, cio.Crc32DevPlan(n) as plan:
        msrc = pack_source(metas, cuda)
        st, crc_cur = cf.init_batch_dev(w, old_t, offs_t, caps_t, *msrc, flags=CK)
        assert not st.cpu().numpy().any()
        assert not cf.write_batch_dev(w, old_t, offs_t, caps_t, *pack_source(first, cuda), crc_cur,
                                      flags=CK).cpu().numpy().any()
        same(old_t, old, "the full images")
        extra = pack_source(more, cuda)
        assert (cf.write_batch_dev(w, old_t, offs_t, caps_t, *extra, crc_cur, flags=CK).cpu().numpy() == -1).all()
        same(old_t, old, "a refused append")
        st, ln = cf.read_batch_dev(w, old_t, offs_t, caps_t, IMAGE, new_t, new_offs_t, new_caps_t)
        m = model.read_placed(old, offs, caps, IMAGE, new, new_offs, new_caps)
        assert not st.cpu().numpy().any() and np.array_equal(u64(ln), caps) and np.array_equal(u64(ln), m[1])
        new = m[2]
        same(new_t, new, "the relocated images")
        assert not cf.write_batch_dev(w, new_t, new_offs_t, new_caps_t, *extra, crc_cur, flags=CK).cpu().numpy().any()
        assert not cf.seal_batch_dev(w, new_t, new_offs_t, new_caps_t, crc_cur, flags=CK).cpu().numpy().any()
        for i in range(n):
            raw[i] = m_write(new, int(new_offs[i]), more[i], raw[i])
            m_seal(new, int(new_offs[i]), raw[i])
        same(new_t, new, "append and seal after the move")
        assert np.array_equal(crc_cur.cpu().numpy().view(np.uint32), np.asarray(raw, np.uint32))
        assert not cf.verify_batch_dev(plan, new_t, new_offs_t, new_caps_t, flags=CK)[0].cpu().numpy().any()


# ------------------------------------------------------------------ 8. graph replay

def test_graph_replay_reads_the_lengths_at_run_time(cuda):
    import torch
    n = 40
    rng = np.random.default_rng(11)
    caps = np.asarray([24 + 12000 + i for i in range(n)], np.uint64)
    offs, end = model.layout(caps, [(5 * i + 3) % 16 for i in range(n)])
    base_t = dev_u8(np.full(end + 3, 0x66, np.uint8), cuda)
    offs_t, caps_t = dev_i64(offs, cuda), dev_i64(caps, cuda)
    out = fill(n * 12000)
    out_t = dev_u8(out, cuda)
    status = torch.full((n,), 99, dtype=torch.int32, device=cuda)
    po_t = torch.zeros(n, dtype=torch.int64, device=cuda)
    ln_t = torch.zeros(n, dtype=torch.int64, device=cuda)
    total_t = torch.zeros(1, dtype=torch.int64, device=cuda)

    def call():
        cf.read_packed_batch_dev(w, base_t, offs_t, caps_t, CONTENT, out_t, align=4, flags=NUL, out_offs=po_t,
                                 out_lens=ln_t, total=total_t, status=status)

    def append():
        recs = [pattern(int(c), int(rng.integers(0, 99))).tobytes() for c in rng.integers(0, 5000, n)]
        assert not cf.write_batch_dev(w, base_t, offs_t, caps_t, *pack_source(recs, cuda), crc_cur,
                                      flags=CK).cpu().numpy().any()

    def check(what):
        torch.cuda.synchronize()
        m = model.read_packed(base_t.cpu().numpy(), offs, caps, CONTENT, out, align=4, flags=NUL)
        got = (status.cpu().numpy(), u64(po_t), u64(ln_t), u64(total_t))
        for g, r in zip(got, m):
            assert np.array_equal(g, r), what
        same(out_t, m[4], what)
        return m

    with cio.DevWriter(n) as w:
        st, crc_cur = cf.init_batch_dev(w, base_t, offs_t, caps_t, flags=CK)
        append()
        call()                                # warm-up outside the capture
        check("warm-up")
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            call()
        out_t.copy_(torch.from_numpy(out))
        status.fill_(99)
        graph.replay()
        one = check("replay 1")
        append()
        out_t.copy_(torch.from_numpy(out))
        status.fill_(99)
        graph.replay()
        two = check("replay 2")
        del graph
    assert int(two[3][0]) > int(one[3][0]) and (two[2] >= one[2]).all() and (two[2] > one[2]).any()


# ------------------------------------------------------------------ 9. meta_cmp

def test_meta_cmp(cuda):
    rng = np.random.default_rng(12)
    cases = []                                # (metadata, candidate)
    for m in (1, 2, 15, 16, 17, 31, 100, 1024, 1040, 4099):
        meta = rng.integers(0, 256, m, dtype=np.uint8).tobytes()
        for pos in (None, 0, m // 2, m - 1):  # equal; the first, a middle, the last byte differs
            cand = bytearray(meta)
            if pos is not None:
                cand[pos] ^= 0x80
            cases.append((meta, bytes(cand)))
        cases.append((meta, meta[:-1]))       # shorter
        cases.append((meta, meta + b"\0"))    # longer
    cases.append((b"", b""))
    cases.append((b"", b"x"))
    cases.append((b"abc", b""))
    long_meta = rng.integers(0, 256, 65535, dtype=np.uint8).tobytes()
    cases.append((long_meta, long_meta))
    cases.append((long_meta, long_meta[:-1] + bytes([long_meta[-1] ^ 1])))
    cases.append((long_meta, long_meta[:70] + bytes([long_meta[70] ^ 1]) + long_meta[71:]))
    for r in range(16):                       # every residue of both sides
        meta = rng.integers(0, 256, 40 + r, dtype=np.uint8).tobytes()
        cases.append((meta, meta))
        cases.append((meta, meta[:17] + bytes([meta[17] ^ 4]) + meta[18:]))
    n0 = len(cases)
    cases += [(b"meta", b"meta")] * 3         # a failed image, a candidate outside cand_bytes, a 65536-byte candidate
    items = [(m, pattern(i % 50, i).tobytes()) for i, (m, _) in enumerate(cases)]
    base, offs, caps = images_of(items, residue=lambda i: (i * 7 + i // 16) % 16, seed=13)
    base[int(offs[n0]) + 1] = 0x01
    cl = [len(c) for _, c in cases]
    co, cend = model.layout(cl, [(i * 5 + i // 16) % 16 for i in range(len(cases))])
    cand = rng.integers(0, 256, cend + 4, dtype=np.uint8)
    for o, (_, c) in zip(co, cases):
        cand[int(o):int(o) + len(c)] = np.frombuffer(c, np.uint8)
    co, cl = co.copy(), np.asarray(cl, np.uint64)
    co[n0 + 1] = len(cand) - 2
    cl[n0 + 2] = 65536
    assert {(int(offs[i]) + 24) % 16 for i in range(n0)} == set(range(16)) == {int(o) % 16 for o in co[:n0]}
    res, st = cf.meta_cmp_batch_dev(dev_u8(base, cuda), dev_i64(offs, cuda), dev_i64(caps, cuda), dev_u8(cand, cuda),
                                    dev_i64(co, cuda), dev_i64(cl, cuda))
    res, st = res.cpu().numpy(), st.cpu().numpy()
    mres, mst = model.meta_cmp(base, offs, caps, cand, co, cl)
    assert np.array_equal(res, mres), np.flatnonzero(res != mres)
    assert np.array_equal(st, mst)
    assert res.tolist()[:n0] == [0 if m == c else -1 for m, c in cases[:n0]]
    assert st[:n0].tolist() == [0] * n0 and st[n0:].tolist() == [-1] * 3 and res[n0:].tolist() == [-1] * 3
