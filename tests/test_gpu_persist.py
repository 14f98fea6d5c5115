"""cio_file_load_paths_dev and cio_file_store_paths_dev
(include/chunkio_amd/cio_persist_dev.h): chunk images in device memory down to
chunk files and up again, against the reference's fixtures
(tests/golden/chunks), cio_file_verify_batch_dev, the numpy models
(persist_model.py over alloc_set_model.py) and this repository's host chunk
layer.  Every file lives in tmp_path."""
import hashlib
import os
import shutil

import numpy as np
import pytest

import chunkio_amd as cio
from chunkio_amd import chunkfile as cf

import persist_model as pmodel
from test_gpu_grow_dev import dev_i32, dev_i64, dev_u8, fill, u64
from test_gpu_pool_set import PoolSet
from test_gpu_verify_dev import CHUNKS, GDIR, NAMES
from test_gpu_write_dev import Images, buildable, pattern, u32

pytestmark = pytest.mark.gpu

CK, OK, ERR = cf.CIO_CHECKSUM, cf.CIO_OK, cf.CIO_ERROR
TRIM = cf.CIOA_STORE_TRIM
NONE = pmodel.NONE
BY = {s["name"]: s for s in CHUNKS}
FILES = [os.path.join(GDIR, "files", n) for n in NAMES]
SIZES = [os.path.getsize(p) for p in FILES]


def sha(b):
    return hashlib.sha256(bytes(b)).hexdigest()


def stage_of(nbytes, cuda):
    import torch
    return torch.zeros(nbytes, dtype=torch.uint8, device=cuda)


def geometry(img):
    """(meta_len, content_len) of the header in img."""
    return (int(img[22]) << 8) | int(img[23]), int.from_bytes(bytes(img[10:14]), "big")


# ------------------------------------------------------------------ 1. load against the reference

def load_set(cuda, at):
    """Three classes around the fixtures' sizes, two free slots each, from
    `at` on.  Returns (set, the first byte behind the slots)."""
    classes, entries = [(4096, 16), (36864, 16), (69632, 16)], []
    for cls, _ in classes:
        entries.append([(at, cls), (at + cls + 64, cls + 32)])
        at += 2 * cls + 128
    return PoolSet(cuda, classes, 4, entries=entries), at


def verify_same_bytes(cuda, flags):
    """cio_file_verify_batch_dev over the 14 files in one buffer."""
    images = [open(p, "rb").read() for p in FILES]
    offs = np.cumsum([0] + [-(-len(b) // 128) * 128 for b in images])[:-1].astype(np.uint64)
    buf = np.zeros(int(offs[-1]) + len(images[-1]) + 128, np.uint8)
    for o, b in zip(offs, images):
        buf[int(o):int(o) + len(b)] = np.frombuffer(b, np.uint8)
    with cio.Crc32DevPlan(len(images)) as plan:
        st, er, cr, ml, cl = cf.verify_batch_dev(plan, dev_u8(buf, cuda), dev_i64(offs, cuda),
                                                 dev_i64(np.asarray(SIZES, np.uint64), cuda), flags=flags)
        return (st.cpu().numpy(), er.cpu().numpy(), cr.cpu().numpy().view(np.uint32), ml.cpu().numpy(),
                cl.cpu().numpy())


def load_fixtures(cuda, stage_bytes, paths=FILES, flags=CK):
    """One load of `paths` over a sentinel-filled buffer with load_set's set;
    the placement compared with the model.  Returns (outputs, the device
    buffer afterwards, the buffer before, which files are over the round
    maximum)."""
    n = len(paths)
    pset, top = load_set(cuda, 4096)
    top += 7
    buf = fill(top + sum(SIZES) + 16 * n + 4096)
    arena = [top, len(buf) - 64]
    base_t, arena_t = dev_u8(buf, cuda), dev_i64(arena, cuda)
    with cio.DevWriter(n) as w:
        out = cf.load_paths_dev(w, base_t, paths, stage_of(stage_bytes, cuda), arena_t, set=pset.arg(), flags=flags,
                                align=16)
    st, er, fs, offs, caps, crc, dst = out
    assert np.array_equal(dst.cpu().numpy(), st)
    sizes = [os.path.getsize(p) if os.path.exists(p) else 0 for p in paths]
    assert fs.tolist() == sizes
    want = pmodel.m_load_place(buf, sizes, [s == OK for s in st], stage_bytes, arena, *pset.model_args(), align=16)
    over = [s > pmodel.m_round_max(stage_bytes) for s in sizes]
    assert [int(s) == OK for s in st] == [s == OK for s in want[0]]
    assert u64(offs).tolist() == want[1] and u64(caps).tolist() == want[2]
    assert u64(arena_t).tolist() == arena                       # rejected files took no slot
    pset.check("load")
    return out, base_t.cpu().numpy(), buf, over


@pytest.mark.parametrize("zero", [0, cf.CIOA_LOAD_ZERO])
def test_reference_files_load_as_the_reference_loads_them(cuda, zero):
    """The 14 reference-written files through one load, at least three rounds,
    over a sentinel-filled buffer; load_set's pool slots and the arena slots
    (rounded up to 16) are larger than most files.  With CIOA_LOAD_ZERO
    [fs_size, cap) of every slot taken is zero and every other byte of the
    buffer is what it was; without it the tails keep the sentinel too."""
    stage_bytes = cf.persist_round_max(max(SIZES))
    assert stage_bytes == max(SIZES) and cf.persist_rounds(SIZES, stage_bytes)[0] >= 3
    (st, er, fs, offs, caps, crc, dst), got, before, over = load_fixtures(cuda, stage_bytes, flags=CK | zero)
    assert not any(over)
    vst, ver, vcr, vml, vcl = verify_same_bytes(cuda, CK)
    assert st.tolist() == vst.tolist() and er.tolist() == ver.tolist()
    offs, caps, crc = u64(offs), u64(caps), u32(crc)
    touched, tails = np.zeros(len(got), bool), 0
    for i, name in enumerate(NAMES):
        ld, spec = BY[name]["load"], BY[name]
        if spec["load_flags"] == CK:              # where test_gpu_verify_dev.py holds this call to the manifest
            assert int(st[i]) == (OK if ld["ok"] else ld["err"]) and int(er[i]) == ld["last_chunk_error"], name
        if int(st[i]) != OK:
            assert (int(offs[i]), int(caps[i]), int(crc[i])) == (NONE, 0, 0), name
            continue
        o = int(offs[i])
        img = got[o:o + SIZES[i]]
        assert int(crc[i]) == int(vcr[i]) and geometry(img) == (int(vml[i]), int(vcl[i])), name
        if spec["load_flags"] == CK:
            assert int(crc[i]) == ld["crc_cur"] and geometry(img) == (ld["meta_size"], ld["content_size"]), name
        assert sha(img) == spec["sha256_after_load"], name
        assert int(caps[i]) >= SIZES[i]
        touched[o:o + SIZES[i]] = True
        tail = got[o + SIZES[i]:o + int(caps[i])]
        tails += len(tail)
        if zero:
            assert not tail.any(), name
            touched[o + SIZES[i]:o + int(caps[i])] = True
    assert BY["c07_legacy_exact"]["sha256_after_load"] != BY["c07_legacy_exact"]["sha256"]
    assert int(st[NAMES.index("c07_legacy_exact")]) == OK       # the one whose length is written back
    assert tails > 100 and before.all()                         # there are tails, and the sentinel has no zero byte
    assert np.array_equal(got[~touched], before[~touched])      # and nothing else in the buffer


@pytest.mark.parametrize("zero", [0, cf.CIOA_LOAD_ZERO])
def test_a_load_that_accepts_no_file_changes_no_byte(cuda, tmp_path, zero):
    """Two rounds in which no file is accepted -- damaged files, a missing one,
    an empty one -- with and without CIOA_LOAD_ZERO: no slot, no byte of the
    buffer, no set word and no arena word changes."""
    bad = [FILES[NAMES.index(n)] for n in ("c10_bad_crc", "c12_bad_magic", "c13_short_header", "c09_truncated")]
    (tmp_path / "empty").write_bytes(b"")
    paths = bad[:2] + [str(tmp_path / "missing"), str(tmp_path / "empty")] + bad[2:]
    assert cf.persist_rounds([os.path.getsize(p) if os.path.exists(p) else 0 for p in paths], 8192)[0] == 2
    (st, er, fs, offs, caps, crc, dst), got, before, _ = load_fixtures(cuda, 8192, paths, flags=CK | zero)
    assert (st != OK).all() and st[2] == ERR and u64(offs).tolist() == [NONE] * 6 and not u64(caps).any()
    assert np.array_equal(got, before)


def test_a_stage_one_byte_too_small_rejects_that_file_alone(cuda):
    big = NAMES.index("c03_meta_content")
    assert SIZES[big] == max(SIZES)
    (st, er, *_), _, _, over = load_fixtures(cuda, SIZES[big] - 1)
    assert over == [i == big for i in range(len(NAMES))]
    vst = verify_same_bytes(cuda, CK)[0]
    assert st.tolist() == [ERR if i == big else int(vst[i]) for i in range(len(NAMES))] and int(er[big]) == 0


def test_paths_that_do_not_exist_change_nothing_else(cuda, tmp_path):
    paths = list(FILES)
    paths.insert(3, str(tmp_path / "missing-a"))
    paths.append(str(tmp_path / "no-such-dir" / "missing-b"))
    (st, er, *_), _, _, _ = load_fixtures(cuda, max(SIZES), paths)
    vst = verify_same_bytes(cuda, CK)[0].tolist()
    assert st.tolist() == vst[:3] + [ERR] + vst[3:] + [ERR] and int(er[3]) == 0 and int(er[-1]) == 0


# ------------------------------------------------------------------ 2. store against the reference

def build_scenarios(cuda, w, fill_byte):
    """The four buildable scenarios of the manifest, built on the device in
    slots of the files' sizes (test_gpu_write_dev.py's construction)."""
    specs = [s for s in CHUNKS if buildable(s)]
    assert [s["name"] for s in specs] == ["c01_empty", "c02_content", "c03_meta_content", "c06_close_no_sync"]
    sizes = [s["size"] for s in specs]
    offs, pos = [], 0
    for i, size in enumerate(sizes):
        pos = ((pos + 4095) & ~4095) + 16 * i
        offs.append(pos)
        pos += size
    im = Images(cuda, offs, sizes, pos + 100, fill=fill_byte)
    metas = [(s["ops"][0]["meta"].encode() if s["ops"][0]["op"] == "meta_write" else b"") for s in specs]
    writes = [[pattern(o["len"], o["seed"]) for o in s["ops"] if o["op"] == "write"] for s in specs]
    assert not im.init(w, metas).any()
    for k in range(max(len(x) for x in writes)):
        assert not im.write(w, [x[k] if k < len(x) else b"" for x in writes], seed=k).any()
    assert not im.seal(w).any()
    return specs, im


def test_stored_scenarios_are_the_reference_files(cuda, tmp_path):
    with cio.DevWriter(4) as w:
        specs, im = build_scenarios(cuda, w, 0)
        paths = [str(tmp_path / s["name"]) for s in specs]
        stage = stage_of(max(s["size"] for s in specs), cuda)
        st, fs, dst = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t, paths, stage)
        assert not st.any() and not dst.cpu().numpy().any() and fs.tolist() == [s["size"] for s in specs]
        for p, s in zip(paths, specs):
            assert sha(open(p, "rb").read()) == s["sha256"], s["name"]
        vst, ver, vcr = cf.verify_paths(paths, CK)
        assert not vst.any() and vcr.tolist() == [s["load"]["crc_cur"] for s in specs]
        im.check("store reads only")
        # trimmed, from slots whose slack is 0xA5: the tail is ftruncate's zeros, never the slot's bytes
        specs, im = build_scenarios(cuda, w, 0xA5)
        for page in (4096, 1):
            paths = [str(tmp_path / f"{s['name']}.trim{page}") for s in specs]
            st, fs, dst = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t, paths, stage, flags=TRIM, page=page)
            assert not st.any() and not dst.cpu().numpy().any()
            for i, (p, s) in enumerate(zip(paths, specs)):
                used = 24 + s["load"]["meta_size"] + s["load"]["content_size"]
                data = open(p, "rb").read()
                assert len(data) == -(-used // page) * page == int(fs[i]), (s["name"], page)
                ref = open(os.path.join(GDIR, "files", s["name"]), "rb").read()
                assert data[:used] == ref[:used] and not any(data[used:]), (s["name"], page)
        im.check("trimmed store reads only")


# ------------------------------------------------------------------ 3. gates and failures

def test_gates_and_failures(cuda, tmp_path):
    """Five images of 300 used bytes in 400-byte slots: stored; gated off;
    bad magic; under a path whose parent is a plain file (and, for a user who
    is not root, in a directory without write permission); stored.  Then three
    images of 124, 1500 and 124 used bytes through a stage of 1499 bytes: the
    middle one is over the round maximum."""
    n = 5
    offs, caps = [512 * i + 16 for i in range(n)], [400] * n
    im = Images(cuda, offs, caps, 512 * n + 2048, fill=0xA5)
    (tmp_path / "plain-file").write_bytes(b"not a directory")
    paths = [str(tmp_path / f"g{i}") for i in range(n)]
    paths[3] = str(tmp_path / "plain-file" / "g3")
    old = {1: b"an older file at the gated path", 2: b"an older file at the ill-formed image's path"}
    for i, b in old.items():
        open(paths[i], "wb").write(b)
    with cio.DevWriter(n) as w:
        assert not im.init(w, [b"m%d" % i for i in range(n)]).any()
        assert not im.write(w, [pattern(274, i) for i in range(n)]).any()
        assert not im.seal(w).any()
        bad = im.model.copy()
        bad[offs[2]] = 0xC0
        im.model[:] = bad
        im.base.copy_(dev_u8(bad, cuda))
        gate = dev_i32(np.asarray([0, -3, 0, 0, 0], np.int32).view(np.uint32), cuda)
        st, fs, dst = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t, paths, stage_of(4096, cuda), gate=gate,
                                         flags=cf.CIOA_STORE_SYNC)      # fdatasync before close: the same files
        assert st.tolist() == [OK, ERR, ERR, ERR, OK] == dst.cpu().numpy().tolist() and fs.tolist() == [400, 0, 0, 0, 400]
        for i in (0, 4):
            assert open(paths[i], "rb").read() == im.model[offs[i]:offs[i] + 300].tobytes() + bytes(100)
        for i, b in old.items():
            assert open(paths[i], "rb").read() == b         # byte-identical
        assert sorted(os.listdir(tmp_path)) == ["g0", "g1", "g2", "g4", "plain-file"]      # no partial file
        if os.geteuid() != 0:                     # a directory without write permission (root may write it anyway)
            ro = tmp_path / "read-only"
            ro.mkdir()
            ro.chmod(0o555)
            st, _, _ = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t,
                                          [str(ro / f"g{i}") if i == 0 else paths[i] for i in range(n)],
                                          stage_of(4096, cuda), gate=gate)
            assert st.tolist() == [ERR, ERR, ERR, ERR, OK] and os.listdir(ro) == []
            ro.chmod(0o755)
        im.check("store reads only")
    # an image over the round maximum
    offs, caps = [0, 2048, 4096], [400, 1600, 400]
    im = Images(cuda, offs, caps, 8192, fill=0)
    paths = [str(tmp_path / f"r{i}") for i in range(3)]
    with cio.DevWriter(3) as w:
        assert not im.init(w).any()
        assert not im.write(w, [pattern(100, 1), pattern(1476, 2), pattern(100, 3)]).any()
        assert not im.seal(w).any()
        assert cf.persist_round_max(1499) == 1408 < 1500
        st, fs, dst = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t, paths, stage_of(1499, cuda), flags=TRIM,
                                         page=1)
        assert st.tolist() == [OK, ERR, OK] == dst.cpu().numpy().tolist() and fs.tolist() == [124, 0, 124]
        assert not os.path.exists(paths[1])


# ------------------------------------------------------------------ 4. width

def test_1025_small_images_stored_and_loaded_back(cuda, tmp_path):
    """n = 1025 images with 24 to 200 used bytes, stored exact over several
    rounds of a 16 KiB stage and loaded back into a second arena: content and
    metadata equal what was appended."""
    n = 1025
    rng = np.random.default_rng(1025)
    metas = [bytes(rng.integers(1, 256, int(m), dtype=np.uint8)) for m in rng.integers(0, 21, n)]
    recs = [bytes(rng.integers(0, 256, int(rng.integers(0, 177 - len(m))), dtype=np.uint8)) for m in metas]
    metas[0], recs[0] = b"", b""                                    # 24 used bytes
    metas[1], recs[1] = bytes(range(1, 21)), bytes(156)             # 200
    offs, caps = [256 * i for i in range(n)], [256 - i % 50 for i in range(n)]
    im = Images(cuda, offs, caps, 256 * n + 64, fill=0xA5)
    paths = [str(tmp_path / f"w{i:04d}") for i in range(n)]
    stage = stage_of(16384, cuda)
    with cio.DevWriter(n) as w:
        assert not im.init(w, metas).any()
        assert not im.write(w, recs).any()
        assert not im.seal(w).any()
        used = [24 + len(m) + len(r) for m, r in zip(metas, recs)]
        assert min(used) == 24 and max(used) == 200 and cf.persist_rounds(used, 16384)[0] >= 5
        st, fs, _ = cf.store_paths_dev(w, im.base, im.offs_t, im.caps_t, paths, stage, flags=TRIM, page=1)
        assert not st.any() and fs.tolist() == used
        buf = fill(n * 208 + 4096)
        arena = [13, len(buf) - 64]
        base_t, arena_t = dev_u8(buf, cuda), dev_i64(arena, cuda)
        lst, ler, lfs, lo, lc, lcrc, ldst = cf.load_paths_dev(w, base_t, paths, stage, arena_t, flags=CK, align=16)
    assert not lst.any() and not ler.any() and lfs.tolist() == used and not ldst.cpu().numpy().any()
    want = pmodel.m_load_place(buf, used, [True] * n, 16384, arena, [], [], [], 0, 0, align=16)
    assert u64(lo).tolist() == want[1] and u64(lc).tolist() == want[2] == used and u64(arena_t).tolist() == arena
    got, lo = base_t.cpu().numpy(), u64(lo)
    assert u32(lcrc).tolist() == [int(x) for x in im.raw]
    for i in range(n):
        img = got[int(lo[i]):int(lo[i]) + used[i]].tobytes()
        assert img[24:24 + len(metas[i])] == metas[i] and img[24 + len(metas[i]):] == recs[i], i
        assert img == im.model[offs[i]:offs[i] + used[i]].tobytes(), i


# ------------------------------------------------------------------ 5. the chain the feature exists for

def host_append(root, name, first_file, records):
    """This repository's host chunk layer on the same inputs: open the stored
    file, write the same records, sync.  Returns the file's bytes."""
    os.makedirs(os.path.join(root, "s"), exist_ok=True)
    path = os.path.join(root, "s", name)
    shutil.copyfile(first_file, path)
    with cf.Context(root, CK) as ctx:
        c, err = ctx.stream("s").open(name, cf.CIO_OPEN, 0)
        assert c is not None, err
        for r in records:
            assert c.write(r) == 0
        assert c.sync() == 0
        c.close()
    return open(path, "rb").read()


def test_the_chain_for_three_cycles(cuda, tmp_path):
    """append -> rotate -> verify -> store(gate = verify) -> release_set(gate =
    store's dev_status) -> load of the previous cycle's files out of the set,
    on one buffer with a three-class set.  The loaded images take a further
    append and a seal; a second store of them equals what the host chunk layer
    makes of the first file and the same record.  From the second cycle on the
    arena top stands still."""
    import torch
    n, cap, align, cycles = 6, 4096, 16, 3
    pset = PoolSet(cuda, [(4096, 16), (8192, 16), (16384, 16)], 32)
    cls0 = cf.pool_set_class(pset.arg(), 0)
    dev_bytes = 64 * cap
    base_t = torch.zeros(dev_bytes, dtype=torch.uint8, device=cuda)
    arena_t = dev_i64([48, dev_bytes], cuda)
    stage = stage_of(3 * cap, cuda)               # two rounds of three
    rng = np.random.default_rng(3)
    tops, stored = [], {}
    with cio.DevWriter(64) as w, cio.Crc32DevPlan(64) as plan:
        need = dev_i64([cap] * n, cuda)
        st, _, offs_t, caps_t = cf.alloc_set_batch_dev(w, base_t, need, arena_t, set=pset.arg(), align=align)
        metas = [b"chain-%d" % i for i in range(n)]
        msrc = np.frombuffer(b"".join(metas), np.uint8).copy()
        ist, crc = cf.init_batch_dev(w, base_t, offs_t, caps_t, dev_u8(msrc, cuda),
                                     dev_i64(np.arange(n) * 7, cuda), dev_i64([7] * n, cuda))
        assert not st.cpu().numpy().any() and not ist.cpu().numpy().any()
        for c in range(cycles):
            recs = [bytes(rng.integers(0, 256, int(rng.integers(150, 400)), dtype=np.uint8)) for _ in range(n)]
            src = np.frombuffer(b"".join(recs), np.uint8).copy()
            lens = np.asarray([len(r) for r in recs], np.uint64)
            so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
            wst = cf.write_batch_dev(w, base_t, offs_t, caps_t, dev_u8(src, cuda), dev_i64(so, cuda),
                                     dev_i64(lens, cuda), crc)
            rst, _, lo, lc, li, lcount = cf.rotate_pool_batch_dev(
                w, base_t, offs_t, caps_t, None, limit=100, new_cap=cap, align=align, arena=arena_t,
                pool_offs=cls0[0], pool_caps=cls0[1], pool=cls0[2], crc_cur=crc)
            vst = cf.verify_batch_dev(plan, base_t, lo, lc)[0]
            paths = [str(tmp_path / f"c{c}-{i}") for i in range(n)]
            sst, fs, dst = cf.store_paths_dev(w, base_t, lo, lc, paths, stage, gate=vst)
            lst, _ = cf.release_set_batch_dev(w, base_t, lo, lc, pset.arg(), gate=dst)
            for t in (wst, rst, vst, lst):
                assert not t.cpu().numpy().any(), c
            assert not sst.any() and fs.tolist() == [cap] * n and u64(lcount)[0] == n
            assert not cf.verify_paths(paths, CK)[0].any()
            order = u32(li).tolist()               # the list's entry e is image order[e]
            for e, p in enumerate(paths):
                data = open(p, "rb").read()
                i = order[e]
                assert data[24:31] == metas[i] and data[31:31 + len(recs[i])] == recs[i], (c, e)
                assert not any(data[31 + len(recs[i]):])
                stored[p] = i
            if c >= 1:                            # the previous cycle's files come up again, out of the set
                prev = [str(tmp_path / f"c{c - 1}-{i}") for i in range(n)]
                ust, uer, ufs, uo, uc, ucrc, udst = cf.load_paths_dev(w, base_t, prev, stage, arena_t,
                                                                      set=pset.arg(), flags=CK, align=align)
                assert not ust.any() and not uer.any() and u64(uc).tolist() == [cap] * n
                more = [bytes(rng.integers(0, 256, int(rng.integers(1, 300)), dtype=np.uint8)) for _ in range(n)]
                src = np.frombuffer(b"".join(more), np.uint8).copy()
                lens = np.asarray([len(r) for r in more], np.uint64)
                so = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)
                wst = cf.write_batch_dev(w, base_t, uo, uc, dev_u8(src, cuda), dev_i64(so, cuda),
                                         dev_i64(lens, cuda), ucrc)
                est = cf.seal_batch_dev(w, base_t, uo, uc, ucrc)
                vst = cf.verify_batch_dev(plan, base_t, uo, uc)[0]
                again = [p + ".again" for p in prev]
                sst, fs, dst = cf.store_paths_dev(w, base_t, uo, uc, again, stage, gate=vst)
                lst, _ = cf.release_set_batch_dev(w, base_t, uo, uc, pset.arg(), gate=dst)
                for t in (wst, est, vst, lst):
                    assert not t.cpu().numpy().any(), c
                assert not sst.any()
                for k, p in enumerate(prev):
                    want = host_append(str(tmp_path / f"host{c}"), f"h{k}", p, [more[k]])
                    assert open(again[k], "rb").read() == want, (c, k)
            tops.append(int(u64(arena_t)[0]))
            assert u64(pset.words_t)[0] == n      # every slot taken from the set came back
    assert tops[0] > 48 and tops[1] == tops[2] == tops[0]
