"""Transactions on chunk images in device memory
(include/chunkio_amd/cio_write_dev_tx.h), without a GPU: the four symbols and
the Python exports exist with the declared prototypes, every argument check
runs before any device call, the host check of the kernels' text (`make
txcheck`, a stand-alone program under ASan + UBSan) passes, and the numpy model
the GPU tests compare against is asserted by hand on a batch of eight images,
one per branch of the rollback's order."""
import ctypes
import inspect
import os
import re
import struct
import subprocess

import numpy as np
import pytest

import chunkio_amd
from chunkio_amd import _lib
from chunkio_amd import chunkfile as cf

import tx_dev_model as model
from write_dev_move_model import M32, m_init, m_meta_write, m_write, m_write_at, raw_update

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
BEGIN, ROLLBACK, COMMIT = ("cio_file_tx_begin_batch_dev", "cio_file_tx_rollback_batch_dev",
                           "cio_file_tx_commit_batch_dev")
COND = "cio_file_tx_cond_records_batch_dev"
CK, REC, ZERO = cf.CIO_CHECKSUM, cf.CIOA_TX_RECOMPUTE, cf.CIOA_TX_ZERO

CTYPE = {"int": ctypes.c_int, "uint32_t": ctypes.c_uint32, "uint64_t": ctypes.c_uint64, "size_t": ctypes.c_size_t}


def declarations():
    """{name: (result, [argument types])} of the header, pointers as c_void_p."""
    with open(os.path.join(ROOT, "include", "chunkio_amd", "cio_write_dev_tx.h")) as f:
        raw = f.read()
    text = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    out = {}
    for res, name, args in re.findall(r"^(\w+)\s+(cio_[a-z_]+)\s*\(([^;]*)\);", text, flags=re.M):
        types = []
        for a in args.split(","):
            a = a.strip()
            types.append(ctypes.c_void_p if "*" in a else CTYPE[a.replace("const ", "").split()[0]])
        out[name] = (CTYPE[res], types)
    return out, raw


def aligned_buffer(size, residue=0):
    """A host buffer whose address is `residue` modulo 16 (kept alive by the
    returned owner)."""
    owner = ctypes.create_string_buffer(size + 32)
    addr = (ctypes.addressof(owner) + 15) // 16 * 16 + residue
    return owner, ctypes.c_void_p(addr)


def begin_args(writer, buf, n=1, flags=0):
    """A full argument list over one host buffer (never dereferenced: every
    call here is refused, or is a no-op, before that)."""
    return [writer, buf, 64, buf, buf, n, flags, buf, buf, buf, None]


def act_args(writer, buf, n=1, flags=0):
    return [writer, buf, 64, buf, buf, n, buf, flags, buf, buf, buf, None]


CALLS = ((BEGIN, begin_args, CK), (ROLLBACK, act_args, CK | REC | ZERO), (COMMIT, act_args, CK))


def test_symbols_are_exported_with_the_declared_prototypes():
    lib = chunkio_amd.lib()
    decl, raw = declarations()
    assert set(decl) == {BEGIN, ROLLBACK, COMMIT, COND}
    for name, nargs in ((BEGIN, 11), (ROLLBACK, 12), (COMMIT, 12), (COND, 7)):
        res, args = decl[name]
        assert name in _lib.EXPORTS
        fn = getattr(lib, name)
        assert fn.restype is res
        bound = [ctypes.c_void_p if (t is ctypes.c_void_p or hasattr(t, "contents")) else t for t in fn.argtypes]
        assert bound == args and len(args) == nargs, name
    assert decl[ROLLBACK] == decl[COMMIT]
    assert '#include "cio_write_dev.h"' in raw
    flat = " ".join(raw.replace("*", " ").split())
    assert "typedef struct { uint32_t active, content_len, crc, meta_len; } cio_dev_tx_state;" in flat
    assert "#define CIOA_TX_RECOMPUTE 256" in flat and "#define CIOA_TX_ZERO 512" in flat
    assert (cf.CIOA_TX_RECOMPUTE, cf.CIOA_TX_ZERO) == (256, 512)
    low = flat.lower()
    assert "two differences from the reference" in low and "preconditions, not checked" in low
    assert "must be rolled back with cioa_tx_recompute" in low


def test_python_binding_exports():
    for name in ("tx_state", "tx_begin_batch_dev", "tx_rollback_batch_dev", "tx_commit_batch_dev",
                 "tx_cond_records_batch_dev", "CIOA_TX_RECOMPUTE", "CIOA_TX_ZERO"):
        assert getattr(chunkio_amd, name) is getattr(cf, name)
    assert list(inspect.signature(cf.tx_state).parameters) == ["n", "device"]
    p = inspect.signature(cf.tx_begin_batch_dev).parameters
    assert list(p) == ["writer", "base", "img_offs", "img_caps", "tx", "crc_cur", "flags", "status", "stream"]
    for fn in (cf.tx_rollback_batch_dev, cf.tx_commit_batch_dev):
        q = inspect.signature(fn).parameters
        assert list(q) == ["writer", "base", "img_offs", "img_caps", "tx", "crc_cur", "cond", "flags", "status",
                           "stream"]
        assert q["cond"].default is None and q["flags"].default == cf.CIO_CHECKSUM
    r = inspect.signature(cf.tx_cond_records_batch_dev).parameters
    assert list(r) == ["rec_img", "rec_status", "n_img", "img_status", "cond", "stream"]


@pytest.mark.parametrize("name,make,allowed", CALLS)
def test_bad_values_are_refused_without_a_gpu(name, make, allowed):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    owner, buf = aligned_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # just a non-null address: refused before it is looked at
    err = lib.cio_gpu_last_error
    for flags in (1, 2, 8, 128, 1024, 5, 1 << 30, -1) + tuple(f for f in (REC, ZERO, CK | REC) if f & ~allowed):
        assert fn(*make(writer, buf, flags=flags)) == -1, flags
        assert (name + ": unknown flags").encode() in err(), flags
    if name == ROLLBACK:
        for flags in (REC, REC | ZERO):
            for n in (0, 1):
                assert fn(*make(writer, buf, n=n, flags=flags)) == -1
                assert (name + ": CIOA_TX_RECOMPUTE needs CIO_CHECKSUM").encode() in err()
    # the same with an empty batch: the values are checked first
    assert fn(*make(writer, buf, n=0, flags=2)) == -1
    for n in (0, 1):
        assert fn(*make(None, buf, n=n)) == -1
        assert (name + ": null writer").encode() in err()


@pytest.mark.parametrize("name,make,allowed", CALLS)
def test_null_pointers_and_oversized_batches_are_refused_without_a_gpu(name, make, allowed):
    """Null buffers are refused before the writer is looked at; then a
    misaligned state array; then the writer's capacity (the block stands in
    for a writer: max_chunks, its first word, 4, everything else zero).
    dev_cond may be NULL, and dev_crc_cur without CIO_CHECKSUM."""
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    owner, buf = aligned_buffer(64)
    owner2, odd = aligned_buffer(64, residue=8)
    writer = ctypes.create_string_buffer(1024)
    ctypes.memmove(writer, ctypes.byref(ctypes.c_uint32(4)), 4)
    err = lib.cio_gpu_last_error
    for flags in (0, CK):
        full = make(writer, buf, n=5, flags=flags)
        if name == BEGIN:
            required, crc, optional, tx = (1, 3, 4, 8, 9), 7, (), 8
        else:
            required, crc, optional, tx = (1, 3, 4, 9, 10), 8, (6,), 9
        for j in required + ((crc,) if flags else ()):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (name + ": null pointer").encode() in err(), j
        for j in optional + (() if flags else (crc,)):
            a = list(full)
            a[j] = None
            assert fn(*a) == -1, j
            assert (name + ": more images than the writer").encode() in err(), j
        a = list(full)
        a[tx] = odd
        assert fn(*a) == -1
        assert (name + ": dev_tx must be 16-byte aligned").encode() in err()
        assert fn(*full) == -1
        assert (name + ": more images than the writer").encode() in err()


@pytest.mark.parametrize("name,make,allowed", CALLS)
def test_empty_batches_are_accepted_without_a_gpu(name, make, allowed):
    lib = chunkio_amd.lib()
    fn = getattr(lib, name)
    owner, buf = aligned_buffer(64)
    writer = ctypes.create_string_buffer(1024)    # max_chunks reads 0: an empty batch never gets that far
    for flags in (0, CK, allowed):
        assert fn(*make(writer, buf, n=0, flags=flags)) == 0
    assert fn(*[None if x is buf else x for x in make(writer, buf, n=0)]) == 0


def test_cond_argument_checks_without_a_gpu():
    lib = chunkio_amd.lib()
    fn = getattr(lib, COND)
    owner, buf = aligned_buffer(64)
    err = lib.cio_gpu_last_error
    assert fn(buf, buf, 5, buf, 0, buf, None) == 0          # no images: a no-op
    assert fn(None, None, 0, None, 0, None, None) == 0
    assert fn(buf, buf, 5, buf, 3, None, None) == -1
    assert (COND + ": null pointer").encode() in err()
    assert fn(None, buf, 5, buf, 3, buf, None) == -1 and (COND + ": null pointer").encode() in err()
    assert fn(buf, None, 5, None, 3, buf, None) == -1 and (COND + ": null pointer").encode() in err()
    assert fn(buf, buf, 1 << 32, None, 3, buf, None) == -1
    assert (COND + ": more than 2^32 - 2 images or records").encode() in err()
    assert fn(buf, buf, 5, None, 0xFFFFFFFF, buf, None) == -1
    assert (COND + ": more than 2^32 - 2 images or records").encode() in err()


def test_txcheck():
    """The kernels' text on the host over real image bytes, every workgroup
    order, against a sequential loop, and the condition kernel wave by wave
    with its atomics counted, under ASan + UBSan (a stand-alone program)."""
    r = subprocess.run(["make", "-C", ROOT, "txcheck"], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    assert "tx_check: ok" in r.stdout


# ------------------------------------------------------------------ the model, by hand

META = b"tag!"


def hand_batch():
    """Eight images of capacity 90 at 1, 101, .. 701 with metadata "tag!" and
    ten bytes of content (image 7: none), a transaction begun on all of them,
    and inside it: 0 seven more bytes -- and the condition says it succeeded;
    1 seven more bytes, but its entry is not active; 2 its magic broken; 3 cut
    to five bytes by write_at and four written there (nine in all, fewer than
    at begin); 4 its metadata replaced by five bytes; 5 seven more bytes; 6
    nothing; 7 seven bytes into the empty image.  Returns (buf, offs, caps,
    crc_cur, tx, cond, the crc_cur at begin)."""
    buf = np.full(1024, 0xA5, np.uint8)
    offs, caps = [100 * i + 1 for i in range(8)], [90] * 8
    crc = []
    for i in range(8):
        raw = m_init(buf, offs[i], META)
        crc.append(raw if i == 7 else m_write(buf, offs[i], bytes([0x30 + i]) * 10, raw))
    tx = model.new_state(8)
    assert not model.m_tx_begin(buf, offs, caps, tx, crc).any()
    assert tx == [[1, 0 if i == 7 else 10, crc[i], 4] for i in range(8)]
    at_begin = list(crc)
    for i in (0, 1, 5, 7):
        crc[i] = m_write(buf, offs[i], bytes([0x60 + i]) * 7, crc[i])
    tx[1][0] = 0
    buf[offs[2] + 1] = 0x01
    crc[3] = m_write_at(buf, offs[3], 5, b"wxyz", crc[3])
    crc[4] = m_meta_write(buf, offs[4], b"tag!!", crc[4])
    return buf, offs, caps, crc, tx, [0] + [-1] * 7, at_begin


def header(content, raw):
    return struct.pack("<Q", raw), struct.pack(">I", content)


@pytest.mark.parametrize("flags", [CK, CK | ZERO, 0, ZERO])
def test_model_rollback_on_a_hand_written_batch(flags):
    buf, offs, caps, crc, tx, cond, at_begin = hand_batch()
    before, crc_before, tx_before = buf.copy(), list(crc), [list(t) for t in tx]
    # begin again: a no-op on the active entries, even for the image that is broken by now; entry 1 begins
    tx2 = [list(t) for t in tx]
    assert not model.m_tx_begin(buf, offs, caps, tx2, crc).any() and np.array_equal(buf, before)
    assert tx2 == [[1, 17, crc[1], 4] if i == 1 else tx_before[i] for i in range(8)]
    st, rolled = model.m_tx_rollback(buf, offs, caps, tx, crc, cond, flags=flags)
    # 0 skipped, 1 not active, 2 no image, 3 shorter than at begin, 4 another metadata length
    assert st.tolist() == [0, -1, -1, -1, -1, 0, 0, 0] and rolled == [5, 6, 7]
    want = before.copy()
    for i in (5, 6, 7):
        o, kept = offs[i], 0 if i == 7 else 10
        want[o + 10:o + 14] = np.frombuffer(struct.pack(">I", kept), np.uint8)
        if flags & CK:
            want[o + 2:o + 10] = np.frombuffer(struct.pack("<Q", at_begin[i]), np.uint8)
        if flags & ZERO and i != 6:
            want[o + 28 + kept:o + 28 + kept + 7] = 0
    assert np.array_equal(buf, want)
    assert crc == [at_begin[i] if i in (5, 6, 7) and flags & CK else crc_before[i] for i in range(8)]
    assert [t[0] for t in tx] == [1, 0, 1, 1, 1, 0, 0, 0] and [t[1:] for t in tx] == [t[1:] for t in tx_before]
    # once more: the rolled-back entries are not active any more
    again = buf.copy()
    st, rolled = model.m_tx_rollback(buf, offs, caps, tx, crc, cond, flags=flags)
    assert st.tolist() == [0] + [-1] * 7 and rolled == [] and np.array_equal(buf, again)
    # the commit with the same condition acts on image 0 alone and seals it with all 17 bytes
    st, done = model.m_tx_commit(buf, offs, caps, tx, crc, cond, flags=flags)
    assert not st.any() and done == [0] and tx[0] == [0, 10, at_begin[0], 4]
    if flags & CK:
        again[offs[0] + 2:offs[0] + 10] = np.frombuffer(struct.pack(">I", crc[0] ^ M32) + b"\0" * 4, np.uint8)
    assert np.array_equal(buf, again)
    assert struct.unpack(">I", buf[offs[0] + 10:offs[0] + 14].tobytes())[0] == 17


def test_model_rollback_with_recompute():
    """CIOA_TX_RECOMPUTE: image 4, whose metadata grew by a byte inside the
    transaction, is rolled back too, to ten bytes behind the NEW metadata, and
    its crc_cur is the CRC of what is kept; image 3 is still too short."""
    buf, offs, caps, crc, tx, cond, at_begin = hand_batch()
    before = buf.copy()
    st, rolled = model.m_tx_rollback(buf, offs, caps, tx, crc, cond, flags=CK | REC | ZERO)
    assert st.tolist() == [0, -1, -1, -1, 0, 0, 0, 0] and rolled == [4, 5, 6, 7]
    o = offs[4]
    kept = before[o + 22:o + 24 + 5 + 10].tobytes()
    assert kept[:2] == b"\0\5" and kept[2:7] == b"tag!!" and kept[7:] == bytes([0x34]) * 10
    assert crc[4] == raw_update(M32, kept) and crc[4] != at_begin[4]
    assert buf[o + 2:o + 14].tobytes() == struct.pack("<Q", crc[4]) + struct.pack(">I", 10)
    assert np.array_equal(buf[o + 14:o + 90], before[o + 14:o + 90])          # nothing was dropped: cur was 10
    for i in (5, 6, 7):
        assert crc[i] == at_begin[i]                                          # the recomputed state is the saved one
    assert not buf[offs[5] + 38:offs[5] + 45].any() and buf[offs[5] + 45] == 0xA5


def test_model_commit_on_inactive_and_broken_images():
    buf, offs, caps, crc, tx, cond, at_begin = hand_batch()
    before = buf.copy()
    st, done = model.m_tx_commit(buf, offs, caps, tx, crc, None, flags=CK)
    assert st.tolist() == [0, 0, -1, 0, 0, 0, 0, 0] and done == [0, 1, 3, 4, 5, 6, 7]
    want = before.copy()
    for i in done:                                # image 1 was not active: sealed all the same
        want[offs[i] + 2:offs[i] + 10] = np.frombuffer(struct.pack(">I", crc[i] ^ M32) + b"\0" * 4, np.uint8)
    assert np.array_equal(buf, want)
    assert [t[0] for t in tx] == [0, 0, 1, 0, 0, 0, 0, 0]
    # without CIO_CHECKSUM no byte is written
    st, done = model.m_tx_commit(buf, offs, caps, tx, crc, None, flags=0)
    assert np.array_equal(buf, want) and st.tolist() == [0, 0, -1, 0, 0, 0, 0, 0]


def test_model_condition():
    n = 6
    rec_img = [0, 0, 1, 3, 3, 3, 5]
    rec_st = [0, 0, -1, 0, 0, -3, 0]
    assert model.m_tx_cond(rec_img, rec_st, n).tolist() == [0, -1, 0, -1, 0, 0]
    assert model.m_tx_cond(rec_img, rec_st, n, img_status=[0, 0, -1, 0, 0, 0]).tolist() == [0, -1, -1, -1, 0, 0]
    assert model.m_tx_cond(rec_img[::-1], rec_st[::-1], n).tolist() == [0, -1, 0, -1, 0, 0]
    assert model.m_tx_cond(rec_img + [6], rec_st + [0], n).tolist() == [-1] * n
    assert model.m_tx_cond([], [], n).tolist() == [0] * n
    assert model.m_tx_cond([], [], n, img_status=[-1, 0, 0, 0, 0, -1]).tolist() == [-1, 0, 0, 0, 0, -1]
