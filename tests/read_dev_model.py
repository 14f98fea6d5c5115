"""A numpy restatement of the device read path (include/chunkio_amd/
cio_read_dev.h) over host copies of the buffers: the image check, the gate,
the record selection, the caller-placed and the packed placement, the copy and
the terminators, and cio_meta_cmp's file-system branch.  Every function
returns what the device call is specified to leave: statuses, lengths,
offsets, the total, and the expected output buffer -- a copy of the buffer
passed in, so bytes the call must not write keep their fill.  Shared by
test_read_dev_abi.py (which pins it to the reference-written fixtures and to
the host chunk layer) and test_gpu_read_dev.py (which pins the device to it).
Not a test."""
import numpy as np

OK, ERROR = 0, -1
META, CONTENT, IMAGE = 0, 1, 2
NUL = 1
HDR = 24
U64_MAX = (1 << 64) - 1


def image_check(base, dev_bytes, off, cap):
    """(ok, meta_len, content_len): the write path's image check."""
    off, cap = int(off), int(cap)
    if off + cap > U64_MAX or off + cap > dev_bytes or cap < HDR:
        return False, 0, 0
    if base[off] != 0xC1 or base[off + 1] != 0x00:
        return False, 0, 0
    meta = (int(base[off + 22]) << 8) | int(base[off + 23])
    content = int.from_bytes(base[off + 10:off + 14].tobytes(), "big")
    return HDR + meta + content <= cap, meta, content


def select(what, meta, content):
    """(first byte from the image's start, length) of record `what`."""
    if what == META:
        return HDR, meta
    if what == CONTENT:
        return HDR + meta, content
    if what == IMAGE:
        return 0, HDR + meta + content
    raise ValueError(what)


def _records(base, offs, caps, what, gate, dev_bytes):
    """Per entry: None, or (absolute first byte, length)."""
    dev_bytes = len(base) if dev_bytes is None else dev_bytes
    out = []
    for i in range(len(offs)):
        ok, meta, content = image_check(base, dev_bytes, offs[i], caps[i])
        if not ok or (gate is not None and int(gate[i]) != OK):
            out.append(None)
            continue
        first, ln = select(what, meta, content)
        out.append((int(offs[i]) + first, ln))
    return out


def _finish(base, recs, places, nul, out):
    n = len(recs)
    status = np.full(n, ERROR, np.int32)
    lens = np.zeros(n, np.uint64)
    want = None if out is None else out.copy()
    for i, (r, d) in enumerate(zip(recs, places)):
        if r is None or d is None:
            continue
        status[i] = OK
        lens[i] = r[1]
        if want is not None:
            want[d:d + r[1]] = base[r[0]:r[0] + r[1]]
            if nul:
                want[d + r[1]] = 0
    return status, lens, want


def read_placed(base, offs, caps, what, out, out_offs=None, out_caps=None, gate=None, flags=0, dev_bytes=None,
                out_bytes=None):
    """cio_file_read_batch_dev: (status, lens, expected out).  out = None is the
    size query."""
    recs = _records(base, offs, caps, what, gate, dev_bytes)
    nul = 1 if flags & NUL else 0
    places = []
    for i, r in enumerate(recs):
        if r is None or out is None:
            places.append(0 if r is not None else None)
            continue
        room = len(out) if out_bytes is None else out_bytes
        o, c = int(out_offs[i]), int(out_caps[i])
        fits = o + c <= U64_MAX and o + c <= room and r[1] + nul <= c
        places.append(o if fits else None)
    return _finish(base, recs, places, nul, out)


def read_packed(base, offs, caps, what, out, align=1, gate=None, flags=0, dev_bytes=None, out_bytes=None):
    """cio_file_read_packed_batch_dev: (status, out_offs, lens, total, expected
    out).  out = None is the size query: placed as if unbounded."""
    assert align >= 1 and align <= 4096 and align & (align - 1) == 0
    recs = _records(base, offs, caps, what, gate, dev_bytes)
    nul = 1 if flags & NUL else 0
    room = U64_MAX if out is None else (len(out) if out_bytes is None else out_bytes)
    run, places, out_offs = 0, [], np.zeros(len(recs), np.uint64)
    for i, r in enumerate(recs):
        slot = 0 if r is None else min((r[1] + nul + align - 1) & ~(align - 1), U64_MAX)
        out_offs[i] = min(run, U64_MAX)
        fits = r is not None and run < U64_MAX and run + slot < U64_MAX and run + slot <= room
        places.append(run if fits else None)
        run = min(run + slot, U64_MAX)
    status, lens, want = _finish(base, recs, places, nul, out)
    return status, out_offs, lens, np.asarray([run], np.uint64), want


def meta_cmp(base, offs, caps, cand, cand_offs, cand_lens, dev_bytes=None, cand_bytes=None):
    """cio_meta_cmp_batch_dev: (result, status)."""
    dev_bytes = len(base) if dev_bytes is None else dev_bytes
    cand_bytes = len(cand) if cand_bytes is None else cand_bytes
    n = len(offs)
    result, status = np.full(n, -1, np.int32), np.full(n, ERROR, np.int32)
    for i in range(n):
        ok, meta, _ = image_check(base, dev_bytes, offs[i], caps[i])
        co, cl = int(cand_offs[i]), int(cand_lens[i])
        if not ok or cl > 65535 or co + cl > U64_MAX or co + cl > cand_bytes:
            continue
        status[i] = OK
        o = int(offs[i]) + HDR
        if cl == meta and np.array_equal(base[o:o + meta], cand[co:co + cl]):
            result[i] = 0
    return result, status


def layout(lengths, gaps, start=0):
    """Offsets of back-to-back ranges of `lengths` with gaps[i] bytes before
    range i; (offsets, end)."""
    offs, pos = [], start
    for ln, g in zip(lengths, gaps):
        pos += int(g)
        offs.append(pos)
        pos += int(ln)
    return np.asarray(offs, np.uint64), pos


def make_image(buf, off, meta, content):
    """Write a valid image (header with a zero CRC field, metadata, content)
    at buf[off:]; its used bytes."""
    meta = np.frombuffer(bytes(meta), np.uint8) if isinstance(meta, (bytes, bytearray)) else meta
    content = np.frombuffer(bytes(content), np.uint8) if isinstance(content, (bytes, bytearray)) else content
    m, c = len(meta), len(content)
    buf[off:off + HDR] = 0
    buf[off], buf[off + 1] = 0xC1, 0x00
    buf[off + 10:off + 14] = np.frombuffer(c.to_bytes(4, "big"), np.uint8)
    buf[off + 22:off + 24] = np.frombuffer(m.to_bytes(2, "big"), np.uint8)
    buf[off + HDR:off + HDR + m] = meta
    buf[off + HDR + m:off + HDR + m + c] = content
    return HDR + m + c
