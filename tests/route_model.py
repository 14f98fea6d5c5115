"""A numpy restatement of routing records to chunk images by their metadata
(include/chunkio_amd/cio_route_dev.h) over host copies of the buffers.  The
route itself knows nothing of hashing: for each record, the lowest image index
that satisfies R4's conditions by direct comparison.  The directory of R1 is
modelled beside it with zlib, and `collide` makes byte strings of a chosen key
so that tests can put several different tags under one key.  Shared by
test_route_abi.py (which asserts it by hand) and test_gpu_route.py (which pins
the device to it).  Not a test."""
import zlib

import numpy as np

from read_dev_model import HDR, U64_MAX, image_check

OK, ERROR, RETRY = 0, -1, -2
MAX_TAG = 65535
EMPTY_KEY = 0xFFFFFFFF


def key(data):
    """R0: the raw (un-finalized) CRC-32 state of a byte string."""
    return ~zlib.crc32(bytes(data)) & 0xFFFFFFFF


def metadata(base, dev_bytes, off, cap):
    """The metadata bytes of an image that passes the image check, else None."""
    ok, meta, _ = image_check(base, dev_bytes, off, cap)
    if not ok:
        return None
    o = int(off) + HDR
    return bytes(base[o:o + meta])


def build(base, offs, caps, dev_bytes=None):
    """R1: (dir_keys, dir_imgs, dir_hdr)."""
    dev_bytes = len(base) if dev_bytes is None else dev_bytes
    metas = [metadata(base, dev_bytes, offs[i], caps[i]) for i in range(len(offs))]
    pairs = sorted((key(m if m is not None else b""), i) for i, m in enumerate(metas))
    hdr = np.asarray([len(offs), sum(m is not None for m in metas), 0, 0], np.uint32)
    return (np.asarray([k for k, _ in pairs], np.uint32), np.asarray([i for _, i in pairs], np.uint32), hdr)


def tag_ok(off, ln, tag_bytes):
    """R2."""
    off, ln = int(off), int(ln)
    return ln == 0 or (ln <= MAX_TAG and off + ln <= U64_MAX and off + ln <= tag_bytes)


def route(base, offs, caps, tags, tag_offs, tag_lens, miss_img, gate=None, dev_bytes=None, tag_bytes=None,
          dir_n=None):
    """R2, R4, R5, R7, R8 with a directory that R1 built over the same images:
    (rec_img, rec_status, total, miss_list).  dir_n: dev_dir_hdr[0] when it is
    not the number of images.  miss_list holds the missed records alone."""
    dev_bytes = len(base) if dev_bytes is None else dev_bytes
    tag_bytes = (0 if tags is None else len(tags)) if tag_bytes is None else tag_bytes
    n_img, n_rec = len(offs), len(tag_offs)
    metas = [metadata(base, dev_bytes, offs[i], caps[i]) for i in range(n_img)]
    if gate is not None:
        metas = [m if int(gate[i]) == OK else None for i, m in enumerate(metas)]
    rec_img = np.full(n_rec, miss_img, np.uint32)
    status = np.full(n_rec, ERROR, np.int32)
    if dir_n is not None and dir_n != n_img:
        return rec_img, status, np.asarray([0, 0, n_rec], np.uint64), np.zeros(0, np.uint32)
    for r in range(n_rec):
        o, ln = int(tag_offs[r]), int(tag_lens[r])
        if not tag_ok(o, ln, tag_bytes):
            continue
        tag = bytes(tags[o:o + ln]) if ln else b""
        status[r] = RETRY
        for i, m in enumerate(metas):
            if m is not None and m == tag:
                rec_img[r], status[r] = i, OK
                break
    total = np.asarray([(status == OK).sum(), (status == RETRY).sum(), (status == ERROR).sum()], np.uint64)
    return rec_img, status, total, np.flatnonzero(status == RETRY).astype(np.uint32)


def judge(base, offs, caps, tags, tag_offs, tag_lens, rec_img, status, gate=None, dev_bytes=None):
    """R6: every record with status OK names an image < n_img that passes the
    gate and the image check and whose metadata equals the tag."""
    dev_bytes = len(base) if dev_bytes is None else dev_bytes
    for r in np.flatnonzero(np.asarray(status) == OK):
        i = int(rec_img[r])
        assert i < len(offs), (r, i)
        assert gate is None or int(gate[i]) == OK, (r, i)
        o, ln = int(tag_offs[r]), int(tag_lens[r])
        assert metadata(base, dev_bytes, offs[i], caps[i]) == (bytes(tags[o:o + ln]) if ln else b""), (r, i)


# ------------------------------------------------------------------ colliding tags

def _table():
    t = []
    for n in range(256):
        c = n
        for _ in range(8):
            c = (c >> 1) ^ 0xEDB88320 if c & 1 else c >> 1
        t.append(c)
    return t


_T = _table()
_TOP = {c >> 24: n for n, c in enumerate(_T)}     # the table entry with a given top byte: one each


def collide(prefix, target):
    """The four bytes X with key(prefix + X) == target, by the backward walk
    through the CRC table: the state after X is `target`; the top byte of a
    state names the table entry of its last step, which gives the state before
    it up to its low byte, and the four unknown low bytes are what X must be."""
    target &= 0xFFFFFFFF
    state, idx = target, []
    for _ in range(4):
        n = _TOP[state >> 24]
        idx.append(n)
        state = ((state ^ _T[n]) << 8) & 0xFFFFFFFF
    # forward: from the state after the prefix, the byte that selects each table entry
    cur, out = key(prefix), bytearray()
    for n in reversed(idx):
        out.append((cur ^ n) & 0xFF)
        cur = (cur >> 8) ^ _T[n]
    assert cur == target
    return bytes(out)


def colliding(prefixes, target):
    """One byte string per prefix, all of key `target`."""
    return [bytes(p) + collide(p, target) for p in prefixes]


def pack_tags(tags, gap=lambda r: 2 * (r % 3) + 1, fill=0xA5):
    """The tags packed at odd offsets into one buffer: (buffer, offs, lens)."""
    offs, pos = [], 1
    for r, t in enumerate(tags):
        pos += gap(r)
        pos |= 1
        offs.append(pos)
        pos += len(t)
    buf = np.full(pos + 3, fill, np.uint8)
    for o, t in zip(offs, tags):
        buf[o:o + len(t)] = np.frombuffer(bytes(t), np.uint8)
    return buf, np.asarray(offs, np.uint64), np.asarray([len(t) for t in tags], np.uint64)
