"""A numpy model of the reference's write operations on one chunk image inside
a byte buffer: what write_init_header, cio_file_write + update_checksum,
cio_file_write_metadata + adjust_layout, cio_chunk_write_at and
finalize_checksum (src/cio_file.c, src/cio_chunk.c) leave in the map, done
literally -- the same memcpy / memmove, in the same order.  Shared by
test_write_dev_move_abi.py (which pins it to the reference-written fixtures)
and test_gpu_write_dev_move.py (which pins the device to it).  Not a test."""
import struct
import zlib

import numpy as np

M32 = 0xFFFFFFFF
EMPTY_RAW = 0xBE26ED00
INIT = bytes([0xC1, 0x00, 0xFF, 0x12, 0xD9, 0x41] + [0] * 18)


def raw_update(raw, data):
    """crc_update on the raw (not finalized) state."""
    return zlib.crc32(bytes(data), raw ^ M32) ^ M32


def pattern(length, seed):
    """The fixtures' content bytes (tests/golden/chunks/manifest.json)."""
    i = np.arange(length, dtype=np.uint64)
    return (((i * 131 + seed * 7 + 17) % 251) + 1).astype(np.uint8).tobytes()


def m_geometry(buf, off):
    meta = struct.unpack(">H", buf[off + 22:off + 24].tobytes())[0]
    content = struct.unpack(">I", buf[off + 10:off + 14].tobytes())[0]
    return meta, content


def m_region_crc(buf, off):
    """cio_file_calculate_checksum: bytes [22, 24 + meta + content)."""
    meta, content = m_geometry(buf, off)
    return raw_update(M32, buf[off + 22:off + 24 + meta + content].tobytes())


def m_init(buf, off, meta=b"", checksum=True):
    buf[off:off + 24] = np.frombuffer(INIT, np.uint8)
    if not checksum:
        buf[off + 2:off + 6] = 0
    buf[off + 22:off + 24] = np.frombuffer(struct.pack(">H", len(meta)), np.uint8)
    buf[off + 24:off + 24 + len(meta)] = np.frombuffer(bytes(meta), np.uint8)
    return raw_update(M32, buf[off + 22:off + 24 + len(meta)].tobytes())


def m_write(buf, off, data, raw, checksum=True):
    """cio_file_write + update_checksum; the new raw state."""
    if len(data) == 0:
        return raw
    meta, content = m_geometry(buf, off)
    if checksum:
        raw = raw_update(raw, data)
        buf[off + 2:off + 10] = np.frombuffer(struct.pack("<Q", raw), np.uint8)
    pos = off + 24 + meta + content
    buf[pos:pos + len(data)] = np.frombuffer(bytes(data), np.uint8)
    buf[off + 10:off + 14] = np.frombuffer(struct.pack(">I", content + len(data)), np.uint8)
    return raw


def m_meta_write(buf, off, meta, raw, checksum=True):
    """cio_file_write_metadata (:1075-1145): a shorter or equal metadata is
    copied first and the content moved down after it; a longer one moves the
    content up first.  adjust_layout stores the length and recomputes crc_cur
    over the new layout; it does not touch bytes 2..9."""
    old, content = m_geometry(buf, off)
    m = len(meta)
    cur, new = off + 24 + old, off + 24 + m
    if old >= m:
        buf[off + 24:new] = np.frombuffer(bytes(meta), np.uint8)
        buf[new:new + content] = buf[cur:cur + content].copy()          # memmove
    else:
        buf[new:new + content] = buf[cur:cur + content].copy()          # memmove
        buf[off + 24:new] = np.frombuffer(bytes(meta), np.uint8)
    buf[off + 22:off + 24] = np.frombuffer(struct.pack(">H", m), np.uint8)
    return m_region_crc(buf, off) if checksum else raw


def m_write_at(buf, off, at, data, raw, checksum=True):
    """cio_chunk_write_at (:184-209) for a record that is not empty: data_size
    = at, the header's content length follows (cio_file_write:1054-1056),
    update_checksum recomputes crc_cur over the kept prefix (crc_reset) and
    chains the record."""
    if len(data) == 0:
        return raw
    buf[off + 10:off + 14] = np.frombuffer(struct.pack(">I", at), np.uint8)
    if checksum:
        raw = m_region_crc(buf, off)
    return m_write(buf, off, data, raw, checksum)


def m_seal(buf, off, raw):
    buf[off + 2:off + 10] = np.frombuffer(struct.pack(">I", raw ^ M32) + b"\0\0\0\0", np.uint8)


def replay(buf, off, ops, raw=None):
    """The manifest's ops on the image at off (zeroed, of the file's size);
    the final raw state.  close seals what sync did not."""
    raw = m_init(buf, off) if raw is None else raw
    for op in ops:
        if op["op"] == "write":
            raw = m_write(buf, off, pattern(op["len"], op["seed"]), raw)
        elif op["op"] == "write_at":
            raw = m_write_at(buf, off, op["offset"], pattern(op["len"], op["seed"]), raw)
        elif op["op"] == "meta_write":
            raw = m_meta_write(buf, off, op["meta"].encode(), raw)
        elif op["op"] in ("sync", "close"):
            m_seal(buf, off, raw)
    return raw
