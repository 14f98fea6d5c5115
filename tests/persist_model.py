"""The numpy model of the two file calls of
include/chunkio_amd/cio_persist_dev.h: how a batch is cut into rounds of the
stage (the stage is used whole), where a load places its files -- round by
round through alloc_set_model.m_alloc_set, gated by the verdicts -- and what
the file of a stored image holds."""
import numpy as np

from alloc_set_model import ERR, NONE, OK, m_alloc_set

SLOT = 128                                    # a file's slot in the stage
NO_ROUND = 0xFFFFFFFF
LOAD_ZERO, STORE_TRIM, STORE_SYNC = 512, 1, 2


def m_round_max(stage_bytes):
    return stage_bytes // SLOT * SLOT


def m_rounds(sizes, stage_bytes):
    """(rounds, round_of): files in order; a round is a maximal run of
    consecutive files whose 128-byte-aligned sizes fit the stage; a file over
    the maximum has NO_ROUND and closes the round before it."""
    room = m_round_max(stage_bytes)
    rounds, used, is_open, out = 0, 0, False, []
    for s in (int(x) for x in sizes):
        if s > room:
            out.append(NO_ROUND)
            is_open = False
            continue
        slot = -(-s // SLOT) * SLOT
        if not is_open or used + slot > room:
            rounds, used, is_open = rounds + 1, 0, True
        out.append(rounds - 1)
        used += slot
    return rounds, np.asarray(out, np.uint32)


def m_file_size(used, cap, trim, page):
    return -(-used // page) * page if trim else cap


def m_file(image, used, cap, trim=False, page=4096):
    """The bytes of the file of a stored image: `image` holds at least its used
    bytes."""
    size = m_file_size(used, cap, trim, page)
    out = np.zeros(size, np.uint8)
    k = min(used, size)
    out[:k] = np.asarray(image[:k], np.uint8)
    return out.tobytes()


def m_load_place(buf, sizes, verdict_ok, stage_bytes, arena, set_offs, set_caps, words, n_cls, stride, align=16):
    """Where cio_file_load_paths_dev puts files of these sizes: per round one
    m_alloc_set with need = the size, gated by the verdicts (verdict_ok[i]: the
    file was read and verified).  arena and words are changed in place.
    Returns (status, offs, caps) per file."""
    n = len(sizes)
    _, round_of = m_rounds(sizes, stage_bytes)    # sizes as stat gives them: 0 for a file that is not there
    status, offs, caps = [ERR] * n, [NONE] * n, [0] * n
    for r in sorted(set(int(x) for x in round_of if x != NO_ROUND)):
        idx = [i for i in range(n) if round_of[i] == r]
        gate = [OK if verdict_ok[i] else ERR for i in idx]
        st, _, o, c = m_alloc_set(buf, [int(sizes[i]) for i in idx], gate, arena, set_offs, set_caps, words, n_cls,
                                  stride, align=align)
        for k, i in enumerate(idx):
            status[i], offs[i], caps[i] = int(st[k]), o[k], c[k]
    return status, offs, caps
