#!/usr/bin/env python3
"""Rotating full chunk images (cio_file_rotate_batch_dev) against what a caller
did before it existed, in one process (profiles/r15/rotate_dev_ab.json).

    python tools/rotate_dev_ab.py [--cfg cfg2,cfg4k] [--iters 20] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r15/rotate_dev_ab.json

Per shape, n images of `used` bytes (24 + 32 bytes of metadata + content)
without any room, a need of one byte each, no limit, new_cap = used, align 16:
every image is full and is rotated.  Event times on one stream, warm, image
buffers (images + arena) rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round.  What a rotate call rewrites (offsets,
capacities, crc_cur, the arena's top, the list's count) is restored before the
first event of every call.

  a    the whole rotate call                   header, scan, place, planner, append_copy, CRC, commit
  a2   the same again                          the A/A spread (noise)
  b    the floor of what a caller does today,  cio_file_seal_batch_dev over the images, then
       with a library of the PARENT commit     cio_file_init_batch_dev into slots computed on the host (the
                                               same slots, the same buffer) with the metadata copied out
                                               beforehand, untimed.  The read-back of the statuses or lengths
                                               that recipe needs to FIND the full images is NOT in it, nor the
                                               host's work on them.  Skipped (and recorded so) without
                                               --parent-lib.
  c    the bookkeeping kernels alone           cioa_debug_rotate_events section 2: rotate_headers, rotate_scan,
                                               rotate_place
  d    a batch in which nothing is full        the same images with 64 bytes of room each: the fixed cost every
                                               guarded append pays
  e1w  the pre-reduced sums, distinct images   section 6 of the records variant: grow_clear + rotate_sums_wave,
                                               one record per image
  e1m  the same again                          the A/A spread of the sums legs
  e2w  the pre-reduced sums, one image         all records to image 0: one atomic per wave
  e1n  the sums the calls run, distinct        section 1: grow_clear + grow_need (plain atomics; the grow unit's
  e2n  the sums the calls run, one image       kernels through launch_need_sums)
  e1p  the same kernels through grow's hook,   cioa_debug_grow_events section 1: grow_clear + grow_need, what
  e2p  distinct images / one image             r15 measured as "the parent's sums"

a - b is what the device-side decision costs over the parent's two calls.
"""
import argparse
import ctypes
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALIGN, ROOM, META = 16, 64, 32
SHAPES = {"cfg2": (1024, 409600), "cfg4k": (102400, 4096)}     # n, used bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="libchunkio_amd.so built from the parent commit (leg b)")
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    V, U64, S, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    lib.cioa_debug_rotate_events.restype = I
    lib.cioa_debug_rotate_events.argtypes = [V, V, U64, V, V, S, V, V, V, S, U64, U64, U64, V, V, V, V, V, I, V, V, V,
                                             V, I, V, V]
    lib.cioa_debug_grow_events.restype = I
    lib.cioa_debug_grow_events.argtypes = [V, V, U64, V, V, S, V, V, V, S, V, U64, U64, U64, I, V, V, V, I, V, V]
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.cio_dev_writer_create.restype, parent.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        parent.cio_dev_writer_destroy.restype, parent.cio_dev_writer_destroy.argtypes = None, [V]
        parent.cio_file_seal_batch_dev.restype = I
        parent.cio_file_seal_batch_dev.argtypes = [V, V, U64, V, V, S, I, V, V, V]
        parent.cio_file_init_batch_dev.restype = I
        parent.cio_file_init_batch_dev.argtypes = [V, V, U64, V, V, S, V, U64, V, V, I, V, V, V]
        parent.cio_gpu_last_error.restype = ctypes.c_char_p
        parent.cio_gpu_version.restype = ctypes.c_char_p
        assert not hasattr(parent, "cio_file_rotate_batch_dev"), "--parent-lib already has the rotate call"
    if not torch.cuda.is_available():
        raise SystemExit("rotate_dev_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    CK = cf.CIO_CHECKSUM

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters,
                    "rounds": args.rounds, "version": lib.cio_gpu_version().decode(),
                    "parent_version": parent.cio_gpu_version().decode() if parent else None,
                    "align": ALIGN, "meta_bytes": META})
    for cfg in args.cfg.split(","):
        n, used = SHAPES[cfg]
        stride = used + ROOM                                   # leg d claims the room, the others do not
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        caps = np.full(n, used, np.uint64)
        new_cap = used                                         # a multiple of ALIGN: slot = new_cap
        top = (n * stride + 4095) // 4096 * 4096
        slots = np.uint64(top) + np.arange(n, dtype=np.uint64) * np.uint64(new_cap)
        end = top + n * new_cap
        nbytes = end
        nrot = 2
        hdr = np.zeros((n, 24 + META), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = np.full(n, used - 24 - META, np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
        hdr[:, 23] = META
        hdr[:, 24:] = (np.arange(n * META, dtype=np.uint64) * 7 % 251 + 1).astype(np.uint8).reshape(n, META)
        hdr_t = torch.from_numpy(hdr).to(dev)
        hdr_idx = (i64(offs)[:, None] + torch.arange(24 + META, device=dev)[None, :]).reshape(-1)
        bufs = []
        for b in range(nrot):
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            t[:top] = torch.arange(top, device=dev, dtype=torch.int32).mul_(37 + b).to(torch.uint8)
            t[hdr_idx] = hdr_t.reshape(-1)
            bufs.append(t)
        del hdr_idx
        # the parent recipe's metadata, copied out first (untimed)
        meta_src = torch.from_numpy(np.ascontiguousarray(hdr[:, 24:]).reshape(-1)).to(dev)
        meta_offs, meta_lens = i64(np.arange(n, dtype=np.uint64) * META), i64(np.full(n, META, np.uint64))
        offs0, caps0, capsd0, arena0 = i64(offs), i64(caps), i64(caps + np.uint64(ROOM)), i64([top, end])
        crc0 = torch.arange(n, dtype=torch.int32, device=dev)
        count0 = i64([0, n])
        offs_t, caps_t, arena_t, crc_t, count_t = (offs0.clone(), caps0.clone(), arena0.clone(), crc0.clone(),
                                                   count0.clone())
        need_t, slots_t, slotcaps_t = i64(np.ones(n, np.uint64)), i64(slots), i64(np.full(n, new_cap, np.uint64))
        lo_t, lc_t = torch.zeros(n, dtype=torch.int64, device=dev), torch.zeros(n, dtype=torch.int64, device=dev)
        li_t = torch.zeros(n, dtype=torch.int32, device=dev)
        rec_distinct = torch.arange(n, dtype=torch.int32, device=dev)
        rec_one = torch.zeros(n, dtype=torch.int32, device=dev)
        writer = cf.DevWriter(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(2, dtype=torch.int64, device=dev)
        pcrc = crc0.clone()
        pw = V()
        if parent:
            assert parent.cio_dev_writer_create(ctypes.byref(pw), n) == 0, parent.cio_gpu_last_error()

        def restore(room=False):
            offs_t.copy_(offs0)
            caps_t.copy_(capsd0 if room else caps0)
            arena_t.copy_(arena0)
            crc_t.copy_(crc0)
            count_t.copy_(count0)

        def rot_hook(k, section, ev, rec):
            _lib.check(lib.cioa_debug_rotate_events(
                writer._handle, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n,
                need_t.data_ptr() if rec is None else None, rec.data_ptr() if rec is not None else None,
                need_t.data_ptr() if rec is not None else None, n if rec is not None else 0, 0, new_cap, ALIGN,
                arena_t.data_ptr(), lo_t.data_ptr(), lc_t.data_ptr(), li_t.data_ptr(), count_t.data_ptr(), CK,
                crc_t.data_ptr(), total.data_ptr(), status.data_ptr(), stream, section, ev[0], ev[1]),
                "rotate section")

        def grow_hook(k, ev, rec):
            _lib.check(lib.cioa_debug_grow_events(
                writer._handle, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n, None,
                rec.data_ptr(), need_t.data_ptr(), n, arena_t.data_ptr(), 32768, 4096, ALIGN, 0, total.data_ptr(),
                status.data_ptr(), stream, 1, ev[0], ev[1]), "grow section")

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            restore(room=name == "d")
            if name == "c":
                return rot_hook(k, 2, ev, None)
            if name in ("e1n", "e2n"):
                return rot_hook(k, 1, ev, rec_one if name == "e2n" else rec_distinct)
            if name in ("e1w", "e1m", "e2w"):
                return rot_hook(k, 6, ev, rec_one if name == "e2w" else rec_distinct)
            if name in ("e1p", "e2p"):
                return grow_hook(k, ev, rec_one if name == "e2p" else rec_distinct)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name in ("a", "a2", "d"):
                cf.rotate_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, limit=0, new_cap=new_cap, align=ALIGN,
                                    arena=arena_t, out_offs=lo_t, out_caps=lc_t, out_img=li_t, out_count=count_t,
                                    flags=CK, crc_cur=crc_t, total=total, status=status)
            elif name == "b":
                rc = parent.cio_file_seal_batch_dev(pw, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(),
                                                    caps_t.data_ptr(), n, CK, pcrc.data_ptr(), status.data_ptr(),
                                                    stream)
                assert rc == 0, parent.cio_gpu_last_error()
                rc = parent.cio_file_init_batch_dev(pw, bufs[k].data_ptr(), nbytes, slots_t.data_ptr(),
                                                    slotcaps_t.data_ptr(), n, meta_src.data_ptr(), n * META,
                                                    meta_offs.data_ptr(), meta_lens.data_ptr(), CK, pcrc.data_ptr(),
                                                    status.data_ptr(), stream)
                assert rc == 0, parent.cio_gpu_last_error()
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "b", "c", "d", "e1w", "e1p", "e2w", "e2p", "e1n", "e2n", "e1m", "a2"]
        if not parent:
            order.remove("b")
        # correctness at the timed size
        fresh = hdr.copy()
        fresh[:, 2:6] = np.frombuffer(bytes([0xFF, 0x12, 0xD9, 0x41]), np.uint8)
        fresh[:, 10:14] = 0
        for k in range(nrot):
            for name in order:
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                if name in ("a", "a2", "b", "c", "d", "e1n", "e1m", "e2n", "e1w", "e2w"):
                    assert not status.cpu().numpy().any(), f"{cfg}: leg {name}: an entry was refused"
                if name in ("a", "a2", "c", "e1n", "e1m", "e1w"):       # the hooks run the whole call
                    assert torch.equal(offs_t, slots_t) and torch.equal(lo_t, offs0), f"{cfg}: leg {name}: offsets"
                    assert arena_t.cpu().tolist() == [end, end] and count_t.cpu().tolist() == [n, n], (cfg, name)
                    assert total.cpu().tolist() == [n * new_cap, n], (cfg, name)
                if name == "d":
                    assert torch.equal(offs_t, offs0) and count_t.cpu().tolist() == [0, n], f"{cfg}: leg {name}"
                if name in ("e2n", "e2w"):
                    assert count_t.cpu().tolist() == [1, n] and total.cpu().tolist() == [new_cap, 1], (cfg, name)
                if name in ("a", "b"):
                    for i in (0, n // 3, n - 1):
                        d = int(slots[i])
                        got = bufs[k][d:d + 24 + META].cpu().numpy()
                        assert np.array_equal(got, fresh[i]), f"{cfg}: leg {name}: fresh image {i}"
        info = {"n": n, "used_bytes": used, "new_cap": new_cap, "buffer_bytes": nbytes, "rotating_buffers": nrot,
                "copy_workgroups": cus * 8}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                leg("a", k % nrot, evs[0])
            torch.cuda.synchronize()
        per_round = {k: [] for k in order}
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                for i in range(3):
                    leg(name, i % nrot, evs[0])
                for i in range(args.iters):
                    leg(name, i % nrot, evs[i])
                torch.cuda.synchronize()
                times = [lib.cio_gpu_event_elapsed_ms(e0, e1) for e0, e1 in evs]
                per_round[name].append(float(np.mean(times)) * 1e3)
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        info["us"] = {k: round(v, 2) for k, v in med.items()}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["aa_spread_us"] = round(abs(med["a2"] - med["a"]), 2)
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["b_measured"] = bool(parent)
        info["a_over_b"] = round(med["a"] / med["b"], 3) if parent else None
        info["a_minus_b_us"] = round(med["a"] - med["b"], 2) if parent else None
        # the decision on the pre-reduction: faster on the one-image list by more than the A/A spread, and not
        # slower on the distinct list by more than three times the A/A spread (the larger of the two spreads)
        spread = max(abs(med["a2"] - med["a"]), abs(med["e1m"] - med["e1w"]))
        info["sums"] = {"aa_spread_us": round(spread, 2),
                        "aa_spread_sums_legs_us": round(abs(med["e1m"] - med["e1w"]), 2),
                        "one_image_parent_minus_new_us": round(med["e2p"] - med["e2w"], 2),
                        "distinct_new_minus_parent_us": round(med["e1w"] - med["e1p"], 2),
                        "one_image_faster": bool(med["e2p"] - med["e2w"] > spread),
                        "distinct_not_slower": bool(med["e1w"] - med["e1p"] <= 3 * spread)}
        info["sums"]["keep_pre_reduction"] = info["sums"]["one_image_faster"] and info["sums"]["distinct_not_slower"]
        results["shapes"][cfg] = info
        print(cfg, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        if parent:
            parent.cio_dev_writer_destroy(pw)
        del bufs
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
