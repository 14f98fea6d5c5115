#!/usr/bin/env python3
"""Growing chunk images out of an arena (cio_file_grow_batch_dev) against what a
caller did before it existed, in one process (profiles/r14/grow_dev_ab.json).

    python tools/grow_dev_ab.py [--cfg cfg2,cfg4k] [--iters 20] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r14/grow_dev_ab.json

Per shape, n images of `used` bytes (24 + content, no metadata) without any
room, a need of one byte each, realloc_size 32768, page 4096, align 16: every
image grows by one realloc_size.  Event times on one stream, warm, image
buffers (images + arena) rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round.  The arrays a grow call rewrites (offsets,
capacities, the arena's top) are restored before the first event of every call.

  a    the whole grow call                     header, scan, place, planner, append_copy, commit
  a2   the same again                          the A/A spread (noise)
  az   the whole call with CIOA_GROW_ZERO      + planner, grow_zero
  b    what a caller does today, with a        INTEGRATION.md's relocate recipe: a placed CIOA_READ_IMAGE
       library of the PARENT commit            cio_file_read_batch_dev of --parent-lib into slots computed on
                                               the host (the same slots, the same buffer); the statuses are NOT
                                               read back, so the host round trip of the recipe is not in it.
                                               Skipped (and recorded so) without --parent-lib.
  c    the bookkeeping kernels alone           cioa_debug_grow_events section 2: grow_headers, grow_scan,
                                               grow_place
  d    grow_zero alone                         section 4 (its planner untimed)
  dm   one contiguous hipMemsetAsync           of the same byte count, over the arena
  e1   the need kernels, distinct images       section 1 of the records variant: grow_clear + grow_need, one
                                               record per image
  e2   the need kernels, one image             all records to image 0: the contended atomic
  f    a batch in which no image grows         the same images with 64 bytes of room each: the fixed cost
                                               every guarded append pays

a - b is what the device-side decision costs over the same copy kernel.
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

REALLOC, PAGE, ALIGN, ROOM = 32768, 4096, 16, 64
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
    lib.cioa_debug_grow_events.restype = I
    lib.cioa_debug_grow_events.argtypes = [V, V, U64, V, V, S, V, V, V, S, V, U64, U64, U64, I, V, V, V, I, V, V]
    hip = ctypes.CDLL(os.path.join(os.path.dirname(torch.__file__), "lib", "libamdhip64.so"))
    hip.hipMemsetAsync.restype, hip.hipMemsetAsync.argtypes = I, [V, I, S, V]
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.cio_dev_writer_create.restype, parent.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        parent.cio_dev_writer_destroy.restype, parent.cio_dev_writer_destroy.argtypes = None, [V]
        parent.cio_file_read_batch_dev.restype = I
        parent.cio_file_read_batch_dev.argtypes = [V, V, U64, V, V, S, I, V, V, U64, V, V, I, V, V, V]
        parent.cio_gpu_last_error.restype = ctypes.c_char_p
        parent.cio_gpu_version.restype = ctypes.c_char_p
        assert not hasattr(parent, "cio_file_grow_batch_dev"), "--parent-lib already has the grow call"
    if not torch.cuda.is_available():
        raise SystemExit("grow_dev_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters,
                    "rounds": args.rounds, "version": lib.cio_gpu_version().decode(),
                    "parent_version": parent.cio_gpu_version().decode() if parent else None,
                    "realloc_size": REALLOC, "page": PAGE, "align": ALIGN})
    for cfg in args.cfg.split(","):
        n, used = SHAPES[cfg]
        stride = used + ROOM                                   # leg f claims the room, the others do not
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride)
        caps = np.full(n, used, np.uint64)
        new_cap = (used + REALLOC + PAGE - 1) // PAGE * PAGE
        top = (n * stride + 4095) // 4096 * 4096
        slots = np.uint64(top) + np.arange(n, dtype=np.uint64) * np.uint64(new_cap)
        end = top + n * new_cap
        nbytes = end
        payload, tail = n * used, n * (new_cap - used)
        nrot = 2
        hdr = np.zeros((n, 24), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = np.full(n, used - 24, np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
        hdr_t = torch.from_numpy(hdr).to(dev)
        hdr_idx = (i64(offs)[:, None] + torch.arange(24, device=dev)[None, :]).reshape(-1)
        bufs = []
        for b in range(nrot):
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            t[:top] = torch.arange(top, device=dev, dtype=torch.int32).mul_(37 + b).to(torch.uint8)
            t[hdr_idx] = hdr_t.reshape(-1)
            bufs.append(t)
        del hdr_idx
        offs0, caps0, capsf0, arena0 = i64(offs), i64(caps), i64(caps + np.uint64(ROOM)), i64([top, end])
        offs_t, caps_t, arena_t = offs0.clone(), caps0.clone(), arena0.clone()
        need_t, slots_t, slotcaps_t = i64(np.ones(n, np.uint64)), i64(slots), i64(np.full(n, new_cap, np.uint64))
        rec_distinct = torch.arange(n, dtype=torch.int32, device=dev)
        rec_one = torch.zeros(n, dtype=torch.int32, device=dev)
        writer = cf.DevWriter(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        ln = torch.zeros(n, dtype=torch.int64, device=dev)
        pw = V()
        if parent:
            assert parent.cio_dev_writer_create(ctypes.byref(pw), n) == 0, parent.cio_gpu_last_error()

        def restore(room=False):
            offs_t.copy_(offs0)
            caps_t.copy_(capsf0 if room else caps0)
            arena_t.copy_(arena0)

        def hook(k, section, ev, need, rec, flags):
            _lib.check(lib.cioa_debug_grow_events(
                writer._handle, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n,
                need.data_ptr() if need is not None else None, rec.data_ptr() if rec is not None else None,
                need_t.data_ptr() if rec is not None else None, n if rec is not None else 0, arena_t.data_ptr(),
                REALLOC, PAGE, ALIGN, flags, total.data_ptr(), status.data_ptr(), stream, section, ev[0], ev[1]),
                "grow section")

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            restore(room=name == "f")
            if name == "c":
                return hook(k, 2, ev, need_t, None, 0)
            if name == "d":
                return hook(k, 4, ev, need_t, None, cf.CIOA_GROW_ZERO)
            if name in ("e1", "e2"):
                return hook(k, 1, ev, None, rec_distinct if name == "e1" else rec_one, 0)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name in ("a", "a2", "az", "f"):
                cf.grow_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, arena_t, realloc=REALLOC, page=PAGE,
                                  align=ALIGN, flags=cf.CIOA_GROW_ZERO if name == "az" else 0, total=total,
                                  status=status)
            elif name == "b":
                rc = parent.cio_file_read_batch_dev(
                    pw, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n, cf.CIOA_READ_IMAGE, None,
                    bufs[k].data_ptr(), nbytes, slots_t.data_ptr(), slotcaps_t.data_ptr(), 0, ln.data_ptr(),
                    status.data_ptr(), stream)
                assert rc == 0, parent.cio_gpu_last_error()
            elif name == "dm":
                assert hip.hipMemsetAsync(bufs[k].data_ptr() + top, 0, tail, stream) == 0
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "b", "az", "c", "d", "dm", "e1", "e2", "f", "a2"]
        if not parent:
            order.remove("b")
        # correctness at the timed size
        for k in range(nrot):
            for name in order:
                bufs[k][top:].fill_(0x5A)
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                if name != "dm":
                    assert not status.cpu().numpy().any(), f"{cfg}: leg {name}: an entry was refused"
                grew = name in ("a", "a2", "az", "c", "d", "e1")
                if name not in ("b", "dm", "e2"):
                    assert torch.equal(offs_t, slots_t if grew else offs0), f"{cfg}: leg {name}: offsets"
                    assert int(arena_t.cpu()[0]) == (end if grew else top), f"{cfg}: leg {name}: top"
                if name in ("a", "az", "b"):
                    for i in (0, n // 3, n - 1):
                        s, d = int(offs[i]), int(slots[i])
                        assert torch.equal(bufs[k][d:d + used], bufs[k][s:s + used]), f"{cfg}: leg {name}: image {i}"
                        tail_i = bufs[k][d + used:d + new_cap]
                        assert bool((tail_i == (0 if name == "az" else 0x5A)).all()), f"{cfg}: leg {name}: tail {i}"
        info = {"n": n, "used_bytes": used, "new_cap": new_cap, "payload_bytes": payload, "tail_bytes": tail,
                "buffer_bytes": nbytes, "rotating_buffers": nrot, "copy_workgroups": cus * 8}

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
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["b_measured"] = bool(parent)
        info["a_over_b"] = round(med["a"] / med["b"], 3) if parent else None
        info["a_minus_b_us"] = round(med["a"] - med["b"], 2) if parent else None
        info["az_minus_a_us"] = round(med["az"] - med["a"], 2)
        info["d_over_dm"] = round(med["d"] / med["dm"], 3)
        info["copy_payload_GBps_in_a"] = round(payload / med["a"] / 1e3, 1)
        info["zero_GBps"] = {"d": round(tail / med["d"] / 1e3, 1), "dm": round(tail / med["dm"] / 1e3, 1)}
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
