#!/usr/bin/env python3
"""Recycling drained chunk slots (cio_file_release_batch_dev,
cio_file_rotate_pool_batch_dev) in one process (profiles/r17/pool_dev_ab.json).

    python tools/pool_dev_ab.py [--cfg cfg2,cfg4k] [--iters 10] [--rounds 3] \\
        --out profiles/r17/pool_dev_ab.json

Per shape, n images of `used` bytes (24 + 32 bytes of metadata + content)
without any room -- they are the drained chunks of the release legs and the
full images of the rotate legs --, an arena of n slots behind them and n free
slots of the same size behind the arena.  Event times on one stream, warm,
image buffers rotating, the legs alternating ABBA inside each round.  What a
call rewrites -- the magic or the whole header of a released slot, the list,
the counts, the pool's words, offsets, capacities, crc_cur, the arena's top --
is restored, untimed, before the first event of every call.  Every leg runs
twice (x and x2): |x2 - x| is its A/A spread.

  r     release without flags                 every entry is pushed and bytes 0..1 of its slot zeroed
  rc    release with CIOA_RELEASE_COMPACT     the same, and the (now empty) list compacted
  rz    release with CIOA_RELEASE_ZERO        the same as r, and every slot zeroed by the byte-balanced fill
  ms    one hipMemsetAsync over n * used      contiguous bytes, the floor of rz's fill
  pp    rotate_pool, every slot from the pool n pool entries: no arena slot is taken
  pe    rotate_pool with an empty pool        F = 0: every slot from the arena
  pr    cio_file_rotate_batch_dev             the same library, the same images: pe's reference

Not isolated: the release's bookkeeping kernels from its commit; the fill's
planner from the fill (rz - r holds both); a pool or list that cuts the batch;
gates and live offsets (NULL here); the records variant; align other than 16.
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

ALIGN, META = 16, 32
SHAPES = {"cfg2": (1024, 409600), "cfg4k": (102400, 4096)}     # n, used bytes
LEGS = ["r", "rc", "rz", "ms", "pp", "pe", "pr"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    if not torch.cuda.is_available():
        raise SystemExit("pool_dev_ab.py needs a GPU")
    with open("/proc/self/maps") as f:                  # the HIP runtime this process already runs on
        loaded = sorted({ln.split()[-1] for ln in f if "libamdhip64" in ln})
    hip = ctypes.CDLL(loaded[0] if loaded else "libamdhip64.so")
    hip.hipMemsetAsync.restype = ctypes.c_int
    hip.hipMemsetAsync.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_size_t, ctypes.c_void_p]
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
                    "rounds": args.rounds, "version": lib.cio_gpu_version().decode(), "align": ALIGN,
                    "meta_bytes": META})
    for cfg in args.cfg.split(","):
        n, used = SHAPES[cfg]
        offs = np.arange(n, dtype=np.uint64) * np.uint64(used)
        caps = np.full(n, used, np.uint64)
        new_cap = used                                         # a multiple of ALIGN: slot = new_cap
        top = n * used
        end = top + n * new_cap
        arena_slots = np.uint64(top) + np.arange(n, dtype=np.uint64) * np.uint64(new_cap)
        free_slots = np.uint64(end) + np.arange(n, dtype=np.uint64) * np.uint64(new_cap)
        nbytes = end + n * new_cap
        nrot = 2
        hdr = np.zeros((n, 24 + META), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = np.full(n, used - 24 - META, np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
        hdr[:, 23] = META
        hdr[:, 24:] = (np.arange(n * META, dtype=np.uint64) * 7 % 251 + 1).astype(np.uint8).reshape(n, META)
        hdr_t = torch.from_numpy(hdr).to(dev).reshape(-1)
        hdr_idx = (i64(offs)[:, None] + torch.arange(24 + META, device=dev)[None, :]).reshape(-1)
        bufs = []
        for b in range(nrot):
            t = torch.empty(nbytes, dtype=torch.uint8, device=dev)
            t[:top] = torch.arange(top, device=dev, dtype=torch.int32).mul_(37 + b).to(torch.uint8)
            t[hdr_idx] = hdr_t
            bufs.append(t)
        offs0, caps0, arena0 = i64(offs), i64(caps), i64([top, end])
        crc0 = torch.arange(n, dtype=torch.int32, device=dev)
        img0 = torch.arange(n, dtype=torch.int32, device=dev)
        count0, full0 = i64([0, n]), i64([n, n])
        pool_full, pool_empty = i64([n, n, new_cap, ALIGN]), i64([0, n, new_cap, ALIGN])
        free_t, freecaps_t = i64(free_slots), i64(np.full(n, new_cap, np.uint64))
        offs_t, caps_t, arena_t, crc_t = offs0.clone(), caps0.clone(), arena0.clone(), crc0.clone()
        count_t, pool_t = count0.clone(), pool_empty.clone()
        po_t, pc_t = free_t.clone(), freecaps_t.clone()
        lo_t, lc_t, li_t = offs0.clone(), caps0.clone(), img0.clone()
        need_t = i64(np.ones(n, np.uint64))
        writer = cf.DevWriter(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(2, dtype=torch.int64, device=dev)

        def restore(name, k):
            if name != "ms":
                bufs[k][hdr_idx] = hdr_t                   # a release took the magic or the slot, a rotate sealed
            if name in ("r", "rc", "rz"):
                lo_t.copy_(offs0)
                lc_t.copy_(caps0)
                li_t.copy_(img0)
                count_t.copy_(full0)
                pool_t.copy_(pool_empty)
            elif name != "ms":
                offs_t.copy_(offs0)
                caps_t.copy_(caps0)
                arena_t.copy_(arena0)
                crc_t.copy_(crc0)
                count_t.copy_(count0)
                pool_t.copy_(pool_full if name == "pp" else pool_empty)
                po_t.copy_(free_t)
                pc_t.copy_(freecaps_t)

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            name = name.rstrip("2")
            restore(name, k)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name in ("r", "rc", "rz"):
                flags = {"r": 0, "rc": cf.CIOA_RELEASE_COMPACT, "rz": cf.CIOA_RELEASE_ZERO}[name]
                cf.release_batch_dev(writer, bufs[k], lo_t, lc_t, po_t, pc_t, pool_t, img=li_t, count=count_t,
                                     flags=flags, total=total, status=status)
            elif name == "ms":
                assert hip.hipMemsetAsync(bufs[k].data_ptr() + end, 0, n * used, stream) == 0    # the free slots
            elif name in ("pp", "pe"):
                cf.rotate_pool_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, limit=0, new_cap=new_cap,
                                         align=ALIGN, arena=arena_t, pool_offs=po_t, pool_caps=pc_t, pool=pool_t,
                                         out_offs=lo_t, out_caps=lc_t, out_img=li_t, out_count=count_t, flags=CK,
                                         crc_cur=crc_t, total=total, status=status)
            else:
                cf.rotate_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, limit=0, new_cap=new_cap, align=ALIGN,
                                    arena=arena_t, out_offs=lo_t, out_caps=lc_t, out_img=li_t, out_count=count_t,
                                    flags=CK, crc_cur=crc_t, total=total, status=status)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = LEGS + [x + "2" for x in LEGS]
        # correctness at the timed size
        for k in range(nrot):
            for name in LEGS:
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                if name == "ms":
                    continue
                assert not status.cpu().numpy().any(), f"{cfg}: leg {name}: an entry was refused"
                if name in ("r", "rc", "rz"):
                    assert pool_t.cpu().tolist() == [n, n, new_cap, ALIGN] and total.cpu().tolist() == [n, 0], (cfg, name)
                    assert torch.equal(po_t, offs0) and torch.equal(pc_t, caps0), (cfg, name)
                    assert count_t.cpu().tolist() == [0 if name == "rc" else n, n], (cfg, name)
                    for i in (0, n // 3, n - 1):
                        got = bufs[k][int(offs[i]):int(offs[i]) + used].cpu().numpy()
                        assert not got[:2].any() and (got[2:].any() != (name == "rz")), (cfg, name, i)
                    if name == "rc":
                        assert not lo_t.cpu().numpy().any() and (li_t.cpu().numpy() == -1).all(), (cfg, name)
                else:
                    want = free_t.flip(0) if name == "pp" else i64(arena_slots)
                    assert torch.equal(offs_t, want) and torch.equal(lo_t, offs0), f"{cfg}: leg {name}: offsets"
                    assert count_t.cpu().tolist() == [n, n], (cfg, name)
                    assert arena_t.cpu().tolist() == ([top, end] if name == "pp" else [end, end]), (cfg, name)
                    assert total.cpu().tolist() == [0 if name == "pp" else n * new_cap, n], (cfg, name)
                    assert int(pool_t[0]) == 0, (cfg, name)
            bufs[k][hdr_idx] = hdr_t
        info = {"n": n, "used_bytes": used, "new_cap": new_cap, "buffer_bytes": nbytes, "rotating_buffers": nrot,
                "copy_workgroups": cus * 8}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                leg("pe", k % nrot, evs[0])
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
        info["us"] = {k: round(med[k], 2) for k in LEGS}
        info["us_second_run"] = {k: round(med[k + "2"], 2) for k in LEGS}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["aa_spread_us"] = {k: round(abs(med[k + "2"] - med[k]), 2) for k in LEGS}
        info["rz_GBps"] = round(n * used / med["rz"] / 1e3, 1)
        info["ms_GBps"] = round(n * used / med["ms"] / 1e3, 1)
        info["rz_minus_r_over_ms"] = round((med["rz"] - med["r"]) / med["ms"], 3)
        info["pe_minus_pr_us"] = round(med["pe"] - med["pr"], 2)
        info["pe_slower_than_three_spreads_of_pr"] = bool(med["pe"] - med["pr"] > 3 * abs(med["pr2"] - med["pr"]))
        results["shapes"][cfg] = info
        print(cfg, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        del bufs, hdr_idx
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
