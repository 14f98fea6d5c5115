#!/usr/bin/env python3
"""The device-side append (cio_file_write_batch_dev) against its ceiling, in one
process (profiles/r08/).

    python tools/write_dev_ab.py [--cfg cfg2,cfg4k,cfg3x8192] [--iters 20] [--rounds 4] --out profiles/r08/write_dev_ab.json

Per shape, one append of every record into an EMPTY image of exactly its size
(images packed back to back, so the destination alignment follows from the
lengths; sources packed with 0..15 byte gaps).  Event times on one stream, warm,
source and image buffers rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round:

  a   the append copy kernel alone                 cioa_debug_write_dev_copy_events: the header kernel
                                                   and the planner untimed, then the copy kernel
                                                   between the two events
  a2  the same again                               the A/A spread (noise)
  b   ONE contiguous device-to-device copy of      Tensor.copy_ between uint8 tensors of one device
      the same total bytes                         (hipMemcpyAsync): the ceiling of a
  c   a whole write_batch_dev with CIO_CHECKSUM    header kernel, planner, copy, CRC, finish
  c0  the same without CIO_CHECKSUM                no CRC launch
  d   planner + CRC alone                          cio_crc32_devplan_exec over the source records
  e   the host route, cfg2                         an existing figure, for context (not measured here)

The images are re-initialised (init_batch_dev, outside the timed events) before
every timed a / a2 / c / c0, and the statuses are checked after every round.  Rates are payload bytes (sum of the record lengths) over
time: a copy reads and writes each of them once.

c - a - d is the launch chain's own cost (header and finish kernels, gaps);
that plus the CRC's second read of the source is what a fused copy+CRC kernel
could recover.
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

# (e) the host-memory route for the same bytes (cioa_chunk_write /
# cio_file_sync_batch: pinned staging + H2D + CRC), for context only and not
# measured here: README.md, "the PCIe link (<= 57 GB/s) bounds the GPU path".
HOST_ROUTE = {"source": "README.md: data in host memory is bounded by the PCIe link", "GBps_upper_bound": 57.0,
              "measured_here": False}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k,cfg3x8192")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--aligned", action="store_true",
                    help="lay sources out congruent to their destinations modulo 16 (every source load is then "
                         "aligned as well): what the unaligned source loads cost leg a")
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf
    from chunkio_amd import workloads as wl

    lib = cio.lib()
    V = ctypes.c_void_p
    U64 = ctypes.c_uint64
    lib.cioa_debug_write_dev_copy_events.restype = ctypes.c_int
    lib.cioa_debug_write_dev_copy_events.argtypes = [V, V, U64, V, V, ctypes.c_size_t, V, U64, V, V, V, V, V, V]
    if not torch.cuda.is_available():
        raise SystemExit("write_dev_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters, "rounds": args.rounds,
               "version": lib.cio_gpu_version().decode(), "aligned_sources": bool(args.aligned), "shapes": {}}
    results["e_host_route_cfg2"] = HOST_ROUTE
    for cfg in args.cfg.split(","):
        lens = {"cfg2": wl.cfg2_lens, "cfg4k": lambda: np.full(wl.CFG4K_N, wl.CFG4K_LEN, np.uint64),
                "cfg3x8192": lambda: wl.cfg3_lens(8192)}[cfg]()
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n, payload = len(lens), int(lens.sum())
        caps = lens + np.uint64(24)
        img_offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
        gaps = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(16)
        src_offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]]).astype(np.uint64) + gaps
        if args.aligned:                      # the same 0..15 byte gaps, chosen to match the destination
            want = (img_offs + np.uint64(24)) % np.uint64(16)
            pos, src_offs = 0, np.zeros(n, np.uint64)
            for i in range(n):
                pos += (int(want[i]) - pos) % 16
                src_offs[i] = pos
                pos += int(lens[i])
        src_bytes = int(src_offs[-1] + lens[-1])
        img_bytes = int(caps.sum())
        nrot = max(2, min(4, int(1.2e9 // max(payload, 1)) + 1))
        srcs, imgs = [], []
        offs_t, lens_t = i64(src_offs), i64(lens)
        for b in range(nrot):
            t = torch.empty(src_bytes + 64, dtype=torch.uint8, device=dev)
            cio.fill_synthetic(t, src_offs, lens, 0xE0E0 + b)
            srcs.append(t)
            imgs.append(torch.zeros(img_bytes, dtype=torch.uint8, device=dev))
        flat = [torch.empty(payload, dtype=torch.uint8, device=dev) for _ in range(nrot)]     # leg b's target
        img_offs_t, caps_t = i64(img_offs), i64(caps)
        writer, plan = cf.DevWriter(n), cio.Crc32DevPlan(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        crc_cur = torch.zeros(n, dtype=torch.int32, device=dev)
        crc_out = torch.zeros(n, dtype=torch.int32, device=dev)

        def init(k):
            cf.init_batch_dev(writer, imgs[k], img_offs_t, caps_t, crc_cur=crc_cur, status=status)

        def leg(name, k, ev):
            """Queue leg `name` over buffer pair k, between the events ev[0] and ev[1]."""
            if name in ("a", "a2"):
                init(k)
                _lib.check(lib.cioa_debug_write_dev_copy_events(
                    writer._handle, imgs[k].data_ptr(), imgs[k].numel(), img_offs_t.data_ptr(), caps_t.data_ptr(), n,
                    srcs[k].data_ptr(), srcs[k].numel(), offs_t.data_ptr(), lens_t.data_ptr(), status.data_ptr(),
                    stream, ev[0], ev[1]), "copy kernel")
                return
            if name in ("c", "c0"):
                init(k)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name == "b":
                flat[k].copy_(srcs[k][:payload])
            elif name in ("c", "c0"):
                cf.write_batch_dev(writer, imgs[k], img_offs_t, caps_t, srcs[k], offs_t, lens_t, crc_cur,
                                   flags=cf.CIO_CHECKSUM if name == "c" else 0, status=status)
            else:
                plan.exec(srcs[k], offs_t, lens_t, crc_out)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        # correctness at the timed size: every record lands, seals and verifies
        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        for k in range(nrot):
            leg("c", k, evs[0])
            assert not status.cpu().numpy().any(), f"{cfg}: write refused"
            cf.seal_batch_dev(writer, imgs[k], img_offs_t, caps_t, crc_cur, status=status)
            st = cf.verify_batch_dev(plan, imgs[k], img_offs_t, caps_t)[0]
            assert not st.cpu().numpy().any(), f"{cfg}: a sealed image does not verify"
            for i in (0, n // 3, n - 1):
                o, s, ln = int(img_offs[i]) + 24, int(src_offs[i]), int(lens[i])
                assert torch.equal(imgs[k][o:o + ln], srcs[k][s:s + ln]), f"{cfg}: record {i} differs"
        info = {"n": n, "payload_bytes": payload, "rotating_buffers": nrot, "copy_workgroups": cus * 8,
                "crc_workgroups": plan.workgroups}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                leg("a", k % nrot, evs[0])
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any(), f"{cfg}: write refused while warming"
        order = ["a", "b", "c", "d", "c0", "a2"]
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
                if name != "b" and name != "d":
                    assert not status.cpu().numpy().any(), f"{cfg}: write refused in the timed loop"
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        info["us"] = {k: round(v, 2) for k, v in med.items()}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["payload_GBps"] = {k: round(payload / med[k] / 1e3, 1) for k in order}
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["a_over_b"] = round(med["a"] / med["b"], 3)
        info["c_minus_a_minus_d_us"] = round(med["c"] - med["a"] - med["d"], 2)
        info["c0_minus_a_us"] = round(med["c0"] - med["a"], 2)
        results["shapes"][cfg] = info
        print(cfg, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        plan.close()
        del srcs, imgs, flat
        torch.cuda.empty_cache()
    text = json.dumps(results, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
