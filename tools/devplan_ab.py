#!/usr/bin/env python3
"""Device-planned CRC-32 against host plans, in one process (profiles/r07/).

    python tools/devplan_ab.py [--cfg cfg2,cfg4k,cfg3x8192] [--iters 20] [--rounds 4] --out profiles/r07/devplan_ab.json

Per geometry, HIP-event times (warm, batches rotating past the 256 MB Infinity
Cache, the variants alternating ABBA inside each round):

  a   host plan, shipped kernel selection          CRC kernel (cio_crc32_plan_exec_events)
  b   host plan, general stream kernel on one      the same; CIO_GPU_DIAG=1 CIO_GPU_UNIFORM=0
      workgroup per CU                             CIO_GPU_AHEAD=0 CIO_GPU_SMALL=0 CIO_GPU_ANTICAMP=0
                                                   CIO_GPU_GRID=<CUs> at plan creation
  b2  a second plan made exactly like b            the A/A spread (noise)
  c   device plan (cio_crc32_devplan_exec)         end to end, and split: planner kernels / CRC kernel
  d   cio_crc32_plan_create                        host wall time (median of --creates)

The CRC kernel of c runs the code of b over the same plan image, so c_crc
should equal b within the b/b2 spread; a - b is what giving up the host-only
selections costs; d / c_planner is what the device planner saves.
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k,cfg3x8192")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--creates", type=int, default=5)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import workloads as wl

    lib = cio.lib()
    V = ctypes.c_void_p
    lib.cioa_debug_devplan_exec_events.restype = ctypes.c_int
    lib.cioa_debug_devplan_exec_events.argtypes = [V, V, ctypes.c_uint64, V, V, ctypes.c_size_t, V, V, V, V, V]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    general_env = {"CIO_GPU_DIAG": "1", "CIO_GPU_UNIFORM": "0", "CIO_GPU_AHEAD": "0", "CIO_GPU_SMALL": "0",
                   "CIO_GPU_ANTICAMP": "0", "CIO_GPU_GRID": str(cus)}

    def host_plan(offs, lens, env):
        saved = {k: os.environ.get(k) for k in env}
        os.environ.update(env)
        try:
            return cio.Crc32Plan(offs, lens)
        finally:
            for k, v in saved.items():
                if v is None:
                    os.environ.pop(k, None)
                else:
                    os.environ[k] = v

    def new_events(n):
        evs = [lib.cio_gpu_event_create() for _ in range(n)]
        assert all(evs)
        return evs

    def ms(a, b):
        return float(lib.cio_gpu_event_elapsed_ms(a, b))

    results = {"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters, "rounds": args.rounds,
               "version": lib.cio_gpu_version().decode(), "geometries": {}}
    for cfg in args.cfg.split(","):
        lens = {"cfg2": wl.cfg2_lens, "cfg4k": lambda: np.full(wl.CFG4K_N, wl.CFG4K_LEN, np.uint64),
                "cfg3x8192": lambda: wl.cfg3_lens(8192)}[cfg]()
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        offs = np.ascontiguousarray(wl.packed_offsets(lens, align=16), dtype=np.uint64)
        n, total = len(lens), int(wl.batch_bytes(offs, lens))
        nrot = max(2, min(4, int(1.2e9 // max(total, 1)) + 1))
        bufs = []
        for b in range(nrot):
            t = torch.empty(total + 64, dtype=torch.uint8, device=dev)
            cio.fill_synthetic(t, offs, lens, 0xD0D0 + b)
            bufs.append(t)
        offs_t = torch.from_numpy(offs.view(np.int64)).to(dev)
        lens_t = torch.from_numpy(lens.view(np.int64)).to(dev)

        # d: host wall time of plan creation (default selection), plans destroyed at once
        creates = []
        for _ in range(args.creates):
            t0 = time.perf_counter()
            p = cio.Crc32Plan(offs, lens)
            creates.append((time.perf_counter() - t0) * 1e6)
            p.close()

        plans = {"a": host_plan(offs, lens, {}), "b": host_plan(offs, lens, general_env),
                 "b2": host_plan(offs, lens, general_env), "c": cio.Crc32DevPlan(n)}
        outs = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in plans}

        def launch(k, buf, evs=None):
            if k == "c":
                if evs is None:
                    plans[k].exec(buf, offs_t, lens_t, outs[k])
                else:
                    _lib.check(lib.cioa_debug_devplan_exec_events(plans[k]._handle, buf.data_ptr(), buf.numel(),
                                                                  offs_t.data_ptr(), lens_t.data_ptr(), n,
                                                                  outs[k].data_ptr(), stream, *evs), "devplan events")
            elif evs is None:
                plans[k].exec(buf, outs[k])
            else:
                plans[k].exec_events(buf, outs[k], evs[0], evs[2])

        for k in plans:
            launch(k, bufs[0])
        torch.cuda.synchronize()
        ref = outs["a"].cpu().numpy()
        for k in plans:
            assert np.array_equal(outs[k].cpu().numpy(), ref), f"{cfg}: variant {k} differs"
        assert plans["c"].status() == 0
        info = {"n": n, "bytes": total, "rotating_buffers": nrot,
                "a_kernel": plans["a"].kernel_name(), "a_workgroups": plans["a"].workgroups,
                "b_kernel": plans["b"].kernel_name(), "b_workgroups": plans["b"].workgroups,
                "c_workgroups": plans["c"].workgroups}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                launch("a", bufs[k % nrot])
            torch.cuda.synchronize()
        evs = {k: [new_events(3) for _ in range(args.iters)] for k in plans}
        per_round = {k: [] for k in ("a", "b", "b2", "c_total", "c_planner", "c_crc")}
        order = ["a", "b", "c", "b2"]
        for r in range(args.rounds):
            for k in (order if r % 2 == 0 else order[::-1]):
                for i in range(3):
                    launch(k, bufs[i % nrot])
                for i in range(args.iters):
                    launch(k, bufs[i % nrot], evs[k][i])
                torch.cuda.synchronize()
                if k == "c":
                    per_round["c_total"].append(np.mean([ms(e[0], e[2]) for e in evs[k]]) * 1e3)
                    per_round["c_planner"].append(np.mean([ms(e[0], e[1]) for e in evs[k]]) * 1e3)
                    per_round["c_crc"].append(np.mean([ms(e[1], e[2]) for e in evs[k]]) * 1e3)
                else:
                    per_round[k].append(np.mean([ms(e[0], e[2]) for e in evs[k]]) * 1e3)
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        info["us"] = {k: round(v, 2) for k, v in med.items()}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["d_plan_create_host_us"] = round(float(np.median(creates)), 1)
        info["GBps"] = {k: round(total / med[k] / 1e3, 1) for k in ("a", "b", "c_crc", "c_total")}
        info["noise_b_vs_b2_pct"] = round(100.0 * abs(med["b2"] - med["b"]) / med["b"], 2)
        info["c_crc_vs_b_pct"] = round(100.0 * (med["c_crc"] - med["b"]) / med["b"], 2)
        info["b_vs_a_pct"] = round(100.0 * (med["b"] - med["a"]) / med["a"], 2)
        info["c_total_vs_a_pct"] = round(100.0 * (med["c_total"] - med["a"]) / med["a"], 2)
        info["host_create_over_planner"] = round(info["d_plan_create_host_us"] / med["c_planner"], 1)
        results["geometries"][cfg] = info
        print(cfg, json.dumps(info), flush=True)
        for k in evs:
            for e3 in evs[k]:
                for e in e3:
                    lib.cio_gpu_event_destroy(e)
        for p in plans.values():
            p.close()
        del bufs, plans, outs
        torch.cuda.empty_cache()
    text = json.dumps(results, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
