#!/usr/bin/env python3
"""Chunk images in HBM down to chunk files and up again
(cio_file_load_paths_dev, cio_file_store_paths_dev) against what the same
bytes cost without the placement and the copy, in one process
(profiles/r21/persist_ab.json).

    python tools/persist_ab.py [--dir /dev/shm] [--shapes cfg2,cfg4k] [--stage-mb 64] [--rounds 3] \\
        --out profiles/r21/persist_ab.json

Per shape n images of cfg2's or cfg4k's content length (n scaled down to a
quarter of what --dir has free, and to --max-files) are built on the device
(init, append, seal) and stored once, untimed: those are the files.  The legs
run interleaved, ABBA inside each round, wall clock around the call (both calls
are host-synchronous):

  load     cio_file_load_paths_dev of the files into a fresh arena (the arena's
           top is reset, untimed, before every call)
  verify   cio_verify_paths over the same files with every batch on the GPU
           route: the same pread -> pinned -> H2D path without the placement
           and the copy.  Run FIVE times per round: the spread of its medians
           is the run-to-run spread the load is held against
  store    cio_file_store_paths_dev of the images, untrimmed, over the files
  bare     one D2H of the same used bytes into a pinned tensor, then the same
           writes from Python on 16 threads (os.pwrite + os.ftruncate)

Not isolated: the file system's page cache (the directory is memory-backed:
every read is a copy from memory); the Python overhead of the bare leg's
writes against the C threads of the store.

Where a load and a store spend their time comes from the library's own marks
(cioa_debug_persist_timing, the last call of each kind): per call the rounds,
the seconds in the file threads, the event milliseconds of the rounds'
transfers and of their device chains (verify, allocation, copy, adopt; the
packed read), the seconds the host waited for the stream, and the seconds
before the first round.  They are the `parts` of the two legs.
"""
import argparse
import ctypes
import json
import os
import shutil
import sys
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--dir", default="/dev/shm")
    ap.add_argument("--shapes", default="cfg2,cfg4k")
    ap.add_argument("--stage-mb", type=int, default=64)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--max-files", type=int, default=20480)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import chunkfile as cf
    from chunkio_amd import workloads as wl

    import resource
    soft, hard = resource.getrlimit(resource.RLIMIT_NOFILE)
    want = 65536 if hard == resource.RLIM_INFINITY else min(hard, 65536)
    if soft < want:
        resource.setrlimit(resource.RLIMIT_NOFILE, (want, hard))
    vbatch = max(64, resource.getrlimit(resource.RLIMIT_NOFILE)[0] - 256)
    dev = torch.device("cuda:0")
    results = {"stage_bytes": args.stage_mb << 20, "dir": args.dir, "verify_batch": vbatch}
    for shape in args.shapes.split(","):
        length, n = {"cfg2": (wl.CFG2_LEN, wl.CFG2_N), "cfg4k": (wl.CFG4K_LEN, wl.CFG4K_N)}[shape]
        cap = (24 + length + 4095) & ~4095
        free = shutil.disk_usage(args.dir).free
        n = max(1, min(n, args.max_files, free // 4 // cap))
        root = os.path.join(args.dir, f"persist_ab_{os.getpid()}_{shape}")
        os.makedirs(root)
        try:
            paths = [os.path.join(root, f"c{i:06d}") for i in range(n)]
            offs = torch.arange(n, dtype=torch.int64, device=dev) * cap
            caps = torch.full((n,), cap, dtype=torch.int64, device=dev)
            base = torch.zeros(n * cap + 4096, dtype=torch.uint8, device=dev)
            src = torch.randint(1, 255, (length + 16,), dtype=torch.uint8, device=dev)
            stage = torch.zeros(args.stage_mb << 20, dtype=torch.uint8, device=dev)
            used = 24 + length
            with cio.DevWriter(n) as w:
                st, crc = cf.init_batch_dev(w, base, offs, caps)
                cf.write_batch_dev(w, base, offs, caps, src, torch.zeros(n, dtype=torch.int64, device=dev),
                                   torch.full((n,), length, dtype=torch.int64, device=dev), crc)
                cf.seal_batch_dev(w, base, offs, caps, crc)
                sst, fs, _ = cf.store_paths_dev(w, base, offs, caps, paths, stage)
                assert not sst.any() and int(fs.sum()) == n * cap
                into = torch.zeros(n * cap + 4096, dtype=torch.uint8, device=dev)
                arena = torch.tensor([0, n * cap], dtype=torch.int64, device=dev)
                pinned = torch.empty(n * used, dtype=torch.uint8).pin_memory()
                packed = torch.zeros(n * used, dtype=torch.uint8, device=dev)
                pst = cf.read_packed_batch_dev(w, base, offs, caps, cf.CIOA_READ_IMAGE, packed)[0]
                assert not pst.cpu().numpy().any()        # the bare leg writes the same bytes the store writes
                cio.route(reset=True, cpu_max=0)

                def parts(which):
                    out = (ctypes.c_double * 6)()
                    fn = cio.lib().cioa_debug_persist_timing
                    fn.argtypes = [ctypes.c_int, ctypes.POINTER(ctypes.c_double), ctypes.c_int]
                    fn(which, out, 6)
                    return dict(zip(("rounds", "files_s", "copy_ms", "chain_ms", "wait_s", "before_s"),
                                    (round(float(x), 5) for x in out)))

                def leg_load():
                    arena[0] = 0
                    torch.cuda.synchronize()
                    t = time.perf_counter()
                    out = cf.load_paths_dev(w, into, paths, stage, arena, flags=cf.CIO_CHECKSUM)
                    dt = time.perf_counter() - t
                    assert not out[0].any()
                    return dt

                def leg_verify():             # it holds every file of a batch open: batches below the limit
                    t = time.perf_counter()
                    bad = []
                    for i in range(0, n, vbatch):
                        vst, ver, _ = cf.verify_paths(paths[i:i + vbatch], cf.CIO_CHECKSUM)
                        bad += [(i + int(k), int(vst[k]), int(ver[k])) for k in np.flatnonzero(vst)]
                    dt = time.perf_counter() - t
                    assert not bad, bad[:8]
                    return dt

                def leg_store():
                    t = time.perf_counter()
                    s2, _, _ = cf.store_paths_dev(w, base, offs, caps, paths, stage)
                    dt = time.perf_counter() - t
                    assert not s2.any()
                    return dt

                def write_one(i):
                    fd = os.open(paths[i], os.O_WRONLY | os.O_CREAT | os.O_TRUNC, 0o644)
                    os.pwrite(fd, memoryview(host)[i * used:(i + 1) * used], 0)
                    os.ftruncate(fd, cap)
                    os.close(fd)

                def leg_bare():
                    t = time.perf_counter()
                    pinned.copy_(packed, non_blocking=True)
                    torch.cuda.synchronize()
                    list(pool.map(write_one, range(n)))
                    return time.perf_counter() - t

                host = pinned.numpy()
                legs = {"load": leg_load, "verify": leg_verify, "store": leg_store, "bare": leg_bare}
                times = {k: [] for k in legs}
                with ThreadPoolExecutor(16) as pool:
                    for k in legs:                # untimed: pinned staging, device scratch, the page cache
                        legs[k]()
                    for r in range(args.rounds):
                        order = ["load"] + ["verify"] * 5 + ["store", "bare"]
                        for k in (order if r % 2 == 0 else order[::-1]):
                            times[k].append(legs[k]())
                    load_parts, store_parts = parts(0), parts(1)
                cio.route(reset=True)
            file_bytes, used_bytes = n * cap, n * used
            res = {"n": n, "file_bytes": file_bytes, "used_bytes": used_bytes,
                   "rounds_of_stage": int(cf.persist_rounds([cap] * n, args.stage_mb << 20)[0])}
            for k, ts in times.items():
                size = used_bytes if k in ("store", "bare") else file_bytes
                res[k] = {"s": [round(x, 5) for x in ts], "median_s": round(float(np.median(ts)), 5),
                          "GBps": round(size / float(np.median(ts)) / 1e9, 2)}
            res["load"]["parts"], res["store"]["parts"] = load_parts, store_parts
            v = np.asarray(times["verify"]).reshape(args.rounds, 5)
            res["verify"]["spread_of_round_medians_s"] = [round(float(np.median(x)), 5) for x in v]
            results[shape] = res
            print(shape, json.dumps(res), flush=True)
        finally:
            shutil.rmtree(root, ignore_errors=True)
    line = json.dumps(results)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
