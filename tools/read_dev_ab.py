#!/usr/bin/env python3
"""The device read path (cio_file_read_packed_batch_dev / cio_file_read_batch_dev)
against the write path's copy of the same records, in one process
(profiles/r10/read_dev_ab.json).

    python tools/read_dev_ab.py [--cfg cfg2,cfg4k,cfg3x8192] [--iters 20] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r10/read_dev_ab.json

Per shape, images of exactly 24 + len bytes (no metadata) packed back to back,
so the content's alignment follows from the lengths, and a CIOA_READ_CONTENT
read of all of them, packed with align 1.  Event times on one stream, warm,
image and output buffers rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round:

  a   the packed read's copy kernel alone      cioa_debug_read_dev_copy_events: header, placement and
                                               planner kernels untimed, append_copy between the events
  a2  the same again                           the A/A spread (noise)
  b   append_copy of the same records by the   cioa_debug_write_dev_copy_events of --parent-lib (a build of the
      write path of the PARENT commit          commit before the read path; without CIO_CHECKSUM there is no
                                               CRC): the records are the content regions of the same image
                                               buffer, appended to empty images laid out so that every
                                               destination has the residue modulo 16 it has in leg a.
                                               Skipped (and recorded so) without --parent-lib.
  c   a whole packed read                      header, scan, place, planner, copy
  c0  a whole placed read, the same slots      header, planner, copy

c - c0 is what the device placement costs (two more launches and the scan).
d2h_at_pcie_us is ARITHMETIC, not a measurement: the capacity-sized slots of
the same images over the README's PCIe rate (<= 57 GB/s), what draining them
through host memory would take at best.
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

PCIE_GBPS = 57.0                              # README.md: "the PCIe link (<= 57 GB/s) bounds the GPU path"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k,cfg3x8192")
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
    from chunkio_amd import workloads as wl

    lib = cio.lib()
    V, U64, S, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    lib.cioa_debug_read_dev_copy_events.restype = I
    lib.cioa_debug_read_dev_copy_events.argtypes = [V, V, U64, V, V, S, I, V, U64, U64, I, V, V, V, V, V, V, V]
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.cioa_debug_write_dev_copy_events.restype = I
        parent.cioa_debug_write_dev_copy_events.argtypes = [V, V, U64, V, V, S, V, U64, V, V, V, V, V, V]
        parent.cio_dev_writer_create.restype, parent.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        parent.cio_dev_writer_destroy.restype, parent.cio_dev_writer_destroy.argtypes = None, [V]
        parent.cio_file_init_batch_dev.restype = I
        parent.cio_file_init_batch_dev.argtypes = [V, V, U64, V, V, S, V, U64, V, V, I, V, V, V]
        parent.cio_gpu_last_error.restype = ctypes.c_char_p
        parent.cio_gpu_version.restype = ctypes.c_char_p
    if not torch.cuda.is_available():
        raise SystemExit("read_dev_ab.py needs a GPU")
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
                    "pcie_GBps_for_the_arithmetic": PCIE_GBPS})
    for cfg in args.cfg.split(","):
        lens = {"cfg2": wl.cfg2_lens, "cfg4k": lambda: np.full(wl.CFG4K_N, wl.CFG4K_LEN, np.uint64),
                "cfg3x8192": lambda: wl.cfg3_lens(8192)}[cfg]()
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n, payload = len(lens), int(lens.sum())
        caps = lens + np.uint64(24)
        img_offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
        img_bytes = int(caps.sum())
        packed = np.concatenate([[0], np.cumsum(lens)[:-1]]).astype(np.uint64)     # leg a's destinations
        # leg b's images: image i where its append lands at the residue modulo 16 of packed[i]
        b_offs, pos = np.zeros(n, np.uint64), 0
        for i in range(n):
            pos += (int(packed[i]) - (pos + 24)) % 16
            b_offs[i] = pos
            pos += int(caps[i])
        b_bytes = pos
        nrot = max(2, min(4, int(1.2e9 // max(payload, 1)) + 1))
        hdr = np.zeros((n, 24), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = lens.astype(">u4").view(np.uint8).reshape(n, 4)
        hdr_t = torch.from_numpy(hdr).to(dev)
        hdr_idx = (i64(img_offs)[:, None] + torch.arange(24, device=dev)[None, :])
        imgs, outs, bdst = [], [], []
        for b in range(nrot):
            t = torch.empty(img_bytes, dtype=torch.uint8, device=dev)
            cio.fill_synthetic(t, img_offs + np.uint64(24), lens, 0xE0E0 + b)
            t[hdr_idx.reshape(-1)] = hdr_t.reshape(-1)
            imgs.append(t)
            outs.append(torch.zeros(payload, dtype=torch.uint8, device=dev))
            if parent:
                bdst.append(torch.zeros(b_bytes, dtype=torch.uint8, device=dev))
        del hdr_idx
        img_offs_t, caps_t = i64(img_offs), i64(caps)
        slots_t, lens_t = i64(packed), i64(lens)
        src_offs_t = i64(img_offs + np.uint64(24))
        b_offs_t = i64(b_offs)
        writer = cf.DevWriter(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        po = torch.zeros(n, dtype=torch.int64, device=dev)
        ln = torch.zeros(n, dtype=torch.int64, device=dev)
        total = torch.zeros(1, dtype=torch.int64, device=dev)
        pw = V()
        if parent:
            assert parent.cio_dev_writer_create(ctypes.byref(pw), n) == 0, parent.cio_gpu_last_error()
            crc = torch.zeros(n, dtype=torch.int32, device=dev)
            for k in range(nrot):
                assert parent.cio_file_init_batch_dev(pw, bdst[k].data_ptr(), b_bytes, b_offs_t.data_ptr(),
                                                      caps_t.data_ptr(), n, None, 0, None, None, 0, crc.data_ptr(),
                                                      status.data_ptr(), stream) == 0, parent.cio_gpu_last_error()
            torch.cuda.synchronize()
            assert not status.cpu().numpy().any(), f"{cfg}: parent init refused"

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            if name in ("a", "a2"):
                _lib.check(lib.cioa_debug_read_dev_copy_events(
                    writer._handle, imgs[k].data_ptr(), img_bytes, img_offs_t.data_ptr(), caps_t.data_ptr(), n,
                    cf.CIOA_READ_CONTENT, outs[k].data_ptr(), payload, 1, 0, po.data_ptr(), ln.data_ptr(),
                    total.data_ptr(), status.data_ptr(), stream, ev[0], ev[1]), "read copy kernel")
                return
            if name == "b":
                rc = parent.cioa_debug_write_dev_copy_events(
                    pw, bdst[k].data_ptr(), b_bytes, b_offs_t.data_ptr(), caps_t.data_ptr(), n, imgs[k].data_ptr(),
                    img_bytes, src_offs_t.data_ptr(), lens_t.data_ptr(), status.data_ptr(), stream, ev[0], ev[1])
                assert rc == 0, parent.cio_gpu_last_error()
                return
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name == "c":
                cf.read_packed_batch_dev(writer, imgs[k], img_offs_t, caps_t, cf.CIOA_READ_CONTENT, outs[k],
                                         out_offs=po, out_lens=ln, total=total, status=status)
            else:
                cf.read_batch_dev(writer, imgs[k], img_offs_t, caps_t, cf.CIOA_READ_CONTENT, outs[k], slots_t,
                                  lens_t, out_lens=ln, status=status)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        def accepted(what):
            assert not status.cpu().numpy().any(), f"{cfg}: {what}: an entry was refused"

        # correctness at the timed size: every record lands where the host would have put it
        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "b", "c", "c0", "a2"] if parent else ["a", "c", "c0", "a2"]
        for k in range(nrot):
            for name in order:
                outs[k].zero_()
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                accepted(name)
                for i in (0, n // 3, n - 1):
                    s, ll = int(img_offs[i]) + 24, int(lens[i])
                    if name == "b":
                        d, where = int(b_offs[i]) + 24, bdst[k]
                    else:
                        d, where = int(packed[i]), outs[k]
                    assert torch.equal(where[d:d + ll], imgs[k][s:s + ll]), f"{cfg}: leg {name}: record {i} differs"
                if name in ("a", "c", "a2"):
                    assert int(total.cpu()[0]) == payload and np.array_equal(po.cpu().numpy().view(np.uint64), packed)
        info = {"n": n, "payload_bytes": payload, "slot_bytes": img_bytes, "rotating_buffers": nrot,
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
                accepted(f"timed {name}")
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        info["us"] = {k: round(v, 2) for k, v in med.items()}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["payload_GBps"] = {k: round(payload / med[k] / 1e3, 1) for k in order}
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["a_over_b"] = round(med["a"] / med["b"], 3) if parent else None
        info["b_measured"] = bool(parent)
        info["c_minus_c0_us"] = round(med["c"] - med["c0"], 2)
        info["c_minus_a_us"] = round(med["c"] - med["a"], 2)
        info["d2h_at_pcie_us"] = {"arithmetic_not_measured": True,
                                  "slots": round(img_bytes / PCIE_GBPS / 1e3, 1),
                                  "c_over_it": round(med["c"] / (img_bytes / PCIE_GBPS / 1e3), 4)}
        results["shapes"][cfg] = info
        print(cfg, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        if parent:
            parent.cio_dev_writer_destroy(pw)
        del imgs, outs, bdst
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
