#!/usr/bin/env python3
"""The in-place move of cio_file_write_metadata_batch_dev against the
non-overlapping copy of the same bytes, in one process (profiles/r09/).

    python tools/write_dev_move_ab.py [--cfg cfg2,cfg4k,cfg3x8192] [--shifts 57,-57,65535] [--iters 20] [--rounds 4] --out profiles/r09/write_dev_move_ab.json

Per shape and shift d, every image holds `old` bytes of metadata and one record
of content and fits the larger layout exactly (images packed back to back);
the new metadata is old + d bytes long (d = +57: 8 -> 65, a tag replaced by a
longer one; d = -57: 65 -> 8; d = +65535: 0 -> 65535).  Event times on one
stream, warm, image buffers rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round:

  a   move_save + move_shift alone            cioa_debug_write_dev_move_events: the header kernel and
                                              the planner untimed, then the two kernels between the
                                              events; bytes 22..23 are not written, so every call
                                              finds the same shift
  a2  the same again                          the A/A spread (noise)
  b   append_copy of the same content bytes   cioa_debug_write_dev_copy_events from the image buffer
      into a second buffer                    into empty images: the non-overlapping copy the move
                                              is measured against (DESIGN.md §14's leg a)
  c   a whole write_metadata_batch_dev        header kernel, planner, move, planner, metadata copy,
      with CIO_CHECKSUM                       planner, CRC, finish
  c0  the same without CIO_CHECKSUM           no third planner run, no CRC launch

Before every timed a / a2 / c / c0 bytes 22..23 of every image are put back to
`old` (outside the timed events), so the call moves again.  The statuses are checked
after every round.  Rates are payload bytes (the content moved) over time: the
move reads and writes each of them once, like the copy.
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
    ap.add_argument("--shifts", default="57,-57,65535")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
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
    lib.cioa_debug_write_dev_move_events.restype = ctypes.c_int
    lib.cioa_debug_write_dev_move_events.argtypes = [V, V, U64, V, V, ctypes.c_size_t, U64, V, V, V, V, V, V]
    if not torch.cuda.is_available():
        raise SystemExit("write_dev_move_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters, "rounds": args.rounds,
               "version": lib.cio_gpu_version().decode(), "shapes": {}}
    meta_pool = torch.from_numpy(np.random.default_rng(1).integers(0, 256, 65536, dtype=np.uint8)).to(dev)
    for cfg in args.cfg.split(","):
        lens = {"cfg2": wl.cfg2_lens, "cfg4k": lambda: np.full(wl.CFG4K_N, wl.CFG4K_LEN, np.uint64),
                "cfg3x8192": lambda: wl.cfg3_lens(8192)}[cfg]()
        lens = np.ascontiguousarray(lens, dtype=np.uint64)
        n, payload = len(lens), int(lens.sum())
        gaps = (np.arange(n, dtype=np.uint64) * np.uint64(7)) % np.uint64(16)
        src_offs = np.concatenate([[0], np.cumsum(lens + gaps)[:-1]]).astype(np.uint64) + gaps
        src = torch.empty(int(src_offs[-1] + lens[-1]) + 64, dtype=torch.uint8, device=dev)
        cio.fill_synthetic(src, src_offs, lens, 0xA0A0)
        src_offs_t, lens_t = i64(src_offs), i64(lens)
        nrot = max(2, min(4, int(1.2e9 // max(payload, 1)) + 1))
        results["shapes"][cfg] = {}
        for d in [int(x) for x in args.shifts.split(",")]:
            old = 8 if 0 < d < 60000 else (0 if d > 0 else 8 - d)
            new = old + d
            assert 0 <= new <= 65535 and 0 <= old <= 65535
            caps = lens + np.uint64(24 + max(old, new))
            img_offs = np.concatenate([[0], np.cumsum(caps)[:-1]]).astype(np.uint64)
            img_bytes = int(caps.sum())
            dcaps = lens + np.uint64(24)                              # leg b's empty images
            dst_offs = np.concatenate([[0], np.cumsum(dcaps)[:-1]]).astype(np.uint64)
            img_offs_t, caps_t, dst_offs_t, dcaps_t = i64(img_offs), i64(caps), i64(dst_offs), i64(dcaps)
            content_offs_t = i64(img_offs + np.uint64(24 + old))
            zeros_t = i64(np.zeros(n, np.uint64))
            old_t, new_t = i64(np.full(n, old, np.uint64)), i64(np.full(n, new, np.uint64))
            writer, writer_b, plan = cf.DevWriter(n, move=True), cf.DevWriter(n), cio.Crc32DevPlan(n)
            status = torch.zeros(n, dtype=torch.int32, device=dev)
            crc_cur = torch.zeros(n, dtype=torch.int32, device=dev)
            crc_b = torch.zeros(n, dtype=torch.int32, device=dev)
            imgs, dsts = [], []
            for b in range(nrot):
                img = torch.zeros(img_bytes, dtype=torch.uint8, device=dev)
                cf.init_batch_dev(writer, img, img_offs_t, caps_t, meta_pool, zeros_t, old_t, crc_cur=crc_cur,
                                  status=status)
                cf.write_batch_dev(writer, img, img_offs_t, caps_t, src, src_offs_t, lens_t, crc_cur, status=status)
                assert not status.cpu().numpy().any(), f"{cfg}: set-up refused"
                imgs.append(img)
                dsts.append(torch.zeros(int(dcaps.sum()), dtype=torch.uint8, device=dev))
            # bytes 22..23 of every image, to put `old` back before a timed whole call
            hdr_idx = torch.from_numpy(np.concatenate([img_offs + np.uint64(22), img_offs + np.uint64(23)])
                                       .astype(np.int64)).to(dev)
            hdr_val = torch.cat([torch.full((n,), old >> 8, dtype=torch.uint8, device=dev),
                                 torch.full((n,), old & 255, dtype=torch.uint8, device=dev)])

            def leg(name, k, ev):
                """Queue leg `name` over buffer k, between the events ev[0] and ev[1]."""
                if name != "b":               # a whole call before left `new` there
                    imgs[k].index_copy_(0, hdr_idx, hdr_val)
                if name in ("a", "a2"):
                    _lib.check(lib.cioa_debug_write_dev_move_events(
                        writer._handle, imgs[k].data_ptr(), imgs[k].numel(), img_offs_t.data_ptr(), caps_t.data_ptr(),
                        n, meta_pool.numel(), zeros_t.data_ptr(), new_t.data_ptr(), status.data_ptr(), stream,
                        ev[0], ev[1]), "move kernels")
                elif name == "b":
                    cf.init_batch_dev(writer_b, dsts[k], dst_offs_t, dcaps_t, crc_cur=crc_b, status=status)
                    _lib.check(lib.cioa_debug_write_dev_copy_events(
                        writer_b._handle, dsts[k].data_ptr(), dsts[k].numel(), dst_offs_t.data_ptr(),
                        dcaps_t.data_ptr(), n, imgs[k].data_ptr(), imgs[k].numel(), content_offs_t.data_ptr(),
                        lens_t.data_ptr(), status.data_ptr(), stream, ev[0], ev[1]), "copy kernel")
                else:
                    _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
                    cf.write_metadata_batch_dev(writer, imgs[k], img_offs_t, caps_t, meta_pool, zeros_t, new_t,
                                                crc_cur, flags=cf.CIO_CHECKSUM if name == "c" else 0, status=status)
                    _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

            evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
            assert all(a and b for a, b in evs)
            # correctness at the timed size: the content lands at its new place, the image seals and verifies
            leg("c", 0, evs[0])
            assert not status.cpu().numpy().any(), f"{cfg}: write_metadata refused"
            cf.seal_batch_dev(writer, imgs[0], img_offs_t, caps_t, crc_cur, status=status)
            st = cf.verify_batch_dev(plan, imgs[0], img_offs_t, caps_t)[0]
            assert not st.cpu().numpy().any(), f"{cfg}: a sealed image does not verify"
            for i in (0, n // 3, n - 1):
                o, s, ln = int(img_offs[i]) + 24 + new, int(src_offs[i]), int(lens[i])
                assert torch.equal(imgs[0][o:o + ln], src[s:s + ln]), f"{cfg}, d = {d}: content {i} differs"
                assert torch.equal(imgs[0][o - new:o], meta_pool[:new]), f"{cfg}, d = {d}: metadata {i} differs"
            info = {"n": n, "payload_bytes": payload, "old": old, "new": new, "rotating_buffers": nrot,
                    "move_segments": writer.move_segments, "copy_workgroups": cus * 8}

            t_end = time.perf_counter() + args.warm_s       # warm clocks before any timed round
            while time.perf_counter() < t_end:
                for k in range(8):
                    leg("a", k % nrot, evs[0])
                torch.cuda.synchronize()
            order = ["a", "b", "c", "c0", "a2"]
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
                    assert not status.cpu().numpy().any(), f"{cfg}: a call was refused in the timed loop"
            med = {k: float(np.median(v)) for k, v in per_round.items()}
            ratios = [a / b for a, b in zip(per_round["a"], per_round["b"])]
            info["us"] = {k: round(v, 2) for k, v in med.items()}
            info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
            info["payload_GBps"] = {k: round(payload / med[k] / 1e3, 1) for k in order}
            info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
            info["a_over_b"] = round(med["a"] / med["b"], 3)
            info["a_over_b_per_round"] = [round(x, 3) for x in ratios]
            info["c_minus_a_us"] = round(med["c"] - med["a"], 2)
            info["c0_minus_a_us"] = round(med["c0"] - med["a"], 2)
            results["shapes"][cfg][str(d)] = info
            print(cfg, d, json.dumps(info), flush=True)
            for e0, e1 in evs:
                lib.cio_gpu_event_destroy(e0)
                lib.cio_gpu_event_destroy(e1)
            writer.close()
            writer_b.close()
            plan.close()
            del imgs, dsts
            torch.cuda.empty_cache()
        del src
    text = json.dumps(results, indent=1)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
