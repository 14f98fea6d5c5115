#!/usr/bin/env python3
"""The grouped append (cio_file_write_records_batch_dev) against what a caller
does without it, in one process (profiles/r12/write_records_ab.json).

    python tools/write_records_ab.py [--shape 1024x100x4096,1024x10x40960] [--iters 10] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r12/write_records_ab.json

A shape IxRxL is I images taking R records of L bytes each.  Event times on one
stream, warm, image and source buffers rotating past the 256 MB Infinity
Cache, the legs alternating ABBA inside each round, medians over the rounds.
Before every timed call the content lengths of the images are put back to 0
(untimed, ahead of the first event), so every call appends to empty images.

  a    the one grouped call, CIO_CHECKSUM       image, record, scan, place kernels; planner + copy over the I R
                                                records; planner + CRC over the I appended ranges; finish
  a2   the same again                           the A/A spread (noise)
  a0   the one grouped call, flags = 0          no CRC planner, no CRC launch
  b    R calls of cio_file_write_batch_dev of   --parent-lib, a build of the commit before the grouped append:
       n = I, round k the k-th record of every  what a caller does today.  The R calls are issued back to back
       image, CIO_CHECKSUM                      from Python between the two events; the host-side regrouping of
                                                the records into rounds is done once, ahead, and NOT timed.
                                                Skipped (and recorded so) without --parent-lib.
  b0   the same, flags = 0
  c    ONE cio_file_write_batch_dev of all I R  the floor for the copy + per-record CRC: every record its own
       records into I R distinct images         image of 24 + L bytes (DESIGN.md §14's row for L = 4096)
  c0   the same, flags = 0
  d    the four bookkeeping kernels alone       cioa_debug_write_records_book_events
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
    ap.add_argument("--shape", default="1024x100x4096,1024x10x40960")
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="libchunkio_amd.so built from the parent commit (legs b, b0)")
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    V, U64, S, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    lib.cioa_debug_write_records_book_events.restype = I
    lib.cioa_debug_write_records_book_events.argtypes = [V, V, U64, V, V, S, U64, V, V, V, S, V, V, V, V, V]
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.cio_file_write_batch_dev.restype = I
        parent.cio_file_write_batch_dev.argtypes = [V, V, U64, V, V, S, V, U64, V, V, I, V, V, V]
        parent.cio_dev_writer_create.restype, parent.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        parent.cio_dev_writer_destroy.restype, parent.cio_dev_writer_destroy.argtypes = None, [V]
        parent.cio_gpu_last_error.restype = ctypes.c_char_p
        parent.cio_gpu_version.restype = ctypes.c_char_p
        assert not hasattr(parent, "cio_file_write_records_batch_dev"), "--parent-lib has the grouped append"
    if not torch.cuda.is_available():
        raise SystemExit("write_records_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    CK = cf.CIO_CHECKSUM

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "rounds": args.rounds,
                    "version": lib.cio_gpu_version().decode(),
                    "parent_version": parent.cio_gpu_version().decode() if parent else None})
    for shape in args.shape.split(","):
        n_img, per, length = (int(x) for x in shape.split("x"))
        n_rec, payload = n_img * per, n_img * per * length
        # grouped: image i holds its `per` records; distinct (leg c): one image per record
        g_cap, c_cap = 24 + per * length + 40, 24 + length
        g_offs = np.arange(n_img, dtype=np.uint64) * np.uint64(g_cap)
        c_offs = np.arange(n_rec, dtype=np.uint64) * np.uint64(c_cap)
        g_bytes, c_bytes = n_img * g_cap, n_rec * c_cap
        rec_offs = np.arange(n_rec, dtype=np.uint64) * np.uint64(length + 3) + np.uint64(5)   # every alignment
        src_bytes = int(rec_offs[-1]) + length + 16
        rec_img = np.repeat(np.arange(n_img, dtype=np.uint32), per)
        nrot = max(2, min(3, int(1.2e9 // max(payload, 1)) + 1))

        def images(n, offs, total):
            t = torch.zeros(total, dtype=torch.uint8, device=dev)
            t[i64(offs)] = 0xC1
            return t

        gimg = [images(n_img, g_offs, g_bytes) for _ in range(nrot)]
        cimg = [images(n_rec, c_offs, c_bytes) for _ in range(nrot)]
        srcs = [torch.randint(0, 256, (src_bytes,), dtype=torch.uint8, device=dev) for _ in range(nrot)]
        g_len_idx = (i64(g_offs)[:, None] + torch.arange(10, 14, device=dev)[None, :]).reshape(-1)
        c_len_idx = (i64(c_offs)[:, None] + torch.arange(10, 14, device=dev)[None, :]).reshape(-1)
        g_offs_t, g_caps_t = i64(g_offs), i64(np.full(n_img, g_cap, np.uint64))
        c_offs_t, c_caps_t = i64(c_offs), i64(np.full(n_rec, c_cap, np.uint64))
        rec_img_t = torch.from_numpy(rec_img.view(np.int32)).to(dev)
        rec_offs_t, rec_lens_t = i64(rec_offs), i64(np.full(n_rec, length, np.uint64))
        # leg b's rounds, regrouped ahead: row k = the k-th record of every image
        rounds_t = i64(rec_offs.reshape(n_img, per).T.copy())
        round_lens_t = i64(np.full(n_img, length, np.uint64))
        writer = cf.DevWriter(n_rec)
        g_crc = torch.zeros(n_img, dtype=torch.int32, device=dev)
        c_crc = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        ist = torch.zeros(n_img, dtype=torch.int32, device=dev)
        rst = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        pw = V()
        if parent:
            assert parent.cio_dev_writer_create(ctypes.byref(pw), n_img) == 0, parent.cio_gpu_last_error()

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            if name in ("c", "c0"):
                cimg[k][c_len_idx] = 0
            else:
                gimg[k][g_len_idx] = 0
            if name == "d":
                _lib.check(lib.cioa_debug_write_records_book_events(
                    writer._handle, gimg[k].data_ptr(), g_bytes, g_offs_t.data_ptr(), g_caps_t.data_ptr(), n_img,
                    src_bytes, rec_img_t.data_ptr(), rec_offs_t.data_ptr(), rec_lens_t.data_ptr(), n_rec,
                    ist.data_ptr(), rst.data_ptr(), stream, ev[0], ev[1]), "bookkeeping kernels")
                return
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name in ("a", "a2", "a0"):
                cf.write_records_batch_dev(writer, gimg[k], g_offs_t, g_caps_t, srcs[k], rec_img_t, rec_offs_t,
                                           rec_lens_t, g_crc, flags=0 if name == "a0" else CK, img_status=ist,
                                           rec_status=rst)
            elif name in ("b", "b0"):
                for r in range(per):
                    rc = parent.cio_file_write_batch_dev(
                        pw, gimg[k].data_ptr(), g_bytes, g_offs_t.data_ptr(), g_caps_t.data_ptr(), n_img,
                        srcs[k].data_ptr(), src_bytes, rounds_t[r].data_ptr(), round_lens_t.data_ptr(),
                        0 if name == "b0" else CK, g_crc.data_ptr(), ist.data_ptr(), stream)
                    assert rc == 0, parent.cio_gpu_last_error()
            else:
                cf.write_batch_dev(writer, cimg[k], c_offs_t, c_caps_t, srcs[k], rec_offs_t, rec_lens_t, c_crc,
                                   flags=0 if name == "c0" else CK, status=rst)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        def accepted(name):
            bad = int(rst.count_nonzero()) if name not in ("b", "b0") else 0
            assert bad == 0 and int(ist.count_nonzero()) == 0, f"{shape}: {name}: an entry was refused"

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "b", "a0", "b0", "c", "c0", "d", "a2"] if parent else ["a", "a0", "c", "c0", "d", "a2"]
        # correctness at the timed size: the records land back to back, the lengths follow
        want_len = torch.tensor(list((per * length).to_bytes(4, "big")), dtype=torch.uint8, device=dev)
        for k in range(nrot):
            for name in order:
                if name in ("c", "c0", "d"):
                    continue
                ist.fill_(7)
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                accepted(name)
                for i in (0, n_img // 3, n_img - 1):
                    o = int(g_offs[i])
                    assert torch.equal(gimg[k][o + 10:o + 14], want_len), f"{shape}: leg {name}: image {i} length"
                    for j in (0, per // 2, per - 1):
                        s, d = int(rec_offs[i * per + j]), o + 24 + j * length
                        assert torch.equal(gimg[k][d:d + length], srcs[k][s:s + length]), \
                            f"{shape}: leg {name}: record {j} of image {i} differs"
        info = {"images": n_img, "records_per_image": per, "record_bytes": length, "records": n_rec,
                "payload_bytes": payload, "rotating_buffers": nrot}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(4):
                leg("a", k % nrot, evs[0])
            torch.cuda.synchronize()
        per_round = {k: [] for k in order}
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                for i in range(2):
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
        info["payload_GBps"] = {k: round(payload / med[k] / 1e3, 1) for k in order if k != "d"}
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["b_measured"] = bool(parent)
        info["a_over_b"] = round(med["a"] / med["b"], 4) if parent else None
        info["a0_over_b0"] = round(med["a0"] / med["b0"], 4) if parent else None
        info["a_over_c"] = round(med["a"] / med["c"], 4)
        info["a0_over_c0"] = round(med["a0"] / med["c0"], 4)
        info["d_share_of_a_pct"] = round(100.0 * med["d"] / med["a"], 2)
        results["shapes"][shape] = info
        print(shape, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        if parent:
            parent.cio_dev_writer_destroy(pw)
        del gimg, cimg, srcs
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
