#!/usr/bin/env python3
"""The ungrouped append (cio_file_write_records_ungrouped_batch_dev) against the
grouped call on pre-sorted records and against what a caller does without it,
in one process (profiles/r13/write_records_ungrouped_ab.json).

    python tools/write_records_ungrouped_ab.py [--shape 1024x100x4096,1024x10x40960] [--iters 10] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r13/write_records_ungrouped_ab.json

A shape IxRxL is I images taking R records of L bytes each; the record list is
randomly permuted (one fixed permutation per shape).  Event times on one
stream, warm, image and source buffers rotating past the 256 MB Infinity
Cache, the legs alternating ABBA inside each round, medians over the rounds.
Before every timed call the content lengths of the images are put back to 0
(untimed, ahead of the first event), so every call appends to empty images.

  a    the one ungrouped call, CIO_CHECKSUM     sort (3 kernels a pass), gather, the grouped chain, unpermute
  a2   the same again                           the A/A spread (noise)
  b    cio_file_write_records_batch_dev of      --parent-lib, a build of the commit before the ungrouped append,
       the SAME records pre-sorted (stably,     on a writer of its own.  a - b is what ungrouped input costs.
       on the host, ahead, not timed)           Without --parent-lib this library's grouped call (recorded so).
  b2   the same again                           the A/A spread of b
  c    the sort, gather and unpermute kernels   cioa_debug_sort_records_events
       alone
  d    what a caller does today: torch.sort(    the sort's values are the grouped image indices; the two gathers
       stable=True), the gathers of the         of offsets and lengths and the status scatter are torch indexing
       offsets and lengths, leg b's grouped     kernels; torch's caching allocator serves the temporaries (warm)
       call, the status scatter
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
    ap.add_argument("--parent-lib", default=None, help="libchunkio_amd.so built from the parent commit (legs b, d)")
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    V, U64, S, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    lib.cioa_debug_sort_records_events.restype = I
    lib.cioa_debug_sort_records_events.argtypes = [V, S, V, V, V, S, V, V, V, V, V]
    glib = lib
    if args.parent_lib:
        glib = ctypes.CDLL(os.path.abspath(args.parent_lib))
        glib.cio_file_write_records_batch_dev.restype = I
        glib.cio_file_write_records_batch_dev.argtypes = [V, V, U64, V, V, S, V, U64, V, V, V, S, I, V, V, V, V]
        glib.cio_dev_writer_create.restype, glib.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        glib.cio_dev_writer_destroy.restype, glib.cio_dev_writer_destroy.argtypes = None, [V]
        glib.cio_gpu_last_error.restype = ctypes.c_char_p
        glib.cio_gpu_version.restype = ctypes.c_char_p
        assert not hasattr(glib, "cio_file_write_records_ungrouped_batch_dev"), "--parent-lib has the ungrouped append"
    if not torch.cuda.is_available():
        raise SystemExit("write_records_ungrouped_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    CK = cf.CIO_CHECKSUM

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    def i32(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "rounds": args.rounds,
                    "version": lib.cio_gpu_version().decode(),
                    "parent_version": glib.cio_gpu_version().decode() if args.parent_lib else None})
    for shape in args.shape.split(","):
        n_img, per, length = (int(x) for x in shape.split("x"))
        n_rec, payload = n_img * per, n_img * per * length
        cap = 24 + per * length + 40
        offs = np.arange(n_img, dtype=np.uint64) * np.uint64(cap)
        total = n_img * cap
        rng = np.random.default_rng(13)
        perm = rng.permutation(n_rec)
        p_img = np.repeat(np.arange(n_img, dtype=np.uint32), per)[perm]
        p_offs = (np.arange(n_rec, dtype=np.uint64) * np.uint64(length + 3) + np.uint64(5))[perm]   # every alignment
        src_bytes = int(p_offs.max()) + length + 16
        srt = np.argsort(p_img, kind="stable")
        nrot = max(2, min(3, int(1.2e9 // max(payload, 1)) + 1))

        def images():
            t = torch.zeros(total, dtype=torch.uint8, device=dev)
            t[i64(offs)] = 0xC1
            return t

        imgs = [images() for _ in range(nrot)]
        srcs = [torch.randint(0, 256, (src_bytes,), dtype=torch.uint8, device=dev) for _ in range(nrot)]
        len_idx = (i64(offs)[:, None] + torch.arange(10, 14, device=dev)[None, :]).reshape(-1)
        offs_t, caps_t = i64(offs), i64(np.full(n_img, cap, np.uint64))
        p_img_t, p_offs_t = i32(p_img), i64(p_offs)
        s_img_t, s_offs_t = i32(p_img[srt]), i64(p_offs[srt])
        lens_t = i64(np.full(n_rec, length, np.uint64))
        writer = cf.DevWriter(n_rec)
        crc = torch.zeros(n_img, dtype=torch.int32, device=dev)
        ist = torch.zeros(n_img, dtype=torch.int32, device=dev)
        rst = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        gst = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        gw = writer._handle if not args.parent_lib else V()
        if args.parent_lib:
            assert glib.cio_dev_writer_create(ctypes.byref(gw), n_rec) == 0, glib.cio_gpu_last_error()

        def grouped(k, img_t, o_t, l_t, st):
            rc = glib.cio_file_write_records_batch_dev(
                gw, imgs[k].data_ptr(), total, offs_t.data_ptr(), caps_t.data_ptr(), n_img, srcs[k].data_ptr(),
                src_bytes, img_t.data_ptr(), o_t.data_ptr(), l_t.data_ptr(), n_rec, CK, crc.data_ptr(),
                ist.data_ptr(), st.data_ptr(), stream)
            assert rc == 0, glib.cio_gpu_last_error()

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            imgs[k][len_idx] = 0
            if name == "c":
                _lib.check(lib.cioa_debug_sort_records_events(
                    writer._handle, n_img, p_img_t.data_ptr(), p_offs_t.data_ptr(), lens_t.data_ptr(), n_rec,
                    rst.data_ptr(), None, stream, ev[0], ev[1]), "sort kernels")
                return
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name in ("a", "a2"):
                cf.write_records_ungrouped_batch_dev(writer, imgs[k], offs_t, caps_t, srcs[k], p_img_t, p_offs_t,
                                                     lens_t, crc, flags=CK, img_status=ist, rec_status=rst)
            elif name in ("b", "b2"):
                grouped(k, s_img_t, s_offs_t, lens_t, rst)
            else:
                vals, idx = torch.sort(p_img_t, stable=True)
                grouped(k, vals, p_offs_t[idx], lens_t[idx], gst)
                rst[idx] = gst
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        def accepted(name):
            if name.endswith("c"):
                return
            assert int(rst.count_nonzero()) == 0 and int(ist.count_nonzero()) == 0, f"{shape}: {name}: refused"

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "b", "c", "d", "b2", "a2"]
        # correctness at the timed size: every leg leaves the images of leg b, byte for byte
        for k in range(nrot):
            want = None
            for name in ("b", "a", "d"):
                crc.zero_()
                ist.fill_(7)
                rst.fill_(7)
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                accepted(name)
                if want is None:
                    want = imgs[k].clone()
                    o = int(offs[n_img // 3])
                    assert int.from_bytes(bytes(want[o + 10:o + 14].tolist()), "big") == per * length
                else:
                    assert torch.equal(imgs[k], want), f"{shape}: leg {name} differs from the grouped call"
            del want
        info = {"images": n_img, "records_per_image": per, "record_bytes": length, "records": n_rec,
                "payload_bytes": payload, "rotating_buffers": nrot, "b_from_parent_lib": bool(args.parent_lib)}

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
        info["noise_a_vs_a2_pct"] = round(100.0 * abs(med["a2"] - med["a"]) / med["a"], 2)
        info["noise_b_vs_b2_pct"] = round(100.0 * abs(med["b2"] - med["b"]) / med["b"], 2)
        info["a_minus_b_us"] = round(med["a"] - med["b"], 2)
        info["a_over_b"] = round(med["a"] / med["b"], 4)
        info["c_us"] = round(med["c"], 2)
        info["a_minus_b_minus_c_us"] = round(med["a"] - med["b"] - med["c"], 2)
        info["d_minus_b_us"] = round(med["d"] - med["b"], 2)
        info["a_over_d"] = round(med["a"] / med["d"], 4)
        info["sort_passes"] = (max(n_img.bit_length(), 1) + 7) // 8
        results["shapes"][shape] = info
        print(shape, json.dumps(info), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        if args.parent_lib:
            glib.cio_dev_writer_destroy(gw)
        writer.close()
        del imgs, srcs
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps(results))


if __name__ == "__main__":
    main()
