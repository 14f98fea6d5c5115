#!/usr/bin/env python3
"""What a device-side transaction costs around a grouped append, in one
process (profiles/r16/tx_dev_ab.json).

    python tools/tx_dev_ab.py [--cfg cfg2,cfg4k] [--iters 20] [--rounds 4] \\
        [--parent-lib PATH] --out profiles/r16/tx_dev_ab.json

Per shape, n images that already hold one record of `rec` bytes behind 32
bytes of metadata and have room for exactly one more.  Event times on one
stream, warm, buffer sets rotating past the 256 MB Infinity Cache, the legs
alternating ABBA inside each round.  What a call rewrites (the image headers,
crc_cur, the transaction state) is restored before the first event of every
call.

  a    the grouped append alone, with a        cio_file_write_records_batch_dev, one record of `rec`
       library of the PARENT commit            bytes per image.  Skipped (and recorded so) without
                                               --parent-lib.
  an   the same with this library              the unit's device code is the parent's byte for byte
  b    begin -> append -> cond -> rollback     nothing fails: the rollback skips every image, the commit
       -> commit                               seals every image
  b2   the same again                          the A/A spread (noise)
  c    the same chain, every image failing     a second record per image that can never fit: the first is
                                               appended, the image fails, the rollback drops `rec` bytes,
                                               the commit skips every image
  d    as c with CIOA_TX_ZERO                  + the planner and the fill over n x rec bytes
  e    as c with CIOA_TX_RECOMPUTE             + the planner and the CRC over the n x rec bytes kept
  f1   the cond kernels alone, distinct images n failing records, one per image
  f2   the cond kernels alone, one image       n failing records, all to image 0

b - a is what the transaction costs a producer whose batches fit; c - b what
a rollback costs over a commit.
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

META = 32
SHAPES = {"cfg2": (1024, 409600), "cfg4k": (102400, 4096)}     # n, record bytes


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--cfg", default="cfg2,cfg4k")
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--parent-lib", default=None, help="libchunkio_amd.so built from the parent commit (leg a)")
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    V, U64, S, I = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int
    parent = None
    if args.parent_lib:
        parent = ctypes.CDLL(os.path.abspath(args.parent_lib))
        parent.cio_dev_writer_create.restype, parent.cio_dev_writer_create.argtypes = I, [ctypes.POINTER(V), S]
        parent.cio_dev_writer_destroy.restype, parent.cio_dev_writer_destroy.argtypes = None, [V]
        parent.cio_file_write_records_batch_dev.restype = I
        parent.cio_file_write_records_batch_dev.argtypes = [V, V, U64, V, V, S, V, U64, V, V, V, S, I, V, V, V, V]
        parent.cio_gpu_last_error.restype = ctypes.c_char_p
        parent.cio_gpu_version.restype = ctypes.c_char_p
        assert not hasattr(parent, "cio_file_tx_begin_batch_dev"), "--parent-lib already has the transaction calls"
    if not torch.cuda.is_available():
        raise SystemExit("tx_dev_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    cus = torch.cuda.get_device_properties(dev).multi_processor_count
    CK, ZERO, REC = cf.CIO_CHECKSUM, cf.CIOA_TX_ZERO, cf.CIOA_TX_RECOMPUTE

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "cus": cus, "iters": args.iters,
                    "rounds": args.rounds, "version": lib.cio_gpu_version().decode(),
                    "parent_version": parent.cio_gpu_version().decode() if parent else None, "meta_bytes": META})
    for cfg in args.cfg.split(","):
        n, rec = SHAPES[cfg]
        cap = 24 + META + 2 * rec
        stride = cap + 40                                      # images at a residue of 8 modulo 16
        offs = np.arange(n, dtype=np.uint64) * np.uint64(stride) + np.uint64(8)
        nbytes = int(n * stride + 64)
        nrot = 2
        hdr = np.zeros((n, 24 + META), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = np.full(n, rec, np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
        hdr[:, 23] = META
        hdr[:, 24:] = (np.arange(n * META, dtype=np.uint64) * 7 % 251 + 1).astype(np.uint8).reshape(n, META)
        hdr_t = torch.from_numpy(hdr).to(dev).reshape(-1)
        hdr_idx = (i64(offs)[:, None] + torch.arange(24 + META, device=dev)[None, :]).reshape(-1)
        bufs = []
        for b in range(nrot):
            t = torch.arange(nbytes, device=dev, dtype=torch.int32).mul_(37 + b).to(torch.uint8)
            t[hdr_idx] = hdr_t
            bufs.append(t)
        src = torch.arange(n * rec + 16, device=dev, dtype=torch.int32).mul_(41).to(torch.uint8)
        offs_t, caps_t = i64(offs), i64(np.full(n, cap, np.uint64))
        crc0 = torch.arange(n, dtype=torch.int32, device=dev)
        crc_t = crc0.clone()
        tx_t = cf.tx_state(n, dev)
        # one record per image; and the failing list: behind each a second one that can never fit
        img1 = torch.arange(n, dtype=torch.int32, device=dev)
        ro1, rl1 = i64(np.arange(n, dtype=np.uint64) * np.uint64(rec)), i64(np.full(n, rec, np.uint64))
        img2 = torch.arange(n, dtype=torch.int32, device=dev).repeat_interleave(2)
        ro2 = i64(np.repeat(np.arange(n, dtype=np.uint64) * np.uint64(rec), 2))
        rl2 = i64(np.tile(np.asarray([rec, rec + 1], np.uint64), n))
        rec_one = torch.zeros(n, dtype=torch.int32, device=dev)
        rec_fail = torch.full((n,), -1, dtype=torch.int32, device=dev)
        writer = cf.DevWriter(2 * n)
        bst, rb, cm, ist = (torch.zeros(n, dtype=torch.int32, device=dev) for _ in range(4))
        rst = torch.zeros(2 * n, dtype=torch.int32, device=dev)
        cond = torch.zeros(n, dtype=torch.int32, device=dev)
        pw = V()
        if parent:
            assert parent.cio_dev_writer_create(ctypes.byref(pw), n) == 0, parent.cio_gpu_last_error()

        def restore(k):
            bufs[k][hdr_idx] = hdr_t
            crc_t.copy_(crc0)
            tx_t.zero_()

        def chain(k, fail, flags):
            base = bufs[k]
            cf.tx_begin_batch_dev(writer, base, offs_t, caps_t, tx_t, crc_t, status=bst)
            if fail:
                cf.write_records_batch_dev(writer, base, offs_t, caps_t, src, img2, ro2, rl2, crc_t, flags=CK,
                                           img_status=ist, rec_status=rst)
                cf.tx_cond_records_batch_dev(img2, rst, n, img_status=ist, cond=cond)
            else:
                cf.write_records_batch_dev(writer, base, offs_t, caps_t, src, img1, ro1, rl1, crc_t, flags=CK,
                                           img_status=ist, rec_status=rst[:n])
                cf.tx_cond_records_batch_dev(img1, rst[:n], n, img_status=ist, cond=cond)
            cf.tx_rollback_batch_dev(writer, base, offs_t, caps_t, tx_t, crc_t, cond=cond, flags=flags, status=rb)
            cf.tx_commit_batch_dev(writer, base, offs_t, caps_t, tx_t, crc_t, cond=cond, status=cm)

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            restore(k)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name == "a":
                rc = parent.cio_file_write_records_batch_dev(
                    pw, bufs[k].data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n, src.data_ptr(),
                    src.numel(), img1.data_ptr(), ro1.data_ptr(), rl1.data_ptr(), n, CK, crc_t.data_ptr(),
                    ist.data_ptr(), rst.data_ptr(), stream)
                assert rc == 0, parent.cio_gpu_last_error()
            elif name == "an":
                cf.write_records_batch_dev(writer, bufs[k], offs_t, caps_t, src, img1, ro1, rl1, crc_t, flags=CK,
                                           img_status=ist, rec_status=rst[:n])
            elif name in ("b", "b2"):
                chain(k, False, CK)
            elif name in ("c", "d", "e"):
                chain(k, True, CK | {"c": 0, "d": ZERO, "e": REC}[name])
            elif name in ("f1", "f2"):
                cf.tx_cond_records_batch_dev(img1 if name == "f1" else rec_one, rec_fail, n, cond=cond)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = ["a", "an", "b", "c", "d", "e", "f1", "f2", "b2"]
        if not parent:
            order.remove("a")

        def lengths(k):
            return bufs[k][hdr_idx].reshape(n, 24 + META)[:, 10:14].cpu().numpy().copy().view(">u4").reshape(n)

        # correctness at the timed size
        for k in range(nrot):
            for name in order:
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                if name in ("a", "an", "b", "b2"):
                    assert not ist.cpu().numpy().any() and not rst[:n].cpu().numpy().any(), (cfg, name)
                    assert (lengths(k) == 2 * rec).all(), f"{cfg}: leg {name}: content lengths"
                if name in ("b", "b2"):
                    assert not cond.cpu().numpy().any() and not cm.cpu().numpy().any() and not rb.cpu().numpy().any()
                    assert not tx_t.cpu().numpy()[:, 0].any(), f"{cfg}: leg {name}: a transaction is still active"
                if name in ("c", "d", "e"):
                    assert (cond.cpu().numpy() == -1).all() and not rb.cpu().numpy().any(), (cfg, name)
                    assert (lengths(k) == rec).all(), f"{cfg}: leg {name}: content lengths after the rollback"
                    assert not tx_t.cpu().numpy()[:, 0].any(), f"{cfg}: leg {name}: a transaction is still active"
                    i = n // 3
                    a0 = int(offs[i]) + 24 + META + rec
                    tail = bufs[k][a0:a0 + rec].cpu().numpy()
                    assert tail.any() != (name == "d"), f"{cfg}: leg {name}: the dropped bytes"
                    if name != "e":
                        assert torch.equal(crc_t, crc0), f"{cfg}: leg {name}: crc_cur"
                if name == "f1":
                    assert (cond.cpu().numpy() == -1).all()
                if name == "f2":
                    assert cond.cpu().numpy().tolist() == [-1] + [0] * (n - 1)
        info = {"n": n, "record_bytes": rec, "image_capacity": cap, "buffer_bytes": nbytes, "rotating_buffers": nrot,
                "copy_workgroups": cus * 8}

        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                leg("b", k % nrot, evs[0])
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
        info["aa_spread_us"] = round(abs(med["b2"] - med["b"]), 2)
        info["noise_b_vs_b2_pct"] = round(100.0 * abs(med["b2"] - med["b"]) / med["b"], 2)
        info["a_measured"] = bool(parent)
        info["b_minus_a_us"] = round(med["b"] - med["a"], 2) if parent else None
        info["b_over_a"] = round(med["b"] / med["a"], 3) if parent else None
        info["b_minus_an_us"] = round(med["b"] - med["an"], 2)
        info["c_minus_b_us"] = round(med["c"] - med["b"], 2)
        info["d_minus_c_us"] = round(med["d"] - med["c"], 2)
        info["e_minus_c_us"] = round(med["e"] - med["c"], 2)
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
