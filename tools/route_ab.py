#!/usr/bin/env python3
"""Routing records to chunk images by their metadata (cio_file_route_build_dev,
cio_file_route_records_batch_dev) beside the ungrouped append that the route
feeds, in one process (profiles/r22/route_ab.json).

    python tools/route_ab.py [--shape 1024x102400,65536x102400] [--rec-bytes 256] [--iters 10] [--rounds 4] \\
        --out profiles/r22/route_ab.json

A shape IxR is I images and R records.  Every image has a metadata of its own,
16..64 bytes; record r goes to a random image and carries that image's metadata
as its tag (all hits), packed at odd offsets, and --rec-bytes of payload.
Event times on one stream, warm, the legs interleaved and reversed in every
other round, the mean of --iters calls per round, medians over the rounds with
their spread; every sample is kept.  Before every timed append the content
lengths of the images are put back to 0 (untimed, ahead of the first event).

  build      cio_file_route_build_dev over the I images
  route      cio_file_route_records_batch_dev over the R records, no gate, no miss list
  route2     the same again: the A/A spread
  append     cio_file_write_records_ungrouped_batch_dev of the same records with the routed indices, CIO_CHECKSUM
  b1..b5     the build with the events around ONE section (cioa_debug_route_build_events): the region kernel, the
             planner's kernels, the CRC launch, the sort, the copy-out and the header
  r1..r5     the route likewise (cioa_debug_route_records_events): the region kernel, the planner's kernels, the
             CRC launch, the probe, the totals

Reported: the route's share of route + append, and the sections' split.

Not isolated: the images and tags (a few MB) stay in the 256 MB Infinity Cache
between calls, as they would behind a producer that has just written the tags;
a section's events add two event records to the chain they time; the append's
time depends on --rec-bytes, which the route's does not.
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

SECTIONS = {"b": ("regions", "planner", "crc", "sort", "out"), "r": ("regions", "planner", "crc", "probe", "totals")}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--shape", default="1024x102400,65536x102400")
    ap.add_argument("--rec-bytes", type=int, default=256)
    ap.add_argument("--iters", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=4)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    if not torch.cuda.is_available():
        raise SystemExit("route_ab.py needs a GPU")
    lib = cio.lib()
    V, U64, S, I, U32 = ctypes.c_void_p, ctypes.c_uint64, ctypes.c_size_t, ctypes.c_int, ctypes.c_uint32
    lib.cioa_debug_route_build_events.restype = I
    lib.cioa_debug_route_build_events.argtypes = [V, V, U64, V, V, S, V, V, V, V, I, V, V]
    lib.cioa_debug_route_records_events.restype = I
    lib.cioa_debug_route_records_events.argtypes = [V, V, U64, V, V, S, V, V, V, V, U64, V, V, S, U32, V, V, V, V, I,
                                                    V, V]
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream
    CK = cf.CIO_CHECKSUM

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"device": torch.cuda.get_device_name(dev), "version": lib.cio_gpu_version().decode(),
               "iters": args.iters, "rounds": args.rounds, "rec_bytes": args.rec_bytes, "shapes": {}}
    for shape in args.shape.split(","):
        n_img, n_rec = (int(x) for x in shape.split("x"))
        rng = np.random.default_rng(22)
        m_lens = rng.integers(16, 65, n_img).astype(np.uint64)
        m_offs = np.cumsum(m_lens) - m_lens
        metas = rng.integers(0, 256, int(m_lens.sum()), dtype=np.uint8)
        for i in range(n_img):                    # a metadata of its own for every image: its index leads
            metas[int(m_offs[i]):int(m_offs[i]) + 8] = np.frombuffer(b"%08x" % i, np.uint8)
        rec_img = rng.integers(0, n_img, n_rec).astype(np.uint32)
        t_lens = m_lens[rec_img]
        t_offs = (np.cumsum(t_lens + 2) - t_lens) | 1
        t_offs = t_offs.astype(np.uint64)
        tags = rng.integers(0, 256, int(t_offs[-1] + t_lens[-1]) + 16, dtype=np.uint8)
        reps = t_lens.astype(np.int64)
        idx = np.repeat(t_offs - np.cumsum(t_lens) + t_lens, reps) + np.arange(int(t_lens.sum()), dtype=np.uint64)
        src_idx = np.repeat(m_offs[rec_img] - np.cumsum(t_lens) + t_lens, reps) + \
            np.arange(int(t_lens.sum()), dtype=np.uint64)
        tags[idx.astype(np.int64)] = metas[src_idx.astype(np.int64)]
        per = np.bincount(rec_img, minlength=n_img).astype(np.uint64)
        caps = (24 + 64 + per * np.uint64(args.rec_bytes) + 63) & ~np.uint64(63)
        offs = np.cumsum(caps) - caps
        total = int(caps.sum())
        s_offs = np.arange(n_rec, dtype=np.uint64) * np.uint64(args.rec_bytes + 3) + np.uint64(5)
        src = torch.randint(0, 256, (int(s_offs[-1]) + args.rec_bytes + 16,), dtype=torch.uint8, device=dev)
        base = torch.zeros(total + 64, dtype=torch.uint8, device=dev)
        offs_t, caps_t = i64(offs), i64(caps)
        tags_t, to_t, tl_t = torch.from_numpy(tags).to(dev), i64(t_offs), i64(t_lens)
        so_t, sl_t = i64(s_offs), i64(np.full(n_rec, args.rec_bytes, np.uint64))
        writer = cf.DevWriter(max(n_img, n_rec))
        st, crc = cf.init_batch_dev(writer, base, offs_t, caps_t, torch.from_numpy(metas).to(dev), i64(m_offs),
                                    i64(m_lens), flags=CK)
        assert int(st.count_nonzero()) == 0
        crc0 = crc.clone()
        len_idx = (offs_t[:, None] + torch.arange(10, 14, device=dev)[None, :]).reshape(-1)
        d = cf.route_dir(n_img, dev)
        rimg = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        rst = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        rtot = torch.zeros(3, dtype=torch.int64, device=dev)
        ist = torch.zeros(n_img, dtype=torch.int32, device=dev)
        wst = torch.zeros(n_rec, dtype=torch.int32, device=dev)
        nbytes = base.numel()

        def build(section, ev):
            if section:
                rc = lib.cioa_debug_route_build_events(writer._handle, base.data_ptr(), nbytes, offs_t.data_ptr(),
                                                       caps_t.data_ptr(), n_img, d[0].data_ptr(), d[1].data_ptr(),
                                                       d[2].data_ptr(), stream, section, ev[0], ev[1])
            else:
                rc = lib.cio_file_route_build_dev(writer._handle, base.data_ptr(), nbytes, offs_t.data_ptr(),
                                                  caps_t.data_ptr(), n_img, d[0].data_ptr(), d[1].data_ptr(),
                                                  d[2].data_ptr(), stream)
            _lib.check(rc, "route build")

        def route(section, ev):
            if section:
                rc = lib.cioa_debug_route_records_events(
                    writer._handle, base.data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n_img,
                    d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), tags_t.data_ptr(), tags_t.numel(),
                    to_t.data_ptr(), tl_t.data_ptr(), n_rec, n_img, rimg.data_ptr(), rst.data_ptr(), rtot.data_ptr(),
                    stream, section, ev[0], ev[1])
            else:
                rc = lib.cio_file_route_records_batch_dev(
                    writer._handle, base.data_ptr(), nbytes, offs_t.data_ptr(), caps_t.data_ptr(), n_img, None,
                    d[0].data_ptr(), d[1].data_ptr(), d[2].data_ptr(), tags_t.data_ptr(), tags_t.numel(),
                    to_t.data_ptr(), tl_t.data_ptr(), n_rec, n_img, 0, rimg.data_ptr(), rst.data_ptr(), None,
                    rtot.data_ptr(), stream)
            _lib.check(rc, "route records")

        def leg(name, ev):
            """Queue leg `name` between the events ev[0] and ev[1]."""
            if name[0] in "br" and name[1:].isdigit():
                (build if name[0] == "b" else route)(int(name[1:]), ev)
                return
            if name == "append":
                base[len_idx] = 0
                crc.copy_(crc0)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name == "build":
                build(0, ev)
            elif name in ("route", "route2"):
                route(0, ev)
            else:
                cf.write_records_ungrouped_batch_dev(writer, base, offs_t, caps_t, src, rimg, so_t, sl_t, crc,
                                                     flags=CK, img_status=ist, rec_status=wst)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        # correctness at the timed size: every record routed to its image, every record appended
        leg("build", evs[0])
        leg("route", evs[0])
        leg("append", evs[0])
        torch.cuda.synchronize()
        assert np.array_equal(rimg.cpu().numpy().view(np.uint32), rec_img), f"{shape}: routed indices"
        assert rtot.cpu().numpy().tolist() == [n_rec, 0, 0] and int(rst.count_nonzero()) == 0
        assert int(ist.count_nonzero()) == 0 and int(wst.count_nonzero()) == 0, f"{shape}: append refused"
        order = ["build", "route", "append"] + [f"b{k}" for k in range(1, 6)] + [f"r{k}" for k in range(1, 6)] + \
            ["route2"]
        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for name in ("build", "route", "append"):
                leg(name, evs[0])
            torch.cuda.synchronize()
        samples = {k: [] for k in order}
        for r in range(args.rounds):
            for name in (order if r % 2 == 0 else order[::-1]):
                for i in range(2):
                    leg(name, evs[0])
                for i in range(args.iters):
                    leg(name, evs[i])
                torch.cuda.synchronize()
                samples[name].append([round(lib.cio_gpu_event_elapsed_ms(e0, e1) * 1e3, 2) for e0, e1 in evs])
        assert np.array_equal(rimg.cpu().numpy().view(np.uint32), rec_img) and int(wst.count_nonzero()) == 0
        per_round = {k: [float(np.mean(x)) for x in v] for k, v in samples.items()}
        med = {k: float(np.median(v)) for k, v in per_round.items()}
        info = {"images": n_img, "records": n_rec, "tag_bytes": int(t_lens.sum()), "payload_bytes": n_rec * args.rec_bytes,
                "image_bytes": total, "sort_passes": 4,
                "us": {k: round(v, 2) for k, v in med.items()},
                "us_round_min_max": {k: [round(min(v), 2), round(max(v), 2)] for k, v in per_round.items()},
                "us_samples": samples,
                "noise_route_vs_route2_pct": round(100.0 * abs(med["route2"] - med["route"]) / med["route"], 2),
                "route_share_of_route_plus_append_pct": round(100.0 * med["route"] / (med["route"] + med["append"]), 2),
                "build_split_us": {s: round(med[f"b{k + 1}"], 2) for k, s in enumerate(SECTIONS["b"])},
                "route_split_us": {s: round(med[f"r{k + 1}"], 2) for k, s in enumerate(SECTIONS["r"])}}
        results["shapes"][shape] = info
        print(shape, json.dumps({k: v for k, v in info.items() if k != "us_samples"}), flush=True)
        for e0, e1 in evs:
            lib.cio_gpu_event_destroy(e0)
            lib.cio_gpu_event_destroy(e1)
        writer.close()
        del base, src, tags_t
        torch.cuda.empty_cache()
        if args.out:
            os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
            with open(args.out, "w") as f:
                f.write(json.dumps(results, indent=1) + "\n")
    print(json.dumps({k: v for k, v in results.items() if k != "shapes"}))


if __name__ == "__main__":
    main()
