#!/usr/bin/env python3
"""The size-classed pool set (cio_file_grow_set_batch_dev,
cio_file_release_set_batch_dev) against the plain calls, in one process
(profiles/r18/pool_set_ab.json).

    python tools/pool_set_ab.py [--cfg cfg2,cfg4k] [--iters 10] [--rounds 3] \\
        --out profiles/r18/pool_set_ab.json

The method is tools/pool_dev_ab.py's.  Per shape, n images of `used` bytes (24
+ 32 bytes of metadata + content) without room at multiples of `used`, an arena
of n slots of used + 4096 bytes behind them and n free slots of that size
behind the arena.  Event times on one stream, warm, two rotating buffer sets,
the legs alternating ABBA inside each round.  What a call rewrites -- the magic
of a released slot, the list, the counts, the set's words, offsets, capacities,
the arena's top -- is restored, untimed, before the first event of every call.
Every leg runs twice (x and x2): |x2 - x| is its A/A spread.

  g      cio_file_grow_batch_dev            every image grows by one page into the arena; the same library, and
                                            its device code is the parent's: the parent's figure
  ge     grow_set, an empty set of 4        nothing to take: every image arena-bound with its class's size
  gp1/4/8  grow_set, every slot from the pool  n entries in the largest of 1, 4, 8 classes: no arena slot is taken
  r, rc  cio_file_release_batch_dev         without flags / with CIOA_RELEASE_COMPACT, one pool
  s1/4/8, sc1/4/8  release_set              the same entries, their capacities spread evenly over 1, 4, 8 classes
  r4     four cio_file_release_batch_dev    the entries sorted by size into four quarters, a pool for each
  s4m    one release_set with n_cls = 4     over the same sorted entries

Not isolated: the bookkeeping kernels from the copy or the commit; a class or an
arena that cuts the batch; gates and live offsets (NULL here); CIOA_GROW_ZERO
and CIOA_RELEASE_ZERO (the fills are the plain calls'); the records variant.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALIGN, META, PAGE, STEP = 16, 32, 4096, 16
SHAPES = {"cfg2": (1024, 409600), "cfg4k": (102400, 4096)}     # n, used bytes
GROW = ["g", "ge", "gp1", "gp4", "gp8"]
REL = ["r", "rc", "s1", "s4", "s8", "sc1", "sc4", "sc8", "r4", "s4m"]
LEGS = GROW + REL


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
        raise SystemExit("pool_set_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "rounds": args.rounds,
                    "version": lib.cio_gpu_version().decode(), "align": ALIGN, "meta_bytes": META})
    for cfg in args.cfg.split(","):
        n, used = SHAPES[cfg]
        new_cap = used + PAGE                                  # one realloc step of a page, a multiple of ALIGN
        offs = np.arange(n, dtype=np.uint64) * np.uint64(used)
        top = n * used
        end = top + n * new_cap
        free_slots = np.uint64(end) + np.arange(n, dtype=np.uint64) * np.uint64(new_cap)
        nbytes = end + n * new_cap
        nrot = 2
        content = used - 24 - META - 8 * STEP                  # valid under every capacity a release leg gives it
        hdr = np.zeros((n, 24 + META), np.uint8)
        hdr[:, 0] = 0xC1
        hdr[:, 10:14] = np.full(n, content, np.uint64).astype(">u4").view(np.uint8).reshape(n, 4)
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
        # grow: the images have used = 24 + META + content and a capacity of exactly that
        gused = 24 + META + content
        offs0, gcaps0, arena0 = i64(offs), i64(np.full(n, gused, np.uint64)), i64([top, end])
        offs_t, caps_t, arena_t = offs0.clone(), gcaps0.clone(), arena0.clone()
        need_t = i64(np.full(n, new_cap - PAGE - gused + 1, np.uint64))    # one byte beyond new_cap - PAGE: new_cap
        gnew = (gused + PAGE + PAGE - 1) // PAGE * PAGE
        assert gnew <= new_cap

        def grow_set_of(k, full):
            classes = [(256 * (j + 1), ALIGN) for j in range(k - 1)] + [(gnew, ALIGN)]
            so, sc, words, n_cls, stride = cf.pool_set_state(classes, n, dev)
            if full:
                so[(k - 1) * n:] = i64(free_slots)
                sc[(k - 1) * n:] = new_cap
                words[4 * (k - 1)] = n
            return [so, sc, words, n_cls, stride], words.clone()
        gsets = {"ge": grow_set_of(4, False), "gp1": grow_set_of(1, True), "gp4": grow_set_of(4, True),
                 "gp8": grow_set_of(8, True)}
        # release: entry i has the capacity of class i % K (spread) or i // (n / 4) (sorted)
        base_cls = used - 8 * STEP
        img0 = torch.arange(n, dtype=torch.int32, device=dev)
        lo_t, lc_t, li_t, count_t = offs0.clone(), offs0.clone(), img0.clone(), i64([n, n])
        full0 = i64([n, n])

        def rel_set_of(k):
            classes = [(base_cls + STEP * j, ALIGN) for j in range(k)]
            s = list(cf.pool_set_state(classes, n, dev))
            return s, s[2].clone()
        rsets = {k: rel_set_of(k) for k in (1, 4, 8)}
        spread = {k: i64(base_cls + STEP * (np.arange(n) % k)) for k in (1, 4, 8)}
        sorted4 = i64(base_cls + STEP * (np.arange(n) // (n // 4)))
        pools = [list(cf.pool_state(n, base_cls + STEP * q, ALIGN, dev)) for q in range(4)]
        pool0 = [p[2].clone() for p in pools]
        writer = cf.DevWriter(n)
        status = torch.zeros(n, dtype=torch.int32, device=dev)
        total = torch.zeros(10, dtype=torch.int64, device=dev)

        def restore(name, k):
            bufs[k][hdr_idx] = hdr_t                       # a release took the magic
            if name in GROW:
                offs_t.copy_(offs0)
                caps_t.copy_(gcaps0)
                arena_t.copy_(arena0)
                if name != "g":
                    gsets[name][0][2].copy_(gsets[name][1])
                return
            lo_t.copy_(offs0)
            li_t.copy_(img0)
            count_t.copy_(full0)
            if name in ("r", "rc"):
                lc_t.copy_(spread[1])
                pools[0][2].copy_(pool0[0])
            elif name in ("r4", "s4m"):
                lc_t.copy_(sorted4)
                for p, w0 in zip(pools, pool0):
                    p[2].copy_(w0)
                rsets[4][0][2].copy_(rsets[4][1])
            else:
                kk = int(name.lstrip("sc"))
                lc_t.copy_(spread[kk])
                rsets[kk][0][2].copy_(rsets[kk][1])

        def leg(name, k, ev):
            """Queue leg `name` over buffer set k, between the events ev[0] and ev[1]."""
            name = name[:-1] if name.endswith("_") else name
            restore(name, k)
            _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
            if name == "g":
                cf.grow_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, arena_t, realloc=PAGE, page=PAGE,
                                  align=ALIGN, total=total[:1], status=status)
            elif name in GROW:
                cf.grow_set_batch_dev(writer, bufs[k], offs_t, caps_t, need_t, arena_t, gsets[name][0], realloc=PAGE,
                                      page=PAGE, align=ALIGN, total=total, status=status)
            elif name in ("r", "rc"):
                cf.release_batch_dev(writer, bufs[k], lo_t, lc_t, *pools[0], img=li_t, count=count_t,
                                     flags=cf.CIOA_RELEASE_COMPACT * (name == "rc"), total=total[:2], status=status)
            elif name == "r4":
                q = n // 4
                for j in range(4):
                    cf.release_batch_dev(writer, bufs[k], lo_t[j * q:(j + 1) * q], lc_t[j * q:(j + 1) * q], *pools[j],
                                         img=li_t[j * q:(j + 1) * q], total=total[:2], status=status[j * q:(j + 1) * q])
            elif name == "s4m":
                cf.release_set_batch_dev(writer, bufs[k], lo_t, lc_t, rsets[4][0], img=li_t, count=count_t,
                                         total=total, status=status)
            else:
                kk = int(name.lstrip("sc"))
                cf.release_set_batch_dev(writer, bufs[k], lo_t, lc_t, rsets[kk][0], img=li_t, count=count_t,
                                         flags=cf.CIOA_RELEASE_COMPACT * name.startswith("sc"), total=total,
                                         status=status)
            _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")

        evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(args.iters)]
        assert all(a and b for a, b in evs)
        order = LEGS + [x + "_" for x in LEGS]
        # correctness at the timed size
        for k in range(nrot):
            for name in LEGS:
                leg(name, k, evs[0])
                torch.cuda.synchronize()
                assert not status.cpu().numpy().any(), f"{cfg}: leg {name}: an entry was refused"
                if name in GROW:
                    pooled = name.startswith("gp")
                    assert torch.equal(offs_t, i64(free_slots).flip(0) if pooled else
                                       i64(np.uint64(top) + np.arange(n, dtype=np.uint64) * np.uint64(
                                           (gnew + ALIGN - 1) // ALIGN * ALIGN))), (cfg, name)
                    assert int(caps_t[0]) == (new_cap if pooled else gnew), (cfg, name)
                    assert (int(arena_t[0]) == top) == pooled, (cfg, name)
                    if name != "g":
                        assert total.cpu().tolist()[1] == (n if pooled else 0), (cfg, name)
                        assert int(gsets[name][0][2][4 * (gsets[name][0][3] - 1)]) == 0, (cfg, name)
                else:
                    assert total.cpu().tolist()[0] == (n // 4 if name == "r4" else n), (cfg, name, total.cpu().tolist())
                    if name in ("rc", "sc1", "sc4", "sc8"):
                        assert count_t.cpu().tolist() == [0, n] and not lo_t.cpu().numpy().any(), (cfg, name)
                    if name not in ("r", "rc", "r4"):
                        kk = 4 if name == "s4m" else int(name.lstrip("sc"))
                        assert rsets[kk][0][2].cpu().tolist()[0::4] == [n // kk] * kk, (cfg, name)
                    for i in (0, n // 3, n - 1):
                        assert not bufs[k][int(offs[i]):int(offs[i]) + 2].cpu().numpy().any(), (cfg, name, i)
        info = {"n": n, "used_bytes": used, "new_cap": new_cap, "buffer_bytes": nbytes, "rotating_buffers": nrot}
        t_end = time.perf_counter() + args.warm_s           # warm clocks before any timed round
        while time.perf_counter() < t_end:
            for k in range(8):
                leg("g", k % nrot, evs[0])
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
        info["us_second_run"] = {k: round(med[k + "_"], 2) for k in LEGS}
        info["us_per_round"] = {k: [round(float(x), 2) for x in v] for k, v in per_round.items()}
        info["aa_spread_us"] = {k: round(abs(med[k + "_"] - med[k]), 2) for k in LEGS}
        info["ge_minus_g_us"] = round(med["ge"] - med["g"], 2)
        info["ge_slower_than_three_spreads_of_g"] = bool(med["ge"] - med["g"] > 3 * abs(med["g_"] - med["g"]))
        info["s1_minus_r_us"] = round(med["s1"] - med["r"], 2)
        info["s1_slower_than_three_spreads_of_r"] = bool(med["s1"] - med["r"] > 3 * abs(med["r_"] - med["r"]))
        info["r4_minus_s4m_us"] = round(med["r4"] - med["s4m"], 2)
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
