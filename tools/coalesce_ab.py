#!/usr/bin/env python3
"""Coalescing a pool set on the device (cio_file_coalesce_set_dev) against what
a caller does today -- copy the set to the host, merge there, copy it back --
in one process (profiles/r19/coalesce_ab.json).

    python tools/coalesce_ab.py [--entries 1024,102400] [--classes 4,8] [--iters 8] [--rounds 2] \\
        --out profiles/r19/coalesce_ab.json

The method is tools/pool_set_ab.py's.  Per shape a set of K classes (cls_k = 256
(k + 1), pal = align = 32, the target the largest) holds E entries of half the
target's size, filed in the class release files them in, each class shuffled.
Three patterns: `pairs` -- the entries adjacent two by two, a gap behind every
pair: E / 2 runs, E / 2 groups; `none` -- a gap behind every entry: no run, no
group, the set is only sorted; `onerun` -- every entry adjacent to the next: ONE
run of E / 2 groups, walked by one thread.  Two rotating sets; what a call
rewrites (the set's words and arrays) is restored, untimed, before every call.
The legs alternate ABBA inside each round; every leg runs twice (x and x2):
|x2 - x| is its A/A spread.

  dev    cio_file_coalesce_set_dev, between two events on one stream
  dry    the same with CIOA_COALESCE_DRY (no commit kernel), between two events
  host   D2H of the three set arrays, the merge in numpy (sort, prefix maximum,
         links vectorised; the group walk and the filing a Python loop), H2D of
         the three; wall clock around a stream synchronise

Not isolated: the sort from the rest of the chain; the single-workgroup scans;
the walk of the groups from the other kernels; bad entries (none here);
several targets; the launch overhead of the chain's kernels (12 + 3 per sort
pass) from their work -- at E = 1024 the figure is mostly launches.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ALIGN = 32
PATTERNS = ["pairs", "none", "onerun"]
LEGS = ["dev", "dry", "host"]


def host_merge(so, sc, words, n_cls, stride, target, align):
    """The merge a caller writes on the host, for sets without ill-formed
    entries.  so, sc, words: numpy uint64 arrays, changed in place.  Returns
    the number of groups."""
    cls = [int(words[4 * k + 2]) for k in range(n_cls)]
    T = cls[target]
    idx = np.concatenate([np.arange(k * stride, k * stride + int(words[4 * k])) for k in range(n_cls)])
    off, cap = so[idx], sc[idx]
    order = np.argsort(off, kind="stable")
    off, cap = off[order], cap[order]
    end = off + cap
    reach = np.maximum.accumulate(np.concatenate([[0], end[:-1]]).astype(np.uint64))
    keep = off >= reach
    off, cap = off[keep], cap[keep]
    nxt = (off + cap + np.uint64(align - 1)) // np.uint64(align) * np.uint64(align)
    linked = np.zeros(len(off), bool)
    linked[1:] = (cap[1:] < T) & (cap[:-1] < T) & (nxt[:-1] == off[1:])
    o, c, ln = off.tolist(), cap.tolist(), linked.tolist()
    outs, groups, i, n = [], 0, 0, len(o)
    while i < n:
        if c[i] >= T:
            outs.append((o[i], c[i]))
            i += 1
            continue
        e = i + 1
        while e < n and ln[e]:
            e += 1
        g = i                                     # pal = align: every entry may start a group
        while g < e:
            h = g + 1
            while h < e and o[h] < o[g] + T:
                h += 1
            span = o[h - 1] + c[h - 1] - o[g]
            if h == e and span < T:
                outs.extend(zip(o[g:e], c[g:e]))
            else:
                outs.append((o[g], span))
                groups += h - g >= 2
            g = h
        i = e
    filed = [[] for _ in range(n_cls)]
    for off_, cap_ in outs:
        k = int(np.searchsorted(cls, cap_, side="right")) - 1
        if k >= 0:
            filed[k].append((off_, cap_))
    for k in range(n_cls):
        if filed[k]:
            a = np.asarray(filed[k], np.uint64)
            so[k * stride:k * stride + len(a)] = a[:, 0]
            sc[k * stride:k * stride + len(a)] = a[:, 1]
        words[4 * k] = len(filed[k])
    return groups


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--entries", default="1024,102400")
    ap.add_argument("--classes", default="4,8")
    ap.add_argument("--iters", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=2)
    ap.add_argument("--warm-s", type=float, default=1.0)
    ap.add_argument("--out", default=None, help="JSON file; shapes measured earlier in it are kept")
    args = ap.parse_args()
    import torch
    import chunkio_amd as cio
    from chunkio_amd import _lib
    from chunkio_amd import chunkfile as cf

    lib = cio.lib()
    if not torch.cuda.is_available():
        raise SystemExit("coalesce_ab.py needs a GPU")
    dev = torch.device("cuda:0")
    stream = torch.cuda.current_stream().cuda_stream

    def i64(a):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint64).view(np.int64)).to(dev)

    results = {"shapes": {}}
    if args.out and os.path.exists(args.out):
        with open(args.out) as f:
            results = json.load(f)
    results.update({"device": torch.cuda.get_device_name(dev), "iters": args.iters, "rounds": args.rounds,
                    "version": lib.cio_gpu_version().decode(), "align": ALIGN})
    for E in (int(x) for x in args.entries.split(",")):
        for K in (int(x) for x in args.classes.split(",")):
            classes = [(256 * (k + 1), ALIGN) for k in range(K)]
            target, T = K - 1, 256 * K
            cap, home = T // 2, K // 2 - 1                    # cls_home = T / 2: where release files such a slot
            stride, dev_bytes = E, 1 << 34
            writer = cf.DevWriter(K * stride)
            for pattern in PATTERNS:
                name = f"E{E}_K{K}_{pattern}"
                j = np.arange(E, dtype=np.uint64)
                if pattern == "pairs":                    # two slots side by side, then a gap of cap + ALIGN
                    offs = np.uint64(4096) + (j // 2) * np.uint64(3 * cap + ALIGN) + (j % 2) * np.uint64(cap)
                else:
                    offs = np.uint64(4096) + j * np.uint64(cap + (ALIGN if pattern == "none" else 0))
                rng = np.random.default_rng(E + K)
                so0, sc0 = np.zeros(K * stride, np.uint64), np.zeros(K * stride, np.uint64)
                so0[home * stride:home * stride + E] = rng.permutation(offs)
                sc0[home * stride:home * stride + E] = cap
                words0 = np.asarray([w for k, (c, p) in enumerate(classes) for w in (E if k == home else 0, stride, c, p)],
                                    np.uint64)
                nrot = 2
                sets = [[i64(so0), i64(sc0), i64(words0), K, stride] for _ in range(nrot)]
                keep = (i64(so0), i64(sc0), i64(words0))
                total = torch.zeros(5 + K, dtype=torch.int64, device=dev)
                # what the host leg computes, and the device call's answer at the timed size
                hs, hc, hw = so0.copy(), sc0.copy(), words0.copy()
                groups = host_merge(hs, hc, hw, K, stride, target, ALIGN)
                cf.coalesce_set_dev(writer, dev_bytes, sets[0], target, align=ALIGN, total=total)
                torch.cuda.synchronize()
                got = total.cpu().tolist()
                assert got[0] == 0 and got[3] == groups == (0 if pattern == "none" else E // 2), (name, got, groups)
                assert np.array_equal(sets[0][2].cpu().numpy().view(np.uint64), hw), name
                for k in range(K):
                    cnt = int(hw[4 * k])
                    sl = slice(k * stride, k * stride + cnt)
                    assert np.array_equal(sets[0][0].cpu().numpy().view(np.uint64)[sl], hs[sl]), (name, k)
                    assert np.array_equal(sets[0][1].cpu().numpy().view(np.uint64)[sl], hc[sl]), (name, k)

                def restore(r):
                    for t, t0 in zip(sets[r][:3], keep):
                        t.copy_(t0)

                def leg(which, r, ev):
                    which = which.rstrip("_")
                    restore(r)
                    if which == "host":
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                        a, b, w = (t.cpu().numpy().view(np.uint64) for t in sets[r][:3])
                        host_merge(a, b, w, K, stride, target, ALIGN)
                        for t, h in zip(sets[r][:3], (a, b, w)):
                            t.copy_(torch.from_numpy(h.view(np.int64)))
                        torch.cuda.synchronize()
                        return (time.perf_counter() - t0) * 1e6
                    _lib.check(lib.cio_gpu_event_record(ev[0], stream), "event record")
                    cf.coalesce_set_dev(writer, dev_bytes, sets[r], target, align=ALIGN,
                                        flags=cf.COALESCE_DRY * (which == "dry"), total=total)
                    _lib.check(lib.cio_gpu_event_record(ev[1], stream), "event record")
                    return None

                iters = args.iters if E <= 4096 or pattern != "onerun" else max(2, args.iters // 4)
                evs = [(lib.cio_gpu_event_create(), lib.cio_gpu_event_create()) for _ in range(iters)]
                order = LEGS + [x + "_" for x in LEGS]
                t_end = time.perf_counter() + args.warm_s
                while time.perf_counter() < t_end:
                    leg("dry", 0, evs[0])
                    torch.cuda.synchronize()
                per_round = {k: [] for k in order}
                for r in range(args.rounds):
                    for which in (order if r % 2 == 0 else order[::-1]):
                        leg(which, 0, evs[0])
                        wall = [leg(which, i % nrot, evs[i]) for i in range(iters)]
                        torch.cuda.synchronize()
                        if which.startswith("host"):
                            per_round[which].append(float(np.mean(wall)))
                        else:
                            per_round[which].append(float(np.mean(
                                [lib.cio_gpu_event_elapsed_ms(e0, e1) for e0, e1 in evs])) * 1e3)
                med = {k: float(np.median(v)) for k, v in per_round.items()}
                info = {"entries": E, "classes": K, "pattern": pattern, "groups": groups, "iters": iters,
                        "us": {k: round(med[k], 2) for k in LEGS},
                        "us_second_run": {k: round(med[k + "_"], 2) for k in LEGS},
                        "aa_spread_us": {k: round(abs(med[k + "_"] - med[k]), 2) for k in LEGS},
                        "host_over_dev": round(med["host"] / med["dev"], 2)}
                results["shapes"][name] = info
                print(name, json.dumps(info), flush=True)
                for e0, e1 in evs:
                    lib.cio_gpu_event_destroy(e0)
                    lib.cio_gpu_event_destroy(e1)
                if args.out:
                    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                    with open(args.out, "w") as f:
                        f.write(json.dumps(results, indent=1) + "\n")
            writer.close()
            torch.cuda.empty_cache()
    print(json.dumps(results))


if __name__ == "__main__":
    main()
