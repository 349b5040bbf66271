#!/usr/bin/env python3
"""What the three launches of --dedup-years cost.

Workload: a synthetic sweep of `--images` partly blank 1024-px images, `--per-group` years to a (pass, tile key) group, and `--cages`
cages of 8 to 40 px spread evenly over the groups, boxes anywhere on the frame.  Every image's mask is the even-odd fill of a ring of one
to six columns side by side, each from its own top to its own bottom (some 4 to 26 vertices).  The groups go through in chunks that keep
the bitmaps under dedup.BUDGET_BYTES, as a sweep's do.  After a warm-up, `--repeats` times, median and range, summed over the chunks:

  fill     aq_dedup_fill_u32: the toggles and the prefix XOR (HIP events)
  sets     aq_dedup_sets_u32: one wavefront per cage (HIP events)
  select   aq_dedup_select_f64: one wavefront per group (HIP events)
  call     dedup.selections_gpu as a caller sees it: host tables in, host arrays out, uploads and downloads included (host clock)
  numpy    dedup.selections_numpy on the same host, once, with its three steps' times, and whether the GPU's bytes equal it

    python tools/bench_dedup.py [--images 2000] [--per-group 2] [--cages 100000] [--repeats 5] [--no-numpy] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

FRAME = 1024


def column_ring(rng):
    import numpy as np
    xs = np.unique(rng.integers(0, FRAME + 1, int(rng.integers(2, 8)))).tolist()
    if len(xs) < 2:
        xs = [0, FRAME]
    mid = int(rng.integers(0, FRAME))
    tops, bottoms = rng.integers(0, mid + 1, len(xs) - 1).tolist(), rng.integers(mid + 1, FRAME + 1, len(xs) - 1).tolist()
    ring = [(xs[0], tops[0])]
    for k in range(len(xs) - 1):
        ring += [(xs[k], tops[k]), (xs[k + 1], tops[k])]
    for k in range(len(xs) - 2, -1, -1):
        ring += [(xs[k + 1], bottoms[k]), (xs[k], bottoms[k])]
    ring.append(ring[0])
    return [v for k, v in enumerate(ring) if k == 0 or v != ring[k - 1]]


def synthetic_problem(images, per_group, cages, seed=0):
    import numpy as np
    from aquaculture_amd import dedup
    rng = np.random.default_rng(seed)
    G = images // per_group
    slots = [[column_ring(rng) for _ in range(per_group)] for _ in range(G)]
    cg = np.arange(cages) % G
    cs = rng.integers(0, per_group, cages)
    x, y = rng.integers(0, FRAME - 8, cages), rng.integers(0, FRAME - 8, cages)
    box = np.stack([x, x + rng.integers(8, 41, cages), y, y + rng.integers(8, 41, cages)], 1)
    order = [list(rng.permutation(per_group)) + [-1] * (dedup.MAX_SLOTS - per_group) for _ in range(G)]
    return dedup.make_problem([FRAME] * G, [FRAME] * G, slots, cg, cs, box, rng.uniform(20.0, 400.0, cages), order)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--images", type=int, default=2000)
    ap.add_argument("--per-group", type=int, default=2)
    ap.add_argument("--cages", type=int, default=100000)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    opt = ap.parse_args()
    import torch
    from aquaculture_amd import dedup
    if not 1 <= opt.per_group <= dedup.MAX_SLOTS or opt.images < opt.per_group:
        ap.error(f"--per-group 1 to {dedup.MAX_SLOTS}, and at least one group")
    p = synthetic_problem(opt.images, opt.per_group, opt.cages)
    parts = dedup.chunks(p)
    res = {"device": torch.cuda.get_device_name(0), "images": int(p["n"].sum()), "groups": len(p["slots"]), "cages": int(p["cage_group"].shape[0]),
           "bitmap_bytes": int(dedup.group_words(p).sum()) * 4, "chunks": len(parts), "repeats": opt.repeats}
    got = dedup.selections_gpu(p)                           # warm-up: the library, the allocator
    torch.cuda.synchronize()
    runs = {"fill_ms": [], "sets_ms": [], "select_ms": [], "call_ms": []}
    for _ in range(opt.repeats):
        times = {}
        t0 = time.perf_counter()
        got = dedup.selections_gpu(p, times=times)
        runs["call_ms"].append((time.perf_counter() - t0) * 1e3)
        for k in ("fill_ms", "sets_ms", "select_ms"):
            runs[k].append(times[k])
    res.update({k: spread(v) for k, v in runs.items()})
    res["survivors"] = {name: int(((got["bits"] & bit) != 0).sum()) for name, bit in dedup.SELECTIONS.items()}
    if not opt.no_numpy:
        times = {}
        t0 = time.perf_counter()
        want = dedup.selections_numpy(p, times=times)
        res["numpy"] = {"call_ms": (time.perf_counter() - t0) * 1e3, **times}
        res["same_bytes"] = all(got[k].tobytes() == want[k].tobytes() for k in want)
    for k in ("fill_ms", "sets_ms", "select_ms", "call_ms"):
        line = f"{k[:-3]:>7}: {res[k]['median']:10.3f} ms ({res[k]['min']:.3f} .. {res[k]['max']:.3f})"
        if "numpy" in res:
            line += f"    numpy {res['numpy'][k]:12.1f} ms"
        print(line)
    print(json.dumps(res))
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(res, f, indent=1)
    return 0 if res.get("same_bytes", True) else 1


if __name__ == "__main__":
    sys.exit(main())
