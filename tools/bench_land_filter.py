#!/usr/bin/env python3
"""What the land filter of --land-filter costs.

Workload: a synthetic coastline in EPSG:3857-sized coordinates -- a star polygon of `--vertices` vertices whose radius (200 km) varies
smoothly by a few sinusoids plus a jitter of the order of one segment, `--islands` small stars at sea around it and as many holes (lakes)
inside it, 200 vertices each -- and `--boxes` detection boxes of 5 to 30 m centred within some 50 m of random coastline vertices.  Per
size, after warm-up, `--repeats` times, median and range:

  table    engine.land_band_table: torch on the device -- bands of every segment, counts, cumsum, repeat_interleave, sort, searchsorted
           (HIP events)
  kernel   aq_land_filter_f64: its two launches, gather and flags (HIP events)
  flags    land.land_flags as a caller sees it: host arrays in, bytes out (host clock; includes both copies)
  numpy    land.land_flags_numpy on the same host for the first `--numpy-boxes` boxes against all segments (it tests every pair, so the
           whole input is out of reach; the figure per box is printed beside it), and whether the GPU's bytes equal it there

and the table's shape: bands, band height, entries, entries per band (mean, median, maximum).  For the shares of the two kernels run it
under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_land_filter.py [--vertices 100000 1000000] [--boxes 1000000] [--islands 20] [--repeats 5] [--numpy-boxes 200] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OX, OY = 5.0e5, 5.4e6


def star(n, radius, centre, rng, waves=((3, 0.15), (7, 0.08), (23, 0.03), (101, 0.01))):
    """n vertices at equal angles: radius (1 + sum a sin(k t + phase)) plus a jitter of a third of a segment -> float64 [n, 2]."""
    import numpy as np
    t = np.arange(n) * (2 * np.pi / n)
    r = np.ones(n)
    for k, a in waves:
        r += a * np.sin(k * t + rng.uniform(0, 2 * np.pi))
    r = radius * r + rng.normal(0, radius * 2 * np.pi / n / 3, n)
    return np.stack([centre[0] + r * np.cos(t), centre[1] + r * np.sin(t)], 1)


def coastline(vertices, islands, seed=0):
    """-> (segments float64 [E, 4], the main ring's vertices): E = vertices + 2 islands 200."""
    import numpy as np
    rng = np.random.default_rng(seed)
    rings = [star(vertices, 2.0e5, (OX, OY), rng)]
    for k in range(islands):
        a = rng.uniform(0, 2 * np.pi)
        rings.append(star(200, 500.0, (OX + 2.8e5 * np.cos(a), OY + 2.8e5 * np.sin(a)), rng))          # at sea: beyond 1.27 radii
        a = rng.uniform(0, 2 * np.pi)
        rings.append(star(200, 500.0, (OX + 0.5e5 * np.cos(a), OY + 0.5e5 * np.sin(a)), rng)[::-1])    # a lake, its ring the other way round
    segs = np.concatenate([np.concatenate([r, np.roll(r, -1, 0)], 1) for r in rings], 0)
    return np.ascontiguousarray(segs), rings[0]


def boxes_near(ring, n, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    c = ring[rng.integers(0, ring.shape[0], n)] + rng.normal(0, 50.0, (n, 2))
    half = rng.uniform(2.5, 15.0, (n, 2))
    return np.ascontiguousarray(np.concatenate([c - half, c + half], 1))


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(vertices, n_boxes, islands, repeats, numpy_boxes):
    import numpy as np
    import torch
    from aquaculture_amd import engine, land
    rows = []
    for v in vertices:
        segs, ring = coastline(v, islands)
        boxes = boxes_near(ring, n_boxes)
        s, b = torch.from_numpy(segs).cuda(), torch.from_numpy(boxes).cuda()
        for _ in range(2):
            engine.land_flags(b, s)
        torch.cuda.synchronize()
        table_ms, kernel_ms, flags_ms = [], [], []
        for _ in range(repeats):
            t = {}
            engine.land_flags(b, s, times=t)
            table_ms.append(t["table_ms"]); kernel_ms.append(t["kernel_ms"])
            t0 = time.perf_counter()
            flags = land.land_flags(boxes, segs)
            flags_ms.append((time.perf_counter() - t0) * 1e3)
        _, band_start, nbands, _, h = engine.land_band_table(s)
        per_band = torch.diff(band_start.to(torch.int64)).cpu().numpy()
        row = {"vertices": v, "segments": int(segs.shape[0]), "boxes": n_boxes, "on_land": int((flags != 0).sum()),
               "bytes_0_to_3": np.bincount(flags, minlength=4).tolist(), "bands": nbands, "band_height_m": h, "entries": int(per_band.sum()),
               "entries_per_band": {"mean": float(per_band.mean()), "median": float(np.median(per_band)), "max": int(per_band.max())},
               "table_ms": spread(table_ms), "kernel_ms": spread(kernel_ms), "land_flags_ms": spread(flags_ms)}
        k = min(numpy_boxes, n_boxes)
        if k > 0:
            t0 = time.perf_counter()
            want = land.land_flags_numpy(boxes[:k], segs)
            dt = (time.perf_counter() - t0) * 1e3
            row["numpy"] = {"boxes": k, "ms": dt, "ms_per_box": dt / k, "equal_to_gpu": bool(np.array_equal(want, flags[:k]))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--vertices", nargs="+", type=int, default=[100_000, 1_000_000], help="vertices of the main coastline ring")
    p.add_argument("--boxes", type=int, default=1_000_000)
    p.add_argument("--islands", type=int, default=20, help="islands at sea, and as many holes inside, 200 vertices each")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-boxes", type=int, default=200, help="boxes the numpy path is timed on (it tests every pair); 0 skips it")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_land_filter: no GPU (timings are taken on the device or not at all)")
    rows = run(opt.vertices, opt.boxes, opt.islands, opt.repeats, opt.numpy_boxes)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "rows": rows}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
