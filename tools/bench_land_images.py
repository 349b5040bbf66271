#!/usr/bin/env python3
"""What marking the images on land (--land-images) costs.

Workload: the synthetic coastline of tools/bench_land_filter.py -- a star polygon of `--vertices` vertices of 200 km radius, `--islands`
small stars at sea and as many lakes, 200 vertices each -- and `--rects` image rectangles of `--side` metres (a 1024-px tile of the
reference's scenes is 307.2 m) centred within some 400 m of random coastline vertices, so that most of them have coast edges within reach.
Per size, after two warm-ups, `--repeats` times, median and range:

  table    engine.land_band_table: torch on the device (HIP events)
  kernel   aq_land_images_f64: its two launches, gather and images (HIP events)
  call     land_images.land_images_gpu as a caller sees it: host arrays in, bytes and doubles out, ending in the copies back, which
           synchronise (host clock)
  numpy    land_images.land_images_numpy on the same host for the first `--numpy-rects` rectangles against all segments (it takes every
           pair, so the whole input is out of reach; the figure per rectangle is printed beside it), and whether the GPU's bytes and
           doubles equal it there

and the table's shape and the length of the searched runs (entries per rectangle: mean, median, maximum), which is what the kernel's cost
per rectangle is proportional to.

    python tools/bench_land_images.py [--vertices 100000 1000000] [--rects 1000000] [--side 307.2] [--indent 5] [--repeats 5] [--numpy-rects 50] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_land_filter import coastline, spread  # noqa: E402


def rects_near(ring, n, side, seed=1):
    import numpy as np
    rng = np.random.default_rng(seed)
    c = ring[rng.integers(0, ring.shape[0], n)] + rng.normal(0, 400.0, (n, 2))
    return np.ascontiguousarray(np.concatenate([c - side / 2, c + side / 2], 1))


def run_lengths(band_start, nbands, Y0, h, rects, indent):
    """Entries each rectangle's wavefront walks: the bands floor((y0 - 3 r - Y0) / h) .. floor((y1 + 3 r - Y0) / h), clamped."""
    import numpy as np
    bs = band_start.cpu().numpy().astype(np.int64)
    lo = np.clip(np.floor((rects[:, 1] - 3 * indent - Y0) / h), 0, nbands - 1).astype(np.int64)
    hi = np.clip(np.floor((rects[:, 3] + 3 * indent - Y0) / h), 0, nbands - 1).astype(np.int64)
    return bs[hi + 1] - bs[lo]


def run(vertices, n_rects, side, indent, islands, repeats, numpy_rects):
    import numpy as np
    import torch
    from aquaculture_amd import engine, land_images
    rows = []
    for v in vertices:
        segs, ring = coastline(v, islands)
        rects = rects_near(ring, n_rects, side)
        s, b = torch.from_numpy(segs).cuda(), torch.from_numpy(rects).cuda()
        for _ in range(2):
            engine.land_images(b, s, indent)
        torch.cuda.synchronize()
        table_ms, kernel_ms, call_ms = [], [], []
        for _ in range(repeats):
            t = {}
            engine.land_images(b, s, indent, times=t)
            table_ms.append(t["table_ms"]); kernel_ms.append(t["kernel_ms"])
            t0 = time.perf_counter()
            flags, dist2 = land_images.land_images_gpu(rects, segs, indent)
            call_ms.append((time.perf_counter() - t0) * 1e3)
        _, band_start, nbands, Y0, h = engine.land_band_table(s)
        run = run_lengths(band_start, nbands, Y0, h, rects, indent)
        row = {"vertices": v, "segments": int(segs.shape[0]), "rects": n_rects, "side_m": side, "indent_m": indent, "on_land": int((flags == 2).sum()),
               "bytes_0_to_3": np.bincount(flags, minlength=4).tolist(), "near_threshold": land_images.near_threshold(dist2, indent),
               "bands": nbands, "band_height_m": h, "entries": int(band_start[-1]),
               "entries_per_rect": {"mean": float(run.mean()), "median": float(np.median(run)), "max": int(run.max())},
               "table_ms": spread(table_ms), "kernel_ms": spread(kernel_ms), "call_ms": spread(call_ms)}
        row["kernel_ns_per_entry_walked"] = row["kernel_ms"]["median"] * 1e6 / max(float(run.sum()), 1.0)
        k = min(numpy_rects, n_rects)
        if k > 0:
            t0 = time.perf_counter()
            want = land_images.land_images_numpy(rects[:k], segs, indent)
            dt = (time.perf_counter() - t0) * 1e3
            row["numpy"] = {"rects": k, "ms": dt, "ms_per_rect": dt / k,
                            "equal_to_gpu": bool(np.array_equal(want[0], flags[:k]) and np.array_equal(want[1].view(np.uint64), dist2[:k].view(np.uint64)))}
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--vertices", nargs="+", type=int, default=[100_000, 1_000_000], help="vertices of the main coastline ring")
    p.add_argument("--rects", type=int, default=1_000_000)
    p.add_argument("--side", type=float, default=307.2, help="side of an image rectangle in metres")
    p.add_argument("--indent", type=float, default=5.0)
    p.add_argument("--islands", type=int, default=20, help="islands at sea, and as many holes inside, 200 vertices each")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-rects", type=int, default=50, help="rectangles the numpy path is timed on (it takes every pair); 0 skips it")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_land_images: no GPU (timings are taken on the device or not at all)")
    rows = run(opt.vertices, opt.rects, opt.side, opt.indent, opt.islands, opt.repeats, opt.numpy_rects)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "rows": rows}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
