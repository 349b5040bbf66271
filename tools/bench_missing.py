#!/usr/bin/env python3
"""What the box-against-coverage test of --tonnage-missing costs.

Workload, about the reference's size: `--passes` passes of `--images` image tiles each (307.2 m a side, laid on a grid of `--columns`
columns, every tenth -- `--ring-share` -- partly blank with a closed staircase ring of about `--ring-vertices` vertices), and `--queries`
cage boxes of 5 to 30 m placed on random tiles, each asked against a random pass.  After warm-up, `--repeats` times, median and range:

  kernel     aq_coverage_first_i32 through the default band tables: its two launches, gather and first (HIP events)
  one_band   the same launches with one band per pass: every query walks its whole pass -- the kernel without a search structure
  first_gpu  missing.first_gpu as a caller sees it: host arrays in, host array out (host clock; includes the copies)
  tables     missing.band_tables on the host (numpy)
  numpy      missing.first_numpy through the same tables for the first `--numpy-queries` queries (a Python loop over the queries; the figure
             per query is printed beside it), and whether the GPU's bytes equal it there

    python tools/bench_missing.py [--passes 6] [--images 30000] [--queries 30000] [--ring-vertices 2000] [--repeats 5] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

OX, OY, SIDE = 3.0e5, 5.2e6, 307.2


def staircase(vertices):
    """A closed pixel ring of about `vertices` vertices inside the 1024-px frame: stairs down to the right, then back along the bottom and
    up the left side."""
    steps = max(1, min(1023, (vertices - 3) // 2))
    ring = [(0, 0)]
    for j in range(steps):
        ring += [(j + 1, j), (j + 1, j + 1)]
    return ring + [(0, steps), (0, 0)]


def problem(passes, images, columns, ring_share, ring_vertices, queries, seed=0):
    import numpy as np
    from aquaculture_amd import missing as ms
    rng = np.random.default_rng(seed)
    walk = np.asarray(staircase(ring_vertices), np.float64)
    rect, rings, pass_id = [], [], []
    for p in range(passes):
        cell = rng.permutation(columns * max(1, (2 * images + columns - 1) // columns))[:images]
        x, y = OX + SIDE * (cell % columns), OY + SIDE * (cell // columns)
        rect.append(np.stack([x, y, x + SIDE, y + SIDE], 1))
        pass_id += [p] * images
        for k in range(images):
            if rng.random() < ring_share:
                w, s, e, n = rect[-1][k].tolist()
                rings.append(ms.ring_metres(walk, w, s, e, n))
            else:
                rings.append(None)
    rect = np.concatenate(rect, 0)
    reg = ms._table([f"pass {p}" for p in range(passes)], pass_id, rect, rings, [str(k) for k in range(rect.shape[0])])
    at = rect[rng.integers(0, rect.shape[0], queries)]
    c = at[:, :2] + rng.random((queries, 2)) * SIDE
    half = rng.uniform(2.5, 15.0, (queries, 2))
    return reg, np.ascontiguousarray(np.concatenate([c - half, c + half], 1)), rng.integers(0, passes, queries).astype(np.int32)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(opt):
    import numpy as np
    import torch
    from aquaculture_amd import engine, missing as ms
    reg, boxes, qpass = problem(opt.passes, opt.images, opt.columns, opt.ring_share, opt.ring_vertices, opt.queries)
    t0 = time.perf_counter()
    tables = ms.band_tables(reg)
    tables_ms = (time.perf_counter() - t0) * 1e3
    one = ms.band_tables(reg, 1)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d = {k: dev(reg[k]) for k in ("rect", "ring_start", "xy")}
    b, q = dev(boxes), dev(qpass)

    def launch(t, td, times=None):
        return engine.coverage_first(d["rect"], d["ring_start"], d["xy"], td["entry_img"], td["band_start"], td["band"], t["nbands"], b, q,
                                     reg["ring_start"], t["band_start"], t["band"], times=times)

    result = {}
    firsts = {}
    for name, t in (("kernel", tables), ("one_band", one)):
        td = {k: dev(t[k]) for k in ("entry_img", "band_start", "band")}
        for _ in range(2):
            launch(t, td)
        torch.cuda.synchronize()
        ms_ = []
        for _ in range(opt.repeats):
            times = {}
            firsts[name] = launch(t, td, times).cpu().numpy()
            ms_.append(times["kernel_ms"])
        per_band = np.diff(t["band_start"].astype(np.int64))
        result[name] = {"ms": spread(ms_), "bands": int(t["nbands"]), "entries": int(t["entry_img"].shape[0]),
                        "entries_per_band": {"mean": float(per_band.mean()), "max": int(per_band.max())}}
    host_ms = []
    for _ in range(opt.repeats):
        t0 = time.perf_counter()
        got = ms.first_gpu(reg, tables, boxes, qpass)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    row = {"passes": opt.passes, "images": int(reg["rect"].shape[0]), "ring_images": int(reg["kind"].sum()), "ring_vertices": int(reg["xy"].shape[0]),
           "queries": opt.queries, "covered": int((got >= 0).sum()), "one_band_equal": bool(np.array_equal(firsts["kernel"], firsts["one_band"])),
           **result, "first_gpu_ms": spread(host_ms), "band_tables_ms": tables_ms}
    k = min(opt.numpy_queries, opt.queries)
    if k > 0:
        t0 = time.perf_counter()
        want = ms.first_numpy(reg, tables, boxes[:k], qpass[:k])
        dt = (time.perf_counter() - t0) * 1e3
        row["numpy"] = {"queries": k, "ms": dt, "ms_per_query": dt / k, "equal_to_gpu": bool(np.array_equal(want, got[:k]))}
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--passes", type=int, default=6)
    p.add_argument("--images", type=int, default=30_000, help="image tiles per pass")
    p.add_argument("--columns", type=int, default=400, help="columns of the tile grid")
    p.add_argument("--ring-share", type=float, default=0.1, help="share of partly blank images")
    p.add_argument("--ring-vertices", type=int, default=2000)
    p.add_argument("--queries", type=int, default=30_000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-queries", type=int, default=30_000, help="queries the numpy path is timed on; 0 skips it")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_missing: no GPU (timings are taken on the device or not at all)")
    row = run(opt)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "row": row}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
