#!/usr/bin/env python3
"""What the DBSCAN of --facilities costs.

Workload: synthetic coast-like point sets in EPSG:3035-sized coordinates -- strings of farms along a wavy coastline, each farm a dense
block of cages 4 to 6 m apart, plus uniformly scattered single detections (a fifth of the points) -- in `--groups` groups, at 1e4, 1e5
and 1e6 points.  Per size, after warm-up, `--repeats` times, median and range:

  sort     torch: cell indices, key packing, torch.sort (HIP events)
  kernel   aq_facility_dbscan_f64: its five launches (HIP events)
  labels   facilities.dbscan_labels as a caller sees it: host arrays in, labels out (host clock; includes both copies and the ranking)
  sklearn  sklearn.cluster.DBSCAN(eps, min_samples).fit per group on the same host, once (skipped above --sklearn-max points)

and whether the labels equal scikit-learn's.  For the shares of the five kernels run it under `rocprofv3 --kernel-trace --stats`.

    python tools/bench_facilities.py [--sizes 10000 100000 1000000] [--groups 4] [--repeats 5] [--sklearn-max 1000000] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def coast_points(n, groups, seed=0):
    """n points (float64 [n, 2], metres) and their groups (int32 [n])."""
    import numpy as np
    r = np.random.default_rng(seed)
    n_noise = n // 5
    n_farm = n - n_noise
    cages = r.integers(6, 40, max(1, n_farm // 20))         # cages per farm
    cages = cages[: max(1, int(np.searchsorted(np.cumsum(cages), n_farm)))]
    cages[-1] += n_farm - int(cages.sum())
    length = max(2.0e4, 60.0 * cages.shape[0])              # metres of coast: a farm every 60 m on average
    s = np.sort(r.uniform(0, length, cages.shape[0]))
    cx = 3.7e6 + s
    cy = 2.2e6 + 3000.0 * np.sin(s / 7000.0) + r.normal(0, 150.0, s.shape[0])
    farm = np.repeat(np.arange(cages.shape[0]), cages)
    k = np.arange(n_farm) - np.repeat(np.cumsum(cages) - cages, cages)     # cage number inside its farm: two rows
    step = r.uniform(4.0, 6.0, cages.shape[0])[farm]
    pts = np.stack([cx[farm] + (k // 2) * step, cy[farm] + (k % 2) * step], 1) + r.normal(0, 0.3, (n_farm, 2))
    noise = np.stack([3.7e6 + r.uniform(0, length, n_noise), 2.2e6 + r.uniform(-4000, 4000, n_noise)], 1)
    xy = np.concatenate([pts, noise])
    group = np.concatenate([r.integers(0, groups, cages.shape[0])[farm], r.integers(0, groups, n_noise)]).astype(np.int32)
    p = r.permutation(n)
    return np.ascontiguousarray(xy[p]), np.ascontiguousarray(group[p])


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(sizes, groups, repeats, sklearn_max, eps=10.0, min_samples=5):
    import numpy as np
    import torch
    from aquaculture_amd import facilities
    from aquaculture_amd.engine import facility_dbscan
    rows = []
    for n in sizes:
        xy, group = coast_points(n, groups)
        x, g = torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda()
        for _ in range(2):
            facility_dbscan(x, g, eps, min_samples)
        torch.cuda.synchronize()
        sort_ms, kernel_ms, labels_ms = [], [], []
        for _ in range(repeats):
            t = {}
            facility_dbscan(x, g, eps, min_samples, times=t)
            sort_ms.append(t["sort_ms"]); kernel_ms.append(t["kernel_ms"])
            t0 = time.perf_counter()
            labels, core = facilities.dbscan_labels(xy, group, eps, min_samples)
            labels_ms.append((time.perf_counter() - t0) * 1e3)
        row = {"points": n, "groups": groups, "clusters": int(sum(labels[group == k].max() + 1 for k in range(groups))), "core": int(core.sum()),
               "noise": int((labels < 0).sum()), "sort_ms": spread(sort_ms), "kernel_ms": spread(kernel_ms), "dbscan_labels_ms": spread(labels_ms)}
        if n <= sklearn_max:
            from sklearn.cluster import DBSCAN
            t0 = time.perf_counter()
            want = np.full(n, -1, np.int64)
            for k in range(groups):
                idx = np.nonzero(group == k)[0]
                want[idx] = DBSCAN(eps=eps, min_samples=min_samples).fit(xy[idx]).labels_
            row["sklearn_ms"] = (time.perf_counter() - t0) * 1e3
            row["equal_to_sklearn"] = bool(np.array_equal(want, labels))
        rows.append(row)
        print(json.dumps(row), flush=True)
    return rows


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--sizes", nargs="+", type=int, default=[10_000, 100_000, 1_000_000])
    p.add_argument("--groups", type=int, default=4)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--sklearn-max", type=int, default=1_000_000)
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_facilities: no GPU (timings are taken on the device or not at all)")
    rows = run(opt.sizes, opt.groups, opt.repeats, opt.sklearn_max)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "rows": rows}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
