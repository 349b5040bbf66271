#!/usr/bin/env python3
"""What --performance costs on the GPU, against the numpy restatement on the same host.

After two warm-ups, `--repeats` times, median and range:

  kernel    aq_bernoulli_counts_i32 at the reference's size (K = 10,000 samples of S = 10,518 draws at ten rates: 5.3e7 Philox calls), HIP
            events around the launch; draws per second from the median
  select    the device's sort of the [K, R] counts, the K // 2-th row and the zero counts (HIP events), ending in the copies to the host
  numpy     performance.simulate(cpu=True) for `--numpy-K` of the K simulations (host clock; the cost is linear in K, the figure scaled
            to K is printed beside it), and whether the GPU's counts equal the restatement's on those rows
  joins     the two box joins of the curves (engine.box_match: tp without payload, R with a [n, 3] payload) and their sorts, HIP events
            (curve_counts' "sort_ms" and "kernel_ms"), and curve_counts as a caller sees it (host clock, ends in copies); at the size of
            tests/golden/g12_humanlabels_1956_1962.json (991 labels, as many synthetic detections) and at `--detections` synthetic detections
            against a tenth as many labels; beside each the numpy path (evaluate.box_match_numpy and the numpy counts) on the same inputs and
            whether the counts are equal

    python tools/bench_performance.py [--repeats 5] [--numpy-K 500] [--detections 100000] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def synthetic(n_det, n_lab, seed=1):
    """evaluate.inputs-shaped data: labels of 10 m in clusters over a 40 km square, three years and both types; detections = jittered
    labels (two thirds) and strays; three domain masks."""
    import numpy as np
    rng = np.random.default_rng(seed)
    centres = rng.uniform(0, 40000.0, (max(1, n_lab // 20), 2))
    lxy = centres[rng.integers(0, centres.shape[0], n_lab)] + rng.normal(0, 60.0, (n_lab, 2))
    lbox = np.concatenate([lxy, lxy + 10.0], 1)
    lgroup = rng.integers(0, 6, n_lab).astype(np.int32)
    src = rng.integers(0, n_lab, n_det)
    dbox = lbox[src] + np.where(rng.random(n_det)[:, None] < 0.67, rng.normal(0, 1.5, (n_det, 4)), np.tile(rng.normal(0, 80.0, (n_det, 2)), 2))
    dbox = np.stack([np.minimum(dbox[:, 0], dbox[:, 2]), np.minimum(dbox[:, 1], dbox[:, 3]), np.maximum(dbox[:, 0], dbox[:, 2]), np.maximum(dbox[:, 1], dbox[:, 3])], 1)
    det = {"box": np.ascontiguousarray(dbox), "group": lgroup[src].copy(), "conf": np.round(rng.beta(5.0, 1.5, n_det), 6)}
    lab = {"box": np.ascontiguousarray(lbox), "group": lgroup, "conf": np.ones(n_lab)}
    ocean = rng.random(n_det) < 0.9
    masks = np.stack([np.ones(n_det, bool), ocean, ocean & (rng.random(n_det) < 0.8)], 1)
    return {"det": det, "lab": lab, "years": np.arange(3)}, masks


def bench_population(repeats, numpy_K):
    import numpy as np
    import torch
    from aquaculture_amd import engine, performance
    K, S, rates = performance.DEFAULT_K, 10518, performance.DEFAULT_RATES
    for _ in range(2):
        performance.simulate(K, S, rates, 0)
    torch.cuda.synchronize()
    kernel_ms, select_ms = [], []
    for _ in range(repeats):
        t = {}
        sim = performance.simulate(K, S, rates, 0, times=t)
        kernel_ms.append(t["kernel_ms"]); select_ms.append(t["select_ms"])
    row = {"K": K, "S": S, "rates": len(rates), "all_zeros_50": sim["all_zeros_50"], "zero_share": sim["zero_share"], "kernel_ms": spread(kernel_ms),
           "select_ms": spread(select_ms)}
    row["draws_per_s"] = K * S / (row["kernel_ms"]["median"] * 1e-3)
    k = min(numpy_K, K)
    if k >= 2:
        t0 = time.perf_counter()
        want = performance.counts_numpy(0, 0, k, S, rates)
        dt = (time.perf_counter() - t0) * 1e3
        got = engine.bernoulli_counts(0, 0, k, S, rates).cpu().numpy()
        row["numpy"] = {"K": k, "ms": dt, "ms_scaled_to_K": dt * K / k, "equal_to_gpu": bool(np.array_equal(want, got))}
    print(json.dumps(row), flush=True)
    return row


def bench_joins(n_det, n_lab, repeats, thresholds=100):
    import numpy as np
    import torch
    from aquaculture_amd import performance
    data, masks = synthetic(n_det, n_lab)
    thr = np.linspace(0, 1, thresholds)
    for _ in range(2):
        performance.curve_counts(data, masks, thr)
    torch.cuda.synchronize()
    sort_ms, kernel_ms, call_ms = [], [], []
    for _ in range(repeats):
        t = {}
        t0 = time.perf_counter()
        got = performance.curve_counts(data, masks, thr, times=t)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        sort_ms.append(t["sort_ms"]); kernel_ms.append(t["kernel_ms"])
    t0 = time.perf_counter()
    want = performance.curve_counts(data, masks, thr, cpu=True)
    dt = (time.perf_counter() - t0) * 1e3
    row = {"detections": n_det, "labels": n_lab, "thresholds": thresholds, "true_positives": int(got["tp"].sum()), "sort_ms": spread(sort_ms),
           "kernel_ms": spread(kernel_ms), "call_ms": spread(call_ms),
           "numpy": {"ms": dt, "equal_to_gpu": bool(all(np.array_equal(got[c], want[c]) for c in ("tp", "n_pred", "n_pred_tp", "n_label_tp")))}}
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-K", type=int, default=500, help="simulations the numpy restatement is timed on; fewer than 2 skips it")
    p.add_argument("--detections", type=int, default=100_000, help="the larger join: synthetic detections, against a tenth as many labels")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_performance: no GPU (timings are taken on the device or not at all)")
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "population": bench_population(opt.repeats, opt.numpy_K),
              "joins": [bench_joins(991, 991, opt.repeats), bench_joins(opt.detections, max(1, opt.detections // 10), opt.repeats)]}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
