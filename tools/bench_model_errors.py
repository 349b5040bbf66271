#!/usr/bin/env python3
"""What the model-error table of --model-errors costs.

Workload: the fixture of tests/test_model_errors.py -- the 991 human labels of two scenes and one jittered detection per label -- copied,
every copy with a seed of its own and shifted 20 km east of the last so that copies never interact, and cut to `--labels` labels and as
many detections: 4,142, the size of the reference's output/humanlabels.geojson, and ten times that.  Per size, after a warm-up pass,
`--repeats` times, median and range:

  sort           torch: the (group, x0) sort of the labels (HIP events)
  kernel         aq_model_error_match_f64 and aq_model_error_moments_f64 (HIP events, summed)
  distributions  model_errors.distributions as a caller sees it, host tables in, table out (host clock; it ends in copies to the host)
  cpu            model_errors.distributions(cpu=True), the numpy restatement (brute force per group), the same repeats (skipped with
                 --no-cpu); its match, error, n, mean and sd have to equal the GPU's byte for byte

    python tools/bench_model_errors.py [--labels 4142 41420] [--repeats 5] [--no-cpu] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scaled_inputs(labels):
    """(table, truth) of `labels` labels and detections: shifted copies of the tests' fixture, cut to size."""
    import numpy as np
    import test_model_errors as fx
    t = fx.truth()
    copies = -(-labels // t["cls"].shape[0])
    tables, truths = [], []
    for c in range(copies):
        d = fx.detection_table(c)
        shift = 20000.0 * c
        tables.append({**d, "xmin_3857": d["xmin_3857"] + shift, "xmax_3857": d["xmax_3857"] + shift})
        truths.append({**t, "xmin_3857": t["xmin_3857"] + shift, "xmax_3857": t["xmax_3857"] + shift})
    cat = lambda parts, k: np.concatenate([p[k] for p in parts])[:labels]
    table = {k: cat(tables, k) for k in tables[0] if k != "stems"}
    table["stems"] = tables[0]["stems"]
    from aquaculture_amd import geocode                      # the EPSG:3035 corners of the shifted boxes, as geocode_detections makes them
    table["e_min_3035"], table["n_max_3035"] = geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(table["xmin_3857"], table["ymax_3857"]))
    table["e_max_3035"], table["n_min_3035"] = geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(table["xmax_3857"], table["ymin_3857"]))
    truth ={k: cat(truths, k) for k in truths[0]}
    return table, truth


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "values": list(v)}


def run_size(labels, repeats, cpu):
    import torch
    from aquaculture_amd import model_errors
    table, truth = scaled_inputs(labels)
    conf = 0.5
    model_errors.distributions(table, truth, conf)          # warm-up: code objects, torch's sort
    parts = {"sort_ms": [], "kernel_ms": [], "distributions_ms": []}
    res = None
    for _ in range(repeats):
        tm = {}
        model_errors.distributions(table, truth, conf, times=tm)
        parts["sort_ms"].append(tm["sort_ms"])
        parts["kernel_ms"].append(tm["kernel_ms"])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        res = model_errors.distributions(table, truth, conf)
        parts["distributions_ms"].append((time.perf_counter() - t0) * 1e3)
    out = {"labels": res["n_labels"], "detections": res["n_queries"], "matched": res["n_matched"], "groups": len(res["errors"]),
           **{k: spread(v) for k, v in parts.items()}}
    if cpu:
        times, want = [], None
        for _ in range(repeats):
            t0 = time.perf_counter()
            want = model_errors.distributions(table, truth, conf, cpu=True)
            times.append((time.perf_counter() - t0) * 1e3)
        out["cpu_distributions_ms"] = spread(times)
        out["cpu_equals_gpu"] = all(res[k].tobytes() == want[k].tobytes() for k in ("match", "overlap", "error", "n", "mean", "sd"))
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--labels", type=int, nargs="+", default=[4142, 41420])
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_model_errors: no GPU (a timing from the CPU says nothing about it)")
    res = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats, "sizes": [run_size(n, opt.repeats, not opt.no_cpu) for n in opt.labels]}
    text = json.dumps(res, indent=1)
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
