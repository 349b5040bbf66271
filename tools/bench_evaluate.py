#!/usr/bin/env python3
"""What the precision / recall grid of --evaluate costs.

Workload: the fixture of tests/test_evaluate.py -- the 991 human labels of two scenes and 1,095 detections derived from them by the tests'
seeded rule -- `--copies` times (default 46: 50,370 detections, 45,586 labels), every copy with a seed of its own and shifted 20 km east
of the last, so that copies never interact; the reference's full grid (82 x 8 x 10 = 6,560 combinations).  After a warm-up pass,
`--repeats` times, median and range:

  sort       torch: the cell sort of every distance and the (group, x0) sorts of the joins (HIP events, summed over the grid)
  kernel     aq_eval_member_conf_f64 for the 8 distances and the 9 aq_box_match_f64 joins (HIP events, summed)
  count      torch.sort / searchsorted of M and R and the copies of the counts to the host (host clock; ends in a synchronise)
  grid       evaluate.grid as a caller sees it, host arrays in, table out (host clock, a run without events)
  files      cluster_performance.csv and evaluation.json (host clock), with the operating point's time beside it

and for comparison, each once:

  per-combination   `--sample` combinations spread over the grid done the only way the code before this module could: filter by
                    confidence, engine.facility_dbscan, members, a numpy join both ways.  The sample's time is SCALED to the grid's 6,560
                    combinations and labelled so; its counts have to equal the grid's rows.
  cpu               evaluate.grid(cpu=True), the numpy / scipy restatement (skipped with --no-cpu); its table has to equal the GPU's.

    python tools/bench_evaluate.py [--copies 46] [--repeats 5] [--sample 8] [--no-cpu] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def scaled_inputs(copies):
    """(table, truth) of `copies` shifted copies of the tests' fixture."""
    import numpy as np
    import test_evaluate as fx
    from aquaculture_amd import evaluate
    t = fx.truth()
    tables, truths = [], []
    for c in range(copies):
        d = fx.detection_table(fx.SEED + c)
        shift = 20000.0 * c
        tables.append({**d, "xmin_3857": d["xmin_3857"] + shift, "xmax_3857": d["xmax_3857"] + shift})
        truths.append({**t, "xmin_3857": t["xmin_3857"] + shift, "xmax_3857": t["xmax_3857"] + shift})
    cat = lambda parts, k: np.concatenate([p[k] for p in parts])
    table = {k: cat(tables, k) for k in ("cls", "det_conf", "year", "image", *evaluate.BOX_COLUMNS)}
    table["stems"] = tables[0]["stems"]
    truth = {k: cat(truths, k) for k in ("cls", "year", "image", *evaluate.BOX_COLUMNS)}
    return table, truth


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "values": list(v)}


def per_combination(data, conf, eps, m):
    """One grid point without this module's kernels -> the four counts."""
    import numpy as np
    import torch
    from aquaculture_amd import engine, evaluate
    det, lab = data["det"], data["lab"]
    take = np.nonzero(det["conf"] >= conf)[0]
    member = np.zeros(det["conf"].shape[0], bool)
    if take.shape[0]:
        _, root = engine.facility_dbscan(torch.from_numpy(det["xy"][take]).cuda(), torch.from_numpy(det["year_id"][take]).cuda(), float(eps), int(m))
        member[take[root.cpu().numpy() >= 0]] = True
    mbox, mgroup = det["box"][member], det["group"][member]
    tp = evaluate.box_match_numpy(mbox, mgroup, lab["box"], lab["group"])[0]
    ltp = evaluate.box_match_numpy(lab["box"], lab["group"], mbox, mgroup)[0]
    return int(member.sum()), int(tp.sum()), int(lab["conf"].shape[0]), int(ltp.sum())


def run(copies, repeats, sample, cpu):
    import numpy as np
    import torch
    from aquaculture_amd import evaluate
    table, truth = scaled_inputs(copies)
    data = evaluate.inputs(table, truth)
    n, L = int(data["det"]["conf"].shape[0]), int(data["lab"]["conf"].shape[0])
    rows = evaluate.DEFAULT_CONF.shape[0] * evaluate.DEFAULT_EPS.shape[0] * evaluate.DEFAULT_MIN.shape[0]
    res = {"device": torch.cuda.get_device_name(0), "detections": n, "labels": L, "combinations": rows, "repeats": repeats}
    evaluate.grid(data)                                     # warm-up: code objects, torch's sort
    parts = {"sort_ms": [], "kernel_ms": [], "count_ms": [], "grid_ms": []}
    g = None
    for _ in range(repeats):
        tm = {}
        evaluate.grid(data, times=tm)
        for k in ("sort_ms", "kernel_ms", "count_ms"):
            parts[k].append(tm[k])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        g = evaluate.grid(data)
        parts["grid_ms"].append((time.perf_counter() - t0) * 1e3)
    res.update({k: spread(v) for k, v in parts.items()})
    t0 = time.perf_counter()
    op = evaluate.operating_point(data, 0.785, 50.0, 5)
    res["operating_point_ms"] = (time.perf_counter() - t0) * 1e3
    with tempfile.TemporaryDirectory() as d:
        t0 = time.perf_counter()
        evaluate.write_performance_csv(os.path.join(d, evaluate.CSV_FILE), g)
        with open(os.path.join(d, evaluate.JSON_FILE), "w") as f:
            json.dump(evaluate.summary(data, g, op), f, indent=1)
        res["files_ms"] = (time.perf_counter() - t0) * 1e3
    best = evaluate.idxmax(g["f_score"])
    res["best_f_score"] = {c: (float(g[c][best]) if g[c].dtype.kind == "f" else int(g[c][best])) for c in evaluate.COLUMNS}

    picks = [int(k) for k in np.linspace(0, rows - 1, sample).round()]
    per_combination(data, float(g["conf_thresh"][picks[0]]), float(g["distance_threshold"][picks[0]]), int(g["min_cluster_size"][picks[0]]))     # warm-up
    t0 = time.perf_counter()
    same = True
    for k in picks:
        got = per_combination(data, float(g["conf_thresh"][k]), float(g["distance_threshold"][k]), int(g["min_cluster_size"][k]))
        same &= got == tuple(int(g[c][k]) for c in ("n_pred", "n_pred_tp", "n_label", "n_label_tp"))
    sample_ms = (time.perf_counter() - t0) * 1e3
    res["per_combination"] = {"sample": len(picks), "sample_ms": sample_ms, "scaled_to_grid_ms": sample_ms * rows / len(picks),
                              "scaled": True, "counts_equal_grid_rows": bool(same)}
    if cpu:
        t0 = time.perf_counter()
        gc = evaluate.grid(data, cpu=True)
        res["cpu_grid_ms"] = (time.perf_counter() - t0) * 1e3
        res["cpu_table_equals_gpu"] = all(np.array_equal(g[c], gc[c], equal_nan=g[c].dtype.kind == "f") for c in evaluate.COLUMNS)
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--copies", type=int, default=46)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--sample", type=int, default=8)
    p.add_argument("--no-cpu", action="store_true")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_evaluate: no GPU (a timing from the CPU says nothing about it)")
    res = run(opt.copies, opt.repeats, opt.sample, not opt.no_cpu)
    text = json.dumps(res, indent=1)
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
