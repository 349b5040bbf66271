#!/usr/bin/env python3
"""What the grid phase of --evaluate-kfold costs, batched against fold by fold (DESIGN.md section "Cross-validated tuning").

Workload: the detection set tools/bench_evaluate.py builds -- the fixture of tests/test_evaluate.py `--copies` times (default 46: 50,370
detections, 45,586 labels on the fixture's 42 images) --, 5 folds (seed 1, a tenth of the images set aside) and the reference's full grid
(82 x 8 x 10 = 6,560 combinations per fold).  After a warm-up pass of both, `--repeats` times, the two alternating, median and range:

  batched    kfold.fold_grids: per distance one engine.eval_member_conf_subsets and one engine.box_match_subsets over the 5 train bits, and one
             join without payload for the true positives; split into
               sort      torch: the cell sort of every distance and the (group, x0) sorts of the joins (HIP events, summed)
               kernel    the 8 + 9 launches' kernels (HIP events, summed)
               count     torch.sort / searchsorted of M and R for all folds and the copies of the counts to the host (host clock; ends in a
                         synchronise)
               wall      the whole call as a caller sees it, host arrays in, five tables out (host clock, a run without events)
  per fold   the same tables the way the code before this module gives them: evaluate.inputs(images=the fold's train images) and evaluate.grid,
             once per fold; the same four numbers, summed over the folds.  The inputs are built outside the timed window.

The ten tables of the two paths have to be equal; the result says so.

    python tools/bench_kfold.py [--copies 46] [--repeats 5] [--folds 5] [--out result.json]
"""
import argparse
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def run(copies, repeats, folds):
    import numpy as np
    import torch
    from bench_evaluate import scaled_inputs, spread
    from aquaculture_amd import evaluate, kfold
    table, truth = scaled_inputs(copies)
    data = evaluate.inputs(table, truth)
    det_image = [str(table["stems"][i]) for i in table["image"][data["det"]["rows"]]]
    names = sorted({evaluate._stem(s) for s in det_image} | {evaluate._stem(s) for s in truth["image"]})
    images = kfold.image_table(names, det_image, data["det"]["conf"], [str(s) for s in truth["image"][data["lab"]["rows"]]])
    split = kfold.split_images(images["bucket"], folds, 1, 0.1)
    words = kfold.subset_words(split, folds)
    dwords, lwords = words[images["det_row"]], words[images["lab_row"]]
    fold_data = [evaluate.inputs(table, truth, images=[n for n, s in zip(names, split) if s >= 0 and s != f]) for f in range(folds)]
    grids = (evaluate.DEFAULT_CONF, evaluate.DEFAULT_EPS, evaluate.DEFAULT_MIN)
    res = {"device": torch.cuda.get_device_name(0), "detections": int(data["det"]["conf"].shape[0]), "labels": int(data["lab"]["conf"].shape[0]),
           "images": len(names), "folds": folds, "train_detections": [int(d["det"]["conf"].shape[0]) for d in fold_data],
           "combinations_per_fold": int(np.prod([g.shape[0] for g in grids])), "repeats": repeats}

    def batched(times=None):
        return kfold.fold_grids(data, dwords, lwords, folds, *grids, times=times)

    def per_fold(times=None):
        out = []
        for d in fold_data:
            tm = {} if times is not None else None
            out.append(evaluate.grid(d, *grids, times=tm))
            for k, v in (tm or {}).items():
                times[k] = times.get(k, 0.0) + v
        return out

    a, b = batched(), per_fold()                            # warm-up: code objects, torch's sort
    res["tables_equal"] = all(np.array_equal(a[f][c], b[f][c], equal_nan=a[f][c].dtype.kind == "f") for f in range(folds) for c in evaluate.COLUMNS)
    parts = {name: {"sort_ms": [], "kernel_ms": [], "count_ms": [], "wall_ms": []} for name in ("batched", "per_fold")}
    for _ in range(repeats):
        for name, fn in (("batched", batched), ("per_fold", per_fold)):      # alternating: the machine's other work falls on both
            tm = {}
            fn(tm)
            for k in ("sort_ms", "kernel_ms", "count_ms"):
                parts[name][k].append(tm[k])
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            parts[name]["wall_ms"].append((time.perf_counter() - t0) * 1e3)
    for name in parts:
        res[name] = {k: spread(v) for k, v in parts[name].items()}
    res["per_fold_over_batched_wall"] = res["per_fold"]["wall_ms"]["median"] / res["batched"]["wall_ms"]["median"]
    res["per_fold_over_batched_kernel"] = res["per_fold"]["kernel_ms"]["median"] / res["batched"]["kernel_ms"]["median"]
    return res


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--copies", type=int, default=46)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--folds", type=int, default=5)
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_kfold: no GPU (a timing from the CPU says nothing about it)")
    res = run(opt.copies, opt.repeats, opt.folds)
    text = json.dumps(res, indent=1)
    print(text)
    if opt.out:
        os.makedirs(os.path.dirname(os.path.abspath(opt.out)), exist_ok=True)
        with open(opt.out, "w") as f:
            f.write(text + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
