#!/usr/bin/env python3
"""What the production bootstrap of --tonnage costs.

Workload: a synthetic facility table of `--facilities` facilities and `--entries` cage entries (facility sizes drawn between 5 and several
hundred, all three cage kinds, a model error of sd 20 m^2 on areas of 60 to 400 m^2, six passes), `--K` simulations.  After warm-up,
`--repeats` times, median and range:

  gpu         tonnage.simulate on the GPU as a caller sees it: the chunks' kernels (simulate, pass sums, moments), T copied back; host clock
              around work that ends in a device synchronise
  kernels     the same chunks' launches alone (HIP events)
  numpy       the restatement (tonnage.simulate with cpu=True) at --numpy-K simulations, once; reported per simulation and scaled to --K
  pandas      a literal per-iteration loop in the reference's style -- a DataFrame copy, explode / merge of the facility-cage table, numpy and
              scipy.stats.truncnorm draws, groupby sums -- at --pandas-K iterations, once; reported per iteration and scaled to --K

and whether the GPU's T equals the restatement's on the first --numpy-K simulations, bit for bit.

    python tools/bench_tonnage.py [--facilities 500] [--entries 20000] [--K 10000] [--repeats 5] [--numpy-K 200] [--pandas-K 20] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PASSES = ("2000-2004", "2005-2009", "2010-2012", "2013-2015", "2016-2018", "2019-2021")


def synthetic_table(F, E, seed=0):
    import numpy as np
    from aquaculture_amd import tonnage as tn
    r = np.random.default_rng(seed)
    w = r.lognormal(0.0, 1.0, F)
    sizes = 5 + np.floor(w / w.sum() * (E - 5 * F)).astype(np.int64)
    sizes[: E - int(sizes.sum())] += 1
    start = np.concatenate([[0], np.cumsum(sizes)])
    kind = r.integers(0, 3, E)
    params = tn.pass_params(r.uniform(10, 16, 6), r.uniform(2, 4, 6), r.uniform(0.6, 1.0, 6), r.uniform(0.05, 0.2, 6))
    return tn.make_table(start, r.uniform(60.0, 400.0, E), r.uniform(-5, 5, E), np.full(E, 20.0), kind, np.full(E, tn.SEL_MIN | tn.SEL_MAX | tn.SEL_RANDOM),
                         r.uniform(2.0, 12.0, F), r.integers(0, 6, F), params)


def pandas_loop(t, K):
    """The reference's loop shape (src/utils_tonnage.py:57-113, :330-458) on the same table: per iteration a frame copy, the exploded
    facility-cage table merged with the cages and the error table, the draws, the groupby sums."""
    import numpy as np
    import pandas as pd
    from scipy.stats import truncnorm
    F = t["depth"].shape[0]
    sizes = np.diff(t["entry_start"])
    cage_ids = [list(range(int(a), int(b))) for a, b in zip(t["entry_start"][:-1], t["entry_start"][1:])]
    q = t["params"][t["pass_id"]]
    fac = pd.DataFrame({"facility_index": np.arange(F), "cage_ids": cage_ids, "pass": [PASSES[p] for p in t["pass_id"]], "cage_depth": t["depth"],
                        "s_mean": q[:, 0], "s_sd": q[:, 1], "h_mean": q[:, 4], "h_sd": q[:, 5]})
    kind = t["flags"] & 3
    cages = pd.DataFrame({"index": np.arange(t["area"].shape[0]), "farm_type": np.where(kind == 2, "square_farm", "circle_farm"),
                          "pass": np.repeat(fac["pass"].to_numpy(), sizes), "area": t["area"], "area_var": np.where(kind == 0, 0.0, 1.0)})
    errs = pd.DataFrame([(p, ft, 0.0, 20.0) for p in PASSES for ft in ("circle_farm", "square_farm")],
                        columns=["pass", "farm_type", "model_error_mean", "model_error_sd"])
    m = t["min_depth"]
    tonnage = {p: [] for p in fac["pass"].unique()}
    for _ in range(K):
        sim = fac.copy()
        fc = sim[["facility_index", "cage_ids"]].explode("cage_ids")
        fc["cage_ids"] = fc["cage_ids"].astype(int)
        fc = fc.merge(cages, how="left", left_on="cage_ids", right_on="index", validate="one_to_one")
        fc = fc.merge(errs, how="left", on=["pass", "farm_type"], validate="many_to_one")
        fc["new"] = fc["area"] + np.random.normal(loc=fc["model_error_mean"], scale=fc["model_error_sd"])
        while fc["new"].min() <= 0:
            e = np.random.normal(loc=fc["model_error_mean"], scale=fc["model_error_sd"])
            fc["new"] = np.where(fc["new"] <= 0, fc["area"] + e, fc["new"])
        full, sq = (fc["farm_type"] == "circle_farm") & (fc["area_var"] == 0.0), fc["farm_type"] == "square_farm"
        fc["min_area"] = np.where(full, fc["new"], np.where(sq, 2 * fc["new"] / 3, 4 * fc["new"] / (2 + np.pi)))
        fc["max_area"] = np.where(full, fc["new"], np.where(sq, 4 * fc["new"] / 3, 2 * np.pi * fc["new"] / (2 + np.pi)))
        sim = sim.merge(fc.groupby("facility_index")[["min_area", "max_area"]].sum().reset_index(), how="left", on="facility_index", validate="one_to_one")
        sim["sim_area"] = np.random.uniform(low=sim["min_area"], high=sim["max_area"])
        sim["b"] = np.random.binomial(n=1, p=t["mix"], size=len(sim))
        d = sim["cage_depth"]
        sim["dA"] = truncnorm.rvs(loc=d, scale=(d - m) / 1.96, a=(m - d) / ((d - m) / 1.96), b=0)
        sim["dB"] = truncnorm.rvs(loc=d, scale=d / 1.96, a=0, b=d / (d / 1.96))
        sim["depth"] = np.where(sim["b"] == 1, sim["dA"], sim["dB"])
        sim["st"] = truncnorm.rvs(loc=sim["s_mean"], scale=sim["s_sd"], a=(5 - sim["s_mean"]) / sim["s_sd"], b=(20 - sim["s_mean"]) / sim["s_sd"])
        sim["hv"] = np.random.normal(loc=sim["h_mean"], scale=sim["h_sd"])
        sim["ton"] = sim["sim_area"] * sim["depth"] * sim["st"]
        sim["ton"] *= sim["hv"] * (1 / 1000)
        per = sim.groupby("pass")["ton"].sum()
        for p in tonnage:
            tonnage[p].append(per[p])
    return {p: float(np.mean(v)) for p, v in tonnage.items()}


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--facilities", type=int, default=500)
    p.add_argument("--entries", type=int, default=20000)
    p.add_argument("--K", type=int, default=10000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-K", type=int, default=200)
    p.add_argument("--pandas-K", type=int, default=20)
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import numpy as np
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_tonnage: no GPU (timings are taken on the device or not at all)")
    from aquaculture_amd import engine, tonnage as tn
    t = synthetic_table(opt.facilities, opt.entries)
    F = opt.facilities
    for _ in range(2):
        res = tn.simulate(t, opt.K, 1)
    torch.cuda.synchronize()
    gpu_ms, kernel_ms = [], []
    dev = {k: torch.from_numpy(t[k]).cuda() for k in ("entry_start", "area", "err", "flags", "depth", "pass_id", "params")}
    for _ in range(opt.repeats):
        t0 = time.perf_counter()
        res = tn.simulate(t, opt.K, 1)                      # ends in the copies of T and the moments: synchronised
        gpu_ms.append((time.perf_counter() - t0) * 1e3)
        mom = torch.zeros((F, 2), dtype=torch.float64, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(2)]
        ev[0].record()
        at = 0
        for n in tn.chunk_sizes(opt.K, F):
            engine.tonnage_simulate(1, at, n, dev["entry_start"], dev["area"], dev["err"], dev["flags"], dev["depth"], dev["pass_id"], dev["params"],
                                    t["mix"], t["min_depth"], t["probs"], mom, t["entry_start"], t["params"])
            at += n
        ev[1].record()
        ev[1].synchronize()
        kernel_ms.append(ev[0].elapsed_time(ev[1]))
    t0 = time.perf_counter()
    cpu = tn.simulate(t, opt.numpy_K, 1, cpu=True)
    numpy_s = time.perf_counter() - t0
    t0 = time.perf_counter()
    pandas_loop(t, opt.pandas_K)
    pandas_s = time.perf_counter() - t0
    g = statistics.median(gpu_ms) / 1e3
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "facilities": F, "entries": opt.entries, "K": opt.K,
              "draws_per_simulation": opt.entries + 5 * F, "gpu_ms": spread(gpu_ms), "kernels_ms": spread(kernel_ms),
              "numpy_K": opt.numpy_K, "numpy_ms_per_simulation": numpy_s / opt.numpy_K * 1e3, "numpy_s_at_K": numpy_s / opt.numpy_K * opt.K,
              "pandas_K": opt.pandas_K, "pandas_ms_per_iteration": pandas_s / opt.pandas_K * 1e3, "pandas_s_at_K": pandas_s / opt.pandas_K * opt.K,
              "numpy_over_gpu": numpy_s / opt.numpy_K * opt.K / g, "pandas_over_gpu": pandas_s / opt.pandas_K * opt.K / g,
              "equal_to_numpy": bool(np.array_equal(res["T"][:opt.numpy_K].view(np.uint64), cpu["T"].view(np.uint64)))}
    print(json.dumps(result), flush=True)
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
