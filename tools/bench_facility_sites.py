#!/usr/bin/env python3
"""What the three device steps of --facility-sites cost.

Workloads:
  fixture     the input of tests/test_facility_sites.py: the 4142 human labels as detections, clustered by pass into 127 facilities, the 13
              known sites inside the download boxes, the labels again as the truth file.  The launches as classify makes them: the facility
              rectangles (127 facilities, 4142 entries), the count join against the sites (127 x 13, one group) and against the labels
              (127 x 4142, six groups), and the list join of all 127 rectangles with themselves (the sets classify joins are smaller).
  synthetic   `--facilities` facilities (default 100,000) of ten cages each on a square lattice 150 m apart, every rectangle some 30 to 210 m
              wide, so that a rectangle meets itself and often a neighbour or two: the rectangles, then the count and the list join of all
              of them with themselves, one group.

Per workload, after a warm-up of every launch, `--repeats` times, median and range:
  kernels     each launch through the library on prepared device tensors, `--inner` launches between two HIP events, per launch
  numpy       the restatements (bounds_numpy, join_count_numpy, join_list_numpy) on the same input, host clock: the baseline, not the code
              under test; their results have to equal the kernels' byte for byte
  classify    (fixture only) facility_sites.classify as a caller sees it, host tables in and out, on the GPU and with cpu=True (host clock)

    python tools/bench_facility_sites.py [--facilities 100000] [--repeats 5] [--inner 200] [--no-synthetic] [--out result.json]
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


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v), "values": list(v)}


def synthetic(F, seed=0):
    """(entry_start, entry_box, entry_use) of F facilities of ten cages on a lattice."""
    import numpy as np
    r = np.random.default_rng(seed)
    side = int(np.ceil(np.sqrt(F)))
    cx, cy = (np.arange(F) % side) * 150.0 + 400000.0, (np.arange(F) // side) * 150.0 + 5300000.0
    reach = r.uniform(15.0, 90.0, F)                         # how far a facility's cages lie from its centre
    at = r.uniform(-1.0, 1.0, (F, 10, 2)) * reach[:, None, None]
    size = r.uniform(10.0, 30.0, (F, 10, 2))
    x0, y0 = cx[:, None] + at[:, :, 0], cy[:, None] + at[:, :, 1]
    box = np.stack([x0, y0, x0 + size[:, :, 0], y0 + size[:, :, 1]], 2).reshape(-1, 4)
    return np.arange(F + 1, dtype=np.int32) * 10, np.ascontiguousarray(box), np.ones(F * 10, np.uint8)


class Launches:
    """The device tensors of one workload and its launches through the library."""

    def __init__(self, entry_start, entry_box, entry_use):
        import numpy as np
        import torch
        from aquaculture_amd import engine
        self.np, self.torch, self.engine, self.lib = np, torch, engine, engine.load_library()
        self.dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
        self.start_h = np.ascontiguousarray(entry_start, dtype=np.int32)
        self.start, self.box, self.use = self.dev(self.start_h, np.int32), self.dev(entry_box, np.float64), self.dev(entry_use, np.uint8)
        self.F, self.E = self.start_h.shape[0] - 1, int(self.box.shape[0])
        self.bounds = torch.empty((self.F, 4), dtype=torch.float64, device="cuda")
        self.joins = {}

    def stream(self):
        return self.torch.cuda.current_stream().cuda_stream

    def run_bounds(self):
        rc = self.lib.aq_facility_bounds_f64(self.start.data_ptr(), self.start_h.ctypes.data, self.F, self.box.data_ptr(), self.use.data_ptr(), self.E,
                                             self.bounds.data_ptr(), self.stream())
        assert rc == 0, self.lib.aq_last_error()

    def add_join(self, name, qbox, qgroup, kbox, kgroup, G):
        """Prepares the join `name`: the sorted keys, the counts and, from them, the offsets and the list."""
        torch, np = self.torch, self.np
        q, g = self.dev(qbox, np.float64), self.dev(qgroup, np.int32)
        keys = self.engine.box_join_keys(self.dev(kbox, np.float64), self.dev(kgroup, np.int32), G)
        count, first = self.engine.box_join_count(q, g, keys=keys)
        offset_h, lst = self.engine.box_join_list(q, g, keys=keys, count=count)
        ptr = lambda t: t.data_ptr() if t.numel() else None
        head = (ptr(q), ptr(g), int(q.shape[0]), ptr(keys["box"]), ptr(keys["kid"]), keys["start"].data_ptr(), keys["start_host"].ctypes.data, keys["N"], keys["G"])
        self.joins[name] = {"q": q, "g": g, "keys": keys, "count": count, "first": first, "offset_h": offset_h, "offset": self.dev(offset_h, np.int64),
                            "list": lst, "head": head, "ptr": ptr}
        return self.joins[name]

    def run_count(self, name):
        j = self.joins[name]
        rc = self.lib.aq_box_join_count_i32(*j["head"], j["ptr"](j["count"]), j["ptr"](j["first"]), self.stream())
        assert rc == 0, self.lib.aq_last_error()

    def run_list(self, name):
        j = self.joins[name]
        rc = self.lib.aq_box_join_list_i32(*j["head"], j["offset"].data_ptr(), j["offset_h"].ctypes.data, j["ptr"](j["list"]), int(j["offset_h"][-1]), self.stream())
        assert rc == 0, self.lib.aq_last_error()

    def time(self, fn, inner, repeats):
        """Microseconds per launch: `inner` launches between two HIP events, `repeats` times, after a warm-up."""
        torch = self.torch
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        out = []
        for _ in range(repeats):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(inner):
                fn()
            b.record()
            b.synchronize()
            out.append(a.elapsed_time(b) * 1e3 / inner)
        return spread(out)


def host_time(fn, repeats):
    times, res = [], None
    for _ in range(repeats):
        t0 = time.perf_counter()
        res = fn()
        times.append((time.perf_counter() - t0) * 1e3)
    return spread(times), res


def run_fixture(repeats, inner):
    import numpy as np
    import torch
    import test_facility_sites as fx
    from aquaculture_amd import evaluate, facility_sites as fs
    fac, table, sites, truth = fx.fixture_facilities(), fx.fixture_table(), fx.fixture_sites(), fx.fixture_truth()
    ent = fs.entries(fac, table)
    L = Launches(*ent)
    L.run_bounds()
    bounds = L.bounds.cpu().numpy()
    F = bounds.shape[0]
    group = np.asarray([fs.PASSES.index(p) for p in fs.facility_passes(fac)], np.int32)
    lg = fs.label_groups(truth)
    lbox = np.stack([truth[c] for c in evaluate.BOX_COLUMNS], 1)
    zero = np.zeros(F, np.int32)
    joins = {"sites": (bounds, zero, sites["box"], np.zeros(sites["box"].shape[0], np.int32), 1), "labels": (bounds, group, lbox, lg.astype(np.int32), len(fs.PASSES)),
             "self": (bounds, zero, bounds, zero, 1)}
    for name, args in joins.items():
        L.add_join(name, *args)
    out = {"facilities": F, "entries": L.E, "sites": int(sites["box"].shape[0]), "labels": int(lbox.shape[0]),
           "self_list_entries": int(L.joins["self"]["offset_h"][-1]),
           "bounds_us": L.time(L.run_bounds, inner, repeats),
           "count_sites_us": L.time(lambda: L.run_count("sites"), inner, repeats), "count_labels_us": L.time(lambda: L.run_count("labels"), inner, repeats),
           "list_self_us": L.time(lambda: L.run_list("self"), inner, repeats)}
    t, want_b = host_time(lambda: fs.bounds_numpy(*ent), repeats)
    out["numpy_bounds_ms"] = t
    t, want_s = host_time(lambda: fs.join_count_numpy(*joins["sites"]), repeats)
    out["numpy_count_sites_ms"] = t
    t, want_l = host_time(lambda: fs.join_count_numpy(*joins["labels"]), repeats)
    out["numpy_count_labels_ms"] = t
    t, want_self = host_time(lambda: fs.join_list_numpy(*joins["self"]), repeats)
    out["numpy_list_self_ms"] = t
    torch.cuda.synchronize()
    same = [bounds.tobytes() == want_b.tobytes()]
    for name, want in (("sites", want_s), ("labels", want_l)):
        same += [L.joins[name]["count"].cpu().numpy().tobytes() == want[0].tobytes(), L.joins[name]["first"].cpu().numpy().tobytes() == want[1].tobytes()]
    same += [L.joins["self"]["offset_h"].tobytes() == want_self[0].tobytes(), L.joins["self"]["list"].cpu().numpy().tobytes() == want_self[1].tobytes()]
    out["numpy_equals_gpu"] = all(same)
    fs.classify(fac, table, sites, truth)                   # warm-up: torch's sort at these sizes
    out["classify_gpu_ms"], res = host_time(lambda: fs.classify(fac, table, sites, truth), repeats)
    out["classify_cpu_ms"], want = host_time(lambda: fs.classify(fac, table, sites, truth, cpu=True), repeats)
    out["classify_equal"] = res["state"] == want["state"] and res["bounds"].tobytes() == want["bounds"].tobytes() and res["location"] == want["location"]
    return out


def run_synthetic(F, repeats, inner):
    import numpy as np
    from aquaculture_amd import facility_sites as fs
    ent = synthetic(F)
    L = Launches(*ent)
    L.run_bounds()
    bounds = L.bounds.cpu().numpy()
    zero = np.zeros(F, np.int32)
    j = L.add_join("self", bounds, zero, bounds, zero, 1)
    out = {"facilities": F, "entries": L.E, "list_entries": int(j["offset_h"][-1]), "longest_list": int(np.diff(j["offset_h"]).max()),
           "bounds_us": L.time(L.run_bounds, inner, repeats), "count_self_us": L.time(lambda: L.run_count("self"), inner, repeats),
           "list_self_us": L.time(lambda: L.run_list("self"), inner, repeats)}
    t, want_b = host_time(lambda: fs.bounds_numpy(*ent), max(1, repeats // 2))
    out["numpy_bounds_ms"] = t
    t, want = host_time(lambda: fs.join_list_numpy(bounds, zero, bounds, zero, 1), max(1, repeats // 2))
    out["numpy_list_self_ms"] = t
    out["numpy_equals_gpu"] = (bounds.tobytes() == want_b.tobytes() and j["offset_h"].tobytes() == want[0].tobytes() and
                               j["list"].cpu().numpy().tobytes() == want[1].tobytes())
    return out


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--facilities", type=int, default=100000)
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--inner", type=int, default=200)
    p.add_argument("--no-synthetic", action="store_true")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        sys.exit("bench_facility_sites: no GPU: the kernels cannot be timed here")
    res = {"device": torch.cuda.get_device_name(0), "repeats": opt.repeats, "inner": opt.inner, "fixture": run_fixture(opt.repeats, opt.inner)}
    if not opt.no_synthetic:
        res["synthetic"] = run_synthetic(opt.facilities, opt.repeats, max(1, opt.inner // 10))
    line = json.dumps(res)
    print(line)
    if opt.out:
        with open(opt.out, "w") as f:
            f.write(line + "\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
