#!/usr/bin/env python3
"""What the overlap de-duplication of --dedup-overlaps costs.

Workload, the reference's size: `--boxes` download boxes (4,545) -- the 375 boxes of the reference's own file that overlap another
(tests/golden/g15_wanted_bboxes.csv, in their order and with their overlaps: 194 with earlier partners, at most 8, 97 without a region),
then 1200 m boxes side by side on a grid away from them, as the rest of that file is -- and `--detections` boxes of 5 to 30 m, each in a
random download box, `--overlap-share` of them (at least 5 %) placed on the overlap of a box with one of its earlier partners.  After
warm-up, `--repeats` times, median and range:

  partners   aq_overlap_partners_f64, both calls (count + scan, fill) through the default band table (HIP events; the host's read of the
             list size lies between them)
  one_band   the same with one band: every box walks every earlier box -- the kernel without a search structure
  clip       aq_overlap_clip_f64: its two launches, the boxes' has_region and the detections (HIP events)
  clip_gpu   overlaps.clip_gpu as a caller sees it: host arrays in, host arrays out (host clock; includes the copies)
  tables     overlaps.band_table and overlaps.partners_numpy on the host
  numpy      overlaps.clip_numpy for the first `--numpy-detections` detections (whole arrays for the detections of boxes without partners,
             a Python walk for the others; the figure per detection is printed beside it), and whether the GPU's bytes equal it there

    python tools/bench_overlaps.py [--boxes 4545] [--detections 1000000] [--overlap-share 0.08] [--repeats 5] [--out result.json]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SIDE = 1200.0


def problem(n_boxes, n_dets, share, seed=0):
    import numpy as np
    from aquaculture_amd import overlaps
    rng = np.random.default_rng(seed)
    _, boxes = overlaps.load_boxes(os.path.join(ROOT, "tests", "golden", "g15_wanted_bboxes.csv"))
    boxes = boxes[:n_boxes]
    rest = n_boxes - boxes.shape[0]
    if rest > 0:                                            # a grid of 64 columns north of everything in the fixture
        k = np.arange(rest)
        x, y = boxes[:, 0].min() + SIDE * (k % 64), boxes[:, 3].max() + 10 * SIDE + SIDE * (k // 64)
        boxes = np.concatenate([boxes, np.stack([x, y, x + SIDE, y + SIDE], 1)], 0)
    start, partner = overlaps.partners_numpy(boxes)
    with_partner = np.nonzero(np.diff(start) > 0)[0]
    size = rng.uniform(5.0, 30.0, (n_dets, 2))
    row = rng.integers(0, n_boxes, n_dets)
    lo, hi = boxes[row, :2], boxes[row, 2:] - size
    n_over = int(round(share * n_dets)) if with_partner.size else 0
    if n_over:
        i = rng.choice(with_partner, n_over)
        j = partner[start[i] + (rng.random(n_over) * (start[i + 1] - start[i])).astype(np.int64)]
        row[:n_over] = i
        lo[:n_over] = np.maximum(boxes[i, :2], boxes[j, :2]) - size[:n_over] / 2          # on the overlap, across its sides too
        hi[:n_over] = np.minimum(boxes[i, 2:], boxes[j, 2:]) - size[:n_over] / 2
    c = lo + rng.random((n_dets, 2)) * (hi - lo)
    order = rng.permutation(n_dets)
    dets = np.ascontiguousarray(np.concatenate([c, c + size], 1)[order])
    return np.ascontiguousarray(boxes), row[order].astype(np.int32), dets, n_over


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(opt):
    import numpy as np
    import torch
    from aquaculture_amd import engine, overlaps
    boxes, det_row, dets, n_over = problem(opt.boxes, opt.detections, opt.overlap_share)
    t0 = time.perf_counter()
    table = overlaps.band_table(boxes)
    table_ms = (time.perf_counter() - t0) * 1e3
    t0 = time.perf_counter()
    want_start, want_partner = overlaps.partners_numpy(boxes)
    partners_numpy_ms = (time.perf_counter() - t0) * 1e3
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    b, r, d = dev(boxes), dev(det_row), dev(dets)
    result = {}
    for name, t in (("partners", table), ("one_band", overlaps.band_table(boxes, 1))):
        e, s = dev(t["entry_box"]), dev(t["band_start"])
        launch = lambda times=None: engine.overlap_partners(b, e, s, t["nbands"], t["Y0"], t["h"], times=times)
        for _ in range(2):
            launch()
        torch.cuda.synchronize()
        ms_ = []
        for _ in range(opt.repeats):
            times = {}
            start, partner = launch(times)
            ms_.append(times["partners_ms"])
        per_band = np.diff(t["band_start"].astype(np.int64))
        result[name] = {"ms": spread(ms_), "bands": int(t["nbands"]), "entries": int(t["entry_box"].shape[0]),
                        "entries_per_band": {"mean": float(per_band.mean()), "max": int(per_band.max())},
                        "equal_to_numpy": bool(np.array_equal(start.cpu().numpy(), want_start) and np.array_equal(partner.cpu().numpy(), want_partner))}
    for _ in range(2):
        engine.overlap_clip(b, start, partner, r, d)
    torch.cuda.synchronize()
    clip_ms = []
    for _ in range(opt.repeats):
        times = {}
        out = engine.overlap_clip(b, start, partner, r, d, times=times)
        clip_ms.append(times["clip_ms"])
    state = out[0].cpu().numpy()
    host_ms = []
    for _ in range(opt.repeats):
        t0 = time.perf_counter()
        got = overlaps.clip_gpu(boxes, want_start, want_partner, det_row, dets)
        host_ms.append((time.perf_counter() - t0) * 1e3)
    counts = np.bincount(state, minlength=4)
    row = {"boxes": int(boxes.shape[0]), "boxes_with_partners": int((np.diff(want_start) > 0).sum()), "partners_max": int(np.diff(want_start).max()),
           "boxes_dropped": int((got["has_region"] == 0).sum()), "detections": int(dets.shape[0]), "placed_on_overlaps": n_over,
           "states": {n_: int(counts[k]) for k, n_ in enumerate(overlaps.STATE_NAMES)}, **result, "clip": {"ms": spread(clip_ms)},
           "clip_gpu_ms": spread(host_ms), "band_table_ms": table_ms, "partners_numpy_ms": partners_numpy_ms}
    k = min(opt.numpy_detections, dets.shape[0])
    if k > 0:
        t0 = time.perf_counter()
        want = overlaps.clip_numpy(boxes, want_start, want_partner, det_row[:k], dets[:k])
        dt = (time.perf_counter() - t0) * 1e3
        row["numpy"] = {"detections": k, "ms": dt, "ms_per_detection": dt / k,
                        "equal_to_gpu": bool(all(want[c].tobytes() == got[c][:k].tobytes() for c in ("state", "clip_bounds", "clip_area"))
                                             and want["has_region"].tobytes() == got["has_region"].tobytes())}
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--boxes", type=int, default=4545)
    p.add_argument("--detections", type=int, default=1_000_000)
    p.add_argument("--overlap-share", type=float, default=0.08, help="share of the detections placed on overlaps")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--numpy-detections", type=int, default=100_000, help="detections the numpy path is timed on; 0 skips it")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_overlaps: no GPU (timings are taken on the device or not at all)")
    row = run(opt)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "row": row}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
