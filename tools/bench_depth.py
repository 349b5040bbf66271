#!/usr/bin/env python3
"""What the facility depths of --bathymetry cost.

Workload: a synthetic depth raster of `--rows` x `--cols` cells of 1/960 degree (EMODnet's grid; one of its tiles holds some 80 M
numbers), written as an ESRI ASCII grid with two decimals as EMODnet writes them and, for the GeoTIFF reader, as a float32 GeoTIFF; and
`--facilities` facilities of 5 to `--max-cages` cages of 10 to 40 m, the cages of one facility within some 150 m of its centre, the
centres along a band of the raster `--span` of its width and height.  After warm-up, `--repeats` times, median and range:

  read     bathymetry.load_window: the header, the rows down to the window's last parsed from the text (or the TIFF decoded), the
           window cut out (host clock); the window bounds all cages, so its size follows from --span
  upload   the window, float32, to the device (host clock around a synchronise)
  ranges   aq_depth_ranges_f64 (HIP events)
  stats    aq_depth_stats_f64 (HIP events); between the two the windows come back and the bitmap is laid out
  call     bathymetry.stats_gpu as a caller sees it: host arrays in, host arrays out, upload included (host clock)
  numpy    bathymetry.stats_numpy on the same host, and whether the GPU's bytes equal it

    python tools/bench_depth.py [--rows 9000] [--cols 9000] [--facilities 3000] [--max-cages 60] [--span 0.5] [--repeats 5] [--dir DIR] [--out result.json]
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

CELL = 1.0 / 960
X0, Y0 = 2.0, 44.0                                          # the raster's north-west corner


def synthetic_depths(rows, cols, seed=0):
    """float32 [rows, cols]: a shelf that deepens to the south-east, ripples, land (positive) in the north-west corner, 2 % nodata."""
    import numpy as np
    rng = np.random.default_rng(seed)
    r, c = np.arange(rows, dtype=np.float32)[:, None], np.arange(cols, dtype=np.float32)[None, :]
    d = -(0.02 * r + 0.015 * c) + 5.0 * np.sin(r / 37.0) * np.cos(c / 53.0) + 20.0
    d = np.round(d + rng.normal(0, 0.5, (rows, cols)).astype(np.float32), 2).astype(np.float32)
    d[rng.random((rows, cols)) < 0.02] = -9999.0
    return d


def write_asc(path, data):
    import numpy as np
    rows, cols = data.shape
    with open(path, "w") as f:
        f.write(f"ncols {cols}\nnrows {rows}\nxllcorner {X0!r}\nyllcorner {Y0 - rows * CELL!r}\ncellsize {CELL!r}\nNODATA_value -9999\n")
        for a in range(0, rows, 256):
            np.savetxt(f, data[a:a + 256], fmt="%.2f")


def write_tiff(path, data):
    from PIL import Image, TiffImagePlugin
    ifd = TiffImagePlugin.ImageFileDirectory_v2()
    ifd[33550] = (CELL, CELL, 0.0)
    ifd[33922] = (0.0, 0.0, 0.0, X0, Y0, 0.0)
    ifd[42113] = "-9999"
    Image.fromarray(data).save(path, tiffinfo=ifd)


def facilities(n, max_cages, rows, cols, span, seed=1):
    """-> (entry_start int32 [n + 1], cages float64 [E, 4] lon_min, lon_max, lat_min, lat_max)."""
    import numpy as np
    rng = np.random.default_rng(seed)
    counts = rng.integers(5, max_cages + 1, n)
    lat_m = 111_000.0
    cx = X0 + cols * CELL * rng.uniform(0.5 - span / 2, 0.5 + span / 2, n)
    cy = Y0 - rows * CELL * rng.uniform(0.5 - span / 2, 0.5 + span / 2, n)
    owner = np.repeat(np.arange(n), counts)
    E = owner.shape[0]
    x = cx[owner] + rng.normal(0, 150.0, E) / (lat_m * 0.72)
    y = cy[owner] + rng.normal(0, 150.0, E) / lat_m
    w, h = rng.uniform(10, 40, E) / (lat_m * 0.72), rng.uniform(10, 40, E) / lat_m
    cages = np.stack([x, x + w, y, y + h], 1)
    return np.ascontiguousarray(np.concatenate([[0], np.cumsum(counts)]), dtype=np.int32), np.ascontiguousarray(cages)


def spread(v):
    return {"median": statistics.median(v), "min": min(v), "max": max(v)}


def run(opt, work):
    import numpy as np
    import torch
    from aquaculture_amd import bathymetry as bt
    data = synthetic_depths(opt.rows, opt.cols)
    asc, tif = os.path.join(work, "depth.asc"), os.path.join(work, "depth.tif")
    t0 = time.perf_counter()
    write_asc(asc, data)
    write_tiff(tif, data)
    made_s = time.perf_counter() - t0
    start, cages = facilities(opt.facilities, opt.max_cages, opt.rows, opt.cols, opt.span)
    bounds = (float(cages[:, 0].min()), float(cages[:, 1].max()), float(cages[:, 2].min()), float(cages[:, 3].max()))
    row = {"rows": opt.rows, "cols": opt.cols, "numbers": opt.rows * opt.cols, "asc_bytes": os.path.getsize(asc), "tif_bytes": os.path.getsize(tif),
           "files_written_s": made_s, "facilities": opt.facilities, "cages": int(cages.shape[0])}
    read = {"asc": [], "tif": []}
    for _ in range(opt.repeats):
        for kind, path in (("asc", asc), ("tif", tif)):
            t0 = time.perf_counter()
            grid = bt.load_window([path], bounds)
            read[kind].append(time.perf_counter() - t0)
            if kind == "asc":
                first = grid
            else:
                assert np.array_equal(grid["data"], first["data"], equal_nan=True) and grid["offset"] == first["offset"]
    grid = first
    row.update(window=list(grid["data"].shape), window_offset=list(grid["offset"]), window_bytes=int(grid["data"].nbytes),
               read_asc_s=spread(read["asc"]), read_tif_s=spread(read["tif"]))
    for _ in range(2):
        bt.stats_gpu(start, cages, grid)
    torch.cuda.synchronize()
    upload_ms, ranges_ms, stats_ms, call_ms = [], [], [], []
    for _ in range(opt.repeats):
        t0 = time.perf_counter()
        dev = torch.from_numpy(grid["data"]).cuda()
        torch.cuda.synchronize()
        upload_ms.append((time.perf_counter() - t0) * 1e3)
        del dev
        t = {}
        t0 = time.perf_counter()
        got = bt.stats_gpu(start, cages, grid, t)
        call_ms.append((time.perf_counter() - t0) * 1e3)
        ranges_ms.append(t["ranges_ms"]); stats_ms.append(t["stats_ms"])
    t0 = time.perf_counter()
    want = bt.stats_numpy(start, cages, grid)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    cols_ = bt.depth_columns(got[0], got[1])
    row.update(bitmap_words=t["bitmap_words"], upload_ms=spread(upload_ms), ranges_ms=spread(ranges_ms), stats_ms=spread(stats_ms), stats_gpu_call_ms=spread(call_ms),
               numpy_ms=numpy_ms, equal_to_numpy=bool(got[0].tobytes() == want[0].tobytes() and got[1].tobytes() == want[1].tobytes()),
               cells_per_facility={"mean": float(got[1].mean()), "max": int(got[1].max())}, without_valid_cell=int((got[1] == 0).sum()),
               cage_depth_m={"min": min(cols_["cage_depth"]), "median": statistics.median(cols_["cage_depth"]), "max": max(cols_["cage_depth"])})
    print(json.dumps(row), flush=True)
    return row


def main():
    p = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    p.add_argument("--rows", type=int, default=9000)
    p.add_argument("--cols", type=int, default=9000)
    p.add_argument("--facilities", type=int, default=3000)
    p.add_argument("--max-cages", type=int, default=60)
    p.add_argument("--span", type=float, default=0.5, help="share of the raster's width and height the facilities' centres lie in")
    p.add_argument("--repeats", type=int, default=5)
    p.add_argument("--dir", default=None, help="where the raster files are written (default: a temporary directory, removed afterwards)")
    p.add_argument("--out", default=None)
    opt = p.parse_args()
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("bench_depth: no GPU (timings are taken on the device or not at all)")
    if opt.dir:
        os.makedirs(opt.dir, exist_ok=True)
        row = run(opt, opt.dir)
    else:
        with tempfile.TemporaryDirectory() as work:
            row = run(opt, work)
    result = {"device": torch.cuda.get_device_name(0), "host_cpus": len(os.sched_getaffinity(0)), "rows": [row]}
    if opt.out:
        with open(opt.out, "w") as f:
            json.dump(result, f, indent=1)
    return 0


if __name__ == "__main__":
    sys.exit(main())
