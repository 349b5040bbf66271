"""--bathymetry on the GPU: aq_depth_ranges_f64 / aq_depth_stats_f64 (csrc/depth.hip) through engine.depth_stats against the numpy
restatement, byte for byte (min, max, sum, count), on the cases of tests/test_bathymetry.py and on a random case of several thousand
wavefronts; the launcher's refusals by arguments alone; the two command lines against their --cpu files."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_bathymetry import HAND, NODATA, box, hand_entries, hand_grid, order_grid, random_case, synthetic_raster
from test_tonnage import synthetic_run, write

from aquaculture_amd import bathymetry as bt, engine, tonnage as tn

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def same_bytes(got, want):
    return all(np.ascontiguousarray(g).tobytes() == np.ascontiguousarray(w).tobytes() for g, w in zip(got, want))


def test_hand_cases_are_the_restatements_bytes(lib):
    names, start, cages = hand_entries()
    grid = hand_grid()
    stats, count = bt.stats_gpu(start, cages, grid)
    for k, name in enumerate(names):
        assert (*stats[k].tolist(), int(count[k])) == HAND[name][1], name
    assert same_bytes((stats, count), bt.stats_numpy(start, cages, grid))
    # the ranges and the windows themselves
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    _, _, windows = engine.depth_stats(dev(start), dev(cages), dev(grid["data"]), float(grid["x0"]), float(grid["y0"]), float(grid["dx"]), float(grid["dy"]), NODATA)
    assert np.array_equal(windows, bt.cell_ranges_numpy(start, cages, *grid["data"].shape, grid["x0"], grid["y0"], grid["dx"], grid["dy"])[1])
    # no facility, no cage, no raster cell
    for s, c, g in (([0], cages[:0], grid), ([0, 0, 0], cages[:0], grid), (start, cages, dict(grid, data=np.zeros((0, 0), np.float32)))):
        assert same_bytes(bt.stats_gpu(s, c, g), bt.stats_numpy(s, c, g))


def test_the_sum_is_added_in_the_definitions_order(lib):
    grid, start, cages = order_grid()
    stats, count = bt.stats_gpu(start, cages, grid)
    assert stats[0].tolist() == [1.0, 2.0 ** 53, 2.0 ** 53 + 138] and int(count[0]) == 135
    assert same_bytes((stats, count), bt.stats_numpy(start, cages, grid))


@functools.lru_cache(maxsize=None)
def large_case():
    """3,000 facilities of 1 .. 200 cages on a 512 x 512 window (one wavefront each in both launches): cages of up to a few cells around
    the facility's centre, some past the edges; empty facilities first, last and in between; three facilities whose cages lie all over
    the window, with cages up to 100 cells wide (rows of several bitmap words, windows of thousands of steps per lane)."""
    rng = np.random.default_rng(11)
    n = 512
    data = rng.uniform(-120, 3, (n, n)).astype(np.float32)
    data[rng.random((n, n)) < 0.03] = NODATA
    data[rng.random((n, n)) < 0.03] = np.nan
    data[rng.random((n, n)) < 0.01] = 0.0
    data[rng.random((n, n)) < 0.01] = -0.0
    grid = {"data": data, "x0": np.float64(2.75), "y0": np.float64(43.5), "dx": np.float64(1 / 960), "dy": np.float64(1 / 960), "nodata": NODATA}
    start, cages = [0], []
    for f in range(3000):
        empty = f in (0, 2999) or f % 97 == 50
        wide = f in (700, 1500, 2200)
        cx, cy = rng.uniform(-5, n + 5), rng.uniform(-5, n + 5)
        k = 0 if empty else int(rng.integers(1, 201))
        if wide:
            x, y, w, h = rng.uniform(-20, n, k), rng.uniform(-20, n, k), rng.uniform(0.1, 100, k), rng.uniform(0.1, 6, k)
        else:
            x, y, w, h = cx + rng.uniform(-12, 12, k), cy + rng.uniform(-12, 12, k), rng.uniform(0.02, 3, k), rng.uniform(0.02, 3, k)
        cages.append(np.stack(box(x, x + w, y, y + h, 2.75, 43.5, 1 / 960), 1))
        start.append(start[-1] + k)
    start, cages = np.asarray(start, np.int32), np.concatenate(cages, 0)
    return grid, start, cages, bt.stats_numpy(start, cages, grid)


def test_three_thousand_facilities_are_the_restatements_bytes(lib):
    grid, start, cages, want = large_case()
    assert int((want[1] == 0).sum()) >= 33 and int(want[1].max()) > 10000 and np.isfinite(want[0][want[1] > 0]).all()
    times = {}
    got = bt.stats_gpu(start, cages, grid, times)
    assert same_bytes(got, want)
    print(f"{start.shape[0] - 1} facilities, {cages.shape[0]} cages, {times['bitmap_words']} bitmap words: ranges {times['ranges_ms']:.3f} ms, "
          f"stats {times['stats_ms']:.3f} ms")
    assert same_bytes(bt.stats_gpu(start, cages, grid), want)          # and again: nothing depends on the order of the atomics
    # a slice of the facilities (entry offsets that do not start at 0) and another nodata value
    sub = start[1000:1101]
    assert same_bytes(bt.stats_gpu(sub, cages, grid), bt.stats_numpy(sub, cages, grid))
    other = dict(grid, nodata=None)
    assert same_bytes(bt.stats_gpu(sub, cages, other), bt.stats_numpy(sub, cages, other))


def test_random_case_of_the_cpu_suite(lib):
    grid, start, cages = random_case()
    assert same_bytes(bt.stats_gpu(start, cages, grid), bt.stats_numpy(start, cages, grid))


def test_the_size_guard_refuses_by_arguments_alone(lib):
    """No launch: every device pointer is null.  A call the guard lets through ends at the null pointer check."""
    def call(windows, word_start, words, nrows=1 << 16, ncols=1 << 16, F=None, E=0):
        w = np.ascontiguousarray(windows, dtype=np.int32).reshape(-1, 4)
        s = np.ascontiguousarray(word_start, dtype=np.int64)
        rc = lib.aq_depth_stats_f64(None, w.shape[0] if F is None else F, None, E, None, w.ctypes.data, None, s.ctypes.data, None, nrows, ncols, NODATA,
                                    None, words, None, None, None)
        return rc, lib.aq_last_error()

    rc, msg = call([[0, 65535, 0, 32767]], [0, 1 << 26], 1 << 26)           # 2^31 cells in one window
    assert rc != 0 and b"fewer than 2^31" in msg
    rc, msg = call([[0, 65535, 0, 32766]], [0, 1 << 26], 1 << 26)           # 2^31 - 65536 cells: let through
    assert rc != 0 and b"null pointer" in msg
    big = [[0, 32767, 0, 32767]] * 64                                       # 64 windows of 2^30 cells: 2^31 words
    rc, msg = call(big, np.arange(65, dtype=np.int64) << 25, 1 << 31)
    assert rc != 0 and b"bitmap of 2147483648 words" in msg
    rc, msg = call(big[:63], np.arange(64, dtype=np.int64) << 25, 63 << 25)
    assert rc != 0 and b"null pointer" in msg
    for kw, text in ((dict(windows=[[0, 9, 0, 9]], word_start=[0, 3], words=3), b"3 bitmap words for 100 cells"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[0, 4], words=3), b"end at 4 of 3"),
                     (dict(windows=[[0, 9, 0, 9], [0, 9, 0, 9]], word_start=[0, 4, 3], words=8), b"end at"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[-1, 4], words=8), b"start at -1"),
                     (dict(windows=[[0, 16, 0, 9]], word_start=[0, 8], words=8, ncols=16), b"leaves the"),
                     (dict(windows=[[0, 9, -1, 9]], word_start=[0, 8], words=8), b"leaves the"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[0, 4], words=4, F=1 << 31), b"facilities"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[0, 4], words=4, E=1 << 31), b"cages"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[0, 4], words=-1), b"bitmap of -1 words"),
                     (dict(windows=[[0, 9, 0, 9]], word_start=[0, 4], words=4, nrows=-1), b"window of")):
        rc, msg = call(**kw)
        assert rc != 0 and msg.startswith(b"depth:") and text in msg, (kw, msg)
    assert call(np.zeros((0, 4)), [0], 0)[0] == 0                           # no facility: nothing to do
    # and engine.depth_stats checks what it is given
    with pytest.raises(ValueError, match="contiguous CUDA"):
        engine.depth_stats(torch.zeros(2, dtype=torch.int64, device="cuda"), torch.zeros((0, 4), dtype=torch.float64, device="cuda"),
                           torch.zeros((2, 2), dtype=torch.float32, device="cuda"), 0.0, 0.0, 1.0, 1.0)
    with pytest.raises(RuntimeError, match="depth: cell size"):
        engine.depth_stats(torch.zeros(2, dtype=torch.int32, device="cuda"), torch.zeros((0, 4), dtype=torch.float64, device="cuda"),
                           torch.zeros((2, 2), dtype=torch.float32, device="cuda"), 0.0, 0.0, 0.0, 1.0)


# ---- the command lines ----

def test_command_line_writes_the_cpu_runs_bytes(lib, tmp_path):
    labels, csv_path = synthetic_run(tmp_path)
    raster = synthetic_raster(tmp_path)
    files = []
    for extra in ((), ("--cpu",)):
        out = tmp_path / ("cpu.csv" if extra else "gpu.csv")
        r = subprocess.run([sys.executable, "-m", "aquaculture_amd.bathymetry", "--labels", labels, "--geocode-bboxes", csv_path, "--bathymetry", raster,
                            "--out", str(out), *extra], cwd=ROOT, capture_output=True, text=True, timeout=240)
        assert r.returncode == 0, r.stderr[-3000:]
        assert "2 facilities, 0 without a valid cell" in r.stdout, r.stdout
        files.append(open(out, "rb").read())
    assert files[0] == files[1] and len(files[0].decode().splitlines()) == 3


def test_detect_py_takes_the_depths_of_its_own_sweep_from_the_raster(lib, tmp_path):
    """The tiny sweep of tests/test_gpu_tonnage.py's last test with --bathymetry: facility_depths.csv and the tonnage files equal what the
    --cpu route makes of the run's label files, and the facility file carries the reference's five columns."""
    from PIL import Image
    from aquaculture_amd import checkpoint, facilities, geocode, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    raster = synthetic_raster(tmp_path)
    factors = write(tmp_path / "factors.csv", "pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n")
    args = ["--facilities-conf", "0.25", "--facilities-eps", "25", "--facilities-min-cages", "4", "--facilities-by", "year", "--facilities"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "depth",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, *args, "--tonnage", "--tonnage-factors", factors, "--tonnage-K", "200",
                        "--bathymetry", raster, "--bathymetry-statistic", "bathy_depth"], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "depth"
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    bathy = bt.settings([raster], table, None, "bathy_depth")
    want = tn.tonnage_from_table(table, str(tmp_path / "want"), factors, K=200, conf_thresh=0.25, eps=25.0, min_cages=4, widths=640, heights=640, cpu=True,
                                 bathymetry=bathy)
    for f in (bt.DEPTHS_FILE, tn.ESTIMATES_FILE, tn.FACILITIES_FILE):
        assert open(run / f, "rb").read() == open(tmp_path / "want" / f, "rb").read(), f
    rows = open(run / bt.DEPTHS_FILE).read().splitlines()
    assert len(rows) == 1 + len(want["facility_index"]) >= 2 and all(int(row.split(",")[-1]) >= 1 for row in rows[1:])      # real cells, not the default
    doc = json.load(open(run / tn.JSON_FILE))
    assert doc["bathymetry"] == {"files": ["depth.asc"], "statistic": "bathy_depth", "default_depth_facilities": 0}
    fac = facilities.facilities_from_table(table, str(tmp_path / "want.geojson"), "year", 0.25, 25.0, 4, 640, 640, cpu=True, bathymetry=bathy)
    got = json.load(open(run / "facilities.geojson"))
    assert got == json.load(open(tmp_path / "want.geojson")) and len(got["features"]) == len(fac["facility_index"]) >= 1
    assert all(list(f["properties"])[-5:] == list(bt.DEPTH_COLUMNS) and f["properties"]["cage_depth"] > 1.0 for f in got["features"])
    assert "bathymetry" not in json.load(open(run / "run_params.json"))
