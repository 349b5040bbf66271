"""--performance on the GPU: csrc/population.hip (engine.bernoulli_counts) against performance.counts_numpy byte for byte over the sizes at
which a wavefront's strided loop, its odd tail, the blocks of four waves and the counter words can go wrong; chunks and guard rows; the
reference's own case at full size against the figures the restatement gives on a CPU; and the whole step on the device against
``cpu=True``, file for file.  The inputs and the CPU run are those of tests/test_performance.py."""
import os

import numpy as np
import pytest
import torch

from test_performance import PINNED_ALL_ZEROS_50, PINNED_ZERO_SHARE, R_IMAGES, R_LABELS, R_SAMPLE, EPS, MIN_CAGES, cpu_run, inputs
from test_evaluate import truth

from aquaculture_amd import engine, performance

pytestmark = pytest.mark.gpu

SIZES = (1, 2, 63, 64, 127, 128, 129, 257, 1001)           # one lane; an odd tail; fewer calls than lanes; 64 and 128 calls +- 1; several trips
KS = (1, 3, 4, 5, 65)                                       # blocks with idle waves, a full block, more than one block
K0S = (0, 7, (1 << 32) - 65)                                # the last simulation is the counter word's last value
SEEDS = (0, (1 << 63) + 5)                                  # a high key word
RATES = {1: (0.37,),
         3: (0.5, 1.0, 0.07),
         16: (0.3, 0.0, 0.9, 1.0, 0.01, 2.0 ** -53, 0.5, 0.5, 0.62, 0.05, 0.75, 0.2, 0.11, 0.45, 0.83, 0.02)}      # 0, 1, 2^-53, a duplicate, no order


@pytest.mark.parametrize("seed", SEEDS)
@pytest.mark.parametrize("R", sorted(RATES))
def test_counts_are_the_restatements_byte_for_byte(R, seed):
    rates = RATES[R]
    for S in SIZES:
        for k0 in K0S:
            want = performance.counts_numpy(seed, k0, max(KS), S, rates)      # row k depends on (seed, k0 + k, S) alone: one reference for every K
            if S >= 63:                                     # equality has to show something: at the reference's rates every count would be 0
                assert ((want != 0) & (want != S)).mean() >= 0.5, (S, k0)
            for K in KS:
                got = engine.bernoulli_counts(seed, k0, K, S, rates)
                assert got.dtype == torch.int32 and tuple(got.shape) == (K, R) and got.is_cuda
                assert np.array_equal(got.cpu().numpy(), want[:K]), (S, k0, K)
    assert engine.bernoulli_counts(seed, 0, 0, 10, rates).shape == (0, R)


def test_chunks_equal_one_call_and_no_word_outside_the_rows_is_written():
    rates, S, K, G, SENTINEL = RATES[16], 257, 70, 8, -7777
    one = engine.bernoulli_counts(11, 5, K, S, rates).cpu().numpy()
    parts = torch.cat([engine.bernoulli_counts(11, 5, 33, S, rates), engine.bernoulli_counts(11, 5 + 33, K - 33, S, rates)]).cpu().numpy()
    assert np.array_equal(one, parts) and np.array_equal(one, performance.counts_numpy(11, 5, K, S, rates))
    for R in (1, 3, 16):
        buf = torch.full((K + 2 * G, R), SENTINEL, dtype=torch.int32, device="cuda")
        out = engine.bernoulli_counts(11, 5, K, S, rates[:R], out=buf[G:G + K])
        assert out.data_ptr() == buf[G].data_ptr()
        host = buf.cpu().numpy()
        assert (host[:G] == SENTINEL).all() and (host[G + K:] == SENTINEL).all()            # the guards are untouched
        assert (host[G:G + K] != SENTINEL).all() and np.array_equal(host[G:G + K], one[:, :R])      # every owned word is written
    with pytest.raises(ValueError, match="contiguous"):
        engine.bernoulli_counts(0, 0, 4, 10, (0.5, 0.5), out=torch.zeros((4, 4), dtype=torch.int32, device="cuda")[:, :2])


def test_device_pointers_are_checked_before_the_launch(lib):
    import ctypes as C
    rates_h = (C.c_double * 2)(0.25, 0.5)
    rates_d = torch.tensor([0.25, 0.5], dtype=torch.float64, device="cuda")
    out = torch.full((4, 2), -1, dtype=torch.int32, device="cuda")
    f = lambda rd, od: lib.aq_bernoulli_counts_i32(0, 0, 3, 10, rd, rates_h, 2, od, None)
    assert f(None, out.data_ptr()) != 0 and f(rates_d.data_ptr(), None) != 0 and f(rates_d.data_ptr() + 4, out.data_ptr()) != 0
    assert f(rates_d.data_ptr(), out.data_ptr() + 2) != 0 and lib.aq_last_error().startswith(b"population:")
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == -1).all()


def test_the_references_case_at_full_size():
    t = {}
    sim = performance.simulate(10000, R_SAMPLE, performance.DEFAULT_RATES, 0, times=t)
    assert sim["all_zeros_50"] == PINNED_ALL_ZEROS_50 and sim["zero_share"] == PINNED_ZERO_SHARE
    assert t["kernel_ms"] > 0 and t["select_ms"] > 0
    b = performance.population_bound(performance.DEFAULT_RATES, sim["all_zeros_50"], sim["zero_share"], R_IMAGES, R_SAMPLE, R_LABELS)
    assert b["final_rate"] == 7 * 1e-5 and abs(b["final_rate"] - 7e-05) < 1e-19 and b["images_with_cages"] == 55 and b["upper_bound"] == 4285
    counts = engine.bernoulli_counts(0, 0, 64, R_SAMPLE, performance.DEFAULT_RATES).cpu().numpy()
    assert (np.diff(counts, axis=1) >= 0).all() and np.array_equal(counts, performance.counts_numpy(0, 0, 64, R_SAMPLE, performance.DEFAULT_RATES))


def test_the_whole_step_on_the_device_writes_the_cpu_runs_bytes(tmp_path):
    table, names, rects, sites, land, sample = inputs()
    want_s, want = cpu_run()
    s = performance.performance(table, truth(), str(tmp_path), names=names, sample=sample, land=land, rects=rects, sites=sites, thresholds=100,
                                eps=EPS, min_cages=MIN_CAGES, rates=(0.01, 0.05, 0.2), K=64, seed=3, device="test")
    assert sorted(os.listdir(tmp_path)) == sorted(want) == sorted([performance.CURVES_FILE, performance.STRATA_FILE, performance.JSON_FILE])
    for f, data in want.items():
        assert open(tmp_path / f, "rb").read() == data, f
    assert s == want_s
    plain = performance.performance(table, truth(), str(tmp_path / "named"), names=names, sample=sample, land=land, rects=rects, sites=sites, thresholds=2,
                                    rates=(0.5,), K=2)
    assert plain["device"] == torch.cuda.get_device_name()


def test_detect_py_writes_the_three_files_for_its_own_sweep(lib, tmp_path):
    """An engine sweep over eight synthetic 640-px tiles, geocoded, evaluated and then --performance in the same run: the image list is the
    sweep's, and the three files equal what the host path makes of the run's label files."""
    import json
    import subprocess
    import sys
    from PIL import Image
    from test_gpu_evaluate import GRID_ARGS, lattice_truth
    from test_gpu_facilities import synthetic_run
    from aquaculture_amd import checkpoint, geocode, tiles
    ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    (tmp_path / "jpegs").mkdir()
    stems = []
    for k, i in enumerate((0, 3, 19, 20, 1, 2, 4, 5)):
        stems.append(f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * (k % 4)}_{1024 * (k // 4)}")
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / (stems[-1] + ".jpeg"), quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    truth_path = lattice_truth(tmp_path / "truth.geojson", csv_path)
    (tmp_path / "cf.csv").write_text("image\n" + "".join(s + ".jpeg\n" for s in sorted(stems)[:6]))
    args = ["--performance-sample", str(tmp_path / "cf.csv"), "--performance-thresholds", "11", "--performance-eps", "25", "--performance-min-cages", "4",
            "--performance-rates", "0.1,0.3", "--performance-K", "64", "--performance-seed", "4"]
    r = subprocess.run(["timeout", "-k", "10", "300", sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"),
                        "--source", str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "pf",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--evaluate", truth_path, *GRID_ARGS, "--performance", *args],
                       capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "pf"
    assert "performance of " in r.stdout + r.stderr and "performance" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want = tmp_path / "want"
    s = performance.performance_from_options(table, truth_path, str(want), csv_path, names=sorted(stems), sample_file=str(tmp_path / "cf.csv"), cpu=True,
                                             device=torch.cuda.get_device_name(), thresholds=11, eps=25.0, min_cages=4, rates=(0.1, 0.3), K=64, seed=4)
    for f in (performance.CURVES_FILE, performance.STRATA_FILE, performance.JSON_FILE):
        assert open(run / f, "rb").read() == open(want / f, "rb").read(), f
    assert s["n_images"] == 8 and s["n_sampled_images"] == 6 and s["n_detections"] > 0 and s["land_images"] is False
