"""--facilities on the GPU: aq_facility_dbscan_f64 (csrc/facilities.hip) through engine.facility_dbscan / facilities.dbscan_labels against
sklearn.cluster.DBSCAN called as the reference calls it, per group: integer labels and core flags, exactly.  The point sets and their
expected labels are those of tests/test_facilities.py.  The command-line step runs in a child process under its own time limit."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_facilities import CASES, TIE, TIE_CORE, TIE_LABELS, expected, large_case, no_near_ties, sk_labels

from aquaculture_amd import facilities, geocode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("name", sorted(CASES))
def test_labels_and_core_flags_are_sklearns(lib, name):
    xy, group, eps, ms = CASES[name]
    assert no_near_ties(xy, group, eps), "the case has a pair too close to eps for an exact comparison"
    labels, core = facilities.dbscan_labels(xy, group, eps, ms)
    want_l, want_c = expected(name)
    assert core.dtype == bool and np.array_equal(core, want_c), np.nonzero(core != want_c)[0][:10]
    assert labels.dtype == np.int64 and np.array_equal(labels, want_l), np.nonzero(labels != want_l)[0][:10]


def test_roots_are_the_first_core_point_of_the_cluster(lib):
    from aquaculture_amd.engine import facility_dbscan
    for name in ("blobs_0", "two_groups", "border_b_first", "chain_9.99"):
        xy, group, eps, ms = CASES[name]
        core, root = facility_dbscan(torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda(), eps, ms)
        assert core.dtype == torch.uint8 and root.dtype == torch.int32
        _, want_core, want_root = facilities.dbscan_numpy(xy, group, eps, ms)
        assert np.array_equal(root.cpu().numpy(), want_root) and np.array_equal(core.cpu().numpy().astype(bool), want_core)


def test_no_points(lib):
    labels, core = facilities.dbscan_labels(np.zeros((0, 2)), None, 10.0, 5)
    assert labels.shape == (0,) and core.shape == (0,)


def test_exact_tie(lib):
    """Every step of the row is exactly eps: the test is <=, in fp64, on coordinates of 4e6."""
    xy, group, eps, ms = TIE
    labels, core = facilities.dbscan_labels(xy, group, eps, ms)
    assert labels.tolist() == TIE_LABELS and core.tolist() == TIE_CORE
    want_l, want_c = sk_labels(xy, group, eps, ms)
    assert np.array_equal(labels, want_l) and np.array_equal(core, want_c)


def test_many_workgroups_and_the_same_bytes_twice(lib):
    from aquaculture_amd.engine import facility_dbscan
    xy, group, eps, ms = large_case()
    assert no_near_ties(xy, group, eps)
    x, g = torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda()
    core1, root1 = facility_dbscan(x, g, eps, ms)
    core2, root2 = facility_dbscan(x, g, eps, ms)
    assert torch.equal(core1, core2) and torch.equal(root1, root2)
    want_l, want_c = sk_labels(xy, group, eps, ms)
    assert want_c.sum() > 50 and ((want_l >= 0) & ~want_c).sum() > 50 and want_l.max() > 10       # clusters, core and border points in every group
    assert np.array_equal(core1.cpu().numpy().astype(bool), want_c)
    assert np.array_equal(facilities.roots_to_labels(root1.cpu().numpy(), group), want_l)


def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    from aquaculture_amd import engine
    xy, group, eps, ms = CASES["blobs_1"]
    n = xy.shape[0]
    x, g = torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda()
    keys, perm = engine.facility_sort_keys(x, g, eps)
    need = int(lib.aq_facility_scratch_bytes(n))
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    core = torch.full((n,), 0x77, dtype=torch.uint8, device="cuda")
    root = torch.full((n,), -77, dtype=torch.int32, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(keys_p=keys.data_ptr(), n_=n, eps_=eps, ms_=ms, scratch_bytes=need, root_p=root.data_ptr()):
        return lib.aq_facility_dbscan_f64(keys_p, perm.data_ptr(), x.data_ptr(), g.data_ptr(), n_, eps_, ms_, scratch.data_ptr(), scratch_bytes,
                                          core.data_ptr(), root_p, stream)

    for kw, msg in (({"eps_": 0.0}, "eps"), ({"eps_": -1.0}, "eps"), ({"eps_": float("nan")}, "eps"), ({"ms_": 0}, "min_samples"),
                    ({"keys_p": None}, "null pointer"), ({"root_p": None}, "null pointer"), ({"n_": 1 << 31}, "2\\^31"),
                    ({"scratch_bytes": need - 1}, "scratch")):
        assert call(**kw) == -1, kw
        assert __import__("re").search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((core == 0x77).all()) and bool((root == -77).all()) and bool((scratch == 0x5A).all()), kw
    # n = 0 does nothing, whatever the pointers
    assert lib.aq_facility_dbscan_f64(None, None, None, None, 0, eps, ms, None, 0, None, None, stream) == 0
    with pytest.raises(ValueError, match="eps"):
        engine.facility_dbscan(x, g, 0.0, ms)
    with pytest.raises(ValueError, match="min_samples"):
        engine.facility_dbscan(x, g, eps, 0)
    torch.cuda.synchronize()
    assert bool((core == 0x77).all()) and bool((root == -77).all()) and bool((scratch == 0x5A).all())
    assert call() == 0                                      # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert np.array_equal(core.cpu().numpy().astype(bool), expected("blobs_1")[1])


# ---- python -m aquaculture_amd.facilities ----

def synthetic_run(tmp_path):
    """A label directory and a bounds table laid out for exactly two facilities and some noise: scene 3 is 1843.2 m wide in EPSG:3857
    (0.3 m per pixel, 0.22 m on the ground at 43.3 N); tile (0, 0) of 2015 holds six circles 12 px (2.6 m) apart, one of them at the
    image's left border, and a stray square; tile (1024, 0) five squares, a stray circle and a circle of low confidence among the
    squares; the same tile of 2012 three circles (too few)."""
    labels = tmp_path / "labels"
    labels.mkdir()
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    csv_path = tmp_path / "wanted_bboxes.csv"
    x1, y1 = x0 + 1843.2, y0 + 1843.2
    with open(csv_path, "w") as f:
        f.write(",geometry\n")
        f.write(f'3,"POLYGON (({x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}, {x1!r} {y0!r}))"\n')
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    files = {"ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0": [row(0, 5 + 12 * k, 500, 10, 0.9) for k in range(6)] + [row(1, 800, 100, 10, 0.9)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_1024_0": [row(1, 300 + 12 * k, 200 + 5 * (k % 2), 10, 0.8) for k in range(5)]
                                                      + [row(0, 900, 900, 10, 0.9), row(0, 318, 212, 10, 0.3)],
             "ORTHOIMAGERY.ORTHOPHOTOS2012_3_1024_0": [row(0, 300 + 12 * k, 200, 10, 0.9) for k in range(3)]}
    for stem, rows in files.items():
        (labels / (stem + ".txt")).write_text("".join(rows))
    return str(labels), str(csv_path)


def test_command_line_matches_the_host_restatement(lib, tmp_path):
    labels, csv_path = synthetic_run(tmp_path)
    out = str(tmp_path / "facilities.geojson")
    r = subprocess.run([sys.executable, "-m", "aquaculture_amd.facilities", "--labels", labels, "--geocode-bboxes", csv_path, "--out", out],
                       cwd=ROOT, capture_output=True, text=True, timeout=180)
    assert r.returncode == 0, r.stderr[-3000:]
    assert "2 facilities of 11 cages" in r.stdout, r.stdout
    table = geocode.geocode_label_dir(labels, csv_path)
    want_out = str(tmp_path / "want.geojson")
    fac = facilities.facilities_from_table(table, want_out, cpu=True)
    assert len(fac["facility_index"]) == 2 and sorted(fac["noise_points"]) == [2, 2] and fac["year"] == [2015, 2015]
    assert sorted((a, b) for a, b in zip(fac["num_circle_farms"], fac["num_square_farms"])) == [(0, 5), (6, 0)]
    got, want = json.load(open(out)), json.load(open(want_out))
    assert got == want
    got_d, want_d = json.load(open(facilities.detections_path(out))), json.load(open(facilities.detections_path(want_out)))
    assert got_d == want_d and len(got_d["features"]) == 11
    # the circle at the left border of its image (pixel xmin == 0) has the border estimate: a variance
    var = {f["properties"]["xmin"]: f["properties"]["area_var"] for f in got_d["features"] if f["properties"]["type"] == "circle_farm"}
    assert var[0] > 0 and all(v == 0 for k, v in var.items() if k != 0)


# ---- detect.py --facilities ----

def test_detect_py_writes_the_facilities_of_its_own_sweep(lib, tmp_path):
    """An engine sweep over four synthetic 640-px tiles with the synthetic checkpoint, geocoded and clustered in the same run: the two files
    equal what the host restatement makes of the run's label files, with the images' own size (640) in the border test."""
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    args = ["--facilities-conf", "0.25", "--facilities-eps", "25", "--facilities-min-cages", "4", "--facilities-by", "pass"]
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "fac",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--facilities", *args], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "fac"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "facilities of" in l))
    assert "facilities" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want_out = str(tmp_path / "want.geojson")
    fac = facilities.facilities_from_table(table, want_out, "pass", 0.25, 25.0, 4, 640, 640, cpu=True)
    assert f"{len(fac['facility_index'])} facilities of {int((fac['_members'] >= 0).sum())} cages" in r.stdout + r.stderr
    assert json.load(open(run / "facilities.geojson")) == json.load(open(want_out))
    assert json.load(open(run / "facilities_detections.geojson")) == json.load(open(facilities.detections_path(want_out)))
    assert table["image"].shape[0] > 0 and set(fac["pass"]) <= {"2013-2015"}
