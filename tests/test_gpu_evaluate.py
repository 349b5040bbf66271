"""--evaluate on the GPU: aq_eval_member_conf_f64 and aq_box_match_f64 (csrc/evaluate.hip) through engine.eval_member_conf / engine.box_match
against the numpy restatement, bit for bit; the grid and the operating point against the host path and the scikit-learn oracle of
tests/test_evaluate.py; refusals; the two command lines in child processes under their own time limits."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

from test_evaluate import (SMALL_GRID, assert_no_near_ties, check_hand_built, cpu_grid, fixture_data, hand_built_case, oracle, table_counts)
from test_facilities import CASES, TIE
from test_gpu_facilities import synthetic_run

from aquaculture_amd import evaluate, geocode

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEG_INF = float("-inf")


def confidences(n, seed, places=2):
    return np.round(np.random.default_rng(seed).uniform(0.3, 1.0, n), places)      # two places: many ties


def member_gpu(xy, group, conf, eps, K):
    from aquaculture_amd.engine import eval_member_conf
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    return eval_member_conf(dev(xy, np.float64), dev(group, np.int32), dev(conf, np.float64), eps, K)


def check_member(xy, group, conf, eps, K):
    got = member_gpu(xy, group, conf, eps, K).cpu()
    want = torch.from_numpy(evaluate.member_conf_numpy(xy, group, conf, eps, K))
    assert got.dtype == torch.float64 and got.shape == (xy.shape[0], K)
    assert torch.equal(got, want), np.argwhere(got.numpy() != want.numpy())[:10]
    return got.numpy()


# ---- eval_member_conf ----

@pytest.mark.parametrize("K", [1, 10, 16])
def test_member_conf_is_the_host_restatements_bit_for_bit(lib, K):
    for name in ("blobs_0", "blobs_3", "cell_edges"):
        xy, group, eps, _ = CASES[name]
        M = check_member(xy, group, confidences(xy.shape[0], 7), eps, K)
        assert np.isfinite(M[:, 0]).all() and (M[:, 1:] <= M[:, :-1]).all()
    xy, group, eps, _ = CASES["blobs_1"]
    check_member(xy, group, confidences(xy.shape[0], 8, places=6), 3.0 * eps, K)


def test_member_conf_small_neighbourhoods_equal_confidences_groups_and_the_exact_tie(lib):
    xy, group, eps, _ = CASES["four_coincident"]
    M = check_member(xy, group, np.array([0.9, 0.5, 0.7, 0.6]), eps, 6)
    assert M[:, :4].tolist() == [[0.9, 0.7, 0.6, 0.5], [0.5] * 4, [0.7, 0.7, 0.6, 0.5], [0.6, 0.6, 0.6, 0.5]] and (M[:, 4:] == NEG_INF).all()
    xy, group, eps, _ = CASES["one_point"]
    assert check_member(xy, group, np.array([0.8]), eps, 3).tolist() == [[0.8, NEG_INF, NEG_INF]]
    xy, group, eps, _ = CASES["blobs_2"]
    M = check_member(xy, group, np.full(xy.shape[0], 0.5), eps, 10)
    assert set(np.unique(M).tolist()) == {NEG_INF, 0.5}
    xy, group, eps, _ = CASES["two_groups"]                 # every point twice, once per group: the groups never meet
    conf = np.repeat(confidences(190, 9), 2)
    M = check_member(xy, group, conf, eps, 10)
    assert np.array_equal(M[0::2], M[1::2]) and np.array_equal(M[0::2], evaluate.member_conf_numpy(xy[0::2], np.zeros(190), conf[0::2], eps, 10))
    xy, group, eps, _ = TIE                                 # every step of the row is exactly eps
    M = check_member(xy, group, np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4, 0.95, 0.99]), eps, 3)
    assert M[:6, 2].tolist() == [0.7, 0.7, 0.7, 0.6, 0.5, 0.4] and M[6:, 2].tolist() == [NEG_INF, NEG_INF] and M[6:, 0].tolist() == [0.95, 0.99]


def test_member_conf_of_the_fixture_and_many_workgroups_twice(lib):
    det = fixture_data()["det"]
    assert det["conf"].shape[0] == 1095                     # 5 workgroups of 256
    for eps in (10.0, 50.0, 150.0):
        check_member(det["xy"], det["year_id"], det["conf"], eps, 10)
    r = np.random.default_rng(5)
    xy, group, conf = r.uniform(0, 600, (5000, 2)) + [4.0e6, 2.2e6], r.integers(0, 2, 5000).astype(np.int32), confidences(5000, 6, places=3)
    M1 = member_gpu(xy, group, conf, 20.0, 10)
    M2 = member_gpu(xy, group, conf, 20.0, 10)
    assert torch.equal(M1, M2)
    want = evaluate.member_conf_numpy(xy, group, conf, 20.0, 10)
    assert torch.equal(M1.cpu(), torch.from_numpy(want)) and np.isfinite(want[:, 9]).sum() > 1000 and np.isneginf(want[:, 9]).sum() > 100
    assert member_gpu(np.zeros((0, 2)), np.zeros(0), np.zeros(0), 10.0, 4).shape == (0, 4)


# ---- box_match ----

def match_gpu(qbox, qgroup, kbox, kgroup, G, payload=None):
    from aquaculture_amd.engine import box_match
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    hit, out = box_match(dev(np.reshape(qbox, (-1, 4)), np.float64), dev(qgroup, np.int32), dev(np.reshape(kbox, (-1, 4)), np.float64), dev(kgroup, np.int32), G,
                         None if payload is None else dev(payload, np.float64))
    assert hit.dtype == torch.uint8 and (out is None) == (payload is None)
    return hit.cpu().numpy().astype(bool), None if out is None else out.cpu().numpy()


def check_match(qbox, qgroup, kbox, kgroup, G, payload=None):
    hit, out = match_gpu(qbox, qgroup, kbox, kgroup, G, payload)
    want_hit, want_out = evaluate.box_match_numpy(qbox, qgroup, kbox, kgroup, payload)
    assert np.array_equal(hit, want_hit), np.nonzero(hit != want_hit)[0][:10]
    if payload is not None:
        assert out.dtype == np.float64 and np.array_equal(out, want_out), np.argwhere(out != want_out)[:10]
    return hit, out


def test_box_match_edges_corners_and_degenerate_boxes(lib):
    k = np.array([[1.0, 0.0, 2.0, 1.0], [5.0, 4.0, 6.0, 5.0], [0.0, 0.0, 9.0, 9.0], [7.0, 7.0, 7.0, 7.0]])
    kg = np.array([0, 0, 1, 0], np.int32)
    pay = np.array([[0.25, 1.0], [0.5, 2.0], [0.75, 3.0], [0.125, 4.0]])
    q = np.array([[0.0, 0.0, 1.0, 1.0],                    # touches key 0 along an edge
                  [2.0, 1.0, 3.0, 2.0],                    # touches key 0 at a corner
                  [5.0, 5.0, 5.0, 5.0],                    # a point on key 1's edge
                  [7.0, 7.0, 7.0, 7.0],                    # a point on a point
                  [3.0, 0.0, 4.0, 1.0],                    # nothing
                  [np.nextafter(2.0, 3.0), 0.0, 3.0, 1.0]])   # one ulp beside key 0
    hit, out = check_match(q, np.zeros(6, np.int32), k, kg, 2, pay)
    assert hit.tolist() == [True, True, True, True, False, False]
    assert out.tolist() == [[0.25, 1.0], [0.25, 1.0], [0.5, 2.0], [0.125, 4.0], [NEG_INF] * 2, [NEG_INF] * 2]
    hit, _ = check_match(q, np.ones(6, np.int32), k, kg, 2)
    assert hit.tolist() == [True, True, True, True, True, True]
    # a group without keys (G = 4: groups 2 and 3), group ids out of range, one query
    hit, out = check_match(q, np.array([2, 3, -1, 4, 1 << 30, -(1 << 31)], np.int32), k, kg, 4, pay)
    assert not hit.any() and (out == NEG_INF).all()
    hit, out = check_match(q[:1], np.zeros(1, np.int32), k, kg, 2, pay)
    assert hit.tolist() == [True] and out.tolist() == [[0.25, 1.0]]
    hit, out = check_match(q, np.zeros(6, np.int32), np.zeros((0, 4)), np.zeros(0, np.int32), 2, np.zeros((0, 3)))
    assert not hit.any() and out.shape == (6, 3) and (out == NEG_INF).all()
    assert match_gpu(np.zeros((0, 4)), np.zeros(0, np.int32), k, kg, 2, pay)[1].shape == (0, 2)


def test_box_match_long_runs_and_the_x_bound(lib):
    """Group 0: 300 keys that all meet the query (the 64 lanes stride five times), the maximum of each payload column at a different key;
    group 1: 200 keys of which the query's x1 cuts the sorted run after 70; group 2: 130 keys left of the query."""
    r = np.random.default_rng(3)
    x0 = np.concatenate([r.uniform(0, 50, 300), np.arange(200) * 1.0, r.uniform(-500, -100, 130)])
    k = np.stack([x0, np.zeros(630), x0 + 10.0, np.full(630, 10.0)], 1)
    kg = np.repeat(np.array([0, 1, 2], np.int32), [300, 200, 130])
    pay = r.permutation(630 * 16).reshape(630, 16).astype(np.float64)
    q = np.array([[10.0, 2.0, 60.0, 3.0], [-5.0, 2.0, 69.0, 3.0], [0.0, 2.0, 1.0, 3.0]])
    perm = r.permutation(630)
    hit, out = check_match(q, np.array([0, 1, 2], np.int32), k[perm], kg[perm], 3, pay[perm])
    assert hit.tolist() == [True, True, False]
    assert np.array_equal(out[0], pay[:300].max(0)) and np.array_equal(out[1], pay[300:370].max(0)) and len(set(pay[:300].argmax(0))) > 8
    check_match(q, np.array([0, 1, 2], np.int32), k[perm], kg[perm], 3, pay[perm][:, :1])
    check_match(q, np.array([0, 1, 2], np.int32), k[perm], kg[perm], 3)


def test_box_match_random_boxes_on_a_lattice(lib):
    """Integer coordinates, so that touching edges and corners are common; 5 groups, one of them without keys."""
    r = np.random.default_rng(11)

    def boxes(n):
        a, w = r.integers(0, 40, (n, 2)).astype(np.float64), r.integers(0, 4, (n, 2)).astype(np.float64)
        return np.concatenate([a, a + w], 1)

    q, k = boxes(700), boxes(900)
    qg, kg = r.integers(-1, 6, 700).astype(np.int32), r.choice([0, 1, 2, 4], 900).astype(np.int32)
    pay = confidences(900 * 10, 4).reshape(900, 10)
    hit, out = check_match(q, qg, k, kg, 5, pay)
    assert 100 < hit.sum() < 600 and not hit[(qg == 3) | (qg < 0) | (qg > 4)].any()
    h2, o2 = match_gpu(q, qg, k, kg, 5, pay)
    assert np.array_equal(hit, h2) and np.array_equal(out, o2)
    check_match(q, qg, k, kg, 5)


# ---- the grid and the operating point ----

def same_table(got, want):
    for c in evaluate.COLUMNS:
        assert got[c].dtype == want[c].dtype and np.array_equal(got[c], want[c], equal_nan=got[c].dtype.kind == "f"), c


def test_fixture_grid_is_the_host_paths_and_the_oracles(lib):
    data, o = fixture_data(), oracle()
    assert_no_near_ties(data, evaluate.DEFAULT_EPS)
    times = {}
    g = evaluate.grid(data, times=times)
    print({k: round(v, 3) for k, v in times.items()})
    assert set(times) == {"sort_ms", "kernel_ms", "count_ms"} and times["kernel_ms"] > 0
    same_table(g, cpu_grid())
    for k in range(3, 6560, 97):
        assert table_counts(g, k) == o.counts(float(g["conf_thresh"][k]), float(g["distance_threshold"][k]), int(g["min_cluster_size"][k])), k
    same_table(evaluate.grid(data, *SMALL_GRID), evaluate.grid(data, *SMALL_GRID, cpu=True))


def test_operating_point_is_the_host_paths(lib):
    data = fixture_data()
    for conf, eps, m in ((0.785, 50.0, 5), (0.6, 10.0, 2), (0.9, 130.0, 20)):
        np.testing.assert_equal(evaluate.operating_point(data, conf, eps, m), evaluate.operating_point(data, conf, eps, m, cpu=True))
    op = evaluate.operating_point(data, 0.785, 50.0, 5)
    assert (op["cage"]["n_pred"], op["cage"]["n_pred_tp"], op["cage"]["n_label"], op["cage"]["n_label_tp"]) == oracle().counts(0.785, 50.0, 5)
    check_hand_built(evaluate.operating_point(hand_built_case(), 0.5, 20.0, 3))


def test_no_detections_and_no_labels(lib):
    data = fixture_data()
    none = {k: (v[:0] if isinstance(v, np.ndarray) else v) for k, v in data["det"].items()}
    for d in ({"det": none, "lab": data["lab"], "years": data["years"]},
              {"det": data["det"], "lab": {k: v[:0] for k, v in data["lab"].items()}, "years": data["years"]}):
        same_table(evaluate.grid(d, *SMALL_GRID), evaluate.grid(d, *SMALL_GRID, cpu=True))
        np.testing.assert_equal(evaluate.operating_point(d, 0.785, 50.0, 5), evaluate.operating_point(d, 0.785, 50.0, 5, cpu=True))     # (NaN equals NaN here)


# ---- refusals ----

def test_bad_arguments_are_refused_and_nothing_is_launched(lib):
    from aquaculture_amd import engine
    xy, group, eps, _ = CASES["blobs_1"]
    n, K = xy.shape[0], 5
    conf_h = confidences(n, 2)
    x, g, c = torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda(), torch.from_numpy(conf_h).cuda()
    keys, perm = engine.facility_sort_keys(x, g, eps)
    need = int(lib.aq_eval_scratch_bytes(n, K))
    scratch = torch.full((need,), 0x5A, dtype=torch.uint8, device="cuda")
    M = torch.full((n, K), -77.0, dtype=torch.float64, device="cuda")
    stream = torch.cuda.current_stream().cuda_stream

    def call(keys_p=keys.data_ptr(), conf_p=c.data_ptr(), n_=n, eps_=eps, K_=K, scratch_bytes=need, out_p=M.data_ptr(), xy_p=x.data_ptr()):
        return lib.aq_eval_member_conf_f64(keys_p, perm.data_ptr(), xy_p, g.data_ptr(), conf_p, n_, eps_, K_, scratch.data_ptr(), scratch_bytes, out_p, stream)

    for kw, msg in (({"eps_": 0.0}, "eps"), ({"eps_": -1.0}, "eps"), ({"eps_": float("nan")}, "eps"), ({"eps_": float("inf")}, "eps"),
                    ({"K_": 0}, "K = 0"), ({"K_": 17}, "K = 17"), ({"keys_p": None}, "null pointer"), ({"conf_p": None}, "null pointer"),
                    ({"out_p": None}, "null pointer"), ({"n_": 1 << 31}, "2\\^31"), ({"n_": -1}, "2\\^31"), ({"scratch_bytes": need - 1}, "scratch"),
                    ({"xy_p": x.data_ptr() + 8}, "unaligned"), ({"conf_p": c.data_ptr() + 4}, "unaligned")):
        assert call(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((M == -77.0).all()) and bool((scratch == 0x5A).all()), kw
    assert lib.aq_eval_member_conf_f64(None, None, None, None, None, 0, eps, K, None, 0, None, stream) == 0     # n = 0 does nothing
    with pytest.raises(ValueError, match="eps"):
        engine.eval_member_conf(x, g, c, 0.0, K)
    with pytest.raises(ValueError, match="K = 17"):
        engine.eval_member_conf(x, g, c, eps, 17)

    q = torch.tensor([[0.0, 0.0, 1.0, 1.0], [5.0, 5.0, 6.0, 6.0]], dtype=torch.float64, device="cuda")
    qg = torch.zeros(2, dtype=torch.int32, device="cuda")
    kb = torch.tensor([[0.5, 0.5, 2.0, 2.0]], dtype=torch.float64, device="cuda")
    start = torch.tensor([0, 1], dtype=torch.int32, device="cuda")
    pay = torch.tensor([[0.5, 0.25]], dtype=torch.float64, device="cuda")
    hit = torch.full((2,), 0x77, dtype=torch.uint8, device="cuda")
    out = torch.full((2, 2), -77.0, dtype=torch.float64, device="cuda")

    def match(q_p=q.data_ptr(), Q_=2, k_p=kb.data_ptr(), N_=1, start_p=start.data_ptr(), G_=1, pay_p=pay.data_ptr(), K_=2, hit_p=hit.data_ptr(), out_p=out.data_ptr()):
        return lib.aq_box_match_f64(q_p, qg.data_ptr(), Q_, k_p, N_, start_p, G_, pay_p, K_, hit_p, out_p, stream)

    for kw, msg in (({"Q_": 1 << 31}, "2\\^31"), ({"N_": 1 << 31}, "2\\^31"), ({"Q_": -1}, "2\\^31"), ({"G_": -1}, "groups"), ({"K_": 17}, "K = 17"),
                    ({"K_": -1}, "K = -1"), ({"q_p": None}, "null pointer"), ({"k_p": None}, "null pointer"), ({"start_p": None}, "null pointer"),
                    ({"hit_p": None}, "null pointer"), ({"pay_p": None}, "null pointer"), ({"out_p": None}, "null pointer"),
                    ({"q_p": q.data_ptr() + 16}, "unaligned"), ({"k_p": kb.data_ptr() + 8}, "unaligned"), ({"out_p": out.data_ptr() + 4}, "unaligned")):
        assert match(**kw) == -1, kw
        assert re.search(msg, lib.aq_last_error().decode()), (kw, lib.aq_last_error())
        torch.cuda.synchronize()
        assert bool((hit == 0x77).all()) and bool((out == -77.0).all()), kw
    assert lib.aq_box_match_f64(None, None, 0, None, 0, None, 0, None, 0, None, None, stream) == 0             # Q = 0 does nothing
    with pytest.raises(ValueError, match="group ids"):
        engine.box_match(q, qg, kb, torch.tensor([1], dtype=torch.int32, device="cuda"), 1)
    torch.cuda.synchronize()
    assert bool((M == -77.0).all()) and bool((scratch == 0x5A).all()) and bool((hit == 0x77).all()) and bool((out == -77.0).all())
    assert call() == 0 and match() == 0                     # and the same arguments, all valid, run
    torch.cuda.synchronize()
    assert torch.equal(M.cpu(), torch.from_numpy(evaluate.member_conf_numpy(xy, group, conf_h, eps, K)))
    assert hit.tolist() == [1, 0] and out.tolist() == [[0.5, 0.25], [NEG_INF, NEG_INF]]


# ---- the command lines ----

def lattice_truth(path, csv_path, years=(2015, 2014, 2012)):
    """Labels over scene 3 of synthetic_run's bounds table: 60 m squares every 70 m, alternately circle and square cages, and one of a type
    that is dropped, in each of `years`."""
    (x0, y0, x1, y1), = geocode.load_wanted_bboxes(csv_path).values()
    feats = []
    for year in years:
        for k, (i, j) in enumerate((i, j) for i in range(20) for j in range(20)):
            a, b = x0 + 70.0 * i, y1 - 70.0 * j - 60.0
            ty = ("circle_cage", "square_cage", "other")[k % 3 if k % 7 else 2]
            feats.append({"type": "Feature", "properties": {"image": f"ORTHOIMAGERY.ORTHOPHOTOS{year}_3_{1024 * (i // 4)}_0.jpeg", "type": ty, "year": year},
                          "geometry": {"type": "Polygon", "coordinates": [[[a + 60.0, b], [a + 60.0, b + 60.0], [a, b + 60.0], [a, b], [a + 60.0, b]]]}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}, "features": feats}, f)
    return str(path)


GRID_ARGS = ["--evaluate-conf", "0.2:0.95:0.05", "--evaluate-eps", "10,25,60", "--evaluate-min-cages", "1:7:1"]
GRIDS = (np.arange(0.2, 0.95, 0.05), np.array([10, 25, 60]), np.arange(1, 7))


def same_files(got_dir, want_dir):
    assert open(os.path.join(got_dir, evaluate.CSV_FILE)).read() == open(os.path.join(want_dir, evaluate.CSV_FILE)).read()
    got, want = (json.load(open(os.path.join(d, evaluate.JSON_FILE))) for d in (got_dir, want_dir))
    assert got == want
    return got


def test_command_line_matches_the_host_restatement(lib, tmp_path):
    labels, csv_path = synthetic_run(tmp_path)
    truth_path = lattice_truth(tmp_path / "truth.geojson", csv_path)
    (tmp_path / "fold.txt").write_text("ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0.jpeg\nORTHOIMAGERY.ORTHOPHOTOS2015_3_1024_0\n")
    for extra, name in (([], "all"), (["--evaluate-images", str(tmp_path / "fold.txt")], "fold")):
        out = str(tmp_path / ("gpu_" + name))
        r = subprocess.run([sys.executable, "-m", "aquaculture_amd.evaluate", "--labels", labels, "--geocode-bboxes", csv_path, "--truth", truth_path,
                            "--evaluate-out", out, "--facilities-conf", "0.5", "--facilities-eps", "10", "--facilities-min-cages", "5", *GRID_ARGS, *extra],
                           cwd=ROOT, capture_output=True, text=True, timeout=180)
        assert r.returncode == 0, r.stderr[-3000:]
        table = geocode.geocode_label_dir(labels, csv_path)
        want_dir = str(tmp_path / ("cpu_" + name))
        images = evaluate.read_image_list(str(tmp_path / "fold.txt")) if extra else None
        evaluate.evaluate_table(table, truth_path, want_dir, *GRIDS, op=(0.5, 10.0, 5), images=images, cpu=True)
        s = same_files(out, want_dir)
        assert f"evaluated {s['n_detections']} detections against {s['n_labels']} labels over 270 combinations" in r.stdout, r.stdout
        # synthetic_run's two facilities: 6 circles and 5 squares, all of them members at the operating point
        assert s["operating_point"]["cage"]["n_pred"] == 11 and s["n_detections"] == (17 if not extra else 14) and s["grid_rows"] == 270
    assert s["n_labels"] < json.load(open(os.path.join(str(tmp_path / "gpu_all"), evaluate.JSON_FILE)))["n_labels"]


def test_detect_py_scores_its_own_sweep(lib, tmp_path):
    """An engine sweep over the four synthetic 640-px tiles of the facilities test, geocoded, clustered and scored in the same run: both
    files equal what the host path makes of the run's label files."""
    from PIL import Image
    from aquaculture_amd import checkpoint, tiles
    (tmp_path / "jpegs").mkdir()
    for k, i in enumerate((0, 3, 19, 20)):
        Image.fromarray(tiles.synthetic_tile(i, 640)).save(tmp_path / "jpegs" / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - k % 2}_3_{1024 * k}_0.jpeg", quality=95)
    checkpoint.write_synthetic_checkpoint(str(tmp_path / "synth.pt"), "yolov5m", 5)
    _, csv_path = synthetic_run(tmp_path)
    truth_path = lattice_truth(tmp_path / "truth.geojson", csv_path)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(tmp_path / "synth.pt"), "--source",
                        str(tmp_path / "jpegs"), "--save-txt", "--save-conf", "--nosave", "--project", str(tmp_path / "runs"), "--name", "ev",
                        "--batch-size", "4", "--geocode-bboxes", csv_path, "--facilities", "--facilities-conf", "0.25", "--facilities-eps", "25",
                        "--facilities-min-cages", "4", "--evaluate", truth_path, *GRID_ARGS], capture_output=True, text=True, timeout=420)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    run = tmp_path / "runs" / "ev"
    print(" ".join(l for l in (r.stdout + r.stderr).splitlines() if "evaluated" in l))
    assert "evaluate" not in json.load(open(run / "run_params.json"))
    table = geocode.geocode_label_dir(str(run / "labels"), csv_path)
    want_dir = str(tmp_path / "want")
    evaluate.evaluate_table(table, truth_path, want_dir, *GRIDS, op=(0.25, 25.0, 4), cpu=True)
    s = same_files(str(run), want_dir)
    assert s["n_detections"] > 0 and s["n_labels"] > 500 and f"evaluated {s['n_detections']} detections" in r.stdout + r.stderr
