"""--evaluate on the host: the closed form of the precision / recall grid (evaluate.member_conf_numpy, box_match_numpy and the counting)
against the reference's procedure done literally -- filter by confidence, sklearn.cluster.DBSCAN per year, members, brute-force closed-box
join -- on the 991 human labels of two scenes (tests/golden/g12_humanlabels_1956_1962.json) and 1,095 detections derived from them by a
seeded rule; the truth loader, the files, the options and the facility-level numbers of a hand-built case.  The inputs and the oracle are
shared with tests/test_gpu_evaluate.py."""
import functools
import itertools
import json
import os
import tempfile

import numpy as np
import pytest

from test_facilities import no_near_ties

from aquaculture_amd import evaluate, facilities, geocode

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g12_humanlabels_1956_1962.json")
CIRCLE, SQUARE = facilities.CLS_OF["circle_farm"], facilities.CLS_OF["square_farm"]
SEED = 12
SMALL_GRID = (np.array([0.6, 0.785, 0.95]), np.array([10, 50]), np.array([1, 5, 10]))


def write_truth_geojson(path, extra=()):
    """The fixture as the GeoJSON FeatureCollection it was cut from (rings in shapely.geometry.box's order); extra = further features."""
    g = json.load(open(GOLDEN))
    feats = []
    for (x0, y0, x1, y1), im, ty, yr in zip(g["bounds"], g["image"], g["type"], g["year"]):
        feats.append({"type": "Feature", "properties": {"image": g["images"][im], "type": ty, "year": yr},
                      "geometry": {"type": "Polygon", "coordinates": [[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]]}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": g["crs"], "features": feats + list(extra)}, f)
    return path


@functools.lru_cache(maxsize=None)
def truth():
    """The fixture through load_truth_geojson, loaded once and shared; treat as read-only."""
    with tempfile.TemporaryDirectory() as d:
        return evaluate.load_truth_geojson(write_truth_geojson(os.path.join(d, "truth.geojson")))


@functools.lru_cache(maxsize=None)
def detection_table(seed=SEED):
    """1,095 detections as geocode's table, derived from the labels: 895 labels (drawn without replacement) copied with their corners
    jittered by N(0, 1.5 m), 200 strays -- a box of a label's size N(0, 60 m) away from it --, 30 type flips, confidences from a Beta(5, 1.5)
    rounded to 6 places and then, for every fourth detection, copied from another one, so that ties occur."""
    t = truth()
    r = np.random.default_rng(seed)
    L = t["cls"].shape[0]
    src = np.concatenate([r.permutation(L)[:895], r.integers(0, L, 200)])
    box = np.stack([t[c][src] for c in evaluate.BOX_COLUMNS], 1)
    box[:895] += r.normal(0, 1.5, (895, 4))
    box[895:] += np.tile(r.normal(0, 60.0, (200, 2)), 2)
    box = np.stack([np.minimum(box[:, 0], box[:, 2]), np.minimum(box[:, 1], box[:, 3]), np.maximum(box[:, 0], box[:, 2]), np.maximum(box[:, 1], box[:, 3])], 1)
    cls = t["cls"][src].copy()
    flip = r.permutation(1095)[:30]
    cls[flip] = np.where(cls[flip] == SQUARE, CIRCLE, SQUARE)
    conf = np.round(r.beta(5.0, 1.5, 1095), 6)
    conf[::4] = conf[r.integers(0, 1095, conf[::4].shape[0])]
    order = r.permutation(1095)
    stems = sorted({os.path.splitext(s)[0] for s in t["image"]})
    image = np.asarray([stems.index(os.path.splitext(s)[0]) for s in t["image"][src]], np.int64)
    table = {"cls": cls[order], "det_conf": conf[order], "year": t["year"][src][order], "image": image[order], "stems": np.asarray(stems, dtype=object)}
    table.update({c: np.ascontiguousarray(box[order, i]) for i, c in enumerate(evaluate.BOX_COLUMNS)})
    return table


@functools.lru_cache(maxsize=None)
def fixture_data():
    """evaluate.inputs of the fixture, built once and shared; treat as read-only."""
    return evaluate.inputs(detection_table(), truth())


class Oracle:
    """The reference's procedure, literally, for one grid point at a time."""

    def __init__(self, data):
        self.det, self.lab = data["det"], data["lab"]
        d, l = self.det["box"], self.lab["box"]
        meet = ((d[:, None, 0] <= l[None, :, 2]) & (l[None, :, 0] <= d[:, None, 2]) & (d[:, None, 1] <= l[None, :, 3]) & (l[None, :, 1] <= d[:, None, 3]))
        self.meet = meet & (self.det["year"][:, None] == self.lab["year"][None, :]) & (self.det["cls"][:, None] == self.lab["cls"][None, :])

    def members(self, conf, eps, min_size):
        from sklearn.cluster import DBSCAN
        take = self.det["conf"] >= conf                     # predictions_cluster: preds[preds['det_conf'] >= conf_thresh]
        member = np.zeros(take.shape[0], bool)
        for y in np.unique(self.det["year"][take]):         # DBSCAN_cluster: per year
            idx = np.nonzero(take & (self.det["year"] == y))[0]
            labels = DBSCAN(eps=eps, min_samples=int(min_size)).fit(self.det["xy"][idx]).labels_
            member[idx[labels != -1]] = True                # facility_detections
        return member

    def counts(self, conf, eps, min_size):
        """(n_pred, n_pred_tp, n_label, n_label_tp) of get_stats_total"""
        m = self.members(conf, eps, min_size)
        return int(m.sum()), int((m & self.meet.any(1)).sum()), self.meet.shape[1], int(self.meet[m].any(0).sum())


@functools.lru_cache(maxsize=None)
def oracle():
    return Oracle(fixture_data())


def table_counts(table, k):
    return tuple(int(table[c][k]) for c in ("n_pred", "n_pred_tp", "n_label", "n_label_tp"))


def assert_no_near_ties(data, eps_values):
    for eps in eps_values:
        assert no_near_ties(data["det"]["xy"], data["det"]["year_id"], float(eps)), f"a pair too close to eps = {eps} for an exact comparison: change SEED"


# ---- the grid ----

@functools.lru_cache(maxsize=None)
def cpu_grid():
    """The numpy restatement's table over the full default grid, computed once and shared; treat as read-only."""
    return evaluate.grid(fixture_data(), cpu=True)


def test_fixture_is_what_the_tests_assume():
    t, data = truth(), fixture_data()
    assert t["cls"].shape[0] == 991 and os.path.getsize(GOLDEN) < 300 * 1024
    assert data["det"]["conf"].shape[0] == 1095 and data["lab"]["conf"].shape[0] == 991 and (data["lab"]["conf"] == 1.0).all()
    conf = data["det"]["conf"]
    assert np.unique(conf).shape[0] < conf.shape[0] and (np.round(conf, 6) == conf).all()          # ties
    assert set(np.unique(data["det"]["cls"])) == {CIRCLE, SQUARE} and data["years"].tolist() == [2003, 2008, 2011, 2014, 2017, 2020]
    assert (data["det"]["group"] == data["det"]["year_id"] * 2 + (data["det"]["cls"] == SQUARE)).all()


def test_default_grids_are_the_references():
    assert np.array_equal(evaluate.DEFAULT_CONF, np.arange(0.6, 1.01, 0.005)) and evaluate.DEFAULT_CONF.shape[0] == 82
    assert np.array_equal(evaluate.DEFAULT_EPS, np.arange(10, 151, 20)) and np.array_equal(evaluate.DEFAULT_MIN, np.arange(1, 11))


def test_grid_rows_are_in_product_order():
    g = cpu_grid()
    want = list(itertools.product(evaluate.DEFAULT_CONF.tolist(), evaluate.DEFAULT_EPS.tolist(), evaluate.DEFAULT_MIN.tolist()))
    assert len(want) == 6560 and tuple(g) == evaluate.COLUMNS
    assert list(zip(g["conf_thresh"].tolist(), g["distance_threshold"].tolist(), g["min_cluster_size"].tolist())) == want
    assert (g["n_label"] == 991).all() and (g["n_pred_tp"] <= g["n_pred"]).all() and (g["n_label_tp"] <= g["n_label"]).all()
    assert np.isnan(g["precision"][g["n_pred"] == 0]).all() and (g["n_pred"] == 0).any() and (g["n_pred"] > 500).any()


def test_full_grid_every_seventh_point_equals_the_oracle():
    data, g, o = fixture_data(), cpu_grid(), oracle()
    assert_no_near_ties(data, evaluate.DEFAULT_EPS)
    bad = []
    for k in range(0, 6560, 7):
        want = o.counts(float(g["conf_thresh"][k]), float(g["distance_threshold"][k]), int(g["min_cluster_size"][k]))
        if table_counts(g, k) != want:
            bad.append((k, table_counts(g, k), want))
    assert not bad, (len(bad), bad[:5])


def test_small_grid_every_point_equals_the_oracle():
    data, o = fixture_data(), oracle()
    assert_no_near_ties(data, SMALL_GRID[1])
    g = evaluate.grid(data, *SMALL_GRID, cpu=True)
    assert g["n_pred"].shape[0] == 18
    for k, (c, e, m) in enumerate(itertools.product(*(v.tolist() for v in SMALL_GRID))):
        assert (g["conf_thresh"][k], g["distance_threshold"][k], g["min_cluster_size"][k]) == (c, e, m)
        assert table_counts(g, k) == o.counts(c, e, m), (c, e, m)
    # the rates are the reference's expressions on those counts
    with np.errstate(invalid="ignore"):
        p, r = g["n_pred_tp"] / g["n_pred"], g["n_label_tp"] / g["n_label"]
    assert np.isnan(p).any() and np.array_equal(g["precision"], p, equal_nan=True) and np.array_equal(g["recall"], r)
    assert np.array_equal(g["product"], p * r, equal_nan=True) and np.array_equal(g["f_score"], 2 * (p * r / (p + r)), equal_nan=True)


def test_member_conf_is_a_threshold_on_sklearns_membership():
    """M(i, m) itself, not only the counts: at thresholds just at and just above it."""
    data, o = fixture_data(), oracle()
    det = data["det"]
    M = evaluate.member_conf_numpy(det["xy"], det["year_id"], det["conf"], 50.0, 10)
    assert M.shape == (1095, 10) and (np.isin(M, det["conf"]) | np.isneginf(M)).all() and (M[:, 1:] <= M[:, :-1]).all()
    for m in (1, 5, 10):
        for c in (0.7, 0.9):
            assert np.array_equal(M[:, m - 1] >= c, o.members(c, 50.0, m))
    with pytest.raises(ValueError):
        evaluate.member_conf_numpy(det["xy"], det["year_id"], det["conf"], 50.0, 17)
    with pytest.raises(ValueError):
        evaluate.member_conf_numpy(det["xy"], det["year_id"], det["conf"], 0.0, 5)
    assert evaluate.member_conf_numpy(np.zeros((0, 2)), np.zeros(0), np.zeros(0), 10.0, 3).shape == (0, 3)


def test_bad_grids_are_refused():
    data = fixture_data()
    for grids in ((np.array([0.5]), np.array([10]), np.array([0])), (np.array([0.5]), np.array([10]), np.array([17])),
                  (np.array([0.5]), np.array([10]), np.array([2.0])), (np.array([0.5]), np.array([0.0]), np.array([2])),
                  (np.array([]), np.array([10]), np.array([2]))):
        with pytest.raises(ValueError):
            evaluate.grid(data, *grids, cpu=True)


# ---- the truth loader, the image list, the options ----

def test_truth_loader_maps_types_drops_the_others_and_takes_bounds(tmp_path):
    poly = lambda ring: {"type": "Polygon", "coordinates": [ring]}
    extra = [{"type": "Feature", "properties": {"image": "a.jpeg", "type": "other_cage", "year": 2001}, "geometry": poly([[0, 0], [1, 0], [1, 1], [0, 0]])},
             {"type": "Feature", "properties": {"image": "b.jpeg", "type": "circle_cage", "year": 2002},
              "geometry": poly([[5.5, -2.0], [7.25, 1.0], [6.0, 3.5], [4.0, 0.5], [5.5, -2.0]])}]
    t = evaluate.load_truth_geojson(write_truth_geojson(str(tmp_path / "t.geojson"), extra))
    g = json.load(open(GOLDEN))
    assert t["cls"].shape[0] == 992 and t["image"][-1] == "b.jpeg" and t["year"][-1] == 2002 and t["cls"][-1] == CIRCLE
    assert [t[c][-1] for c in evaluate.BOX_COLUMNS] == [4.0, -2.0, 7.25, 3.5]
    assert np.array_equal(np.stack([t[c][:991] for c in evaluate.BOX_COLUMNS], 1), np.asarray(g["bounds"]))
    want_cls = [CIRCLE if ty == "circle_cage" else SQUARE for ty in g["type"]]
    assert t["cls"][:991].tolist() == want_cls and t["year"][:991].tolist() == g["year"]
    assert t["image"][:991].tolist() == [g["images"][i] for i in g["image"]]
    bad = {"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::4326"}}, "features": []}
    (tmp_path / "bad.geojson").write_text(json.dumps(bad))
    with pytest.raises(ValueError, match="3857"):
        evaluate.load_truth_geojson(str(tmp_path / "bad.geojson"))


def test_only_circle_and_square_detections_and_kept_rows_take_part():
    table = {k: (v.copy() if k != "stems" else v) for k, v in detection_table().items()}
    table["cls"][:10] = facilities.CLS_OF["rectangle_farm"]
    keep = np.ones(1095, bool)
    keep[10:30] = False
    data = evaluate.inputs(table, truth(), keep=keep)
    assert data["det"]["rows"].tolist() == list(range(30, 1095))
    with pytest.raises(ValueError, match="keep"):
        evaluate.inputs(table, truth(), keep=keep[:5])


def test_image_list_restricts_detections_and_labels(tmp_path):
    t, table = truth(), detection_table()
    names = sorted(set(t["image"]))[:10]
    (tmp_path / "fold.txt").write_text("\n".join(names[:5]) + "\n\n" + "\n".join(os.path.splitext(n)[0] for n in names[5:]) + "\n")
    images = evaluate.read_image_list(str(tmp_path / "fold.txt"))
    assert len(images) == 10
    data = evaluate.inputs(table, t, images=images)
    want_l = np.nonzero(np.isin(t["image"], names))[0]
    stems = {os.path.splitext(n)[0] for n in names}
    want_d = np.nonzero([table["stems"][i] in stems for i in table["image"]])[0]
    assert 0 < want_l.shape[0] < 991 and 0 < want_d.shape[0] < 1095
    assert np.array_equal(data["lab"]["rows"], want_l) and np.array_equal(data["det"]["rows"], want_d)
    # the restricted grid is the oracle's on the restricted inputs
    g = evaluate.grid(data, np.array([0.7]), np.array([50]), np.array([3]), cpu=True)
    assert table_counts(g, 0) == Oracle(data).counts(0.7, 50, 3)


def test_grid_options():
    assert np.array_equal(evaluate.parse_grid("0.6:1.01:0.005"), np.arange(0.6, 1.01, 0.005))
    assert np.array_equal(evaluate.parse_grid("10:151:20"), np.arange(10, 151, 20)) and evaluate.parse_grid("10:151:20").dtype.kind == "i"
    assert evaluate.parse_grid("0.785").tolist() == [0.785] and evaluate.parse_grid("10, 50,90.5").tolist() == [10.0, 50.0, 90.5]
    assert evaluate.parse_grid("1:11:1", integer=True).tolist() == list(range(1, 11)) and evaluate.parse_grid("5,3", integer=True).tolist() == [5, 3]
    for bad, integer in (("", False), ("a:b:c", False), ("1:2", False), ("1:1:1", False), ("2.5", True), ("x", False)):
        with pytest.raises(ValueError):
            evaluate.parse_grid(bad, integer)
    c, e, m = evaluate.grids_from_options(None, None, None)
    assert c is evaluate.DEFAULT_CONF and e is evaluate.DEFAULT_EPS and m is evaluate.DEFAULT_MIN
    c, e, m = evaluate.grids_from_options("0.5,0.6", "10:31:10", "2,4")
    assert c.tolist() == [0.5, 0.6] and e.tolist() == [10, 20, 30] and m.tolist() == [2, 4]


def test_detect_py_options():
    from aquaculture_amd import detect
    with pytest.raises(SystemExit):
        detect.parse_opt(["--evaluate", "truth.geojson"])                        # needs --geocode-bboxes
    with pytest.raises(SystemExit):
        detect.parse_opt(["--evaluate", "truth.geojson", "--geocode-bboxes", "wb.csv", "--evaluate-min-cages", "1.5"])
    with pytest.raises(ValueError, match="--geocode-bboxes"):
        detect.run("w.pt", "src", evaluate="truth.geojson")
    opt = detect.parse_opt(["--evaluate", "truth.geojson", "--geocode-bboxes", "wb.csv", "--evaluate-eps", "10,50", "--evaluate-images", "fold.txt"])
    assert (opt.evaluate, opt.evaluate_out, opt.evaluate_conf, opt.evaluate_eps, opt.evaluate_min_cages, opt.evaluate_images) == \
        ("truth.geojson", None, None, "10,50", None, "fold.txt")
    assert detect.parse_opt([]).evaluate is None
    assert "evaluate" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)


# ---- the files ----

def test_idxmax_is_pandas():
    import pandas as pd
    nan = float("nan")
    for v in ([nan, 0.2, 0.7, 0.7, nan, 0.1], [0.3], [nan, nan, 0.0], [0.5, nan, 0.9, 0.9]):
        assert evaluate.idxmax(v) == int(pd.Series(v).idxmax()), v
    assert evaluate.idxmax([nan, nan]) is None and evaluate.idxmax([]) is None


def test_csv_and_json_round_trip(tmp_path):
    data = fixture_data()
    conf = np.array([0.6, 0.95, 1.0, 1.5])                  # nothing survives 1.5: NaN precision
    g = evaluate.grid(data, conf, np.array([10, 50]), np.array([2, 5]), cpu=True)
    assert np.isnan(g["precision"][-4:]).all() and (g["n_pred"][-4:] == 0).all()
    path = str(tmp_path / "perf.csv")
    assert evaluate.write_performance_csv(path, g) == 16
    lines = open(path).read().splitlines()
    assert lines[0] == ",".join(evaluate.COLUMNS) and len(lines) == 17
    assert lines[-1].split(",")[:5] == ["1.5", "50", "5", "", "0.0"] and lines[-1].split(",")[5:7] == ["", ""]
    back = evaluate.read_performance_csv(path)
    for c in evaluate.COLUMNS:
        assert np.array_equal(back[c], np.asarray(g[c], back[c].dtype), equal_nan=True), c
    op = evaluate.operating_point(data, 0.785, 50.0, 5, cpu=True)
    s = evaluate.summary(data, g, op)
    text = json.dumps(s)
    assert "NaN" not in text and json.loads(text) == s
    k = evaluate.idxmax(g["f_score"])
    assert s["best_f_score"]["row"] == k and s["best_f_score"]["f_score"] == float(g["f_score"][k]) and s["best_f_score"]["n_pred"] == int(g["n_pred"][k])
    assert s["best_product"]["row"] == evaluate.idxmax(g["product"]) and s["n_detections"] == 1095 and s["n_labels"] == 991 and s["grid_rows"] == 16


def test_evaluate_table_writes_both_files(tmp_path):
    truth_path = write_truth_geojson(str(tmp_path / "truth.geojson"))
    out = str(tmp_path / "out")
    s = evaluate.evaluate_table(detection_table(), truth_path, out, *SMALL_GRID, op=(0.785, 50.0, 5), cpu=True)
    assert json.load(open(os.path.join(out, evaluate.JSON_FILE))) == s
    back = evaluate.read_performance_csv(os.path.join(out, evaluate.CSV_FILE))
    want = evaluate.grid(fixture_data(), *SMALL_GRID, cpu=True)
    for c in evaluate.COLUMNS:
        assert np.array_equal(back[c], np.asarray(want[c], back[c].dtype), equal_nan=True), c
    assert "evaluated 1095 detections against 991 labels over 18 combinations" in evaluate.describe(s)


# ---- the operating point ----

def test_operating_point_cage_level_is_the_grid_row_and_the_oracle():
    data, o = fixture_data(), oracle()
    assert_no_near_ties(data, [50.0])
    op = evaluate.operating_point(data, 0.785, 50.0, 5, cpu=True)
    cage = op["cage"]
    assert (cage["n_pred"], cage["n_pred_tp"], cage["n_label"], cage["n_label_tp"]) == o.counts(0.785, 50.0, 5)
    g = evaluate.grid(data, np.array([0.785]), np.array([50]), np.array([5]), cpu=True)
    assert table_counts(g, 0) == o.counts(0.785, 50.0, 5) and cage["precision"] == g["precision"][0] and cage["f_score"] == g["f_score"][0]
    fac = op["facility"]
    assert 0 < fac["n_pred_tp"] <= fac["n_pred"] and 0 < fac["n_label_tp"] <= fac["n_label"]


def hand_built_case():
    """Year 2015, squares of 10 m every 15 m (EPSG:3857; about 11 m on the ground at 43.3 N): label facilities A (4 cages) and B (4 cages,
    1 km east); detections on A's cages (shifted by 1 m), 4 more 3 km east where there is no label, and one stray of low confidence on B."""
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    row = lambda x: [[x + 15.0 * k, y0, x + 15.0 * k + 10.0, y0 + 10.0] for k in range(4)]
    lab = np.asarray(row(x0) + row(x0 + 1000.0))
    det = np.asarray(row(x0 + 1.0) + row(x0 + 3000.0) + [[x0 + 1000.0, y0, x0 + 1010.0, y0 + 10.0]])
    truth_ = {c: lab[:, i].copy() for i, c in enumerate(evaluate.BOX_COLUMNS)}
    truth_.update(cls=np.full(8, SQUARE, np.int64), year=np.full(8, 2015, np.int64), image=np.asarray(["t.jpeg"] * 8, dtype=object))
    table = {c: det[:, i].copy() for i, c in enumerate(evaluate.BOX_COLUMNS)}
    table.update(cls=np.full(9, SQUARE, np.int64), year=np.full(9, 2015, np.int64), image=np.zeros(9, np.int64), stems=np.asarray(["t"], dtype=object),
                 det_conf=np.asarray([0.9] * 8 + [0.4]))
    return evaluate.inputs(table, truth_)


def check_hand_built(op):
    fac, cage = op["facility"], op["cage"]
    assert (fac["n_pred"], fac["n_pred_tp"], fac["n_label"], fac["n_label_tp"]) == (2, 1, 2, 1)
    assert fac["precision"] == 0.5 and fac["recall"] == 0.5 and fac["product"] == 0.25 and fac["f_score"] == 0.5
    assert (cage["n_pred"], cage["n_pred_tp"], cage["n_label"], cage["n_label_tp"]) == (8, 4, 8, 4)


def test_facility_level_numbers_of_a_hand_built_case():
    data = hand_built_case()
    check_hand_built(evaluate.operating_point(data, 0.5, 20.0, 3, cpu=True))
    # at threshold 0.3 the stray is still no member (it has no neighbour), so nothing changes; with min 1 it is a facility of its own on B
    check_hand_built(evaluate.operating_point(data, 0.3, 20.0, 3, cpu=True))
    fac = evaluate.operating_point(data, 0.3, 20.0, 1, cpu=True)["facility"]
    assert (fac["n_pred"], fac["n_pred_tp"], fac["n_label"], fac["n_label_tp"]) == (3, 2, 2, 2)
    # a different year never matches
    data["det"]["year_id"] = data["det"]["year_id"] + 1
    data["det"]["group"] = data["det"]["group"] + 2
    data["years"] = np.array([2015, 2016])
    fac = evaluate.operating_point(data, 0.5, 20.0, 3, cpu=True)["facility"]
    assert (fac["n_pred"], fac["n_pred_tp"], fac["n_label"], fac["n_label_tp"]) == (2, 0, 2, 0)


def test_box_match_numpy_is_a_closed_join():
    q = np.array([[0.0, 0.0, 1.0, 1.0], [1.0, 1.0, 2.0, 2.0], [5.0, 5.0, 5.0, 5.0], [3.0, 0.0, 4.0, 1.0]])
    k = np.array([[1.0, 0.0, 2.0, 1.0], [5.0, 4.0, 6.0, 5.0], [0.0, 0.0, 9.0, 9.0]])
    pay = np.array([[0.25, 1.0], [0.5, 2.0], [0.75, 3.0]])
    hit, out = evaluate.box_match_numpy(q, [0, 0, 0, 0], k, [0, 0, 1], payload=pay)
    assert hit.tolist() == [True, True, True, False]        # an edge, a corner, a point on an edge, nothing
    assert out.tolist() == [[0.25, 1.0], [0.25, 1.0], [0.5, 2.0], [-np.inf, -np.inf]]
    hit, out = evaluate.box_match_numpy(q, [1, 1, 7, 1], k, [0, 0, 1])
    assert hit.tolist() == [True, True, False, True] and out is None


# ---- the ABI ----

def test_symbols_are_declared_exported_and_bound(lib):
    """Fails without the feature: the header declares the three entry points, engine.py lists and binds them, the library has them."""
    import ctypes
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_eval_scratch_bytes", "aq_eval_member_conf_f64", "aq_box_match_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.aq_eval_scratch_bytes.restype is ctypes.c_size_t
    assert lib.aq_eval_scratch_bytes(0, 4) == 0 and lib.aq_eval_scratch_bytes(1 << 31, 4) == 0
    assert lib.aq_eval_scratch_bytes(1000, 0) == 0 and lib.aq_eval_scratch_bytes(1000, 17) == 0
    assert lib.aq_eval_scratch_bytes(1000, 10) == 16000 + 24000 + 8000 + 80000
    assert lib.aq_eval_scratch_bytes(1001, 1) == 16016 + 24032 + 8016 + 8016
    assert engine.EVAL_MAX_K == evaluate.MAX_K == 16
    assert ("evaluate.hip", ["-ffp-contract=off"]) in build.SOURCES
