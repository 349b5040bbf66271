"""--model-errors on the host: the numpy restatement of the two kernels (model_errors.match_numpy, moments_numpy) against the reference's
procedure done pair by pair (literal_numpy) and scipy.stats.norm.fit, on the 991 human labels of tests/golden/g13_model_error_labels.json
and as many detections made from them by a seeded jitter; the EPSG:3857-rectangle overlap against a polygon clip in EPSG:3035; the match
and moment rules on hand-built cases; the truth loader, the files and the options.  The inputs are shared with
tests/test_gpu_model_errors.py."""
import functools
import json
import os
import tempfile

import numpy as np
import pytest

from aquaculture_amd import evaluate, facilities, geocode, model_errors, tonnage

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "g13_model_error_labels.json")
CIRCLE, SQUARE = facilities.CLS_OF["circle_farm"], facilities.CLS_OF["square_farm"]
CONF = 0.5
NAN = float("nan")


def truth_feature(x0, y0, x1, y1, ty, year, image="ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0.jpeg", px=(100.0, 100.0, 200.0, 200.0), size=(1024, 1024)):
    props = {"image": image, "type": ty, "year": year, "xmin": px[0], "ymin": px[1], "xmax": px[2], "ymax": px[3],
             "jpeg_width": size[0], "jpeg_height": size[1]}
    return {"type": "Feature", "properties": props,
            "geometry": {"type": "Polygon", "coordinates": [[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]]}}


def write_features(path, feats, crs=None):
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": crs or {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}},
                   "features": list(feats)}, f)
    return str(path)


def write_truth_geojson(path):
    """The fixture as the GeoJSON FeatureCollection it was cut from (rings in shapely.geometry.box's order)."""
    g = json.load(open(GOLDEN))
    feats = []
    for k, ((x0, y0, x1, y1), im, ty, yr) in enumerate(zip(g["bounds"], g["image"], g["type"], g["year"])):
        feats.append(truth_feature(x0, y0, x1, y1, ty, yr, g["images"][im], tuple(g[c][k] for c in ("xmin", "ymin", "xmax", "ymax")),
                                   (g["jpeg_width"][k], g["jpeg_height"][k])))
    return write_features(path, feats, g["crs"])


@functools.lru_cache(maxsize=None)
def truth():
    """The fixture through model_errors.load_truth_geojson, loaded once and shared; treat as read-only."""
    with tempfile.TemporaryDirectory() as d:
        return model_errors.load_truth_geojson(write_truth_geojson(os.path.join(d, "truth.geojson")))


def table_from_boxes(box, cls, year, conf, px, stems, image):
    """geocode's detection table for EPSG:3857 boxes [n, 4]: the EPSG:3035 columns as geocode_detections makes them (two corners)."""
    box = np.asarray(box, np.float64).reshape(-1, 4)
    e_min, n_max = geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(box[:, 0], box[:, 3]))
    e_max, n_min = geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(box[:, 2], box[:, 1]))
    px = np.asarray(px, np.int64).reshape(-1, 4)
    t = {"cls": np.asarray(cls, np.int64), "det_conf": np.asarray(conf, np.float64), "year": np.asarray(year, np.int64),
         "image": np.asarray(image, np.int64), "stems": np.asarray(stems, dtype=object),
         "e_min_3035": e_min, "e_max_3035": e_max, "n_min_3035": n_min, "n_max_3035": n_max,
         "xmin": px[:, 0], "ymin": px[:, 1], "xmax": px[:, 2], "ymax": px[:, 3]}
    t.update({c: np.ascontiguousarray(box[:, i]) for i, c in enumerate(evaluate.BOX_COLUMNS)})
    return t


@functools.lru_cache(maxsize=None)
def detection_table(seed=0):
    """One detection per label: its corners jittered by N(0, 0.15 x side) (seed 0), its type, year, image and (truncated) pixel box kept, a
    confidence above CONF.  The labels of a facility lie side by side, so nearly every detection meets several labels."""
    t = truth()
    r = np.random.default_rng(seed)
    box = np.stack([t[c] for c in evaluate.BOX_COLUMNS], 1)
    w, h = box[:, 2] - box[:, 0], box[:, 3] - box[:, 1]
    box = box + r.normal(0.0, 1.0, box.shape) * 0.15 * np.stack([w, h, w, h], 1)
    box = np.stack([np.minimum(box[:, 0], box[:, 2]), np.minimum(box[:, 1], box[:, 3]), np.maximum(box[:, 0], box[:, 2]), np.maximum(box[:, 1], box[:, 3])], 1)
    stems = sorted({os.path.splitext(s)[0] for s in t["image"]})
    image = [stems.index(os.path.splitext(s)[0]) for s in t["image"]]
    px = np.trunc(np.stack([t[c] for c in ("xmin", "ymin", "xmax", "ymax")], 1))
    return table_from_boxes(box, t["cls"], t["year"], r.uniform(0.6, 1.0, box.shape[0]), px, stems, image)


@functools.lru_cache(maxsize=None)
def fixture_samples():
    """model_errors.samples of the fixture, built once and shared; treat as read-only."""
    return model_errors.samples(detection_table(), truth(), CONF)


@functools.lru_cache(maxsize=None)
def fixture_match():
    s = fixture_samples()
    q, k = s["q"], s["k"]
    return model_errors.match_numpy(q["box"], q["group"], q["area"], k["box"], k["group"], k["area"])


def candidates(q, k):
    """bool [Q, N]: the candidate pairs by brute force."""
    a, b = q["box"][:, None, :], k["box"][None, :, :]
    return ((b[..., 0] <= a[..., 2]) & (a[..., 0] <= b[..., 2]) & (b[..., 1] <= a[..., 3]) & (a[..., 1] <= b[..., 3]) &
            (q["group"][:, None] == k["group"][None, :]))


# ---- (a) the restatement against the literal procedure and scipy ----

def test_fixture_is_what_the_tests_assume():
    t, s = truth(), fixture_samples()
    assert t["cls"].shape[0] == 991 and os.path.getsize(GOLDEN) < 300 * 1024 and len(set(t["image"])) == 42
    assert np.array_equal(t["feature"], np.arange(991)) and set(t["jpeg_width"]) == {1024.0}
    assert s["q"]["box"].shape == (991, 4) and s["k"]["box"].shape == (991, 4) and s["G"] == 12
    assert s["passes"] == ["2000-2004", "2005-2009", "2010-2012", "2013-2015", "2016-2018", "2019-2021"] and (s["q"]["mgroup"] >= 0).all()
    cand = candidates(s["q"], s["k"])
    per_query = cand.sum(1)
    assert (per_query >= 2).sum() >= 900 and per_query.max() >= 5, ((per_query >= 2).sum(), per_query.max())      # no easy join
    # no exact tie, and the best and the second best overlap apart by far more than the 2.4e-4 the projections differ by
    a, b = s["q"]["box"][:, None, :], s["k"]["box"][None, :, :]
    inter = np.where(cand, (np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0])) *
                     (np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1])), -1.0)
    top = np.sort(inter, 1)[:, -2:]
    two = top[:, 0] >= 0
    assert ((top[two, 1] - top[two, 0]) / top[two, 1]).min() > 1e-3


def test_match_and_moments_are_the_literal_procedures():
    from scipy.stats import norm
    s = fixture_samples()
    q, k, passes = s["q"], s["k"], s["passes"]
    match, overlap, error = fixture_match()
    assert (candidates(q, k).sum(1) >= 2).sum() >= 900      # not an easy join: nearly every query has to choose
    lit = model_errors.literal_numpy(q, k, passes)
    assert match.dtype == np.int32 and np.array_equal(match, lit["match"])
    assert error.tobytes() == lit["error"].tobytes()
    assert (match >= 0).sum() > 950 and (overlap[match >= 0] > 0).all() and (overlap[match >= 0] <= 100.0 * (1 + 4e-16)).all()      # (three roundings)
    assert np.isnan(overlap[match < 0]).all() and np.isnan(error[match < 0]).all()
    n, mean, sd = model_errors.moments_numpy(error, match, q["mgroup"], 2 * len(passes))
    fitted = 0
    for i, g in enumerate((p, t) for p in passes for t in model_errors.FARM_TYPES):
        errs = lit["errors"][g]
        assert n[i] == len(errs), g
        if not errs:
            assert np.isnan(mean[i]) and np.isnan(sd[i])
            continue
        mu, std = norm.fit(np.asarray(errs))
        print(g, int(n[i]), mean[i], sd[i], mu, std)
        np.testing.assert_allclose(mean[i], mu, rtol=1e-10)
        np.testing.assert_allclose(sd[i], std, rtol=1e-10)
        fitted += 1
        assert n[i] == 1 or sd[i] > 0.05 * np.abs(np.asarray(errs)).max()           # an sd of the order of the errors
    assert fitted >= 6 and n.sum() == (match >= 0).sum()


# ---- (b) the EPSG:3857-rectangle overlap against a polygon clip in EPSG:3035 ----

def to_3035(box):
    """[n, 4] EPSG:3857 boxes -> [n, 4, 2] quadrilaterals in EPSG:3035 (shapely.geometry.box's ring)."""
    x0, y0, x1, y1 = box[:, 0], box[:, 1], box[:, 2], box[:, 3]
    en = [geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(x, y)) for x, y in ((x1, y0), (x1, y1), (x0, y1), (x0, y0))]
    return np.stack([np.stack(c, 1) for c in en], 1)


def shoelace(poly):
    x, y = poly[:, 0], poly[:, 1]
    return 0.5 * float(np.sum(x * np.roll(y, -1) - np.roll(x, -1) * y))


def clip(subject, clipper):
    """Sutherland-Hodgman: the part of the convex polygon `subject` inside the convex, counter-clockwise polygon `clipper` ([m, 2] each)."""
    out = subject
    for i in range(clipper.shape[0]):
        a, b = clipper[i], clipper[(i + 1) % clipper.shape[0]]
        if out.shape[0] == 0:
            break
        side = (b[0] - a[0]) * (out[:, 1] - a[1]) - (b[1] - a[1]) * (out[:, 0] - a[0])       # >= 0: inside
        nxt, side_n = np.roll(out, -1, 0), np.roll(side, -1)
        pts = []
        for p, pn, s0, s1 in zip(out, nxt, side, side_n):
            if s0 >= 0:
                pts.append(p)
            if (s0 >= 0) != (s1 >= 0):
                pts.append(p + (pn - p) * (s0 / (s0 - s1)))
        out = np.asarray(pts, np.float64).reshape(-1, 2)
    return out


def test_rectangle_overlap_chooses_the_label_the_polygon_clip_chooses():
    s = fixture_samples()
    q, k = s["q"], s["k"]
    match, overlap, _ = fixture_match()
    cand = candidates(q, k)
    qp, kp = to_3035(q["box"]), to_3035(k["box"])
    worst = 0.0
    for i in range(q["box"].shape[0]):
        origin = qp[i, 0]
        poly = qp[i] - origin
        if shoelace(poly) < 0:
            poly = poly[::-1]
        area_q = shoelace(poly)
        best, best_j = -1.0, -1
        for j in np.nonzero(cand[i])[0]:
            other = kp[j] - origin
            if shoelace(other) < 0:
                other = other[::-1]
            part = clip(poly, other)
            ov = 100.0 * (shoelace(part) if part.shape[0] >= 3 else 0.0) / area_q
            if ov > best:
                best, best_j = ov, int(j)
        assert best_j == match[i], (i, best_j, match[i])
        if best_j >= 0:
            worst = max(worst, abs(best - overlap[i]) / overlap[i])
    print(f"largest relative difference of overlap, EPSG:3035 polygons against EPSG:3857 rectangles: {worst:.3e}")
    assert worst < 1e-3          # far below the smallest gap between a best and a second-best candidate (test_fixture_is_what_the_tests_assume)


# ---- (c) the rules ----

def run_match(qbox, kbox, qgroup=None, kgroup=None, qarea=None, karea=None):
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup = np.zeros(qbox.shape[0], np.int32) if qgroup is None else np.asarray(qgroup, np.int32)
    kgroup = np.zeros(kbox.shape[0], np.int32) if kgroup is None else np.asarray(kgroup, np.int32)
    qarea = np.ones(qbox.shape[0]) if qarea is None else np.asarray(qarea, np.float64)
    karea = np.arange(kbox.shape[0], dtype=np.float64) + 10.0 if karea is None else np.asarray(karea, np.float64)
    return model_errors.match_numpy(qbox, qgroup, qarea, kbox, kgroup, karea)


def test_match_rules():
    q = [[0.0, 0.0, 10.0, 10.0]]
    # identical labels: the smaller row, wherever it stands
    m, ov, err = run_match(q, [[20.0, 0.0, 30.0, 9.0], [2.0, 2.0, 8.0, 8.0], [2.0, 2.0, 8.0, 8.0]])
    assert m.tolist() == [1] and ov.tolist() == [36.0] and err.tolist() == [10.0]
    # a touching label (inter = 0) loses to an overlapping one and wins against none
    m, ov, _ = run_match(q, [[10.0, 0.0, 20.0, 10.0], [9.0, 9.0, 20.0, 20.0]])
    assert m.tolist() == [1] and ov.tolist() == [1.0]
    m, ov, err = run_match(q, [[10.0, 0.0, 20.0, 10.0], [30.0, 0.0, 40.0, 10.0]])
    assert m.tolist() == [0] and ov.tolist() == [0.0] and err.tolist() == [9.0]
    m, ov, err = run_match(q, [[11.0, 0.0, 20.0, 10.0]])
    assert m.tolist() == [-1] and np.isnan(ov).all() and np.isnan(err).all()
    # groups (year and type) must agree
    m, _, _ = run_match(q * 3, [[1.0, 1.0, 9.0, 9.0], [2.0, 2.0, 8.0, 8.0]], qgroup=[0, 1, 2], kgroup=[1, 0])
    assert m.tolist() == [1, 0, -1]
    # a NaN box matches nothing, on either side
    m, _, _ = run_match([[0.0, 0.0, NAN, 10.0], [0.0, 0.0, 10.0, 10.0]], [[1.0, NAN, 9.0, 9.0], [4.0, 4.0, 5.0, 5.0]])
    assert m.tolist() == [-1, 1]
    # a NaN inter (an unbounded box against a touching one: inf x 0) never wins over a number, and wins against nothing else
    inf = float("inf")
    m, ov, _ = run_match([[0.0, 0.0, inf, 10.0]], [[0.0, 10.0, inf, 20.0], [0.0, 10.0, 5.0, 20.0], [0.0, 10.0, inf, 30.0]])
    assert m.tolist() == [1]
    m, ov, _ = run_match([[0.0, 0.0, inf, 10.0]], [[5.0, 10.0, inf, 30.0], [0.0, 10.0, inf, 20.0]])
    assert m.tolist() == [0] and np.isnan(ov).all()
    # a query without area: the overlap is 0 / 0, stored as the canonical NaN; the error is a number
    m, ov, err = run_match([[5.0, 5.0, 5.0, 5.0]], [[0.0, 0.0, 10.0, 10.0]])
    assert m.tolist() == [0] and ov.tobytes() == np.array([np.nan]).tobytes() and err.tolist() == [9.0]
    m, ov, err = run_match(np.zeros((0, 4)), [[0.0, 0.0, 10.0, 10.0]])
    assert m.shape == (0,) and m.dtype == np.int32 and ov.shape == (0,) and err.shape == (0,)


def test_moment_rules():
    error = np.array([1.0, 2.0, 4.0, NAN, 7.0, float("inf"), 5.0, 100.0])
    match = np.array([0, 0, 0, 0, 0, 0, -1, 0], np.int32)
    mgroup = np.array([0, 0, 0, 0, 2, 0, 0, -1], np.int32)
    n, mean, sd = model_errors.moments_numpy(error, match, mgroup, 4)
    assert n.dtype == np.int64 and n.tolist() == [3, 0, 1, 0]
    assert mean[0] == 7.0 / 3.0 and sd[0] == np.sqrt(((1 - 7 / 3) ** 2 + (2 - 7 / 3) ** 2 + (4 - 7 / 3) ** 2) / 3)       # population sd
    assert mean[2] == 7.0 and sd[2] == 0.0                                       # n = 1: sd 0
    assert mean[[1, 3]].tobytes() == np.array([np.nan, np.nan]).tobytes() == sd[[1, 3]].tobytes()
    # the written order: 64 lanes, each its rows in increasing q, then the fold by halves
    r = np.random.default_rng(3)
    e = r.normal(0, 1e3, 1000) * 10.0 ** r.integers(-8, 8, 1000)
    n, mean, _ = model_errors.moments_numpy(e, np.zeros(1000, np.int32), np.zeros(1000, np.int32), 1)
    lanes = [0.0] * 64
    for i, v in enumerate(e.tolist()):
        lanes[i % 64] += v
    h = 32
    while h:
        lanes = [lanes[i] + lanes[i + h] for i in range(h)]
        h //= 2
    assert n.tolist() == [1000] and mean[0] == lanes[0] / 1000
    n, mean, sd = model_errors.moments_numpy(np.zeros(0), np.zeros(0, np.int32), np.zeros(0, np.int32), 2)
    assert n.tolist() == [0, 0] and np.isnan(mean).all() and np.isnan(sd).all()


def hand_built(tmp_path, conf_of=(0.5, 0.6), label_px=((100.0, 100.0, 200.0, 200.0),) * 3):
    """Scene 3 of a one-row bounds table; three circle labels of 2015 (pass 2013-2015) side by side, a square one of 2020 (2019-2021); two
    circle detections of 2015 over the first label, one of 2008 (2005-2009: a pass without labels) and a square one of 2015 over the 2020
    label's place."""
    x, y = 1.0e6, 5.2e6
    feats = [truth_feature(x, y, x + 20, y + 20, "circle_cage", 2015, px=label_px[0]),
             truth_feature(x + 30, y, x + 50, y + 20, "circle_cage", 2015, px=label_px[1]),
             truth_feature(x + 60, y, x + 80, y + 20, "circle_cage", 2015, px=label_px[2]),
             truth_feature(x + 90, y, x + 110, y + 20, "other", 2015),
             truth_feature(x + 90, y, x + 110, y + 20, "square_cage", 2020)]
    path = write_features(tmp_path / "truth.geojson", feats)
    box = [[x + 1, y + 1, x + 19, y + 19], [x + 2, y + 2, x + 21, y + 21], [x + 31, y + 1, x + 49, y + 19], [x + 91, y + 1, x + 109, y + 19]]
    table = table_from_boxes(box, [CIRCLE, CIRCLE, CIRCLE, SQUARE], [2015, 2015, 2008, 2015], [*conf_of, 0.9, 0.9], [[300, 300, 400, 400]] * 4,
                             ["ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0"], [0] * 4)
    return table, path


def test_threshold_year_type_and_passes(tmp_path):
    table, path = hand_built(tmp_path)
    t = model_errors.load_truth_geojson(path)
    assert t["feature"].tolist() == [0, 1, 2, 4] and t["xmin"].tolist() == [100.0] * 4 and t["jpeg_height"].tolist() == [1024.0] * 4
    res = model_errors.distributions(table, t, 0.5, cpu=True)
    # det_conf 0.5 is not above 0.5; the 2008 circle and the 2015 square find no label of their year
    assert res["rows"].tolist() == [1, 2, 3] and res["match"].tolist() == [0, -1, -1] and res["n_queries"] == 3 and res["n_matched"] == 1
    assert res["passes"] == ["2013-2015", "2019-2021"] and res["groups"] == [("2013-2015", "circle_farm"), ("2013-2015", "square_farm"),
                                                                            ("2019-2021", "circle_farm"), ("2019-2021", "square_farm")]
    assert res["n"].tolist() == [1, 0, 0, 0] and list(res["errors"]) == [("2013-2015", "circle_farm")] and len(res["empty"]) == 3
    mean, sd = res["errors"][("2013-2015", "circle_farm")]
    assert sd == 0.0 and mean == res["area_label"][0] - res["area"][0] == res["error"][0]
    res = model_errors.distributions(table, t, 0.49, cpu=True)
    assert res["rows"].tolist() == [0, 1, 2, 3] and res["match"].tolist() == [0, 0, -1, -1] and res["n"].tolist() == [2, 0, 0, 0]
    keep = np.array([True, False, True, True])
    assert model_errors.distributions(table, t, 0.49, keep=keep, cpu=True)["rows"].tolist() == [0, 2, 3]
    # labels of 2008: now the 2008 detection has a pass, and a label of its year
    feats = json.load(open(path))["features"] + [truth_feature(1.0e6 + 30, 5.2e6, 1.0e6 + 50, 5.2e6 + 20, "circle_cage", 2008)]
    t2 = model_errors.load_truth_geojson(write_features(tmp_path / "truth2.geojson", feats))
    res = model_errors.distributions(table, t2, 0.5, cpu=True)
    assert res["passes"] == ["2005-2009", "2013-2015", "2019-2021"] and res["match"].tolist() == [0, 4, -1] and res["n"].tolist() == [1, 0, 1, 0, 0, 0]


def test_label_border_flags_change_the_area_as_areas_says(tmp_path):
    px = ((100.0, 100.0, 200.0, 200.0), (0.0, 100.0, 200.0, 200.0), (100.0, 0.0, 1024.0, 200.0))
    _, path = hand_built(tmp_path, label_px=px)
    t = model_errors.load_truth_geojson(path)
    area = model_errors.label_areas(t)
    q = to_3035(np.stack([t[c] for c in evaluate.BOX_COLUMNS], 1))
    w, h = q[:, :, 0].max(1) - q[:, :, 0].min(1), q[:, :, 1].max(1) - q[:, :, 1].min(1)
    assert area[0] == np.pi * (w[0] / 2) * (h[0] / 2)                                                   # inside the image: the ellipse
    assert area[1] == (h[1] * w[1] / 2 + np.pi * (h[1] / 2) * w[1] / 2) / 2                              # xmin == 0: triangle .. half ellipse
    assert area[2] == (h[2] * w[2] / 2 + np.pi * h[2] * w[2] / 4) / 2                                    # ymin == 0 and xmax == jpeg_width
    assert area[3] == (w[3] * h[3] * (1 / 2) + w[3] * h[3]) / 2                                         # a square: half the box .. the box
    assert 150.0 < area[0] < 200.0 and area[1] < area[0] and area[2] < area[1]      # (20 m of EPSG:3857 are about 15 m on the ground at 42 N)
    want = facilities._areas(w, h, t["cls"] == CIRCLE, t["cls"] == SQUARE, np.array([False, True, True, False]), np.array([False, False, True, False]))
    assert area.tobytes() == want["area"].tobytes()


def test_truth_without_the_pixel_columns_is_refused(tmp_path):
    feats = [truth_feature(0.0, 0.0, 1.0, 1.0, "other", 2015), truth_feature(0.0, 0.0, 1.0, 1.0, "circle_cage", 2015),
             truth_feature(0.0, 0.0, 1.0, 1.0, "square_cage", 2015), truth_feature(0.0, 0.0, 1.0, 1.0, "square_cage", 2015)]
    del feats[0]["properties"]["xmin"]                                           # a type that is dropped: not looked at
    del feats[2]["properties"]["jpeg_width"], feats[2]["properties"]["ymax"], feats[3]["properties"]["xmin"]
    with pytest.raises(ValueError, match=r"feature 2 lacks ymax, jpeg_width"):
        model_errors.load_truth_geojson(write_features(tmp_path / "t.geojson", feats))
    assert evaluate.load_truth_geojson(str(tmp_path / "t.geojson"))["cls"].shape[0] == 3                 # evaluate's loader stays as it is


# ---- (d) the files and the options ----

FACTORS = "pass,s_mean,s_sd,h_mean,h_sd\n" + "".join(f"{a}-{b},12.0,2.0,0.8,0.1\n" for a, b in facilities.IMAGE_PASSES)
TONNAGE_JSON_KEYS = ["device", "cpu", "mix", "min_depth", "default_depth", "factors", "errors", "depths_file", "facilities_conf", "facilities_eps",
                     "facilities_min_cages", "K", "seed", "passes", "tonnage_var"]


def read_all(d, names):
    return {n: open(os.path.join(d, n), "rb").read() for n in names}


def test_files_and_the_hand_over_to_the_bootstrap(tmp_path):
    table = detection_table()
    truth_path = write_truth_geojson(str(tmp_path / "truth.geojson"))
    out = str(tmp_path / "me")
    res = model_errors.model_errors_from_table(table, truth_path, out, CONF, cpu=True)
    errs = tonnage.read_errors(os.path.join(out, model_errors.CSV_FILE))          # the extra column n is tolerated
    assert errs == res["errors"] and len(errs) >= 6
    lines = open(os.path.join(out, model_errors.CSV_FILE)).read().splitlines()
    assert lines[0] == "pass,farm_type,model_error_mean,model_error_sd,n" and len(lines) == 1 + len(errs)
    p, t, mean, sd, n = lines[1].split(",")
    i = res["groups"].index((p, t))
    assert (mean, sd, n) == (repr(float(res["mean"][i])), repr(float(res["sd"][i])), str(int(res["n"][i])))
    cages = open(os.path.join(out, model_errors.CAGES_FILE)).read().splitlines()
    assert cages[0] == "index,label,overlap,area,area_label,error" and len(cages) == 1 + res["n_matched"]
    first = int(np.nonzero(res["match"] >= 0)[0][0])
    assert cages[1].split(",") == [str(int(res["rows"][first])), str(int(res["match"][first])), repr(float(res["overlap"][first])),
                                   repr(float(res["area"][first])), repr(float(res["area_label"][first])), repr(float(res["error"][first]))]
    s = json.load(open(os.path.join(out, model_errors.JSON_FILE)))
    assert s["conf"] == CONF and s["device"] == "cpu" and s["n_detections"] == 991 and s["n_labels"] == 991 and s["n_matched"] == res["n_matched"]
    assert [tuple(g) for g in s["empty"]] == res["empty"] and len(s["groups"]) + len(s["empty"]) == 12 and s["truth"] == "truth.geojson"
    again = str(tmp_path / "me2")
    model_errors.model_errors_from_table(table, truth_path, again, CONF, cpu=True)
    names = (model_errors.CSV_FILE, model_errors.CAGES_FILE, model_errors.JSON_FILE)
    assert read_all(out, names) == read_all(again, names)

    # the bootstrap: the file and the table made in this process give the same bytes; without either the files are what they were
    (tmp_path / "factors.csv").write_text(FACTORS)
    ton_names = (tonnage.ESTIMATES_FILE, tonnage.FACILITIES_FILE, tonnage.JSON_FILE)
    args = dict(K=64, seed=3, conf_thresh=CONF, eps=25.0, min_cages=3, cpu=True)
    by_file, in_process, without = (str(tmp_path / d) for d in ("ton_file", "ton_mem", "ton_none"))
    est = tonnage.tonnage_from_table(table, by_file, str(tmp_path / "factors.csv"), os.path.join(out, model_errors.CSV_FILE), **args)
    tonnage.tonnage_from_table(table, in_process, str(tmp_path / "factors.csv"), errors=res["errors"], **args)
    tonnage.tonnage_from_table(table, without, str(tmp_path / "factors.csv"), **args)
    assert len(est["facility_index"]) > 10
    assert read_all(by_file, ton_names) == read_all(in_process, ton_names)
    recorded = json.load(open(os.path.join(in_process, tonnage.JSON_FILE)))["errors"]
    assert recorded == [[*k, *v] for k, v in sorted(res["errors"].items())]
    plain = json.load(open(os.path.join(without, tonnage.JSON_FILE)))
    assert list(plain) == TONNAGE_JSON_KEYS and plain["errors"] == []
    assert read_all(without, ton_names)[tonnage.ESTIMATES_FILE] != read_all(by_file, ton_names)[tonnage.ESTIMATES_FILE]
    with pytest.raises(ValueError, match="not from both"):
        tonnage.tonnage_from_table(table, without, str(tmp_path / "factors.csv"), os.path.join(out, model_errors.CSV_FILE), errors=res["errors"], **args)


def test_detect_py_options():
    from aquaculture_amd import detect
    with pytest.raises(SystemExit):
        detect.parse_opt(["--model-errors", "truth.geojson"])                    # needs --geocode-bboxes
    with pytest.raises(SystemExit):
        detect.parse_opt(["--model-errors", "truth.geojson", "--geocode-bboxes", "wb.csv", "--tonnage-errors", "errors.csv"])
    with pytest.raises(ValueError, match="--geocode-bboxes"):
        detect.run("w.pt", "src", model_errors="truth.geojson")
    with pytest.raises(ValueError, match="not from both"):
        detect.run("w.pt", "src", model_errors="truth.geojson", geocode_bboxes="wb.csv", tonnage_errors="errors.csv")
    opt = detect.parse_opt(["--model-errors", "truth.geojson", "--geocode-bboxes", "wb.csv", "--model-errors-conf", "0.7"])
    assert (opt.model_errors, opt.model_errors_conf, opt.model_errors_out) == ("truth.geojson", 0.7, None)
    opt = detect.parse_opt([])
    assert (opt.model_errors, opt.model_errors_conf, opt.model_errors_out) == (None, None, None)
    assert "model_errors" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)


def test_command_line_on_the_cpu(tmp_path):
    _, path = hand_built(tmp_path)
    (tmp_path / "labels").mkdir()
    (tmp_path / "labels" / "ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0.txt").write_text("0 0.107422 0.107422 0.0175781 0.0175781 0.9\n1 0.25 0.25 0.01 0.01 0.8\n")
    # a scene of 1 m pixels whose pixel (100, 100) is the first label's upper left corner: the circle detection covers pixels 101 .. 119 of it
    (tmp_path / "wb.csv").write_text(',geometry\n3,"POLYGON ((999900 5193976, 999900 5200120, 1006044 5200120, 1006044 5193976, 999900 5193976))"\n')
    assert model_errors.main(["--labels", str(tmp_path / "labels"), "--geocode-bboxes", str(tmp_path / "wb.csv"), "--truth", path, "--cpu",
                              "--model-errors-out", str(tmp_path / "out"), "--model-errors-conf", "0.85"]) == 0
    s = json.load(open(tmp_path / "out" / model_errors.JSON_FILE))
    assert s["n_detections"] == 1 and s["n_labels"] == 4 and s["conf"] == 0.85 and s["cpu"] is True and s["n_matched"] == 1
    assert [(g["pass"], g["farm_type"], g["n"], g["model_error_sd"]) for g in s["groups"]] == [("2013-2015", "circle_farm", 1, 0.0)]
    assert open(tmp_path / "out" / model_errors.CAGES_FILE).read().splitlines()[1].startswith("0,0,100.0,")
    assert os.path.exists(tmp_path / "out" / model_errors.CSV_FILE) and os.path.exists(tmp_path / "out" / model_errors.CAGES_FILE)


# ---- (e) the ABI surface ----

def test_symbols_are_declared_exported_and_bound(lib):
    from aquaculture_amd import engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_model_error_match_f64", "aq_model_error_moments_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    guards = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "size_guards.h")).read()
    assert guards.count("model_error_count_fits(ll n)") == 1
    assert "sg::model_error_count_fits" in open(os.path.join(ROOT, "aquaculture_amd", "csrc", "model_errors.hip")).read()
