"""--facilities on the host: the numpy restatement of the DBSCAN kernels against scikit-learn (labels and core flags, exactly), the area
estimates against recorded results of the reference's two functions, the projection round trip, and the facility table.  The point sets
and their expected labels are shared with tests/test_gpu_facilities.py."""
import functools
import json
import os
import re

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OFFSET = np.array([4.0e6, 2.2e6])                           # EPSG:3035 coordinates of the French coast are of this size


def sk_labels(xy, group, eps, min_samples):
    """sklearn.cluster.DBSCAN as the reference calls it, per group -> (labels int64 [n], core bool [n])."""
    from sklearn.cluster import DBSCAN
    xy, group = np.asarray(xy, np.float64).reshape(-1, 2), np.asarray(group)
    labels, core = np.full(xy.shape[0], -1, np.int64), np.zeros(xy.shape[0], bool)
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        db = DBSCAN(eps=eps, min_samples=min_samples).fit(xy[idx])
        labels[idx] = db.labels_
        core[idx[db.core_sample_indices_]] = True
    return labels, core


def no_near_ties(xy, group, eps):
    """True if no pair of a group has |d^2 - eps^2| <= 1e-9 eps^2, about: the pairs within eps (1 + 1e-9) are those within eps (1 - 1e-9)."""
    from scipy.spatial import cKDTree
    for g in np.unique(group):
        t = cKDTree(np.asarray(xy)[np.asarray(group) == g])
        if len(t.query_pairs(eps * (1 + 1e-9))) != len(t.query_pairs(eps * (1 - 1e-9))):
            return False
    return True


def blobs(seed):
    """190 points: 150 in 2 to 7 Gaussian blobs of sigma 9 m in a 120 m square and 40 uniform ones, shuffled, at OFFSET."""
    r = np.random.default_rng(seed)
    k = int(r.integers(2, 8))
    c = r.uniform(0, 120, (k, 2))
    p = np.concatenate([c[r.integers(0, k, 150)] + r.normal(0, 9, (150, 2)), r.uniform(0, 120, (40, 2))])
    return p[r.permutation(190)] + OFFSET


def two_clusters_and_a_border_point(a_first):
    """Two clusters of five core points each, 18 m apart at their nearest points, and between those one point with three neighbours
    (itself and the two): not core, within eps of both clusters."""
    a = np.array([(-9, 0), (-13, 0), (-13, 2), (-13, -2), (-15, 0)], float)
    b = a * [-1, 1]
    return np.concatenate([a, b] if a_first else [b, a]) + OFFSET, np.zeros((1, 2)) + OFFSET


def chain(step, n=3000, seed=5):
    i = np.arange(n, dtype=np.float64)[np.random.default_rng(seed).permutation(n)]
    return np.stack([i * (step / np.sqrt(2.0)), i * (step / np.sqrt(2.0))], 1) + OFFSET


def cell_edges():
    """Points on and beside the edges of the sort grid's cells (edge h = eps (1 + 2^-20), origin at the minimum), with a negative minimum,
    and 60 coincident points in one cell."""
    h = 10.0 * (1 + 2.0 ** -20)
    d = np.array([-1e-7, 0.0, 1e-7])
    k = np.arange(4) * h
    x = (k[:, None] + d[None, :]).reshape(-1)
    grid = np.stack(np.meshgrid(x, x), -1).reshape(-1, 2)
    grid = grid[(grid >= 0).all(1)]                         # the origin stays the minimum
    pts = np.concatenate([grid, np.tile([[2.5 * h, 1.5 * h]], (60, 1)), [[3 * h + 4.0, 3 * h + 4.0]]])
    return pts[np.random.default_rng(3).permutation(pts.shape[0])] + [-50.0, -70.0]


def _cases():
    z = lambda n: np.zeros(n, np.int32)
    out = {"one_point": (np.zeros((1, 2)) + OFFSET, z(1), 10.0, 5),
           "four_coincident": (np.zeros((4, 2)) + OFFSET, z(4), 10.0, 5),
           "five_coincident": (np.zeros((5, 2)) + OFFSET, z(5), 10.0, 5)}
    for s in range(5):
        out[f"blobs_{s}"] = (blobs(s), z(190), 10.0, 5)
    border_a, p = two_clusters_and_a_border_point(True)
    border_b, _ = two_clusters_and_a_border_point(False)
    out["border_a_first"] = (np.concatenate([p, border_a]), z(11), 10.0, 5)
    out["border_b_first"] = (np.concatenate([p, border_b]), z(11), 10.0, 5)
    out["border_last"] = (np.concatenate([border_b, p]), z(11), 10.0, 5)
    out["chain_9.99"] = (chain(9.99), z(3000), 10.0, 2)
    out["chain_10.01"] = (chain(10.01), z(3000), 10.0, 2)
    two = np.repeat(blobs(11), 2, axis=0)
    out["two_groups"] = (two, np.tile(np.array([0, 1], np.int32), 190), 10.0, 5)
    ce = cell_edges()
    out["cell_edges"] = (ce, z(ce.shape[0]), 10.0, 5)
    return out


CASES = _cases()
TIE = (np.array([(0, 0), (6, 8), (12, 16), (18, 24), (24, 32), (30, 40), (36, 49), (100, 100)], float) + 4.0e6, np.zeros(8, np.int32), 10.0, 3)
TIE_LABELS = [0, 0, 0, 0, 0, 0, -1, -1]
TIE_CORE = [False, True, True, True, True, False, False, False]       # min_samples = 3: the two ends of the row have one neighbour each


@functools.lru_cache(maxsize=None)
def expected(name):
    """(labels, core) of a case from scikit-learn, computed once and shared; treat as read-only."""
    xy, group, eps, ms = CASES[name]
    return sk_labels(xy, group, eps, ms)


def large_case():
    """50 000 uniform points in a 3 km square, 3 groups (the GPU test's many-workgroups case)."""
    r = np.random.default_rng(2024)
    return r.uniform(0, 3000, (50000, 2)) + OFFSET, r.integers(0, 3, 50000).astype(np.int32), 10.0, 5


# ---- dbscan_numpy ----

@pytest.mark.parametrize("name", sorted(CASES))
def test_dbscan_numpy_is_sklearn(name):
    from aquaculture_amd import facilities
    xy, group, eps, ms = CASES[name]
    assert no_near_ties(xy, group, eps), "the case has a pair too close to eps for an exact comparison"
    labels, core, root = facilities.dbscan_numpy(xy, group, eps, ms)
    want_l, want_c = expected(name)
    assert np.array_equal(core, want_c)
    assert np.array_equal(labels, want_l), np.nonzero(labels != want_l)[0][:10]
    assert ((root >= 0) == (labels >= 0)).all() and (root[core] <= np.nonzero(core)[0]).all()


def test_dbscan_numpy_cases_say_what_they_are_built_for():
    from aquaculture_amd import facilities
    assert facilities.dbscan_numpy(np.zeros((0, 2)), None, 10.0, 5)[0].shape == (0,)
    assert expected("one_point")[0].tolist() == [-1] and expected("four_coincident")[0].tolist() == [-1] * 4
    assert expected("five_coincident")[0].tolist() == [0] * 5 and expected("five_coincident")[1].all()
    # the point between the two clusters is not core and takes the cluster whose first core point comes first in the input
    for name, at, first in (("border_a_first", 0, 1), ("border_b_first", 0, 1), ("border_last", 10, 0)):
        labels, core = expected(name)
        assert not core[at] and core.sum() == 10 and labels[at] == labels[first] == 0 and set(labels.tolist()) == {0, 1}
    assert (expected("chain_9.99")[0] == 0).all() and (expected("chain_10.01")[0] == -1).all()
    l2, c2 = expected("two_groups")
    l1, c1 = sk_labels(blobs(11), np.zeros(190), 10.0, 5)
    assert np.array_equal(l2[0::2], l1) and np.array_equal(l2[1::2], l1) and np.array_equal(c2[0::2], c1) and np.array_equal(c2[1::2], c1)
    border = sum(int(((expected(f"blobs_{s}")[0] >= 0) & ~expected(f"blobs_{s}")[1]).sum()) for s in range(5))
    assert border >= 20                                     # the blobs do exercise the border rule


def test_dbscan_numpy_exact_tie():
    """Every step of (0,0) (6,8) ... (30,40) is exactly 10 = eps: the test is <=.  (36,49) is sqrt(117) away."""
    from aquaculture_amd import facilities
    xy, group, eps, ms = TIE
    want_l, want_c = sk_labels(xy, group, eps, ms)
    assert want_l.tolist() == TIE_LABELS and want_c.tolist() == TIE_CORE
    labels, core, _ = facilities.dbscan_numpy(xy, group, eps, ms)
    assert labels.tolist() == TIE_LABELS and core.tolist() == TIE_CORE


def test_roots_to_labels_ranks_within_the_group():
    from aquaculture_amd import facilities
    root = np.array([4, 1, -1, 1, 4, 5, 7, 7, -1])
    group = np.array([0, 1, 0, 1, 0, 1, 0, 0, 1])
    assert facilities.roots_to_labels(root, group).tolist() == [0, 0, -1, 0, 0, 1, 1, 1, -1]
    with pytest.raises(ValueError):
        facilities.dbscan_numpy(np.zeros((3, 2)), None, 0.0, 5)
    with pytest.raises(ValueError):
        facilities.dbscan_numpy(np.zeros((3, 2)), None, 10.0, 0)


# ---- areas ----

def test_net_areas_match_the_recorded_reference_results():
    """tests/golden/g11_net_areas.json: results of the reference's get_circle_area_from_bbox / get_square_area_from_bbox.  Recorded
    tolerance: 0 ulp -- the vectorised version has the same operation order and agreed bit for bit."""
    from aquaculture_amd import facilities, geocode
    g = json.load(open(os.path.join(ROOT, "tests", "golden", "g11_net_areas.json")))
    cases = g["cases"]
    assert g["tolerance_ulp"] == 0 and len(cases) >= 12
    assert {(c["x_border"], c["y_border"]) for c in cases if c["type"] == "circle_farm"} == {(a, b) for a in (False, True) for b in (False, True)}
    assert any(c["width"] == 0 for c in cases) and any(c["width"] != c["height"] for c in cases)
    n = len(cases)
    W, H = 1024, 768
    x_border = np.array([c["x_border"] for c in cases])
    y_border = np.array([c["y_border"] for c in cases])
    left = np.arange(n) % 2 == 0                            # both ways of touching a border
    # (boxes from 0, so that e_max - e_min gives the recorded width back exactly)
    table = {"cls": np.array([0 if c["type"] == "circle_farm" else 1 for c in cases]),
             "e_min_3035": np.zeros(n), "e_max_3035": np.array([c["width"] for c in cases]),
             "n_min_3035": np.zeros(n), "n_max_3035": np.array([c["height"] for c in cases]),
             "xmin": np.where(x_border & left, 0, 17), "xmax": np.where(x_border & ~left, W, 300),
             "ymin": np.where(y_border & ~left, 0, 5), "ymax": np.where(y_border & left, H, 200)}
    got = facilities.net_areas(table, W, H)
    for k, c in enumerate(cases):
        assert [float(got[col][k]) for col in facilities.AREA_COLUMNS] == c["result"], (c, [got[col][k] for col in facilities.AREA_COLUMNS])
    # other classes: NaN; the border test reads the image's own size
    other = dict(table, cls=np.full(n, 4))
    assert all(np.isnan(v).all() for v in facilities.net_areas(other, W, H).values())
    one = {k: v[:1] for k, v in table.items()}
    one.update(cls=np.array([0]), xmin=np.array([5]), xmax=np.array([640]), ymin=np.array([5]), ymax=np.array([50]))
    assert facilities.net_areas(one, 640, 640)["area_var"][0] > 0 and facilities.net_areas(one, 1024, 1024)["area_var"][0] == 0
    assert geocode.REVERSE_CLASS_MAPPING[0] == "circle_farm" and geocode.REVERSE_CLASS_MAPPING[1] == "square_farm"


# ---- projections ----

def test_projection_round_trips(capsys):
    """The reverse directions against the forward ones over the French Mediterranean extent, and against the IOGP GN7-2 worked example the
    forward direction is tested with.  Residuals found when this was written (printed again on every run): LAEA lon 5.8e-15 deg, lat
    4.3e-14 deg, i.e. 4.7e-10 m east and 3.3e-9 m north after going forward again; Mercator lon 8.9e-16 deg, lat 2.2e-14 deg.  The bounds
    asserted are 1e-12 deg and 1e-7 m: rounding of 4e6 m coordinates, not a fit to those figures."""
    from aquaculture_amd import geocode
    lon, lat = np.meshgrid(np.linspace(2.5, 8.0, 50), np.linspace(41.0, 44.5, 50))
    e, n = geocode.lonlat_to_laea_europe(lon, lat)
    lon2, lat2 = geocode.laea_europe_to_lonlat(e, n)
    e2, n2 = geocode.lonlat_to_laea_europe(lon2, lat2)
    x, y = geocode.lonlat_to_mercator(lon, lat)
    lon3, lat3 = geocode.mercator_to_lonlat(x, y)
    res = [float(np.abs(a - b).max()) for a, b in ((lon2, lon), (lat2, lat), (e2, e), (n2, n), (lon3, lon), (lat3, lat))]
    with capsys.disabled():
        print(f"\nround trip residuals: laea lon {res[0]:.2e} lat {res[1]:.2e} deg, e {res[2]:.2e} n {res[3]:.2e} m; mercator lon {res[4]:.2e} lat {res[5]:.2e} deg")
    assert max(res[0], res[1], res[4], res[5]) < 1e-12 and max(res[2], res[3]) < 1e-7
    # IOGP worked example: 50 N 5 E <-> E 3962799.45 N 2999718.85 (given to the centimetre: 0.01 m is 1.4e-7 deg of longitude there)
    lo, la = geocode.laea_europe_to_lonlat(np.float64(3962799.45), np.float64(2999718.85))
    assert abs(lo - 5.0) < 2e-7 and abs(la - 50.0) < 2e-7, (lo, la)
    lo, la = geocode.laea_europe_to_lonlat(np.float64(geocode.LAEA_FE), np.float64(geocode.LAEA_FN))
    assert (float(lo), float(la)) == (10.0, 52.0)
    xm, ym = geocode.lonlat_to_mercator(np.float64(-(100 + 20 / 60)), np.float64(24 + 22 / 60 + 54.433 / 3600))
    assert abs(xm - -11169055.58) < 0.01 and abs(ym - 2800000.00) < 0.01


def test_centroid_of_a_box_is_its_centre_up_to_the_projection():
    from aquaculture_amd import facilities, geocode
    x0, y0 = geocode.lonlat_to_mercator(np.array([3.5, 6.0]), np.array([43.3, 43.0]))
    t = {"xmin_3857": x0, "xmax_3857": x0 + 12.0, "ymin_3857": y0, "ymax_3857": y0 + np.array([9.0, 0.0])}       # the second has no area
    c = facilities.centroids_3035(t)
    mid = np.stack(geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(x0 + 6.0, y0 + np.array([4.5, 0.0]))), 1)
    assert np.abs(c - mid).max() < 1e-3                     # (a 12 m box: the projection bends it by far less than a millimetre)
    assert facilities.centroids_3035({k: v[:0] for k, v in t.items()}).shape == (0, 2)


# ---- the facility table ----

def hand_table():
    """22 detections; 4 m in EPSG:3857 at 43.35 N is 2.9 m on the ground, so a cage of a row sees three neighbours on either side.
    Year 2015 (listed first): seven circles in a row, the middle one below the confidence threshold and the first exactly at it; five
    cages 700 m east (3 squares, 1 rectangle, 1 triangle whose area is NaN); two stray cages.  Year 2012: three cages (too few).  Year
    2014 (pass 2013-2015, as 2015): five squares beside the five cages of 2015, which they join when clustering by pass."""
    from aquaculture_amd import geocode
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.6), np.float64(43.35)))
    rows = []                                               # (x, y offset in EPSG:3857 metres, cls, year, conf)
    for k in range(7):
        rows.append((k * 4.0, 0.0, 0, 2015, 0.49 if k == 3 else 0.5 if k == 0 else 0.9))
    for k, cls in enumerate((1, 1, 1, 4, 2)):
        rows.append((700.0 + k * 4.0, 40.0, cls, 2015, 0.8))
    rows += [(300.0, 300.0, 0, 2015, 0.9), (-200.0, 100.0, 1, 2015, 0.9)]
    rows += [(k * 4.0, 0.0, 0, 2012, 0.9) for k in range(3)]
    rows += [(700.0 + k * 4.0, 43.0, 1, 2014, 0.7) for k in range(5)]
    r = np.array(rows)
    n = r.shape[0]
    t = {"xmin_3857": x0 + r[:, 0], "xmax_3857": x0 + r[:, 0] + 3.0, "ymin_3857": y0 + r[:, 1], "ymax_3857": y0 + r[:, 1] + 3.0,
         "cls": r[:, 2].astype(np.int64), "year": r[:, 3].astype(np.int64), "det_conf": r[:, 4],
         "xmin": np.full(n, 10), "xmax": np.full(n, 40), "ymin": np.full(n, 10), "ymax": np.full(n, 40), "image": np.zeros(n, np.int64)}
    for a, b, cx, cy in (("e_min_3035", "n_min_3035", "xmin_3857", "ymin_3857"), ("e_max_3035", "n_max_3035", "xmax_3857", "ymax_3857")):
        t[a], t[b] = geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(t[cx], t[cy]))
    return t


ROW6, FIVE, LATER = [0, 1, 2, 4, 5, 6], list(range(7, 12)), list(range(17, 22))


def test_cluster_builds_the_reference_columns():
    from aquaculture_amd import facilities
    t = hand_table()
    fac = facilities.cluster(t, "year", conf_thresh=0.5, eps=10.0, min_cages=5, labels_fn=facilities.dbscan_numpy)
    # groups in order of first appearance (2015, 2012, 2014), then labels (sklearn's: in order of each cluster's first core point)
    assert fac["facility_index"] == [0, 1, 2] and fac["year"] == [2015, 2015, 2014]
    assert fac["cage_ids"] == [ROW6, FIVE, LATER]           # detection 3 (0.49) is out, detection 0 (exactly 0.5) is in: >=
    assert fac["noise_points"] == [2, 2, 0]                 # of the group: the two strays of 2015; 2012 has no facility, so no row
    assert (fac["num_square_farms"], fac["num_circle_farms"], fac["num_rectangle_farms"]) == ([0, 3, 5], [6, 0, 0], [0, 1, 0])
    low = facilities.cluster(t, "year", conf_thresh=0.49, labels_fn=facilities.dbscan_numpy)
    assert low["cage_ids"][0] == list(range(7)) and low["noise_points"][0] == 2 and low["num_circle_farms"][0] == 7 and low["facility_index"] == [0, 1, 2]
    at = facilities.cluster(t, "year", conf_thresh=0.9, labels_fn=facilities.dbscan_numpy)              # the cages at exactly 0.9 stay
    assert at["cage_ids"] == [[1, 2, 4, 5, 6]] and at["noise_points"] == [2]
    # area sums skip the NaN of the rectangle and the triangle (only circles and squares have an estimate)
    areas = facilities.net_areas(t, 1024, 1024)
    assert np.isnan(areas["area"][10:12]).all() and not np.isnan(areas["area"][7:10]).any()
    for c in facilities.AREA_COLUMNS:
        assert fac[c][1] == float(np.nansum(areas[c][7:12])) and fac[c][1] > 0
    assert fac["_members"].tolist() == [0, 0, 0, -1, 0, 0, 0] + [1] * 5 + [-1] * 5 + [2] * 5
    # by pass: 2015 and 2014 are one group, 2012 another; the 2014 cages join the five of 2015
    by_pass = facilities.cluster(t, "pass", labels_fn=facilities.dbscan_numpy)
    assert by_pass["pass"] == ["2013-2015"] * 2 and by_pass["cage_ids"] == [ROW6, FIVE + LATER]
    assert by_pass["noise_points"] == [2, 2] and facilities.image_pass(2012) == "2010-2012" and facilities.image_pass(1999) == "No group"
    # the WKT parses: MULTIPOLYGON of closed five-point rings of the members' own boxes, or EMPTY
    assert fac["circle_farm_geoms"][1:] == ["MULTIPOLYGON EMPTY"] * 2 and fac["circle_farm_geoms"][0].count("))") == 6
    rings = re.findall(r"\(\(([^()]*)\)\)", fac["square_farm_geoms"][1])
    assert fac["square_farm_geoms"][1].startswith("MULTIPOLYGON (((") and len(rings) == 3
    for ring, k in zip(rings, (7, 8, 9)):
        pts = [tuple(float(v) for v in p.split()) for p in ring.split(", ")]
        assert len(pts) == 5 and pts[0] == pts[-1] == (t["xmax_3857"][k], t["ymin_3857"][k]) and pts[2] == (t["xmin_3857"][k], t["ymax_3857"][k])
    # the point: mean of the members' EPSG:3035 centroids, delivered in EPSG:3857 (here the centre of the middle cage)
    c = facilities.centroids_3035(t)[7:12].mean(0)
    assert abs(fac["x_3035"][1] - c[0]) < 1e-9 and abs(fac["y_3035"][1] - c[1]) < 1e-9
    assert abs(fac["x_3857"][1] - (t["xmin_3857"][9] + 1.5)) < 0.01 and abs(fac["y_3857"][1] - (t["ymin_3857"][9] + 1.5)) < 0.01
    with pytest.raises(ValueError, match="year.*pass"):
        facilities.cluster(t, "month", labels_fn=facilities.dbscan_numpy)


def test_files_and_command_line(tmp_path):
    from aquaculture_amd import detect, facilities
    t = hand_table()
    out = str(tmp_path / "f.geojson")
    fac = facilities.facilities_from_table(t, out, cpu=True)
    doc = json.load(open(out))
    assert doc["crs"]["properties"]["name"].endswith("3857") and len(doc["features"]) == 3
    p1 = doc["features"][1]
    assert p1["geometry"] == {"type": "Point", "coordinates": [fac["x_3857"][1], fac["y_3857"][1]]}
    assert p1["properties"]["cage_ids"] == FIVE and p1["properties"]["facility_index"] == 1 and p1["properties"]["year"] == 2015
    assert set(p1["properties"]) >= {"num_square_farms", "num_circle_farms", "num_rectangle_farms", "noise_points", "square_farm_geoms",
                                     "circle_farm_geoms", "rectangle_farm_geoms", "area", "area_var", "min_area", "max_area"}
    det = json.load(open(facilities.detections_path(out)))
    assert facilities.detections_path(out).endswith("f_detections.geojson")
    assert [f["properties"]["index"] for f in det["features"]] == ROW6 + FIVE + LATER
    assert det["features"][10]["properties"]["area"] is None and det["features"][0]["properties"]["area"] > 0      # the triangle's NaN is null
    assert det["features"][0]["geometry"]["type"] == "Polygon" and len(det["features"][0]["geometry"]["coordinates"][0]) == 5
    # detect.py refuses --facilities without --geocode-bboxes, with a message
    with pytest.raises(SystemExit):
        detect.parse_opt(["--facilities"])
    with pytest.raises(ValueError, match="--facilities .*needs --geocode-bboxes"):
        detect.run("w.pt", "src", facilities="")
    opt = detect.parse_opt(["--facilities", "--geocode-bboxes", "wb.csv"])
    assert (opt.facilities, opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages, opt.facilities_by) == ("", 0.5, 10.0, 5, "year")
    # the record --resume checks does not know the flag: it changes nothing a resumed sweep may mix
    assert "facilities" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)


def test_symbols_are_declared_exported_and_bound(lib):
    """Fails without the feature: the header declares the two entry points, engine.py lists and binds them, the library has them."""
    import ctypes
    from aquaculture_amd import engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_facility_scratch_bytes", "aq_facility_dbscan_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.aq_facility_scratch_bytes.restype is ctypes.c_size_t
    assert lib.aq_facility_scratch_bytes(0) == 0 and lib.aq_facility_scratch_bytes(1 << 31) == 0
    assert lib.aq_facility_scratch_bytes(1000) == 16000 + 24000 + 1008
    assert f"#define AQ_FACILITY_CELL_BITS {engine.FACILITY_CELL_BITS}" in header
    from aquaculture_amd import build
    assert ("facilities.hip", ["-ffp-contract=off"]) in build.SOURCES


def test_sort_keys_on_the_host():
    """The key packing and the grid (torch on the CPU): cells from 1, neighbours never two cells apart, refusals."""
    import torch
    from aquaculture_amd import engine
    xy = torch.from_numpy(cell_edges())
    keys, perm = engine.facility_sort_keys(xy, torch.zeros(xy.shape[0], dtype=torch.int32), 10.0)
    assert keys.dtype == torch.int64 and perm.dtype == torch.int32 and bool((keys[1:] >= keys[:-1]).all())
    assert sorted(perm.tolist()) == list(range(xy.shape[0]))
    mask = (1 << engine.FACILITY_CELL_BITS) - 1
    cx, cy = (keys & mask).numpy(), ((keys >> engine.FACILITY_CELL_BITS) & mask).numpy()
    assert cx.min() == 1 and cy.min() == 1 and int((keys >> 42).max()) == 0
    p = xy.numpy()[perm.numpy()]
    d = p[:, None, :] - p[None, :, :]
    near = d[..., 0] ** 2 + d[..., 1] ** 2 <= 100.0
    assert np.abs(cx[:, None] - cx[None, :])[near].max() <= 1 and np.abs(cy[:, None] - cy[None, :])[near].max() <= 1
    g = torch.tensor([0, 5], dtype=torch.int32)
    k2, _ = engine.facility_sort_keys(torch.tensor([[0.0, 0.0], [0.0, 0.0]], dtype=torch.float64), g, 10.0)
    assert k2.tolist() == [(1 << 21) | 1, (5 << 42) | (1 << 21) | 1]
    for bad_xy, bad_g, eps in ((torch.tensor([[0.0, 0.0], [3.0e7, 0.0]], dtype=torch.float64), g, 10.0),
                               (torch.tensor([[0.0, float("nan")], [1.0, 0.0]], dtype=torch.float64), g, 10.0),
                               (torch.zeros((2, 2), dtype=torch.float64), torch.tensor([0, 1 << 21], dtype=torch.int32), 10.0),
                               (torch.zeros((2, 2), dtype=torch.float64), torch.tensor([-1, 0], dtype=torch.int32), 10.0),
                               (torch.zeros((2, 2), dtype=torch.float64), g, 0.0)):
        with pytest.raises(ValueError):
            engine.facility_sort_keys(bad_xy, bad_g, eps)
