"""--facility-sites on the host: the numpy restatements of the three kernels (facility_sites.bounds_numpy, join_count_numpy, join_list_numpy,
through facility_sites.classify(cpu=True)) against the reference's procedure done literally (classify_literal: plain loops and pandas) on
the 4142 human labels of tests/golden/g16_label_boxes.npz clustered into facilities, against the 440 known sites of g16_known_sites.csv
inside the total bounds of g16_wanted_bboxes.csv; every rule on hand-built cases; the files, the command line, the options and the ABI
surface.  The inputs are shared with tests/test_gpu_facility_sites.py."""
import csv
import functools
import inspect
import json
import os

import numpy as np
import pytest

from test_model_errors import table_from_boxes

from aquaculture_amd import evaluate, facilities, facility_sites as fs, geocode, kfold

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
LABELS, SITES, BBOXES = (os.path.join(GOLDEN, f) for f in ("g16_label_boxes.npz", "g16_known_sites.csv", "g16_wanted_bboxes.csv"))
CIRCLE, SQUARE, RECT = (facilities.CLS_OF[t] for t in ("circle_farm", "square_farm", "rectangle_farm"))
NAN, INF = float("nan"), float("inf")
H = kfold.SITE_HALF_SIDE
COLUMNS = ("facility_index", "pass", "state", "num_cages", "unique", "location", "counts", "unique_additional_early", "unique_additional_late")
ARRAYS = ("bounds", "site_hits", "first_site")
SITE_ARRAYS = ("lat", "lon", "num_cages", "xy", "box")


# ---- the fixture ----

@functools.lru_cache(maxsize=None)
def fixture_truth():
    """The labels as evaluate.load_truth_geojson returns them (all 4142 are circle or square cages); shared, treat as read-only."""
    g = np.load(LABELS)
    box = np.asarray(g["bounds"], np.float64).reshape(-1, 4)
    t = {c: np.ascontiguousarray(box[:, i]) for i, c in enumerate(evaluate.BOX_COLUMNS)}
    t["cls"] = np.asarray([facilities.CLS_OF[evaluate.TRUTH_TYPES[ty]] for ty in g["types"][g["type"]].tolist()], np.int64)
    t["year"] = np.asarray(g["year"], np.int64)
    t["image"] = np.asarray([""] * box.shape[0], dtype=object)
    return t


@functools.lru_cache(maxsize=None)
def fixture_table():
    """One detection of confidence 1 per label, as test_model_errors.table_from_boxes makes the table."""
    t = fixture_truth()
    n = t["cls"].shape[0]
    box = np.stack([t[c] for c in evaluate.BOX_COLUMNS], 1)
    return table_from_boxes(box, t["cls"], t["year"], np.ones(n), np.tile([100, 100, 200, 200], (n, 1)), ["labels"], np.zeros(n, np.int64))


@functools.lru_cache(maxsize=None)
def fixture_facilities():
    return facilities.cluster(fixture_table(), "pass", 0.5, 50.0, 5, labels_fn=facilities.dbscan_numpy)


@functools.lru_cache(maxsize=None)
def fixture_sites():
    return fs.site_table(SITES, geocode.load_wanted_bboxes(BBOXES))


@functools.lru_cache(maxsize=None)
def fixture_literal(with_truth=False):
    return fs.classify_literal(fixture_facilities(), fixture_table(), SITES, geocode.load_wanted_bboxes(BBOXES), fixture_truth() if with_truth else None)


def write_truth(path, truth=None):
    """`truth` (default: the fixture) as the GeoJSON file evaluate.load_truth_geojson reads."""
    t = fixture_truth() if truth is None else truth
    names = {v: k for k, v in evaluate.TRUTH_TYPES.items()}
    feats = []
    for k in range(t["cls"].shape[0]):
        x0, y0, x1, y1 = (float(t[c][k]) for c in evaluate.BOX_COLUMNS)
        feats.append({"type": "Feature", "properties": {"type": names[geocode.REVERSE_CLASS_MAPPING[int(t["cls"][k])]], "year": int(t["year"][k]), "image": ""},
                      "geometry": {"type": "Polygon", "coordinates": [[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]]}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}, "features": feats}, f)
    return str(path)


def same(res, lit):
    """Every column of the result, the site table and both unique counts."""
    for k in COLUMNS:
        assert res[k] == lit[k], (k, res[k], lit[k])
    for k in ARRAYS:
        assert res[k].dtype == lit[k].dtype and res[k].tobytes() == lit[k].tobytes(), (k, res[k], lit[k])
    for k in ("label_hits", "first_label"):
        assert (res[k] is None) == (lit[k] is None) and (res[k] is None or np.array_equal(res[k], lit[k])), (k, res[k], lit[k])
    for k in SITE_ARRAYS:
        assert res["sites"][k].tobytes() == lit["sites"][k].tobytes(), (k, res["sites"][k], lit["sites"][k])
    assert (res["sites"]["read"], res["sites"]["rows"], res["sites"]["bounds"]) == (lit["sites"]["read"], lit["sites"]["rows"], lit["sites"]["bounds"])


def test_fixture_restatement_is_the_literal_procedure():
    fac, lit = fixture_facilities(), fixture_literal()
    assert os.path.getsize(LABELS) < 512 * 1024 and fixture_truth()["cls"].shape[0] == 4142
    # the literal procedure's numbers
    state = lit["state"]
    assert len(fac["facility_index"]) == 127 and lit["sites"]["read"] == 440 and lit["sites"]["box"].shape[0] == 13
    assert int((lit["site_hits"] > 0).sum()) == 93 and state.count("additional") == 34 and state.count("known") == 38 and state.count("known_early") == 55
    early = [f for f in range(127) if state[f] == "additional" and lit["pass"][f] in fs.EARLY]
    late = [f for f in range(127) if state[f] == "additional" and lit["pass"][f] in fs.LATE]
    assert (len(early), lit["unique_additional_early"], len(late), lit["unique_additional_late"]) == (18, 7, 16, 9)
    assert set(lit["pass"]) == set(fs.PASSES) and int(lit["site_hits"].max()) >= 2
    res = fs.classify(fac, fixture_table(), fixture_sites(), cpu=True)
    same(res, lit)
    assert res["label_hits"] is None and [u for u in res["unique"] if u is not None].count(True) == 16
    # a merged location points at an earlier unique facility of its own period whose rectangle meets its own
    for f in early + late:
        g = res["location"][f]
        assert res["unique"][g] and (g == f) == res["unique"][f] and g <= f
        assert res["bounds"][f, 0] <= res["bounds"][g, 2] and res["bounds"][g, 0] <= res["bounds"][f, 2]


def test_fixture_with_its_own_labels_as_truth_makes_every_facility_true():
    plain = fixture_literal()
    lit = fixture_literal(True)
    res = fs.classify(fixture_facilities(), fixture_table(), fixture_sites(), fixture_truth(), cpu=True)
    same(res, lit)
    assert res["state"] == plain["state"] and "not_true" not in res["state"] and int(res["label_hits"].min()) >= 5
    # every cage is a label of the facility's pass, so the first label is at most the smallest cage id
    assert all(0 <= int(res["first_label"][f]) <= min(fixture_facilities()["cage_ids"][f]) for f in range(127))


# ---- hand-built cases ----

LAT, LON = 43.3, 3.5


def site_xy(lat=LAT, lon=LON):
    x, y = geocode.lonlat_to_mercator(np.float64(lon), np.float64(lat))
    return float(x), float(y)


def write_case(tmp_path, sites=((LAT, LON, 10),), header="lat,lon,num_cages", span=50000.0):
    """A site file and a wanted-bboxes table of one box of +-span around the default site -> (sites_csv, bboxes_csv)."""
    with open(tmp_path / "sites.csv", "w") as f:
        f.write(header + "\n" + "".join(",".join(str(v) for v in row) + "\n" for row in sites))
    x, y = site_xy()
    x0, y0, x1, y1 = x - span, y - span, x + span, y + span
    with open(tmp_path / "wb.csv", "w") as f:
        f.write(f',geometry\n3,"POLYGON (({x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}, {x1!r} {y0!r}))"\n')
    return str(tmp_path / "sites.csv"), str(tmp_path / "wb.csv")


def hand_table(boxes, cls=None):
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = boxes.shape[0]
    with np.errstate(all="ignore"):
        return table_from_boxes(boxes, np.full(n, SQUARE) if cls is None else cls, np.full(n, 2015), np.ones(n), np.tile([100, 100, 200, 200], (n, 1)),
                                ["hand"], np.zeros(n, np.int64))


def hand_fac(members, passes=None, years=None):
    fac = {"facility_index": list(range(len(members))), "cage_ids": [list(m) for m in members]}
    fac.update({"pass": list(passes)} if passes is not None else {"year": list(years)})
    return fac


def both(tmp_path, boxes, members, passes=None, years=None, cls=None, truth=None, **case):
    """classify(cpu=True) of a hand-built table, checked against the literal procedure."""
    sites_csv, bboxes_csv = write_case(tmp_path, **case)
    wanted = geocode.load_wanted_bboxes(bboxes_csv)
    table, fac = hand_table(boxes, cls), hand_fac(members, passes, years)
    res = fs.classify(fac, table, fs.site_table(sites_csv, wanted), truth, cpu=True)
    same(res, fs.classify_literal(fac, table, sites_csv, wanted, truth))
    return res


def test_touching_a_site_box_counts_and_one_ulp_apart_does_not(tmp_path):
    x, y = site_xy()
    e, n = x + H, y + H                                     # the site box's right and upper edge, as site_regions adds them
    up = lambda v: float(np.nextafter(v, INF))
    boxes = [[e, y - 5, e + 30, y + 5],                     # touches the right edge
             [e, n, e + 30, n + 30],                        # touches the upper right corner
             [up(e), y - 5, e + 30, y + 5],                 # one ulp to the right of the edge
             [e, up(n), e + 30, n + 30],                    # one ulp above the corner
             [x - 5, y - 5, x + 5, y + 5]]                  # on the site
    res = both(tmp_path, boxes, [[0], [1], [2], [3], [4]], ["2013-2015"] * 5)
    assert res["site_hits"].tolist() == [1, 1, 0, 0, 1] and res["first_site"].tolist() == [0, 0, -1, -1, 0]
    assert res["state"] == ["known", "known", "additional", "additional", "known"]
    assert res["sites"]["box"][0].tolist() == [x - H, y - H, e, n]


def test_bounds_rectangle_cages_nan_members_and_facilities_without_a_box(tmp_path):
    x, y = site_xy()
    boxes = [[x + 5000, y, x + 5010, y + 10], [x + 5020, y - 3, x + 5030, y + 4], [x, y, x + 1, y + 1],      # two squares and a rectangle cage on the site
             [x + 7000, y, x + 7010, y + 10],                                                                # a rectangle cage alone
             [NAN, y, x + 9010, NAN], [x + 9000, y + 1, x + 9005, y + 6],                                    # a member with NaNs
             [NAN, NAN, NAN, NAN]]
    cls = [SQUARE, CIRCLE, RECT, RECT, SQUARE, SQUARE, CIRCLE]
    res = both(tmp_path, boxes, [[0, 1, 2], [3], [4, 5], [6], []], ["2016-2018"] * 5, cls=cls)
    assert res["bounds"][0].tolist() == [x + 5000, y - 3, x + 5030, y + 10]                 # the rectangle cage on the site does not enter
    assert res["state"] == ["additional", "no_bounds", "additional", "no_bounds", "no_bounds"] and res["num_cages"] == [3, 1, 2, 1, 0]
    assert np.isnan(res["bounds"][[1, 3, 4]]).all()
    assert res["bounds"][2].tolist() == [x + 9000, y, x + 9010, y + 6]                      # the numbers of the NaN member still count
    assert res["unique"] == [True, None, True, None, None] and res["location"] == [0, None, 2, None, None]


def test_periods_types_two_sites_and_a_site_outside_the_bounds(tmp_path):
    x, y = site_xy()
    second = (LAT + 0.004, LON)                             # some 600 m north: the two site boxes overlap
    far = (LAT + 2.0, LON)                                  # outside the wanted boxes' +-50 km
    fx, fy = site_xy(*far)
    boxes = [[x - 5, y + 300, x + 5, y + 310],              # meets both near sites
             [fx - 5, fy - 5, fx + 5, fy + 5],              # on the far site
             [x + 3000, y, x + 3010, y + 10]]               # near none
    years = [2014, 2014, 2014, 2003, 2003, 1999, 2022]
    members = [[0], [1], [2], [0], [2], [0], [2]]
    res = both(tmp_path, boxes, members, years=years, sites=((LAT, LON, 10), (*second, 20), (*far, 30)))
    assert res["sites"]["read"] == 3 and res["sites"]["box"].shape[0] == 2 and res["sites"]["lat"].tolist() == [LAT, second[0]]
    assert res["pass"] == ["2013-2015"] * 3 + ["2000-2004"] * 2 + ["No group"] * 2
    assert res["state"] == ["known", "additional", "additional", "known_early", "additional", "no_period", "no_period"]
    assert res["site_hits"].tolist() == [2, 0, 0, 2, 0, 2, 0] and res["first_site"].tolist() == [0, -1, -1, 0, -1, 0, -1]
    types = [(f["properties"]["type"], f["properties"]["pass"], f["properties"].get("facility_index")) for f in fs.combined_features(res)]
    assert types == ([("Additional facility", "2000-2004", 4)] + [("Known facility", p, None) for p in fs.EARLY for _ in range(2)] +
                     [("Known facility", "2013-2015", 0), ("Additional facility", "2013-2015", 1), ("Additional facility", "2013-2015", 2)])
    assert res["unique_additional_early"] == 1 and res["unique_additional_late"] == 2


def test_sites_merge_by_lat_lon_and_their_cages_add_up(tmp_path):
    rows = ((LAT, LON, 30), (LAT - 0.1, LON + 0.2, 7), (LAT, LON, 25), (LAT - 0.1, LON + 0.1, ""), (LAT - 0.1, LON + 0.1, "n/a"), ("", LON, 5))
    res = both(tmp_path, [[0, 0, 1, 1]], [[0]], ["2013-2015"], sites=rows)
    s = res["sites"]
    assert (s["rows"], s["read"]) == (5, 3) and s["lat"].tolist() == [LAT - 0.1, LAT - 0.1, LAT] and s["lon"].tolist() == [LON + 0.1, LON + 0.2, LON]
    assert np.isnan(s["num_cages"][0]) and s["num_cages"][1:].tolist() == [7.0, 55.0]
    props = [f["properties"] for f in fs.combined_features(res) if "site_index" in f["properties"]][:3]
    assert [(p["site_index"], p["num_cages"], p["cage_bin"]) for p in props] == [(0, None, None), (1, 7, "(0, 50]"), (2, 55, "(50, 100]")]


def test_site_file_without_num_cages_gives_nulls(tmp_path):
    res = both(tmp_path, [[0, 0, 1, 1]], [[0]], ["2013-2015"], sites=((LAT, LON), (LAT, LON + 0.1)), header="lat,lon")
    assert np.isnan(res["sites"]["num_cages"]).all() and res["sites"]["box"].shape[0] == 2
    assert all(f["properties"]["num_cages"] is None and f["properties"]["cage_bin"] is None for f in fs.combined_features(res)[:6])
    (tmp_path / "bad.csv").write_text("x,y\n1,2\n")
    with pytest.raises(ValueError, match="lat and lon"):
        fs.read_sites(str(tmp_path / "bad.csv"))


def test_cage_bin_is_pandas_cut():
    import pandas as pd
    values = [50, 51, 100, 500, 501, 0, 1, 100.5, -3, NAN]
    want = pd.cut(pd.Series(values, dtype=float), [0, 50, 100, 500]).astype(str).tolist()
    assert fs.cage_bin(values) == [None if w == "nan" else w for w in want]
    assert fs.cage_bin([50, 51, 100, 500, 501, 0]) == ["(0, 50]", "(50, 100]", "(50, 100]", "(100, 500]", None, None]


@pytest.mark.parametrize("order,unique,location", [("ABC", [True, False, True], [0, 0, 2]), ("BAC", [True, False, False], [0, 0, 0]),
                                                   ("CAB", [True, True, False], [0, 1, 0]), ("ACB", [True, True, False], [0, 1, 0])])
def test_chain_of_three_is_walked_in_index_order(tmp_path, order, unique, location):
    """A - B - C with A and C apart.  In index order the first unmarked facility is unique and marks its neighbours, whatever their pass."""
    x, y = site_xy()
    chain = {"A": [x + 5000, y, x + 5010, y + 10], "B": [x + 5008, y, x + 5020, y + 10], "C": [x + 5018, y, x + 5030, y + 10]}
    res = both(tmp_path, [chain[c] for c in order], [[0], [1], [2]], ["2013-2015", "2016-2018", "2019-2021"])
    assert res["state"] == ["additional"] * 3 and res["unique"] == unique and res["location"] == location
    assert res["unique_additional_late"] == unique.count(True) and res["unique_additional_early"] == 0
    # the same three in both periods: the sets are walked apart
    res = both(tmp_path, [chain[c] for c in order] * 2, [[k] for k in range(6)], ["2013-2015"] * 3 + ["2005-2009"] * 3)
    assert res["unique"] == unique * 2 and res["location"] == location + [v + 3 for v in location]


def test_not_true_by_a_pass_mismatch(tmp_path):
    x, y = site_xy()
    boxes = [[x + 5000, y, x + 5010, y + 10], [x + 6000, y, x + 6010, y + 10], [x + 7000, y, x + 7010, y + 10]]
    lab = np.asarray([[x + 5005, y + 5, x + 5006, y + 6], [x + 6005, y + 5, x + 6006, y + 6], [x + 6010, y + 10, x + 6011, y + 11],
                      [x + 5010, y, x + 5011, y + 1], [x + 6002, y + 2, x + 6003, y + 3]])
    truth = {c: np.ascontiguousarray(lab[:, i]) for i, c in enumerate(evaluate.BOX_COLUMNS)}
    truth.update(cls=np.full(5, SQUARE, np.int64), year=np.asarray([2008, 2014, 2015, 2013, 1999], np.int64), image=np.asarray([""] * 5, dtype=object))
    res = both(tmp_path, boxes, [[0], [1], [2]], ["2013-2015"] * 3, truth=truth)
    assert res["label_hits"].tolist() == [1, 2, 0] and res["first_label"].tolist() == [3, 1, -1]      # label 0 is of 2005-2009, label 4 of no pass
    assert res["state"] == ["additional", "additional", "not_true"] and res["unique"] == [True, True, None]
    truth["year"][3] = 2008
    res = both(tmp_path, boxes, [[0], [1], [2]], ["2013-2015"] * 3, truth=truth)
    assert res["label_hits"].tolist() == [0, 2, 0] and res["state"] == ["not_true", "additional", "not_true"]
    assert [f["properties"]["facility_index"] for f in fs.combined_features(res) if "facility_index" in f["properties"]] == [1]


# ---- the restatements on their own ----

def test_join_restatements_against_brute_force():
    r = np.random.default_rng(5)

    def boxes(n):
        a, w = r.integers(0, 40, (n, 2)).astype(np.float64), r.integers(0, 5, (n, 2)).astype(np.float64)
        return np.concatenate([a, a + w], 1)

    q, k = boxes(300), boxes(400)
    q[7], k[11, 2], k[12, 0] = NAN, NAN, NAN
    qg, kg = r.integers(-1, 5, 300).astype(np.int32), r.choice([0, 1, 3], 400).astype(np.int32)
    count, first = fs.join_count_numpy(q, qg, k, kg, 4)
    offset, lst = fs.join_list_numpy(q, qg, k, kg, 4)
    order = fs.key_order(k, kg)
    assert count.dtype == np.int32 and first.dtype == np.int32 and offset.dtype == np.int64 and lst.dtype == np.int32
    for i in range(300):
        hit = [int(j) for j in order if kg[j] == qg[i] and 0 <= qg[i] < 4 and q[i, 0] <= k[j, 2] and k[j, 0] <= q[i, 2] and q[i, 1] <= k[j, 3]
               and k[j, 1] <= q[i, 3]]
        assert count[i] == len(hit) and first[i] == (min(hit) if hit else -1) and lst[offset[i]:offset[i + 1]].tolist() == hit
    assert count[qg == 4].sum() == 0 and count[7] == 0 and 100 < (count > 0).sum() < 300


def test_bounds_restatement_signed_zeros_and_wrong_starts():
    box = np.asarray([[0.0, -0.0, 1.0, 2.0], [-0.0, 0.0, 1.0, 2.0], [5.0, 5.0, INF, 6.0], [NAN, 1.0, 2.0, NAN]])
    use = np.asarray([1, 1, 1, 1], np.uint8)
    b = fs.bounds_numpy([0, 2, 3, 4, 4], box, use)
    assert b[0].tolist() == [0.0, -0.0, 1.0, 2.0] and np.signbit(b[0]).tolist() == [False, True, False, False]   # a later equal value does not replace
    assert np.isnan(b[1:]).all()                            # an infinite selection, a NaN member alone, no member
    assert fs.bounds_numpy([-5, 9], box, np.asarray([1, 1, 0, 1], np.uint8)).tolist() == [[0.0, -0.0, 2.0, 2.0]]    # starts kept inside [0, E]
    assert fs.bounds_numpy([0], box, use).shape == (0, 4) and np.isnan(fs.bounds_numpy([0, 0], np.zeros((0, 4)), np.zeros(0, np.uint8))).all()


# ---- files and the command line ----

def read_csv(path):
    with open(path, newline="") as f:
        return list(csv.DictReader(f))


def test_files_read_back_column_for_column(tmp_path):
    truth_path = write_truth(tmp_path / "truth.geojson")
    res = fs.facility_sites_from_table(fixture_facilities(), fixture_table(), SITES, BBOXES, str(tmp_path / "out"), truth_path, cpu=True)
    same(res, fixture_literal(True))
    rows = read_csv(tmp_path / "out" / fs.CSV_FILE)
    assert list(rows[0]) == list(fs.CSV_COLUMNS) and len(rows) == 127
    opt = lambda v: None if v == "" else int(v)
    assert [int(r["facility_index"]) for r in rows] == res["facility_index"] and [r["pass"] for r in rows] == res["pass"]
    assert [r["state"] for r in rows] == res["state"] and [int(r["num_cages"]) for r in rows] == res["num_cages"]
    assert np.asarray([[float(r[c]) for c in ("x0", "y0", "x1", "y1")] for r in rows]).tobytes() == res["bounds"].tobytes()
    for col in ("label_hits", "first_label", "site_hits", "first_site"):
        assert [int(r[col]) for r in rows] == res[col].tolist(), col
    assert [None if r["unique"] == "" else bool(int(r["unique"])) for r in rows] == res["unique"] and [opt(r["location"]) for r in rows] == res["location"]
    doc = json.load(open(tmp_path / "out" / fs.GEOJSON_FILE))
    assert doc["crs"]["properties"]["name"].endswith("3857") and len(doc["features"]) == 18 + 3 * 13 + 38 + 16
    ours = [f for f in doc["features"] if "facility_index" in f["properties"]]
    assert [f["properties"]["facility_index"] for f in ours] == ([i for i in range(127) if res["state"][i] == "additional" and res["pass"][i] in fs.EARLY] +
                                                                 [i for i in range(127) if res["state"][i] in fs.TYPE_NAMES and res["pass"][i] in fs.LATE])
    for f in ours:
        p, i = f["properties"], f["properties"]["facility_index"]
        b = res["bounds"][i]
        assert f["geometry"] == {"type": "Point", "coordinates": [0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])]}
        assert (p["type"], p["pass"], p["num_cages"], p["first_site"], p["unique"], p["location"]) == \
               (fs.TYPE_NAMES[res["state"][i]], res["pass"][i], res["num_cages"][i], int(res["first_site"][i]), res["unique"][i], res["location"][i])
        assert p["cage_bin"] == fs.cage_bin([p["num_cages"]])[0]
    sites = [f for f in doc["features"] if "site_index" in f["properties"]]
    assert [(f["properties"]["pass"], f["properties"]["site_index"]) for f in sites] == [(p, s) for p in fs.EARLY for s in range(13)]
    assert all(f["properties"]["type"] == "Known facility" and f["geometry"]["coordinates"] == res["sites"]["xy"][f["properties"]["site_index"]].tolist()
               for f in sites)
    assert [f["properties"]["num_cages"] for f in sites[:13]] == [fs._num(v) for v in res["sites"]["num_cages"]]
    s = json.load(open(tmp_path / "out" / fs.JSON_FILE))
    assert (s["sites"], s["bboxes"], s["truth"]) == ("g16_known_sites.csv", "g16_wanted_bboxes.csv", "truth.geojson")
    assert (s["sites_read"], s["sites_in_bounds"], s["facilities"], s["device"], s["cpu"]) == (440, 13, 127, "cpu", True)
    assert (s["unique_additional_early"], s["unique_additional_late"]) == (7, 9) and s["counts"] == res["counts"]
    assert sum(n for c in s["counts"].values() for n in c.values()) == 127 and s["counts"]["2013-2015"] == {"additional": 4, "known": 14}


def test_command_line_on_the_cpu(tmp_path, capsys):
    from test_gpu_facilities import synthetic_run
    labels, csv_path = synthetic_run(tmp_path)
    (x0, y0, _, y1), = geocode.load_wanted_bboxes(csv_path).values()
    lon, lat = (float(v) for v in geocode.mercator_to_lonlat(np.float64(x0 + 200.0), np.float64(y1 - 150.0)))      # among the cages of both facilities
    sites_csv, _ = write_case(tmp_path, sites=((repr(lat), repr(lon), 120), (repr(lat + 1.0), repr(lon), 4)))
    assert fs.main(["--labels", labels, "--geocode-bboxes", csv_path, "--sites", sites_csv, "--cpu", "--out", str(tmp_path / "out")]) == 0
    assert "2 facilities against 1 of 2 known sites: 2 known" in capsys.readouterr().out
    rows = read_csv(tmp_path / "out" / fs.CSV_FILE)
    assert [(r["pass"], r["state"], r["num_cages"], r["site_hits"], r["label_hits"]) for r in rows] == [("2013-2015", "known", "6", "1", ""),
                                                                                                        ("2013-2015", "known", "5", "1", "")]
    s = json.load(open(tmp_path / "out" / fs.JSON_FILE))
    assert s["cpu"] is True and s["truth"] is None and s["sites_in_bounds"] == 1 and s["counts"] == {"2013-2015": {"known": 2}}
    assert len(json.load(open(tmp_path / "out" / fs.GEOJSON_FILE))["features"]) == 3 + 2
    table = geocode.geocode_label_dir(labels, csv_path)
    fac = facilities.cluster(table, "year", 0.5, 10.0, 5, labels_fn=facilities.dbscan_numpy)
    same(fs.classify(fac, table, fs.site_table(sites_csv, geocode.load_wanted_bboxes(csv_path)), cpu=True),
         fs.classify_literal(fac, table, sites_csv, geocode.load_wanted_bboxes(csv_path)))


# ---- options and the ABI surface ----

def test_detect_py_options():
    from aquaculture_amd import detect
    with pytest.raises(SystemExit):
        detect.parse_opt(["--facility-sites", "sites.csv", "--geocode-bboxes", "wb.csv"])                # needs --facilities
    with pytest.raises(SystemExit):
        detect.parse_opt(["--facility-sites", "sites.csv", "--facilities"])                               # needs --geocode-bboxes
    with pytest.raises(ValueError, match="--facility-sites.*needs --facilities and --geocode-bboxes"):
        detect.run("w.pt", "src", facility_sites="sites.csv", geocode_bboxes="wb.csv")
    with pytest.raises(ValueError, match="--facility-sites"):
        detect.run("w.pt", "src", facility_sites="sites.csv", facilities="")
    assert detect.FACILITY_SITES_NEED_FACILITIES.startswith("--facility-sites")
    src = inspect.getsource(detect)
    assert src.index("MODEL_ERRORS_NEED_GEOCODE =") < src.index("FACILITY_SITES_NEED_FACILITIES =") < src.index("def run_params(")
    opt = detect.parse_opt(["--facility-sites", "sites.csv", "--facilities", "--geocode-bboxes", "wb.csv", "--facility-sites-truth", "t.geojson",
                            "--facility-sites-out", "out"])
    assert (opt.facility_sites, opt.facility_sites_truth, opt.facility_sites_out) == ("sites.csv", "t.geojson", "out")
    opt = detect.parse_opt([])
    assert (opt.facility_sites, opt.facility_sites_truth, opt.facility_sites_out) == (None, None, None)
    params = inspect.signature(detect.run).parameters
    assert all(params[k].default is None for k in ("facility_sites", "facility_sites_truth", "facility_sites_out"))
    assert "facility_sites" not in detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)


def test_build_and_exports():
    from aquaculture_amd import build, engine
    assert ("facility_sites.hip", ["-ffp-contract=off"]) in build.SOURCES
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_facility_bounds_f64", "aq_box_join_count_i32", "aq_box_join_list_i32"):
        assert "int " + name + "(" in header and name in engine.EXPORTS
    assert all(callable(getattr(engine, f)) for f in ("facility_bounds", "box_join_count", "box_join_list"))
    guards = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "size_guards.h")).read()
    assert guards.count("facility_sites_count_fits(ll n)") == 1
    source = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "facility_sites.hip")).read()
    assert '#include "box_join.h"' in source and "sg::facility_sites_count_fits" in source and "box_join_run(" in source and "boxes_meet(" in source
    code = "\n".join(line.split("//")[0] for line in source.splitlines())
    assert "atomic" not in code.lower() and "malloc" not in code.lower()                      # comparisons and plain stores only, nothing allocated


def test_symbols_are_bound_and_refuse_bad_arguments_without_a_launch(lib):
    """Every refusal comes from the arguments and the host copies alone: the `device` addresses here are never read."""
    for name in ("aq_facility_bounds_f64", "aq_box_join_count_i32", "aq_box_join_list_i32"):
        assert hasattr(lib, name) and getattr(lib, name).argtypes is not None
    D = 0x10000                                             # an aligned address nothing is behind
    host = lambda v, dt=np.int32: np.ascontiguousarray(v, dtype=dt)
    err = lambda: lib.aq_last_error().decode()

    def bounds(start=(0, 2, 3), F=2, E=3, s_p=D, box_p=D, use_p=D, out_p=D, host_p=True):
        h = host(start)
        return lib.aq_facility_bounds_f64(s_p, h.ctypes.data if host_p else None, F, box_p, use_p, E, out_p, None)

    for kw, msg in (({"F": 1 << 31}, "2^31"), ({"F": -1}, "2^31"), ({"E": 1 << 31}, "2^31"), ({"E": -1}, "2^31"), ({"start": (0, 2, 1)}, "entry start 2"),
                    ({"start": (0, 2, 4)}, "entry start 2"), ({"start": (-1, 2, 3)}, "entry start 0"), ({"host_p": False}, "null pointer"),
                    ({"s_p": None}, "null pointer"), ({"box_p": None}, "null pointer"), ({"use_p": None}, "null pointer"), ({"out_p": None}, "null pointer"),
                    ({"s_p": D + 2}, "unaligned"), ({"box_p": D + 16}, "unaligned"), ({"out_p": D + 8}, "unaligned")):
        assert bounds(**kw) == -1 and msg in err(), (kw, err())
    assert lib.aq_facility_bounds_f64(None, None, 0, None, None, 0, None, None) == 0          # F = 0 does nothing

    def join(fn, start=(0, 1, 2), Q=2, N=2, G=2, q_p=D, g_p=D, k_p=D, id_p=D, s_p=D, host_p=True, tail=()):
        h = host(start)
        return fn(q_p, g_p, Q, k_p, id_p, s_p, h.ctypes.data if host_p else None, N, G, *tail, None)

    common = (({"Q": 1 << 31}, "2^31"), ({"Q": -1}, "2^31"), ({"N": 1 << 31}, "2^31"), ({"N": -1}, "2^31"), ({"G": 1 << 31}, "2^31"), ({"G": -1}, "2^31"),
              ({"start": (0, 2, 1)}, "group start 2"), ({"start": (0, 1, 3)}, "group start 2"), ({"start": (-1, 1, 2)}, "group start 0"),
              ({"host_p": False}, "null pointer"), ({"q_p": None}, "null pointer"), ({"g_p": None}, "null pointer"), ({"k_p": None}, "null pointer"),
              ({"id_p": None}, "null pointer"), ({"s_p": None}, "null pointer"), ({"q_p": D + 16}, "unaligned"), ({"k_p": D + 8}, "unaligned"),
              ({"g_p": D + 2}, "unaligned"), ({"id_p": D + 1}, "unaligned"), ({"s_p": D + 2}, "unaligned"))
    for kw, msg in common:
        assert join(lib.aq_box_join_count_i32, tail=(D, D), **kw) == -1 and msg in err(), (kw, err())
    for tail, msg in (((None, D), "null pointer"), ((D, None), "null pointer"), ((D + 2, D), "unaligned"), ((D, D + 1), "unaligned")):
        assert join(lib.aq_box_join_count_i32, tail=tail) == -1 and msg in err(), (tail, err())
    assert lib.aq_box_join_count_i32(None, None, 0, None, None, None, None, 0, 0, None, None, None) == 0          # Q = 0 does nothing

    def lists(offset=(0, 1, 3), total=3, off_p=D, list_p=D, off_host=True, **kw):
        o = host(offset, np.int64)
        return join(lib.aq_box_join_list_i32, tail=(off_p, o.ctypes.data if off_host else None, list_p, total), **kw)

    for kw, msg in common:
        assert lists(**kw) == -1 and msg in err(), (kw, err())
    for kw, msg in (({"total": 1 << 31}, "2^31"), ({"total": -1}, "2^31"), ({"offset": (0, 2, 1)}, "offset 2"), ({"offset": (0, 1, 4)}, "offset 2"),
                    ({"offset": (-1, 1, 3)}, "offset 0"), ({"off_host": False}, "null pointer"), ({"off_p": None}, "null pointer"),
                    ({"list_p": None}, "null pointer"), ({"off_p": D + 4}, "unaligned"), ({"list_p": D + 2}, "unaligned")):
        assert lists(**kw) == -1 and msg in err(), (kw, err())
    assert lib.aq_box_join_list_i32(None, None, 0, None, None, None, None, 0, 0, None, None, None, 0, None) == 0  # Q = 0 does nothing
