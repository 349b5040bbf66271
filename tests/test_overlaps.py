"""--dedup-overlaps on the CPU: the regions of the reference's own overlapping download boxes against the file the reference ships
(tests/golden/g15_*), the clip's two host forms (overlaps.clip_numpy, the kernel's steps, against overlaps.clip_literal, the rule in plain
loops) on named cases with hand-written states and on a random case, the files, and the survivor mask reaching the facility step.
The cases are shared with tests/test_gpu_overlaps.py."""
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
NAN4 = (np.nan,) * 4

# name: (boxes in file order, [(box row, D, expected state, expected bounds, expected area)], expected has_region)
NAMED = {
    "no partner": ([(0, 0, 10, 10)],
                   [(0, (2, 2, 4, 4), 1, (2, 2, 4, 4), 4.0)], [1]),
    "inside a covered part": ([(0, 0, 10, 10), (5, 0, 15, 10)],
                              [(1, (6, 2, 8, 4), 0, NAN4, 0.0), (1, (11, 2, 13, 4), 1, (11, 2, 13, 4), 4.0), (0, (6, 2, 8, 4), 1, (6, 2, 8, 4), 4.0),
                               (1, (6, 2, 6, 4), 0, NAN4, 0.0)], [1, 1]),                    # (the last: a D without area inside the covered part)
    # region of box 1: the square (5, 5, 15, 15) without its lower left quarter.  D's pieces: (10, 8, 12, 10) in the lower row, (8, 10, 10, 12)
    # and (10, 10, 12, 12) in the upper: 4 + (4 + 4)
    "straddling an L": ([(0, 0, 10, 10), (5, 5, 15, 15)],
                        [(1, (8, 8, 12, 12), 2, (8, 8, 12, 12), 12.0), (1, (9, 6, 12, 9), 2, (10, 6, 12, 9), 6.0)], [1, 1]),
    "touching along an edge": ([(0, 0, 10, 10), (5, 0, 15, 10)],
                               [(1, (6, 2, 10, 4), 3, (10, 2, 10, 4), 0.0)], [1, 1]),
    # box 3 keeps only its upper right quarter (10, 10, 15, 15); D lies in the lower left one and reaches the corner (10, 10)
    "touching at a corner": ([(0, 0, 10, 10), (10, 0, 20, 10), (0, 10, 10, 20), (5, 5, 15, 15)],
                             [(3, (6, 6, 10, 10), 3, (10, 10, 10, 10), 0.0), (3, (6, 6, 9, 9), 0, NAN4, 0.0)], [1, 1, 1, 1]),
    "a dropped box": ([(0, 0, 10, 10), (2, 2, 8, 8)],
                      [(1, (3, 3, 4, 4), 0, NAN4, 0.0), (1, (2, 2, 8, 8), 0, NAN4, 0.0)], [1, 0]),
    # an earlier box strictly inside: rows (3..4, 4..6, 6..7) of D give (1 + 2 + 1) + (2 + 2) + (1 + 2 + 1)
    "a region with a hole": ([(4, 4, 6, 6), (0, 0, 10, 10)],
                             [(1, (4.5, 4.5, 5.5, 5.5), 0, NAN4, 0.0), (1, (3, 3, 7, 7), 2, (3, 3, 7, 7), 12.0), (1, (1, 1, 3, 3), 1, (1, 1, 3, 3), 4.0),
                              (1, (4, 4, 6, 6), 3, (4, 4, 6, 6), 0.0)], [1, 1]),
    "two cells meeting diagonally": ([(-5, -5, 5, 5), (5, 5, 15, 15), (0, 0, 10, 10)],
                                     [(2, (4, 4, 6, 6), 2, (4, 4, 6, 6), 2.0), (2, (1, 1, 3, 3), 0, NAN4, 0.0), (2, (6, 1, 8, 3), 1, (6, 1, 8, 3), 4.0)],
                                     [1, 1, 1]),
    "a D without area": ([(0, 0, 10, 10)],
                         [(0, (3, 3, 3, 5), 3, (3, 3, 3, 5), 0.0), (0, (3, 3, 3, 3), 3, (3, 3, 3, 3), 0.0), (0, (12, 3, 12, 5), 0, NAN4, 0.0)], [1]),
}


def named_arrays(name):
    boxes, dets, has = NAMED[name]
    return (np.asarray(boxes, np.float64).reshape(-1, 4), np.asarray([d[0] for d in dets], np.int32),
            np.asarray([d[1] for d in dets], np.float64).reshape(-1, 4))


def named_expected(name):
    _, dets, has = NAMED[name]
    return {"state": np.asarray([d[2] for d in dets], np.uint8), "clip_bounds": np.asarray([d[3] for d in dets], np.float64).reshape(-1, 4),
            "clip_area": np.asarray([d[4] for d in dets], np.float64), "has_region": np.asarray(has, np.uint8)}


def same_bytes(a, b):
    for k in ("state", "clip_bounds", "clip_area", "has_region"):
        x, y = np.asarray(a[k]), np.asarray(b[k])
        assert x.dtype == y.dtype and x.shape == y.shape and x.tobytes() == y.tobytes(), (k, x[:8], y[:8])


_random = {}


def random_case():
    """300 boxes of a jittered 20 x 15 grid (pitch 100, sides 50 .. 200, no two coordinates alike) in a shuffled order and 4,000 detections:
    half anywhere in their box; the others placed on the overlap O of their box and one of its earlier partners -- inside O, inside O with
    one side exactly on O's, or across one side of O.  -> (boxes, det_row, dets, literal), computed once."""
    if _random:
        return _random["case"]
    from aquaculture_amd import overlaps
    rng = np.random.default_rng(20261019)
    gx, gy = np.meshgrid(np.arange(20), np.arange(15))
    c = np.stack([gx.ravel(), gy.ravel()], 1) * 100.0 + 500000.0 + rng.uniform(-30, 30, (300, 2))
    side = rng.uniform(50.0, 200.0, (300, 2))
    boxes = np.concatenate([c - side / 2, c + side / 2], 1)[rng.permutation(300)]
    assert np.unique(boxes[:, [0, 2]]).size == 600 and np.unique(boxes[:, [1, 3]]).size == 600
    start, partner = overlaps.partners_numpy(boxes)
    with_partner = np.nonzero(np.diff(start) > 0)[0]
    rows, dets = [], []
    for k in range(4000):
        w, h = rng.uniform(3.0, 25.0, 2)
        if k % 2 == 0:
            i = int(rng.integers(300))
            x = rng.uniform(boxes[i, 0], boxes[i, 2] - w)
            y = rng.uniform(boxes[i, 1], boxes[i, 3] - h)
        else:
            i = int(rng.choice(with_partner))
            j = int(rng.choice(partner[start[i]:start[i + 1]]))
            o = (max(boxes[i, 0], boxes[j, 0]), max(boxes[i, 1], boxes[j, 1]), min(boxes[i, 2], boxes[j, 2]), min(boxes[i, 3], boxes[j, 3]))
            w, h = min(w, (o[2] - o[0]) / 2), min(h, (o[3] - o[1]) / 2)
            x, y = rng.uniform(o[0], o[2] - w), rng.uniform(o[1], o[3] - h)
            mode, edge = int(rng.integers(3)), int(rng.integers(4))
            if mode:                                        # 1: a side exactly on O's, from inside; 2: across that side
                shift = 0.0 if mode == 1 else (w if edge in (0, 2) else h) / 2
                if edge == 0:
                    x = o[0] - shift
                elif edge == 1:
                    y = o[1] - shift
                elif edge == 2:
                    x = o[2] - w + shift
                else:
                    y = o[3] - h + shift
                if mode == 1 and edge in (2, 3):            # the far side is a sum: put the exact value there
                    rows.append(i)
                    dets.append((o[2] - w, y, o[2], y + h) if edge == 2 else (x, o[3] - h, x + w, o[3]))
                    continue
        rows.append(i)
        dets.append((x, y, x + w, y + h))
    det_row, dets = np.asarray(rows, np.int32), np.asarray(dets, np.float64)
    assert (dets[:, 0] < dets[:, 2]).all() and (dets[:, 1] < dets[:, 3]).all()
    _random["case"] = (boxes, det_row, dets, overlaps.clip_literal(boxes, det_row, dets))
    return _random["case"]


def strips_case():
    """One box after 70 thin earlier strips that cross it from side to side, every second one: more than 64 partners, a grid of 141 rows."""
    strips = [(-5.0, 1.0 + 2 * k, 205.0, 2.0 + 2 * k) for k in range(70)]
    boxes = np.asarray(strips + [(0.0, 0.0, 200.0, 142.0)], np.float64)
    dets = np.asarray([(10, 0.5, 30, 141.5), (10, 1.25, 30, 1.75), (10, 2, 30, 3), (10, 1, 30, 2), (50, 100.5, 60, 107.5), (-5, 3, 0, 5)], np.float64)
    return boxes, np.full(dets.shape[0], 70, np.int32), dets, np.asarray([2, 0, 1, 3, 2, 3], np.uint8)


# ---- the regions against the reference's shipped file ----

def _normal_ring(ring):
    r = [tuple(p) for p in ring[:-1]] if tuple(ring[0]) == tuple(ring[-1]) else [tuple(p) for p in ring]
    k = len(r)
    r = [r[q] for q in range(k) if not (r[q - 1][0] == r[q][0] == r[(q + 1) % k][0] or r[q - 1][1] == r[q][1] == r[(q + 1) % k][1])]
    if sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(r, r[1:] + r[:1])) < 0:
        r = r[::-1]
    m = r.index(min(r))
    return r[m:] + r[:m]


def _normal_polygons(geom):
    polys = [geom["coordinates"]] if geom["type"] == "Polygon" else geom["coordinates"]
    return sorted([_normal_ring(p[0])] + sorted(_normal_ring(h) for h in p[1:]) for p in polys)


def _shoelace(geom):
    """Polygon area by the shoelace formula on coordinates taken relative to each ring's first vertex (as GEOS does: the products of raw
    EPSG:3857 coordinates are near 2e12, where an ulp is 2.4e-4 m2)."""
    total = 0.0
    for p in ([geom["coordinates"]] if geom["type"] == "Polygon" else geom["coordinates"]):
        for ring in p:
            r = [(q[0] - ring[0][0], q[1] - ring[0][1]) for q in ring]
            total += (1 if ring is p[0] else -1) * abs(sum(a[0] * b[1] - b[0] * a[1] for a, b in zip(r, r[1:]))) / 2
    return total


def test_regions_of_the_reference_boxes_are_the_shipped_polygons():
    from aquaculture_amd import overlaps
    ids, boxes = overlaps.load_boxes(os.path.join(GOLDEN, "g15_wanted_bboxes.csv"))
    shipped = {int(f["properties"]["bbox_ind"]): f["geometry"] for f in json.load(open(os.path.join(GOLDEN, "g15_wanted_bboxes_dedup.json")))["features"]}
    assert ids.shape[0] == 375 and list(ids) == sorted(ids)
    reg = overlaps.regions(boxes)
    dropped = {int(i) for i, g in zip(ids, reg) if g is None}
    assert dropped == set(ids.tolist()) - set(shipped) and len(dropped) >= 1
    assert len(dropped) == 97 and set(shipped) <= set(ids.tolist())
    start, partner = overlaps.partners_numpy(boxes)
    assert int(np.diff(start).max()) == 8 and int((np.diff(start) > 0).sum()) == 194
    has = overlaps.clip_numpy(boxes, start, partner, np.zeros(0, np.int32), np.zeros((0, 4)))["has_region"]
    assert {int(i) for i, h in zip(ids, has) if not h} == dropped
    worst = 0.0
    for k, (i, g) in enumerate(zip(ids.tolist(), reg)):
        if g is None:
            continue
        assert _normal_polygons(g) == _normal_polygons(shipped[i]), i
        a, b = overlaps.region_area(boxes, k), _shoelace(shipped[i])
        ulp = np.spacing(max(a, b))
        worst = max(worst, abs(a - b) / ulp)
        assert abs(a - b) <= 4 * ulp, (i, a, b)
        # exterior rings counter-clockwise, holes clockwise, no collinear vertex
        for p in ([g["coordinates"]] if g["type"] == "Polygon" else g["coordinates"]):
            for ring in p:
                twice = sum(a_[0] * b_[1] - b_[0] * a_[1] for a_, b_ in zip(ring, ring[1:]))
                assert ring[0] == ring[-1] and (twice > 0) == (ring is p[0]) and len(_normal_ring(ring)) == len(ring) - 1
    print(f"largest area difference: {worst:g} ulp")


def test_regions_with_a_hole_and_with_diagonal_cells():
    from aquaculture_amd import overlaps
    hole = overlaps.regions(named_arrays("a region with a hole")[0])
    assert hole[0] == {"type": "Polygon", "coordinates": [[[4.0, 4.0], [6.0, 4.0], [6.0, 6.0], [4.0, 6.0], [4.0, 4.0]]]}
    assert hole[1] == {"type": "Polygon", "coordinates": [[[0.0, 0.0], [10.0, 0.0], [10.0, 10.0], [0.0, 10.0], [0.0, 0.0]],
                                                          [[4.0, 4.0], [4.0, 6.0], [6.0, 6.0], [6.0, 4.0], [4.0, 4.0]]]}
    diag = overlaps.regions(named_arrays("two cells meeting diagonally")[0])[2]
    assert diag["type"] == "MultiPolygon" and sorted(diag["coordinates"]) == [
        [[[0.0, 5.0], [5.0, 5.0], [5.0, 10.0], [0.0, 10.0], [0.0, 5.0]]], [[[5.0, 0.0], [10.0, 0.0], [10.0, 5.0], [5.0, 5.0], [5.0, 0.0]]]]
    ell = overlaps.regions(named_arrays("straddling an L")[0])[1]
    assert ell == {"type": "Polygon", "coordinates": [[[5.0, 10.0], [10.0, 10.0], [10.0, 5.0], [15.0, 5.0], [15.0, 15.0], [5.0, 15.0], [5.0, 10.0]]]}
    assert overlaps.regions(named_arrays("a dropped box")[0])[1] is None and overlaps.regions(np.zeros((0, 4))) == []


# ---- the clip ----

@pytest.mark.parametrize("name", list(NAMED))
def test_named_cases(name):
    from aquaculture_amd import overlaps
    boxes, det_row, dets = named_arrays(name)
    start, partner = overlaps.partners_numpy(boxes)
    got = overlaps.clip_numpy(boxes, start, partner, det_row, dets)
    same_bytes(got, named_expected(name))
    same_bytes(got, overlaps.clip_literal(boxes, det_row, dets))
    assert overlaps.survivors(got["state"]).tolist() == [s != 0 for s in named_expected(name)["state"]]


def test_unknown_bbox_ind_names_the_image():
    from aquaculture_amd import overlaps
    ids = np.asarray([7, 3, 12], np.int64)
    assert overlaps.box_rows(ids, [3, 12, 7, 3], ["a", "b", "c", "d"]).tolist() == [1, 2, 0, 1]
    with pytest.raises(KeyError, match=r"image 'ORTHO2015_5_0_0.jpeg'.*bbox_ind 5 is not in the box table"):
        overlaps.box_rows(ids, [3, 5], ["ORTHO2015_3_0_0.jpeg", "ORTHO2015_5_0_0.jpeg"])
    with pytest.raises(KeyError, match="ORTHO2015_5_0_0"):
        overlaps.table_rows({"stems": np.asarray(["ORTHO2015_5_0_0"], object), "image": np.zeros(2, np.int64)}, ids)
    with pytest.raises(ValueError, match="outside the 1 boxes"):
        overlaps.clip_numpy(np.zeros((1, 4)), [0, 0], [], [1], np.zeros((1, 4)))


def test_random_case_numpy_is_the_literal_rule():
    from aquaculture_amd import overlaps
    boxes, det_row, dets, literal = random_case()
    start, partner = overlaps.partners_numpy(boxes)
    got = overlaps.clip_numpy(boxes, start, partner, det_row, dets)
    same_bytes(got, literal)
    counts = np.bincount(got["state"], minlength=4)
    print("states:", dict(zip(overlaps.STATE_NAMES, counts.tolist())), "boxes without a region:", int((got["has_region"] == 0).sum()),
          "partners at most:", int(np.diff(start).max()))
    assert (counts >= 20).all()                             # all four states occur (a condition on the generator)
    # the clipped area is what is left of D: between 0 and D's own area, and equal to it for a whole one inside its box
    d_area = (dets[:, 2] - dets[:, 0]) * (dets[:, 3] - dets[:, 1])
    clipped = got["state"] == overlaps.CLIPPED
    assert (got["clip_area"][clipped] > 0).all() and (got["clip_area"][clipped] < d_area[clipped]).all()
    assert (got["clip_area"][got["state"] == overlaps.TOUCHING] == 0).all() and np.isnan(got["clip_bounds"][got["state"] == 0]).all()


def test_more_than_64_partners_on_the_host():
    from aquaculture_amd import overlaps
    boxes, det_row, dets, want = strips_case()
    start, partner = overlaps.partners_numpy(boxes)
    assert start[-1] - start[-2] == 70 and partner[start[-2]:].tolist() == list(range(70))
    got = overlaps.clip_numpy(boxes, start, partner, det_row, dets)
    assert got["state"].tolist() == want.tolist() and got["clip_area"][0] == 20 * 71.0 and got["clip_area"][4] == 10 * 3.5
    same_bytes(got, overlaps.clip_literal(boxes, det_row, dets))


def test_band_table_on_the_host():
    from aquaculture_amd import overlaps
    boxes = random_case()[0]
    for nbands in (None, 1, 5, 4000):
        t = overlaps.band_table(boxes, nbands)
        lo, hi = overlaps._band(boxes[:, 1], t["Y0"], t["h"], t["nbands"]), overlaps._band(boxes[:, 3], t["Y0"], t["h"], t["nbands"])
        assert t["band_start"][0] == 0 and t["band_start"][-1] == t["entry_box"].shape[0] == int((hi - lo + 1).sum())
        for b in (0, t["nbands"] // 2, t["nbands"] - 1):
            run = t["entry_box"][t["band_start"][b]:t["band_start"][b + 1]]
            assert run.tolist() == np.nonzero((lo <= b) & (b <= hi))[0].tolist()
    assert overlaps.band_table(np.zeros((0, 4)))["nbands"] == 1
    with pytest.raises(ValueError, match="not finite"):
        overlaps.band_table([[0, 0, np.inf, 1]])


# ---- the files and the command line ----

def overlap_run(tmp_path):
    """Two scenes of 1843.2 m: scene 1, and scene 3 half a scene further east and later in the file, so that scene 3's western half is
    scene 1's eastern half (0.3 m per pixel: pixel p of scene 3 is pixel p + 3072 of scene 1).  Three cages lie in that overlap and were
    detected in both scenes; five more lie in scene 3's own half; one stray lies in scene 1's own.  -> (labels dir, csv path)."""
    from aquaculture_amd import geocode
    labels = tmp_path / "labels"
    labels.mkdir()
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    csv_path = tmp_path / "wanted_bboxes.csv"
    with open(csv_path, "w") as f:
        f.write(",geometry\n")
        for ind, dx in ((1, 0.0), (3, 921.6)):
            a, b, c, d = x0 + dx, y0, x0 + dx + 1843.2, y0 + 1843.2
            f.write(f'{ind},"POLYGON (({c!r} {b!r}, {c!r} {d!r}, {a!r} {d!r}, {a!r} {b!r}, {c!r} {b!r}))"\n')
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    files = {"ORTHOIMAGERY.ORTHOPHOTOS2015_1_3072_0": [row(0, 100 + 12 * k, 500, 10, 0.9) for k in range(3)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_1_0_0": [row(1, 800, 100, 10, 0.9)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0": [row(0, 100 + 12 * k, 500, 10, 0.8) for k in range(3)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_4096_0": [row(1, 300 + 12 * k, 200, 10, 0.8) for k in range(5)],
             # across scene 1's eastern edge (pixel 3072 of scene 3): clipped
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_3072_1024": [row(1, 0, 300, 20, 0.7)],
             "ORTHOIMAGERY.ORTHOPHOTOS2015_3_2048_1024": [row(1, 1000, 600, 10, 0.7)]}
    for stem, rows in files.items():
        (labels / (stem + ".txt")).write_text("".join(rows))
    return str(labels), str(csv_path)


def test_command_line_writes_the_three_files(tmp_path):
    from aquaculture_amd import geocode, overlaps
    labels, csv_path = overlap_run(tmp_path)
    before = str(tmp_path / "before.geojson")
    table = geocode.geocode_label_dir(labels, csv_path, before)
    out = tmp_path / "out"
    assert overlaps.main(["--labels", labels, "--geocode-bboxes", csv_path, "--out", str(out), "--cpu"]) == 0
    assert sorted(os.listdir(out)) == sorted([overlaps.DETECTIONS_FILE, overlaps.REGIONS_FILE, overlaps.SUMMARY_FILE])
    geocode.geocode_label_dir(labels, csv_path, str(tmp_path / "after.geojson"))
    assert open(before, "rb").read() == open(tmp_path / "after.geojson", "rb").read()
    full = json.load(open(before))["features"]
    kept = json.load(open(out / overlaps.DETECTIONS_FILE))
    s = json.load(open(out / overlaps.SUMMARY_FILE))
    stems = [str(v) for v in table["stems"]]
    in_overlap = [k for k in range(len(full)) if stems[int(table["image"][k])].endswith(("_3_0_0", "_3_2048_1024"))]
    want = [k for k in range(len(full)) if k not in in_overlap]
    assert [f["properties"]["index"] for f in kept["features"]] == want and kept["crs"] == geocode.CRS84
    assert s["states"] == {"dropped": 4, "whole": 9, "clipped": 1, "touching": 0} and s["survivors"] == 10 and s["detections"] == 14
    assert (s["boxes"], s["boxes_dropped"], s["partners_max"], s["device"], s["clipped_rows_keep_full_box"]) == (2, 0, 1, "cpu", 1)
    for f in kept["features"]:
        k = f["properties"].pop("index")
        state, area = f["properties"].pop("clip_state"), f["properties"].pop("clip_area")
        assert f["properties"] == full[k]["properties"]
        if state == overlaps.CLIPPED:                       # the part of a box across scene 1's eastern edge that lies beyond it
            edge = overlaps.load_boxes(csv_path)[1][0][2]
            assert table["xmin_3857"][k] < edge < table["xmax_3857"][k]
            assert f["geometry"]["type"] == "Polygon" and area == (table["xmax_3857"][k] - edge) * (table["ymax_3857"][k] - table["ymin_3857"][k])
            xs = [p[0] for p in f["geometry"]["coordinates"][0]]
            full_xs = [p[0] for p in full[k]["geometry"]["coordinates"][0]]
            assert max(xs) == max(full_xs) and min(xs) == float(geocode.mercator_to_lonlat(np.float64(edge), np.float64(0.0))[0])
            assert [p[1] for p in f["geometry"]["coordinates"][0]] == [p[1] for p in full[k]["geometry"]["coordinates"][0]]
        else:
            assert state == overlaps.WHOLE and f["geometry"] == full[k]["geometry"]
    reg = json.load(open(out / overlaps.REGIONS_FILE))
    assert reg["crs"]["properties"]["name"] == "urn:ogc:def:crs:EPSG::3857" and [f["properties"]["bbox_ind"] for f in reg["features"]] == [1, 3]
    ids, boxes = overlaps.load_boxes(csv_path)
    west, east = boxes[0], boxes[1]
    assert reg["features"][1]["geometry"]["coordinates"] == [[[west[2], east[1]], [east[2], east[1]], [east[2], east[3]], [west[2], east[3]], [west[2], east[1]]]]


def test_survivor_mask_reaches_the_facility_step(tmp_path):
    from aquaculture_amd import facilities, geocode, overlaps
    labels, csv_path = overlap_run(tmp_path)
    table = geocode.geocode_label_dir(labels, csv_path)
    dd = overlaps.dedup_from_table(table, csv_path, str(tmp_path / "out"), cpu=True)
    keep = dd["keep"]
    assert keep.dtype == bool and keep.shape == table["image"].shape and keep.sum() == 10
    args = dict(by="pass", conf_thresh=0.5, eps=25.0, min_cages=5, labels_fn=facilities.dbscan_numpy)
    twice = facilities.cluster(table, **args)
    once = facilities.cluster(table, keep=keep, **args)
    # the three cages of the overlap count six times without the mask: a facility of six; with it they are three, too few
    assert sorted(len(c) for c in twice["cage_ids"]) == [5, 6] and [len(c) for c in once["cage_ids"]] == [5]
    assert once["cage_ids"][0] in twice["cage_ids"]


def test_labels_go_through_the_same_clip(tmp_path):
    from aquaculture_amd import geocode, overlaps
    labels, csv_path = overlap_run(tmp_path)
    table = geocode.geocode_label_dir(labels, csv_path)
    stems = [str(v) for v in table["stems"]]
    truth = {"image": np.asarray([stems[int(k)] + ".jpeg" for k in table["image"]], object), "cls": table["cls"], "year": table["year"],
             **{c: table[c] for c in overlaps.BOX_COLUMNS}}
    keep = overlaps.truth_rows(truth, csv_path, cpu=True)
    assert keep.tolist() == overlaps.dedup_from_table(table, csv_path, str(tmp_path / "o"), cpu=True)["keep"].tolist()
    cut = overlaps.filter_truth(truth, csv_path, cpu=True)
    assert cut.keys() == truth.keys() and all(np.array_equal(cut[c], np.asarray(truth[c])[keep]) for c in truth)
    assert overlaps.filter_truth(truth, None) is truth
    truth["image"][2] = "elsewhere/ORTHOIMAGERY.ORTHOPHOTOS2015_9_0_0.jpeg"
    with pytest.raises(KeyError, match="ORTHOPHOTOS2015_9_0_0.jpeg.*bbox_ind 9"):
        overlaps.truth_rows(truth, csv_path, cpu=True)


def test_evaluate_leaves_out_the_labels_of_an_overlap(tmp_path):
    """--evaluate with the flag: the labels go through the clip before the grid.  The labels are the detections' own boxes."""
    from aquaculture_amd import evaluate, geocode, overlaps
    labels, csv_path = overlap_run(tmp_path)
    table = geocode.geocode_label_dir(labels, csv_path)
    stems = [str(v) for v in table["stems"]]
    feats = []
    for k in range(table["image"].shape[0]):
        x0, y0, x1, y1 = (float(table[c][k]) for c in overlaps.BOX_COLUMNS)
        feats.append({"type": "Feature", "properties": {"type": "square_cage" if table["cls"][k] else "circle_cage", "year": int(table["year"][k]),
                                                        "image": stems[int(table["image"][k])] + ".jpeg"},
                      "geometry": {"type": "Polygon", "coordinates": [[[x0, y0], [x1, y0], [x1, y1], [x0, y1], [x0, y0]]]}})
    truth = tmp_path / "humanlabels.geojson"
    truth.write_text(json.dumps({"type": "FeatureCollection", "features": feats}))
    keep = overlaps.dedup_from_table(table, csv_path, str(tmp_path / "o"), cpu=True)["keep"]
    grids = (np.asarray([0.6]), np.asarray([25.0]), np.asarray([1]))
    plain = evaluate.evaluate_table(table, str(truth), str(tmp_path / "a"), *grids, cpu=True)
    both = evaluate.evaluate_table(table, str(truth), str(tmp_path / "b"), *grids, keep=keep, cpu=True, dedup_overlaps=csv_path)
    assert (plain["n_detections"], plain["n_labels"]) == (14, 14) and (both["n_detections"], both["n_labels"]) == (10, 10)


def test_model_errors_leave_out_the_labels_of_an_overlap(tmp_path):
    """--model-errors with the flag, on the hand-built case of tests/test_model_errors.py: an earlier box covers the first label."""
    from test_model_errors import hand_built
    from aquaculture_amd import model_errors
    table, truth_path = hand_built(tmp_path, conf_of=(0.6, 0.6))
    x, y = 1.0e6, 5.2e6
    csv_path = tmp_path / "wanted_bboxes.csv"
    with open(csv_path, "w") as f:
        f.write(",geometry\n")
        for ind, (a, b, c, d) in ((1, (x - 100, y - 100, x + 25, y + 100)), (3, (x - 50, y - 50, x + 1000, y + 1000))):
            f.write(f'{ind},"POLYGON (({c!r} {b!r}, {c!r} {d!r}, {a!r} {d!r}, {a!r} {b!r}, {c!r} {b!r}))"\n')
    plain = model_errors.model_errors_from_table(table, truth_path, str(tmp_path / "a"), 0.5, cpu=True)
    cut = model_errors.model_errors_from_table(table, truth_path, str(tmp_path / "b"), 0.5, cpu=True, dedup_overlaps=str(csv_path))
    assert (plain["n_labels"], plain["n_matched"]) == (4, 2) and (cut["n_labels"], cut["n_matched"]) == (3, 0)


def test_detect_py_options():
    from aquaculture_amd import detect
    with pytest.raises(SystemExit):
        detect.parse_opt(["--dedup-overlaps"])
    with pytest.raises(ValueError, match="--dedup-overlaps needs --geocode-bboxes"):
        detect.run("w.pt", "src", dedup_overlaps="")
    assert detect.parse_opt(["--geocode-bboxes", "wb.csv"]).dedup_overlaps is None
    assert detect.parse_opt(["--dedup-overlaps", "--geocode-bboxes", "wb.csv"]).dedup_overlaps == ""
    assert detect.parse_opt(["--dedup-overlaps", "out", "--geocode-bboxes", "wb.csv"]).dedup_overlaps == "out"


def test_symbols_are_declared_exported_and_bound(lib):
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_overlap_partners_f64", "aq_overlap_clip_f64"):
        assert "int " + name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert ("overlaps.hip", ["-ffp-contract=off"]) in build.SOURCES
