"""--land-filter on the host: the numpy restatement of the box-against-land test against hand-written flags, against the definition written
as a double loop and against matplotlib's Path.intersects_bbox; the GeoJSON loader, the ocean file, the band table and facilities' `keep`.
The cases and their expected bytes are shared with tests/test_gpu_land_filter.py."""
import functools
import json
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
OX, OY = 5.0e5, 5.4e6                                       # EPSG:3857 coordinates of the French Mediterranean coast are of this size


def ring_segments(ring):
    r = np.asarray(ring, np.float64)
    if not np.array_equal(r[0], r[-1]):
        r = np.concatenate([r, r[:1]], 0)
    return np.concatenate([r[:-1], r[1:]], 1)


def square(x0, y0, x1, y1, ccw=True):
    r = [(x0, y0), (x1, y0), (x1, y1), (x0, y1)]
    return r if ccw else r[::-1]


def named_land():
    """A 100 m square with a 20 m square hole (ring directions differ), a second part 100 m east of it and a sliver 0.2 m thick."""
    rings = [square(0, 0, 100, 100), square(40, 40, 60, 60, ccw=False), square(200, 0, 220, 20, ccw=False),
             [(300, 50), (400, 50), (400, 50.2), (300, 50.2)]]
    return np.concatenate([ring_segments(np.asarray(r, np.float64) + [OX, OY]) for r in rings], 0)


NAMED = {  # name: (box relative to (OX, OY), expected byte: bit 0 an edge meets the box, bit 1 the corner (x0, y0) is on land)
    "wholly_on_land": ((10, 10, 20, 20), 2),
    "wholly_in_the_hole": ((45, 45, 55, 55), 0),
    "across_the_outer_edge_corner_at_sea": ((-5, 10, 5, 20), 1),
    "across_the_outer_edge_corner_on_land": ((95, 10, 105, 20), 3),
    "across_the_hole_edge_corner_on_land": ((35, 45, 45, 55), 3),
    "across_the_hole_edge_corner_in_the_hole": ((55, 45, 65, 55), 1),
    "at_sea_east": ((120, 50, 130, 60), 0),
    "at_sea_west_ray_through_land_and_hole": ((-30, 50, -20, 60), 0),
    "at_sea_corner_level_with_the_bottom_edges": ((-10, 0, -5, 5), 0),
    "contains_a_whole_part": ((190, -10, 230, 30), 1),
    "crossed_by_the_sliver": ((340, 40, 350, 60), 1),
    "no_area_on_land": ((30, 30, 30, 30), 2),
    "no_area_at_sea": ((150, 50, 150, 50), 0),
    "above_all_bands": ((10, 150, 20, 160), 0),
    "below_all_bands": ((10, -50, 20, -40), 0),
}


def named_boxes():
    return np.asarray([NAMED[k][0] for k in sorted(NAMED)], np.float64) + [OX, OY, OX, OY]


def named_expected():
    return np.asarray([NAMED[k][1] for k in sorted(NAMED)], np.uint8)


# exact touches: a 4 x 4 square at the origin, integer coordinates, every product and difference exact in fp64
TOUCH_LAND = ring_segments(square(0, 0, 4, 4))
TOUCH = {
    "shares_an_edge_east": ((4, 1, 6, 3), 1),
    "shares_an_edge_west": ((-2, 1, 0, 3), 1),
    "shares_a_corner_north_east": ((4, 4, 6, 6), 1),
    "shares_a_corner_south_west": ((-2, -2, 0, 0), 1),
    "one_unit_east": ((5, 1, 7, 3), 0),
    "one_unit_north_east": ((5, 5, 7, 7), 0),
    "one_unit_south_west": ((-3, -3, -1, -1), 0),
    "inside_touching_nothing": ((1, 1, 3, 3), 2),
}


def touch_boxes():
    return np.asarray([TOUCH[k][0] for k in sorted(TOUCH)], np.float64)


def touch_expected():
    return np.asarray([TOUCH[k][1] for k in sorted(TOUCH)], np.uint8)


def star_polygon(n=400, radius=2000.0, seed=7):
    """n vertices at equal angles around (OX, OY), radii between 0.55 and 1 of `radius`: a simple polygon without holes -> [n, 2]."""
    r = np.random.default_rng(seed)
    a = np.arange(n) * (2 * np.pi / n)
    rad = radius * (0.55 + 0.45 * r.random(n))
    return np.stack([OX + rad * np.cos(a), OY + rad * np.sin(a)], 1)


@functools.lru_cache(maxsize=None)
def random_case():
    """(boxes [4000, 4], segs [400, 4], star vertices): half of the boxes centred within some 30 m of a point of the coastline, half uniform
    over the square around the star; edges of 5 to 60 m.  Computed once and shared; treat as read-only."""
    star = star_polygon()
    segs = ring_segments(star)
    r = np.random.default_rng(11)
    k = r.integers(0, segs.shape[0], 2000)
    t = r.random(2000)[:, None]
    near = segs[k, :2] * (1 - t) + segs[k, 2:] * t + r.normal(0, 30.0, (2000, 2))
    far = np.asarray([OX, OY]) + r.uniform(-2400, 2400, (2000, 2))
    c = np.concatenate([near, far])[r.permutation(4000)]
    half = r.uniform(2.5, 30.0, (4000, 2))
    return np.concatenate([c - half, c + half], 1), segs, star


def orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def flags_by_definition(boxes, segs):
    """The rule set as a plain double loop over Python floats (IEEE doubles, each operation rounded once)."""
    out = np.zeros(len(boxes), np.uint8)
    segs = [tuple(float(v) for v in s) for s in segs]
    for i, (x0, y0, x1, y1) in enumerate(tuple(float(v) for v in b) for b in boxes):
        hit, crossings = False, 0
        for ax, ay, bx, by in segs:
            if (ay <= y0) != (by <= y0):
                o = orient(ax, ay, bx, by, x0, y0)
                if (o > 0) if ay <= y0 else (o < 0):
                    crossings += 1
            if hit or min(ax, bx) > x1 or max(ax, bx) < x0 or min(ay, by) > y1 or max(ay, by) < y0:
                continue
            o = [orient(ax, ay, bx, by, cx, cy) for cx, cy in ((x0, y0), (x1, y0), (x1, y1), (x0, y1))]
            hit = not (all(v > 0 for v in o) or all(v < 0 for v in o))
        out[i] = int(hit) | ((crossings & 1) << 1)
    return out


def no_near_ties(boxes, segs, rel=1e-6):
    """True if no orientation determinant of a (segment, box corner) pair with overlapping bounding boxes, and none of the crossing rule, is
    within rel |b - a| (box diagonal) of zero: the decisions are then the same in exact arithmetic and in any reasonable rounding."""
    boxes, segs = np.asarray(boxes, np.float64), np.asarray(segs, np.float64)
    ax, ay, bx, by = (segs[None, :, k] for k in range(4))
    x0, y0, x1, y1 = (boxes[:, k, None] for k in range(4))
    scale = rel * np.hypot(bx - ax, by - ay) * np.hypot(x1 - x0, y1 - y0)
    near = (np.minimum(ax, bx) <= x1) & (np.maximum(ax, bx) >= x0) & (np.minimum(ay, by) <= y1) & (np.maximum(ay, by) >= y0)
    ok = True
    for cx, cy in ((x0, y0), (x1, y0), (x1, y1), (x0, y1)):
        ok = ok and not (near & (np.abs(orient(ax, ay, bx, by, cx, cy)) <= scale)).any()
    level = (np.minimum(ay, by) <= y0) & (np.maximum(ay, by) >= y0)          # the crossing rule looks at these, whatever their x
    return ok and not (level & (np.abs(orient(ax, ay, bx, by, x0, y0)) <= scale)).any() and not (segs[None, :, 1::2] == y0[..., None]).any()


# ---- land_flags_numpy ----

def test_named_cases_both_bits():
    from aquaculture_amd import land
    got = land.land_flags_numpy(named_boxes(), named_land())
    assert got.dtype == np.uint8 and got.tolist() == named_expected().tolist(), dict(zip(sorted(NAMED), got.tolist()))
    assert set(named_expected().tolist()) == {0, 1, 2, 3}
    # the sliver's box: no vertex of the land inside it, none of its corners on land -- only the edge test can see it
    x0, y0, x1, y1 = NAMED["crossed_by_the_sliver"][0]
    v = named_land()[:, :2] - [OX, OY]
    assert not ((v[:, 0] >= x0) & (v[:, 0] <= x1) & (v[:, 1] >= y0) & (v[:, 1] <= y1)).any()
    corners = np.asarray([(x, y, x, y) for x in (x0, x1) for y in (y0, y1)], np.float64) + [OX, OY, OX, OY]
    assert land.land_flags_numpy(corners, named_land()).tolist() == [0, 0, 0, 0]
    # chunking changes nothing; no boxes and no land
    assert land.land_flags_numpy(named_boxes(), named_land(), chunk_pairs=1).tolist() == named_expected().tolist()
    assert land.land_flags_numpy(np.zeros((0, 4)), named_land()).shape == (0,)
    assert land.land_flags_numpy(named_boxes(), np.zeros((0, 4))).tolist() == [0] * len(NAMED)
    assert flags_by_definition(named_boxes(), named_land()).tolist() == named_expected().tolist()


def test_exact_touches_count_as_on_land():
    from aquaculture_amd import land
    got = land.land_flags_numpy(touch_boxes(), TOUCH_LAND)
    assert got.tolist() == touch_expected().tolist(), dict(zip(sorted(TOUCH), got.tolist()))
    assert flags_by_definition(touch_boxes(), TOUCH_LAND).tolist() == touch_expected().tolist()
    # a segment of no length is a point: in the box (its border included) or not
    point = np.asarray([[4.0, 4.0, 4.0, 4.0]])
    assert land.land_flags_numpy(np.asarray([[4.0, 4, 6, 6], [2.0, 2, 5, 5], [5.0, 5, 7, 7]]), point).tolist() == [1, 1, 0]


def test_random_case_against_the_definition_and_matplotlib():
    from matplotlib.path import Path
    from matplotlib.transforms import Bbox
    from aquaculture_amd import land
    boxes, segs, star = random_case()
    assert boxes.shape == (4000, 4) and segs.shape == (400, 4)
    assert no_near_ties(boxes, segs), "the case has a determinant too close to zero for an exact comparison"
    got = land.land_flags_numpy(boxes, segs)
    on_land = got != 0
    print(f"\n{int(on_land.sum())} boxes on land, {int((~on_land).sum())} not; bytes 0..3: {np.bincount(got, minlength=4).tolist()}")
    assert on_land.sum() >= 500 and (~on_land).sum() >= 500
    assert (np.bincount(got, minlength=4) >= 100).all()                       # every byte value occurs, often
    want = flags_by_definition(boxes, segs)
    assert np.array_equal(got, want), np.nonzero(got != want)[0][:10]
    path = Path(np.concatenate([star, star[:1]], 0), closed=True)
    mpl = np.asarray([path.intersects_bbox(Bbox([[b[0], b[1]], [b[2], b[3]]]), filled=True) for b in boxes])
    assert np.array_equal(on_land, mpl), np.nonzero(on_land != mpl)[0][:10]


# ---- the band table (torch on the CPU) ----

def comb_case():
    """One segment across the whole height, 300 short ones: (0, 0) -> (0, 3000), then a saw down the east side -> (segs [301, 4], boxes)."""
    k = np.arange(1, 300)
    teeth = np.stack([50.0 + 20.0 * (k % 2), 3000.0 - 10.0 * k], 1)
    segs = ring_segments(np.concatenate([[[0.0, 0.0], [0.0, 3000.0]], teeth]) + [OX, OY])
    r = np.random.default_rng(3)
    c = np.asarray([OX, OY]) + np.stack([r.uniform(-40, 110, 600), r.uniform(-60, 3060, 600)], 1)
    half = r.uniform(1.0, 12.0, (600, 2))
    return segs, np.concatenate([c - half, c + half], 1)


def test_band_table_on_the_host():
    import torch
    from aquaculture_amd import engine
    segs, _ = comb_case()
    assert segs.shape == (301, 4)
    t = torch.from_numpy(segs)
    for bh in (None, 7.3, 3000.0 / 4095.5, 1e4):
        entry_seg, band_start, nbands, Y0, h = engine.land_band_table(t, bh)
        assert entry_seg.dtype == torch.int32 and band_start.dtype == torch.int32 and band_start.shape == (nbands + 1,)
        assert Y0 == OY and (bh is None or h == bh)
        es, bs = entry_seg.numpy(), band_start.numpy()
        assert bs[0] == 0 and bs[-1] == es.shape[0] and (np.diff(bs) >= 0).all()
        band_of_entry = np.repeat(np.arange(nbands), np.diff(bs))
        lo = np.floor((np.minimum(segs[:, 1], segs[:, 3]) - Y0) / h)
        hi = np.floor((np.maximum(segs[:, 1], segs[:, 3]) - Y0) / h)
        assert hi.max() == nbands - 1 and lo.min() == 0                     # nobody is clamped
        assert es.shape[0] == int((hi - lo + 1).sum())
        for s in (0, 1, 150, 300):                                           # the long one is in every band, a short one in its own
            assert band_of_entry[es == s].tolist() == list(range(int(lo[s]), int(hi[s]) + 1))
        assert (es == 0).sum() == nbands
        if bh is None:
            assert es.shape[0] <= 8 * 301 + nbands and nbands in (301 // 8, 301 // 8 + 1)      # 3000 / (3000 / 37) rounds to 37 or just below
    assert engine.land_band_table(t, 1e4)[2] == 1 and engine.land_band_table(t, 3000.0 / 4095.5)[2] == 4096
    # the default gives way to long segments: 400 segments that each span the whole height
    tall = torch.tensor([[float(k), 0.0, float(k) + 0.5, 1000.0] for k in range(400)], dtype=torch.float64)
    es, bs, nb, _, h = engine.land_band_table(tall)
    assert es.shape[0] <= 8 * 400 + nb and h > 1000.0 / 50
    flat = torch.tensor([[0.0, 5.0, 3.0, 5.0], [3.0, 5.0, 9.0, 5.0]], dtype=torch.float64)
    assert engine.land_band_table(flat)[2:] == (1, 5.0, 1.0)
    with pytest.raises(ValueError, match=r"\d{13} band entries"):            # the long segment alone: 3000 m / 1e-9 m
        engine.land_band_table(t, 1e-9)
    with pytest.raises(ValueError, match="band height"):
        engine.land_band_table(t, 0.0)
    with pytest.raises(ValueError, match="not finite"):
        engine.land_band_table(torch.tensor([[0.0, float("nan"), 1.0, 1.0]], dtype=torch.float64))


# ---- the land file ----

def lonlat_ring(ring_m):
    from aquaculture_amd import geocode
    lon, lat = geocode.mercator_to_lonlat(np.asarray(ring_m, np.float64)[:, 0], np.asarray(ring_m, np.float64)[:, 1])
    return [[float(a), float(b)] for a, b in zip(lon, lat)]


def test_loader_reads_every_geometry_type(tmp_path):
    from aquaculture_amd import geocode, land
    closed = lambda r: r + r[:1]
    outer = np.asarray(closed(square(0, 0, 100, 100)), np.float64) + [OX, OY]
    hole = np.asarray(closed(square(40, 40, 60, 60, ccw=False)), np.float64) + [OX, OY]
    part = np.asarray(square(200, 0, 220, 20), np.float64) + [OX, OY]         # left open
    poly = {"type": "Polygon", "coordinates": [lonlat_ring(outer), lonlat_ring(hole)]}
    multi = {"type": "MultiPolygon", "coordinates": [[lonlat_ring(outer), lonlat_ring(hole)], [lonlat_ring(part)]]}
    docs = {"polygon": (poly, 8), "multipolygon": (multi, 12),
            "feature": ({"type": "Feature", "properties": {}, "geometry": poly}, 8),
            "collection": ({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {}, "geometry": poly},
                                                                      {"type": "Feature", "properties": {}, "geometry": None},
                                                                      {"type": "Feature", "properties": {}, "geometry": {"type": "Polygon", "coordinates": [lonlat_ring(part)]}}]}, 12),
            "geometries": ({"type": "GeometryCollection", "geometries": [multi, {"type": "Point", "coordinates": [3.0, 43.0]}]}, 12)}
    segs = {}
    for name, (doc, edges) in docs.items():
        p = tmp_path / f"{name}.geojson"
        p.write_text(json.dumps(doc))
        segs[name] = land.load_land_geojson(str(p))
        assert segs[name].dtype == np.float64 and segs[name].shape == (edges, 4), name
    assert np.array_equal(segs["multipolygon"], segs["collection"]) and np.array_equal(segs["multipolygon"], segs["geometries"])
    assert np.array_equal(segs["polygon"], segs["feature"]) and np.array_equal(segs["polygon"], segs["multipolygon"][:8])
    # the hole's edges are there, and the open ring was closed: its last edge returns to its first vertex
    m = segs["multipolygon"]
    assert np.abs(m[:4] - ring_segments(outer)).max() < 1e-6 and np.abs(m[4:8] - ring_segments(hole)).max() < 1e-6
    assert np.array_equal(m[11, 2:], m[8, :2]) and np.abs(m[8:] - ring_segments(part)).max() < 1e-6
    # the loaded land does what the named land does (the first three rings of it)
    assert land.land_flags_numpy(named_boxes(), m).tolist() == land.land_flags_numpy(named_boxes(), named_land()[:12]).tolist()
    # without crs (and with CRS84, EPSG:4326) = the same file projected beforehand and tagged EPSG:3857, to 1e-6 m
    x, y = geocode.lonlat_to_mercator(np.asarray(lonlat_ring(outer))[:, 0], np.asarray(lonlat_ring(outer))[:, 1])
    pre = {"type": "Polygon", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}},
           "coordinates": [[[float(a), float(b)] for a, b in zip(x, y)]]}
    (tmp_path / "pre.geojson").write_text(json.dumps(pre))
    got = land.load_land_geojson(str(tmp_path / "pre.geojson"))
    assert got.shape == (4, 4) and np.abs(got - segs["polygon"][:4]).max() < 1e-6
    assert np.array_equal(got, np.concatenate([np.stack([x, y], 1)[:-1], np.stack([x, y], 1)[1:]], 1))      # EPSG:3857 is taken as it is
    for name in ("urn:ogc:def:crs:OGC:1.3:CRS84", "urn:ogc:def:crs:EPSG::4326"):
        (tmp_path / "tagged.geojson").write_text(json.dumps(dict(poly, crs={"type": "name", "properties": {"name": name}})))
        assert np.array_equal(land.load_land_geojson(str(tmp_path / "tagged.geojson")), segs["polygon"])
    (tmp_path / "lambert.geojson").write_text(json.dumps(dict(poly, crs={"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::2154"}})))
    with pytest.raises(ValueError, match="EPSG::2154"):
        land.load_land_geojson(str(tmp_path / "lambert.geojson"))
    (tmp_path / "what.geojson").write_text(json.dumps({"type": "Topology"}))
    with pytest.raises(ValueError, match="Topology"):
        land.load_land_geojson(str(tmp_path / "what.geojson"))
    (tmp_path / "none.geojson").write_text(json.dumps({"type": "FeatureCollection", "features": []}))
    assert land.load_land_geojson(str(tmp_path / "none.geojson")).shape == (0, 4)


# ---- the ocean file, facilities' keep, the command line ----

def label_run(tmp_path):
    """A label directory of a dozen files in one scene, its bounds table and a land file that covers the scene's western third and an
    islet: (labels dir, csv path, land path).  Scene 3 is 1843.2 m wide in EPSG:3857; tile (1024 i, 1024 j) holds detections on a diagonal."""
    from aquaculture_amd import geocode
    labels = tmp_path / "labels"
    labels.mkdir()
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    x1, y1 = x0 + 1843.2, y0 + 1843.2
    csv_path = tmp_path / "wanted_bboxes.csv"
    csv_path.write_text(f',geometry\n3,"POLYGON (({x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}, {x1!r} {y0!r}))"\n')
    for i in range(4):
        for j in range(3):
            rows = "".join(f"{(i + j + k) % 2} {0.1 + 0.2 * k:g} {0.15 + 0.17 * k:g} 0.02 0.03 {0.5 + 0.1 * k:g}\n" for k in range(1 + (i + 2 * j) % 5))
            (labels / f"ORTHOIMAGERY.ORTHOPHOTOS{2015 - j % 2}_3_{1024 * i}_{1024 * j}.txt").write_text(rows)
    west = [(x0 - 50, y0 - 50), (x0 + 600, y0 - 50), (x0 + 700, y1 + 50), (x0 - 50, y1 + 50)]
    islet = [(x0 + 1200, y0 + 900), (x0 + 1300, y0 + 900), (x0 + 1250, y0 + 1100)]
    land_path = tmp_path / "land.geojson"
    land_path.write_text(json.dumps({"type": "FeatureCollection", "features": [
        {"type": "Feature", "properties": {}, "geometry": {"type": "MultiPolygon", "coordinates": [[lonlat_ring(west)], [lonlat_ring(islet)]]}}]}))
    return str(labels), str(csv_path), str(land_path)


def test_ocean_file_is_the_kept_features_with_their_row_numbers(tmp_path):
    from aquaculture_amd import geocode, land
    labels, csv_path, land_path = label_run(tmp_path)
    det = str(tmp_path / "detections.geojson")
    table = geocode.geocode_label_dir(labels, csv_path, det)
    n = table["image"].shape[0]
    keep = land.ocean_rows(table, land.load_land_geojson(land_path), cpu=True)
    assert keep.dtype == bool and keep.shape == (n,) and 5 <= keep.sum() <= n - 5
    # the western third is land: a detection is kept iff its box lies east of the slanted edge or off the islet; spot checks by position
    assert not keep[table["xmax_3857"] < table["xmin_3857"].min() + 550].any() and keep[(table["xmin_3857"] > table["xmin_3857"].min() + 750) & (table["xmax_3857"] < table["xmin_3857"].min() + 1100)].all()
    out = str(tmp_path / "ocean_detections.geojson")
    assert land.write_ocean_geojson(out, table["stems"], table, keep) == int(keep.sum())
    full, ocean = json.load(open(det)), json.load(open(out))
    assert ocean["crs"] == full["crs"] and ocean["type"] == "FeatureCollection"
    rows = np.nonzero(keep)[0].tolist()
    assert [f["properties"]["index"] for f in ocean["features"]] == rows
    for f in ocean["features"]:
        del f["properties"]["index"]
    assert ocean["features"] == [full["features"][k] for k in rows]
    with pytest.raises(ValueError, match="keep"):
        land.write_ocean_geojson(out, table["stems"], table, keep[:-1])
    # the command line, without a GPU: the same file
    cli = str(tmp_path / "cli.geojson")
    assert land.main(["--labels", labels, "--geocode-bboxes", csv_path, "--land", land_path, "--out", cli, "--cpu"]) == 0
    assert open(cli).read() == open(out).read()


def test_detections_geojson_is_byte_for_byte_what_it_was(tmp_path):
    """write_geojson now shares its feature builder with the ocean file: the bytes of a feature are pinned here."""
    from aquaculture_amd import geocode
    t = {"image": np.array([0]), "xmin": np.array([1]), "xmax": np.array([2]), "ymin": np.array([3]), "ymax": np.array([4]),
         "lon_min": np.array([3.5]), "lon_max": np.array([3.75]), "lat_min": np.array([43.0]), "lat_max": np.array([43.25]),
         "e_min_3035": np.array([1.5]), "e_max_3035": np.array([2.5]), "n_min_3035": np.array([0.5]), "n_max_3035": np.array([0.75]),
         "cls": np.array([1]), "year": np.array([2015]), "det_conf": np.array([0.5])}
    geocode.write_geojson(str(tmp_path / "d.geojson"), ["a_3_0_0"], t)
    assert open(tmp_path / "d.geojson").read() == (
        '{"type": "FeatureCollection", "crs": {"type": "name", "properties": {"name": "urn:ogc:def:crs:OGC:1.3:CRS84"}}, "features": '
        '[{"type": "Feature", "properties": {"image": "a_3_0_0.jpeg", "xmin": 1, "xmax": 2, "ymin": 3, "ymax": 4, "e_min_3035": 1.5, '
        '"e_max_3035": 2.5, "n_min_3035": 0.5, "n_max_3035": 0.75, "type": "square_farm", "year": 2015, "det_conf": 0.5}, "geometry": '
        '{"type": "Polygon", "coordinates": [[[3.75, 43.0], [3.75, 43.25], [3.5, 43.25], [3.5, 43.0], [3.75, 43.0]]]}}]}')


def test_facilities_keep_removes_a_facility_and_leaves_the_row_numbers(tmp_path):
    from test_facilities import FIVE, LATER, ROW6, hand_table
    from aquaculture_amd import facilities
    t = hand_table()
    n = t["det_conf"].shape[0]
    base = facilities.cluster(t, labels_fn=facilities.dbscan_numpy)
    same = facilities.cluster(t, labels_fn=facilities.dbscan_numpy, keep=None)
    every = facilities.cluster(t, labels_fn=facilities.dbscan_numpy, keep=np.ones(n, bool))
    for other in (same, every):
        assert other.keys() == base.keys()
        for k in base:
            if k.startswith("_"):
                continue
            assert other[k] == base[k], k
        assert np.array_equal(other["_members"], base["_members"])
    assert base["cage_ids"] == [ROW6, FIVE, LATER]
    keep = np.ones(n, bool)
    keep[FIVE] = False                                      # the second facility's cages are on land
    fac = facilities.cluster(t, labels_fn=facilities.dbscan_numpy, keep=keep)
    assert fac["cage_ids"] == [ROW6, LATER] and fac["facility_index"] == [0, 1] and fac["year"] == [2015, 2014]
    assert fac["_members"].tolist() == [0, 0, 0, -1, 0, 0, 0] + [-1] * 5 + [-1] * 5 + [1] * 5 and fac["_members"].shape == (n,)
    assert fac["noise_points"] == [2, 0]                    # the two strays of 2015 still count; the five on land do not
    for c in facilities.AREA_COLUMNS:
        assert fac[c][0] == base[c][0] and fac[c][1] == base[c][2]
    # keep is ANDed with the confidence test: keeping detection 3 (0.49) does not bring it in; dropping one cage of five dissolves them
    keep = np.ones(n, bool)
    keep[LATER[0]] = False
    assert facilities.cluster(t, labels_fn=facilities.dbscan_numpy, keep=keep)["cage_ids"] == [ROW6, FIVE]
    with pytest.raises(ValueError, match="keep"):
        facilities.cluster(t, labels_fn=facilities.dbscan_numpy, keep=np.ones(n - 1, bool))
    # the files: identical without keep, and the member detections' index stays the row number with it
    a, b = str(tmp_path / "a.geojson"), str(tmp_path / "b.geojson")
    facilities.facilities_from_table(t, a, cpu=True)
    facilities.facilities_from_table(t, b, cpu=True, keep=None)
    assert open(a).read() == open(b).read()
    assert open(facilities.detections_path(a)).read() == open(facilities.detections_path(b)).read()
    keep = np.ones(n, bool)
    keep[FIVE] = False
    facilities.facilities_from_table(t, b, cpu=True, keep=keep)
    assert [f["properties"]["index"] for f in json.load(open(facilities.detections_path(b)))["features"]] == ROW6 + LATER


def test_detect_py_options():
    from aquaculture_amd import detect
    with pytest.raises(SystemExit):
        detect.parse_opt(["--land-filter", "land.geojson"])
    with pytest.raises(ValueError, match="--land-filter .*needs --geocode-bboxes"):
        detect.run("w.pt", "src", land_filter="land.geojson")
    opt = detect.parse_opt(["--land-filter", "land.geojson", "--geocode-bboxes", "wb.csv"])
    assert (opt.land_filter, opt.ocean_out) == ("land.geojson", None)
    assert detect.parse_opt(["--geocode-bboxes", "wb.csv"]).land_filter is None
    assert detect.parse_opt(["--land-filter", "l.geojson", "--ocean-out", "o.geojson", "--geocode-bboxes", "wb.csv"]).ocean_out == "o.geojson"


def test_symbols_are_declared_exported_and_bound(lib):
    import ctypes
    from aquaculture_amd import build, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_land_scratch_bytes", "aq_land_filter_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert lib.aq_land_scratch_bytes.restype is ctypes.c_size_t
    assert lib.aq_land_scratch_bytes(0) == 0 and lib.aq_land_scratch_bytes(1 << 31) == 0 and lib.aq_land_scratch_bytes(1000) == 32000
    assert ("land_filter.hip", ["-ffp-contract=off"]) in build.SOURCES
