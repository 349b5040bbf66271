"""--blank-geom on the CPU: blank_geom.components_numpy against scipy.ndimage (labels, the outside region, the area inside the exterior
ring, the winner), the ring walk (closed, every outer edge once, shoelace area, crossing-count rasterisation), the map to the tile's bounds,
Douglas-Peucker, and the GeoJSON file (parts, merge, flags, run_params).  scipy is used here only: the package imports neither it nor
oracle/.  Everything is integer-exact."""
import json
import os

import numpy as np
import pytest
from scipy import ndimage

from aquaculture_amd import blank, blank_geom

EIGHT = np.ones((3, 3), int)


def constructed_masks():
    """(name, bool mask): the cases the kernels and the ring walk have to get right."""
    out = []
    m = np.zeros((21, 23), bool)                           # nested rings with islands
    m[1:20, 1:22] = True; m[3:18, 3:20] = False; m[5:16, 5:18] = True; m[7:14, 7:16] = False; m[9:12, 9:12] = True; m[10, 13] = True
    out.append(("nested_rings", m))
    m = np.zeros((6, 6), bool)                             # diagonal pinch points
    m[0, 0] = m[1, 1] = m[2, 2] = m[3, 1] = m[1, 3] = m[0, 4] = True
    out.append(("diagonal_chain", m))
    m = np.ones((5, 5), bool)                              # a hole that touches the outside only diagonally: still a hole
    m[0, 0] = False; m[1, 1] = False
    out.append(("hole_diagonal_to_outside", m))
    m = np.ones((7, 9), bool)                              # a hole whose corners pinch the ring from inside, and a notch from the border
    m[2, 2] = m[3, 3] = m[2, 4] = False; m[0, 6] = m[1, 6] = False
    out.append(("holes_and_notch", m))
    out.append(("all_set", np.ones((4, 7), bool)))
    out.append(("none_set", np.zeros((5, 3), bool)))
    m = np.zeros((5, 9), bool)                             # ties: two components of equal E, the first one wins
    m[1:3, 1:3] = True; m[2:4, 5:7] = True
    out.append(("tie", m))
    m = np.zeros((9, 9), bool)                             # tie between a ring (with its hole) and a solid block of the same E
    m[0:3, 0:3] = True; m[1, 1] = False; m[5:8, 4:7] = True
    out.append(("tie_ring_block", m))
    m = np.zeros((8, 8), bool)                             # a U open to the frame's top border: its inside is outside
    m[0:6, 1] = m[0:6, 5] = True; m[5, 1:6] = True; m[2, 3] = True
    out.append(("u_at_border", m))
    m = np.zeros((3, 130), bool)                           # runs across the 64-pixel pieces of a row
    m[0, 10:129] = True; m[2, 60:70] = True; m[1, 63] = True
    out.append(("across_pieces", m))
    m = np.zeros((70, 70), bool)                           # a spiral: long chains for the union-find
    for k in range(0, 34, 2):
        m[k, k:70 - k] = True; m[k:70 - k, 69 - k] = True; m[69 - k, k:70 - k] = True; m[k + 2:70 - k, k] = True
    out.append(("spiral", m))
    out.append(("one_pixel", np.ones((1, 1), bool)))
    return out


def random_masks():
    rng = np.random.Generator(np.random.PCG64(20261017))
    out = []
    for h, w in ((1, 37), (41, 1), (1, 1), (17, 19), (40, 70), (64, 64), (33, 130)):
        for density in (0.1, 0.35, 0.5, 0.65, 0.9):
            out.append((f"random_{h}x{w}_{density}", rng.random((h, w)) < density))
    for k in range(6):                                     # coarse blobs: holes, islands, nesting
        coarse = rng.random((9, 11)) < 0.55
        m = np.kron(coarse, np.ones((5, 6), bool)).astype(bool)
        m &= rng.random(m.shape) < 0.97
        out.append((f"blobs_{k}", m))
    return out


MASKS = constructed_masks() + random_masks()


def image_of(mask, seed=0):
    """A uint8 RGB image whose non-blank mask is `mask`: on the mask max(R, G, B) in [0, 249], off it in [250, 255]."""
    rng = np.random.Generator(np.random.PCG64(seed))
    h, w = mask.shape
    img = rng.integers(0, 250, (h, w, 3)).astype(np.uint8)
    off = rng.integers(0, 256, (h, w, 3)).astype(np.uint8)
    off[..., rng.integers(0, 3)] = rng.integers(250, 256, (h, w))
    img[~mask] = off[~mask]
    return img


def same_partition(a, b, on):
    """Two labellings give the same partition of the pixels `on`."""
    pairs = np.unique(np.stack([a[on], b[on]], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


@pytest.mark.parametrize("name,mask", MASKS, ids=[n for n, _ in MASKS])
def test_components_against_scipy(name, mask):
    h, w = mask.shape
    c = blank_geom.components_numpy(image_of(mask, len(name)))
    assert (c["mask"] == mask).all()
    assert (blank_geom.components_numpy(mask=mask)["record"] == c["record"]).all()
    # foreground: scipy's 8-connected partition, every label the first pixel of its component
    ref, n = ndimage.label(mask, EIGHT)
    assert ((c["fg"] == blank_geom.NOT_FG) == ~mask).all() and same_partition(c["fg"], ref, mask)
    idx = np.arange(h * w).reshape(h, w)
    for lab in np.unique(c["fg"][mask]):
        assert lab == idx[c["fg"] == lab].min()
    assert c["record"][1] == n == len(c["labels"])
    # background: the 4-connected labelling of the complement in a one-pixel border; the border's region is the outside
    pad = np.pad(~mask, 1, constant_values=True)
    bref, _ = ndimage.label(pad)
    bref_in = bref[1:-1, 1:-1]
    assert ((c["bg"] == blank_geom.NOT_BG) == mask).all() and same_partition(c["bg"], bref_in, ~mask)
    assert ((c["bg"] == blank_geom.OUTSIDE) == (~mask & (bref_in == bref[0, 0]))).all()
    for lab in np.unique(c["bg"][~mask]):
        assert lab == blank_geom.OUTSIDE or lab == idx[c["bg"] == lab].min()
    # E of the winner is the filled area; the winner is the arg max of the filled areas, ties to the smallest label
    filled = {int(lab): int(ndimage.binary_fill_holes(c["fg"] == lab).sum()) for lab in c["labels"]}
    rec = dict(zip(blank_geom.RECORD_FIELDS, c["record"].tolist()))
    if n == 0:
        assert (rec["label"], rec["px"], rec["area_px"], rec["x0"], rec["y0"], rec["x1"], rec["y1"], rec["n_edges"]) == (-1, 0, 0, w, h, -1, -1, 0)
        assert c["edges"].shape == (0, 2)
        return
    best = max(filled.values())
    assert rec["label"] == min(lab for lab, a in filled.items() if a == best) and rec["area_px"] == best
    for lab, e in zip(c["labels"].tolist(), c["areas"].tolist()):
        assert e <= filled[lab] and (e == filled[lab] or e < best)         # exact unless enclosed, and then never the maximum
    win = c["fg"] == rec["label"]
    ys, xs = np.nonzero(win)
    assert (rec["px"], rec["x0"], rec["y0"], rec["x1"], rec["y1"]) == (int(win.sum()), xs.min(), ys.min(), xs.max(), ys.max())
    assert rec["edge_px"] == c["edges"].shape[0] and rec["n_edges"] == sum(bin(s).count("1") for s in c["edges"][:, 1].tolist())
    assert (np.diff(c["edges"][:, 0]) > 0).all()


def crossing_raster(ring, h, w):
    """Pixels whose centre a ray to the right crosses the ring's vertical segments an odd number of times."""
    inside = np.zeros((h, w), bool)
    for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]):
        if x0 == x1 and y0 != y1:
            inside[min(y0, y1):max(y0, y1), :x0] ^= True
    return inside


@pytest.mark.parametrize("name,mask", MASKS, ids=[n for n, _ in MASKS])
def test_ring_of_the_winner(name, mask):
    h, w = mask.shape
    c = blank_geom.components_numpy(mask=mask)
    ring = blank_geom.ring_from_edges(c["edges"], w)
    if c["record"][1] == 0:
        assert ring == []
        return
    rng = np.random.Generator(np.random.PCG64(3))
    assert blank_geom.ring_from_edges(c["edges"][rng.permutation(len(c["edges"]))], w) == ring           # canonical
    assert ring[0] == ring[-1] and ring[0] == min(ring, key=lambda v: (v[1], v[0]))
    units = set()
    for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:]):
        assert (x0 == x1) != (y0 == y1)                                            # axis-parallel, not degenerate
        n = abs(x1 - x0) + abs(y1 - y0)
        dx, dy = (x1 - x0) // n, (y1 - y0) // n
        for k in range(n):
            e = ((x0 + k * dx, y0 + k * dy), (x0 + (k + 1) * dx, y0 + (k + 1) * dy))
            assert e not in units
            units.add(e)
    for a, b, c_ in zip(ring[:-1], ring[1:], ring[2:] + ring[1:2]):                # collinear runs are merged
        assert (b[0] - a[0]) * (c_[1] - b[1]) - (b[1] - a[1]) * (c_[0] - b[0]) != 0
    want = set()
    for i, s in c["edges"].tolist():
        y, x = divmod(i, w)
        for side, (ax, ay, bx, by) in blank_geom._STEP.items():
            if s & side:
                want.add(((x + ax, y + ay), (x + bx, y + by)))
    assert units == want and len(want) == c["record"][9]
    assert blank_geom.ring_area(ring) == c["record"][4]
    assert (crossing_raster(ring, h, w) == ndimage.binary_fill_holes(c["fg"] == c["record"][2])).all()


def test_ring_visits_a_pinch_vertex_twice_and_refuses_open_edge_sets():
    m = np.zeros((2, 2), bool)
    m[0, 0] = m[1, 1] = True
    c = blank_geom.components_numpy(mask=m)
    ring = blank_geom.ring_from_edges(c["edges"], 2)
    assert ring == [(0, 0), (1, 0), (1, 1), (2, 1), (2, 2), (1, 2), (1, 1), (0, 1), (0, 0)] and ring.count((1, 1)) == 2
    with pytest.raises(ValueError):
        blank_geom.ring_from_edges([[0, blank_geom.SIDE_N | blank_geom.SIDE_E]], 2)
    with pytest.raises(ValueError):                                               # two separate squares are not one walk
        blank_geom.ring_from_edges([[0, 15], [3, 15]], 5)


def test_to_bounds_against_hand_computed_corners():
    ring = [(0, 0), (1024, 0), (1024, 1024), (512, 256), (0, 0)]
    got = blank_geom.to_bounds(ring, 1000.0, 2000.0, 3048.0, 6096.0)
    assert got == [(1000.0, 6096.0), (3048.0, 6096.0), (3048.0, 2000.0), (2024.0, 5072.0), (1000.0, 6096.0)]
    # a 640-px image still maps with the reference's fixed 1024
    assert blank_geom.to_bounds([(640, 640)], 0.0, 0.0, 1024.0, 1024.0) == [(640.0, 384.0)]
    table = {7: (100.0, 200.0, 100.0 + 6144 * 0.5, 200.0 + 6144 * 0.25)}
    west, south, east, north = blank_geom.tile_bounds("ORTHOIMAGERY.ORTHOPHOTOS2015_7_1024_2048.jpeg", table)
    assert (west, east) == (100.0 + 1024 * 0.5, 100.0 + 2048 * 0.5)
    assert (north, south) == (200.0 + 6144 * 0.25 - 2048 * 0.25, 200.0 + 6144 * 0.25 - 3072 * 0.25)
    with pytest.raises(KeyError):
        blank_geom.tile_bounds("ORTHOIMAGERY.ORTHOPHOTOS2015_8_0_0.jpeg", table)
    with pytest.raises(ValueError):
        blank_geom.tile_bounds("tile.jpeg", table)


@pytest.mark.parametrize("tol", [0.0, 0.5, 1.0, 3.0])
def test_simplify_dp(tol):
    for name, mask in MASKS:
        c = blank_geom.components_numpy(mask=mask)
        ring = blank_geom.ring_from_edges(c["edges"], mask.shape[1])
        if not ring:
            continue
        ring = blank_geom.to_bounds(ring, 0.0, 0.0, 1024.0 * 0.7, 1024.0 * 0.7)
        got = blank_geom.simplify_dp(ring, tol)
        if tol == 0:
            assert got == ring
            continue
        assert got[0] == ring[0] and got[-1] == ring[-1] and len(got) >= 3
        at = [0]
        for p in got[1:-1]:                                                        # a subsequence of the ring
            at.append(ring.index(p, at[-1] + 1))
        at.append(len(ring) - 1)
        for i, j in zip(at[:-1], at[1:]):                                          # every dropped vertex within tol of the chord that replaces it
            for k in range(i + 1, j):
                assert blank_geom._dist(ring[k], ring[i], ring[j]) <= tol, (name, k)


def _features(names, masks, table=None, tol=0.5):
    return [blank_geom.feature_numpy(n, image_of(m, 5), table, tol) for n, m in zip(names, masks)]


def test_feature_properties_and_geometry():
    m = np.zeros((1024, 1024), bool)
    m[:, :700] = True
    name = "ORTHOIMAGERY.ORTHOPHOTOS2015_7_1024_2048.jpeg"
    f = blank_geom.feature_numpy(name, image_of(m, 1))
    assert f["properties"] == {"image": name, "year": "2015", "bbox_ind": "7", "x_offset": "1024", "y_offset": "2048", "n_components": 1,
                               "px": 700 * 1024, "area_px": 700 * 1024, "x0": 0, "y0": 0, "x1": 699, "y1": 1023,
                               "ring_px": [[0, 0], [700, 0], [700, 1024], [0, 1024], [0, 0]]}
    assert f["geometry"] == {"type": "Polygon", "coordinates": [f["properties"]["ring_px"]]}
    table = {7: (0.0, 0.0, 6144.0, 6144.0)}
    g = blank_geom.feature_numpy(name, image_of(m, 1), table, 0.5)
    assert g["geometry"]["coordinates"] == [[[1024.0, 4096.0], [1724.0, 4096.0], [1724.0, 3072.0], [1024.0, 3072.0], [1024.0, 4096.0]]]
    assert g["properties"] == f["properties"]
    assert blank_geom.feature_numpy(name, np.full((8, 8, 3), 252, np.uint8)) is None


def test_part_files_merge_and_stable_bytes(tmp_path):
    names = [f"ORTHOIMAGERY.ORTHOPHOTOS2015_{k}_0_1024.jpeg" for k in range(5)]
    masks = [mask for _, mask in MASKS[:4]] + [np.zeros((5, 3), bool)]
    feats = _features(names, masks)
    assert feats[4] is None and feats[0] is not None
    d = str(tmp_path)
    p0, p1 = blank_geom.PartFile(d, 0), blank_geom.PartFile(d, 1)
    p0.open(); p1.open()
    p1.append([3, 4], blank_geom.part_rows(names[3:], feats[3:]))
    p0.append([1], blank_geom.part_rows(names[1:2], feats[1:2]))
    p1.append([0], blank_geom.part_rows(names[0:1], feats[0:1]))
    p0.append([2], blank_geom.part_rows(names[2:3], feats[2:3]))
    p0.close(); p1.close()
    with open(blank_geom.part_path(d, 1), "ab") as f:                              # a line a crash cut short, and a repeated row
        f.write(("0," + blank_geom.part_rows(names[0:1], feats[0:1])[0] + "\n").encode() + b'7,{"image":"cut')
    out = os.path.join(d, "a.geojson")
    got = blank_geom.merge_parts(d, out, names)
    assert got == {"features": 4, "actually_blank": [names[4]]}
    doc = json.load(open(out))
    assert doc["type"] == "FeatureCollection" and "crs" not in doc
    assert doc["features"] == [f for f in feats if f is not None]
    first = open(out, "rb").read()
    assert blank_geom.merge_parts(d, out, names) == got and open(out, "rb").read() == first
    assert blank_geom.merge_parts(d, os.path.join(d, "b.geojson"), list(reversed(names)))["features"] == 4
    assert [f["properties"]["image"] for f in json.load(open(os.path.join(d, "b.geojson")))["features"]] == list(reversed(names[:4]))
    blank_geom.merge_parts(d, out, names, crs="urn:ogc:def:crs:EPSG::3857")
    assert json.load(open(out))["crs"] == {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}
    # a part opened again drops the cut line
    p1.open(); p1.close()
    assert open(blank_geom.part_path(d, 1), "rb").read().endswith(b"}\n")
    # the key's part files are other files
    assert not blank.read_parts(d)


def test_flags_and_run_params():
    from aquaculture_amd import detect
    opt = detect.parse_opt(["--weights", "w.pt", "--source", "s"])
    assert opt.blank_geom is None and opt.blank_key is None
    opt = detect.parse_opt(["--weights", "w.pt", "--source", "s", "--blank-geom"])
    assert opt.blank_geom == "" and opt.blank_key == "" and opt.blank_geom_simplify == 0.5        # the flag turns the key on
    opt = detect.parse_opt(["--weights", "w.pt", "--source", "s", "--blank-geom", "g.geojson", "--blank-key", "k.csv", "--blank-geom-simplify", "0"])
    assert (opt.blank_geom, opt.blank_key, opt.blank_geom_simplify) == ("g.geojson", "k.csv", 0.0)
    base = detect.run_params("id", 0.25, 0.45, 1000, (640, 640), "bf16", True)
    assert "blank_geom" not in base and "blank_geom" not in detect.run_params("id", 0.25, 0.45, 1000, (640, 640), "bf16", True, blank_key=True)
    with_geom = detect.run_params("id", 0.25, 0.45, 1000, (640, 640), "bf16", True, blank_key=True, blank_geom=True)
    assert with_geom == {**base, "blank_key": True, "blank_geom": True}


def test_groups_bound_the_scratch():
    from aquaculture_amd import engine
    sizes = [(1024, 1024)] * 40 + [(5000, 5000)] + [(10, 10)] * 3
    groups = engine.blank_geom_groups(sizes)
    assert [k for g in groups for k in g] == list(range(44))
    slots = engine.blank_geom_slots(sizes)
    for g in groups:
        assert slots[g].sum() <= engine.GEOM_GROUP_SLOTS or len(g) == 1
    assert (slots % 4 == 0).all() and slots[0] == 1025 * 1024 + 4
    t = engine.blank_geom_frame_table(np.arange(3) * 100, 30, [(3, 10), (1, 1), (2, 5)])
    assert t["mcu"].tolist() == [0, 36, 40]
