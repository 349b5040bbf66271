"""--tonnage-missing / --tonnage-near-sites on the CPU: the box-against-coverage predicate (missing.first_numpy through the band tables,
missing.first_bruteforce without them) on hand cases, against dedup.literal_mask on frames whose metre map is exact, and on real tile
coordinates; the imputation against the reference's loops as they stand; the simulation and the files through ``--cpu``."""
import functools
import json

import numpy as np
import pytest

from test_dedup import COMPLETE_STATS, PARTLY_STATS, STEM, ring_of, synthetic_sweep, write_geom, write_key

from aquaculture_amd import blank as aqblank, blank_geom as bg, dedup as dd, facilities, geocode, missing as ms, tonnage as tn

GOLDEN_BBOXES = __file__.rsplit("/", 1)[0] + "/golden/g14_wanted_bboxes.csv"
EXACT = {3: (0.0, 0.0, 6144.0, 6144.0)}                    # one metre per pixel: tile (0, 0) is x in [0, 1024], y = 6144 - py
NORTH = 6144.0


def stem(year, ind=3, xo=0, yo=0):
    return f"ORTHOIMAGERY.ORTHOPHOTOS{year}_{ind}_{xo}_{yo}"


def make_reg(images, wanted=EXACT):
    """images: [(stem, None for a complete image or its pixel ring)]."""
    rows = [{"image": s + ".jpeg", "image_status": aqblank.COMPLETE if r is None else aqblank.PARTLY_BLANK} for s, r in images]
    return ms.regions(rows, {s: r for s, r in images if r is not None}, wanted)


def px_box(x0, py0, x1, py1, scale=1.0, north=NORTH):
    """A box given in pixel coordinates (y down) of tile (0, 0) -> metres (x0, y0, x1, y1)."""
    return (x0 * scale, north - py1 * scale, x1 * scale, north - py0 * scale)


def both(reg, boxes, qpass, nbands=(None, 1, 3)):
    """first_bruteforce's answer, which first_numpy has to give for every band count."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    want = ms.first_bruteforce(reg, boxes, qpass)
    for nb in nbands:
        got = ms.first_numpy(reg, ms.band_tables(reg, nb), boxes, qpass)
        assert got.dtype == np.int32 and (got == want).all(), (nb, got.tolist(), want.tolist())
    return want.tolist()


def mask_ring(fill):
    m = np.zeros((1024, 1024), bool)
    fill(m)
    return ring_of(m)[0]


def _l_shape(m):
    m[0:100, 0:100] = True
    m[0:50, 50:100] = False


def _diagonal(m):
    m[10, 10] = m[11, 11] = True


def _big(m):
    m[0:1000, 0:1000] = True


def _small(m):
    m[500:510, 500:510] = True


@functools.lru_cache(None)
def hand_cases():
    """[(name, reg, boxes [n, 4], qpass [n], expected first [n])]; the GPU suite runs the same list."""
    out = []
    L = make_reg([(stem(2014), mask_ring(_l_shape))])
    boxes = [px_box(60, 10, 90, 40),                        # in the notch: the bounding boxes overlap, no segment meets it, the corner is outside
             px_box(100, 100, 110, 110),                    # touches the ring at the corner point (100, 100)
             px_box(100, 60, 110, 80),                      # touches along the edge x = 100
             px_box(50, 40, 60, 50),                        # in the notch, touching its two edges
             px_box(100, 100, 100, 100),                    # no size, on a vertex
             px_box(50, 50, 50, 50),                        # no size, on the inner vertex
             px_box(100.5, 100.5, 110, 110),                # half a pixel off the corner
             px_box(10, 60, 20, 70),                        # inside, away from every segment: the parity decides
             px_box(-50, -50, 0, 0),                        # touches the frame's corner, which is the ring's
             (np.nan, 5000.0, 10.0, 6000.0), (0.0, 5000.0, 10.0, np.nan)]
    out.append(("l_shape", L, boxes, [0] * len(boxes), [-1, 0, 0, 0, 0, 0, -1, 0, 0, -1, -1]))
    B = make_reg([(stem(2014), mask_ring(_big))])
    boxes = [px_box(500, 500, 501, 501), px_box(500, 500, 500, 500), px_box(999.5, 999.5, 1010, 1010), px_box(1000.5, 0, 1010, 10), px_box(-10, -10, 2000, 2000)]
    out.append(("far_inside", B, boxes, [0] * len(boxes), [0, 0, 0, -1, 0]))
    S = make_reg([(stem(2014), mask_ring(_small))])
    boxes = [px_box(400, 400, 600, 600), px_box(400, 400, 499.5, 600), px_box(510, 510, 520, 520), px_box(505, 505, 505, 505)]
    out.append(("box_contains_ring", S, boxes, [0] * len(boxes), [0, -1, 0, 0]))
    D = make_reg([(stem(2014), mask_ring(_diagonal))])
    boxes = [px_box(10.25, 10.25, 10.75, 10.75), px_box(11.25, 11.25, 11.75, 11.75), px_box(11.25, 10.25, 11.75, 10.75), px_box(10.25, 11.25, 10.75, 11.75),
             px_box(11, 11, 11, 11), px_box(11.5, 10.5, 11.5, 10.5), px_box(11.25, 10.25, 12, 11)]
    out.append(("self_touching", D, boxes, [0] * len(boxes), [0, 0, -1, -1, 0, -1, 0]))
    # two images of one pass over each other: a parity over all rings together would call the inside uncovered
    R2 = make_reg([(stem(2014), None), (stem(2015), None), (stem(2017), None)])
    boxes = [px_box(10, 10, 20, 20), px_box(1024, 0, 1030, 10), px_box(1024.5, 0, 1030, 10)]
    out.append(("two_rectangles", R2, boxes + boxes, [0] * 3 + [1] * 3, [0, 0, -1, 2, 2, -1]))
    G2 = make_reg([(stem(2014), mask_ring(_big)), (stem(2015), mask_ring(_big))])
    assert sum(ring_crossings(G2, k, px_box(500, 500, 501, 501)) for k in range(2)) % 2 == 0
    out.append(("two_rings", G2, [px_box(500, 500, 501, 501), px_box(1001, 0, 1002, 1)], [0, 0], [0, -1]))
    # a pass without images: an id outside the table, and the name of a pass make_first does not know
    out.append(("no_such_pass", L, [px_box(10, 60, 20, 70)] * 3, [-1, 1, 7], [-1, -1, -1]))
    # a neighbouring complete tile that shares exactly one edge with the box
    N = make_reg([(stem(2014, xo=1024), None), (stem(2014, yo=1024), mask_ring(_big))])
    boxes = [px_box(1000, 10, 1024, 20), px_box(1000, 10, 1023.5, 20), px_box(2048, 10, 2050, 20), px_box(2048.5, 10, 2050, 20),
             px_box(10, 1020, 20, 1024), px_box(10, 1020, 20, 1023.5), px_box(1000, 1024, 1024, 1030), px_box(1000.5, 2024, 1024, 2030)]
    assert N["names"] == [stem(2014, yo=1024), stem(2014, xo=1024)]       # sorted by name: the ring image is number 0
    out.append(("shared_edge", N, boxes, [0] * len(boxes), [1, -1, 1, -1, 0, -1, 0, -1]))
    return out


def ring_crossings(reg, i, box):
    a = reg["xy"][reg["ring_start"][i]:reg["ring_start"][i + 1]]
    return int((((a[:-1, 1] <= box[1]) != (a[1:, 1] <= box[1])) & (a[:-1, 0] > box[0])).sum())


@pytest.mark.parametrize("k", range(8))
def test_hand_cases(k):
    name, reg, boxes, qpass, want = hand_cases()[k]
    assert both(reg, boxes, qpass) == want, name


def test_hand_case_tables():
    assert len(hand_cases()) == 8
    reg = hand_cases()[0][1]
    assert reg["passes"] == ["2013-2015"] and reg["kind"].tolist() == [ms.KIND_RING] and reg["rect"].tolist() == [[0.0, 5120.0, 1024.0, 6144.0]]
    ring = mask_ring(_l_shape)
    assert reg["xy"].tolist() == [list(v) for v in bg.to_bounds(ring, 0.0, 5120.0, 1024.0, 6144.0)] and reg["ring_start"].tolist() == [0, len(ring)]
    two = hand_cases()[4][1]
    assert two["passes"] == ["2013-2015", "2016-2018"] and two["pass_start"].tolist() == [0, 2, 3] and two["names"] == [stem(2014), stem(2015), stem(2017)]
    assert two["xy"].shape == (0, 2) and two["ring_start"].tolist() == [0, 0, 0, 0]
    fn = ms.make_first(reg, "numpy")
    assert fn([px_box(10, 60, 20, 70)] * 2, ["2013-2015", "2000-2004"]).tolist() == [0, -1]
    # what takes part: blank images, partly blank ones without a ring, names that are no tiles and scenes the table does not list do not
    rows = [{"image": stem(2014) + ".jpeg", "image_status": aqblank.BLANK}, {"image": stem(2015) + ".jpeg", "image_status": aqblank.PARTLY_BLANK},
            {"image": "scene.jpeg", "image_status": aqblank.COMPLETE}, {"image": stem(2016, ind=4) + ".jpeg", "image_status": aqblank.COMPLETE},
            {"image": stem(2011) + ".jpeg", "image_status": aqblank.COMPLETE}]
    assert ms.regions(rows, {}, EXACT)["names"] == [stem(2011)]
    empty = ms.regions([], {}, EXACT)
    assert empty["passes"] == [] and both(empty, [px_box(0, 0, 1, 1)], [0]) == [-1]


# ---- against the pixels ----

def blob_ring(rng, cells):
    """The outer ring of the largest component of a random cells x cells pattern blown up to 1024 x 1024."""
    coarse = rng.random((cells, cells)) < 0.55
    return ring_of(np.kron(coarse, np.ones((1024 // cells, 1024 // cells), bool)))[0]


@functools.lru_cache(None)
def literal_case(seed=5):
    """Six blob images (one per pass) on two exact frames and boxes on multiples of half a pixel around the rings' vertices -> (reg, boxes,
    qpass, closed [n]: the closed box meets a closed pixel square of the mask, kind [n]: 0 disjoint, 1 touching, 2 overlapping, 3 inside)."""
    rng = np.random.default_rng(seed)
    years, scales = (2002, 2007, 2011, 2014, 2017, 2020), (1.0, 0.25, 1.0, 0.25, 1.0, 1.0)
    images, boxes, qpass, closed, kind = [], [], [], [], []
    for k, (year, scale) in enumerate(zip(years, scales)):
        ring = blob_ring(rng, (8, 16, 32, 64, 8, 128)[k])
        images.append((stem(year, ind=10 + k), ring))
        mask = dd.literal_mask(ring, 1024, 1024)
        v = np.asarray(ring, np.float64)
        for j in range(170):
            cx, cy = v[int(rng.integers(0, v.shape[0]))] + rng.integers(-6, 7, 2) * 0.5 if j % 5 else rng.integers(0, 2049, 2) * 0.5
            w, h = (rng.integers(0, 9, 2) * 0.5) if j % 3 else (rng.integers(0, 3, 2) * 0.5)
            x0, x1, py0, py1 = cx - w, cx + w, cy - h, cy + h
            boxes.append(px_box(x0, py0, x1, py1, scale, 6144.0 * scale))
            qpass.append(k)
            c0, c1, r0, r1 = max(int(np.ceil(x0 - 1)), 0), min(int(np.floor(x1)), 1023), max(int(np.ceil(py0 - 1)), 0), min(int(np.floor(py1)), 1023)
            near = bool(mask[r0:r1 + 1, c0:c1 + 1].any()) if c0 <= c1 and r0 <= r1 else False
            o = mask[max(int(np.floor(py0)), 0):min(int(np.ceil(py1)), 1024), max(int(np.floor(x0)), 0):min(int(np.ceil(x1)), 1024)]
            whole = 0 <= x0 and x1 <= 1024 and 0 <= py0 and py1 <= 1024 and o.size > 0
            closed.append(near)
            kind.append(0 if not near else 1 if not o.any() else 3 if whole and o.all() else 2)
    wanted = {10 + k: (0.0, 0.0, 6144.0 * s, 6144.0 * s) for k, s in enumerate(scales)}
    return make_reg(images, wanted), np.asarray(boxes), np.asarray(qpass, np.int32), np.asarray(closed), np.asarray(kind)


def test_literal_pixels():
    reg, boxes, qpass, closed, kind = literal_case()
    assert reg["passes"] == [facilities.image_pass(y) for y in (2002, 2007, 2011, 2014, 2017, 2020)] and (reg["kind"] == ms.KIND_RING).all()
    counts = np.bincount(kind, minlength=4)
    assert (counts >= 20).all(), counts.tolist()           # disjoint, touching without overlap, overlapping, wholly inside
    got = ms.first_numpy(reg, ms.band_tables(reg), boxes, qpass)
    assert ((got >= 0) == closed).all(), np.nonzero((got >= 0) != closed)[0].tolist()
    assert (got[got >= 0] == qpass[got >= 0]).all()         # one image per pass: the image's number is the pass's
    assert (ms.first_bruteforce(reg, boxes, qpass) == got).all()
    assert (ms.first_numpy(reg, ms.band_tables(reg, 1), boxes, qpass) == got).all()


# ---- real coordinates: bands against no bands ----

@functools.lru_cache(None)
def tiles_case(seed=11):
    """Every tile of the two download boxes of the golden table and of a third one laid over both, in two passes, a few of them with blob
    rings; boxes on and beside the tiles' shared edges."""
    rng = np.random.default_rng(seed)
    wanted = dict(geocode.load_wanted_bboxes(GOLDEN_BBOXES))
    a = wanted[1956]
    wanted[9001] = (a[0] + 600.0, a[1] - 600.0, a[2] + 600.0, a[3] - 600.0)
    images = []
    for ind in sorted(wanted):
        for xo in range(0, 6144, 1024):
            for yo in range(0, 6144, 1024):
                year = 2014 if (xo + yo) % 2048 == 0 else 2017 if ind != 9001 else 2015
                images.append((stem(year, ind, xo, yo), blob_ring(rng, 8) if rng.random() < 0.15 else None))
    reg = make_reg(images, wanted)
    boxes, qpass = [], []
    for i in rng.permutation(reg["rect"].shape[0])[:24].tolist():
        w, s, e, n = reg["rect"][i].tolist()
        for x, y in ((w, s), (e, n), (w, n), (e, (s + n) / 2), ((w + e) / 2, s)):
            for dx, dy in ((0.0, 0.0), (1e-9, 0.0), (0.0, -1e-9), (np.spacing(x), np.spacing(y)), (-np.spacing(x), -np.spacing(y))):
                for size in (0.0, 3.0):
                    boxes.append((x + dx, y + dy, x + dx + size, y + dy + size))
                    boxes.append((x + dx - size, y + dy - size, x + dx, y + dy))
                    qpass += [int(reg["pass_id"][i]), 1 - int(reg["pass_id"][i])]
    lo, hi = reg["rect"][:, 1].min(), reg["rect"][:, 3].max()
    boxes += [(656000.0, lo - 500.0, 656010.0, hi + 500.0), (656000.0, hi + 1.0, 656010.0, hi + 50.0), (656000.0, lo - 50.0, 656010.0, lo - 1.0),
              (656000.0, -np.inf, 656010.0, np.inf), (656000.0, hi, 656010.0, np.inf)]
    qpass += [0, 0, 0, 1, 1]
    return reg, np.asarray(boxes), np.asarray(qpass, np.int32)


def test_bands_change_nothing():
    reg, boxes, qpass = tiles_case()
    assert reg["passes"] == ["2013-2015", "2016-2018"] and reg["rect"].shape[0] == 108 and 5 < int(reg["kind"].sum()) < 40
    assert reg["rect"][:, 1].min() > 5.3e6
    want = ms.first_bruteforce(reg, boxes, qpass)
    assert (want >= 0).sum() > 100 and (want < 0).sum() > 100
    for nb in (1, 2, 7, 64, 1000, None):
        t = ms.band_tables(reg, nb)
        assert t["band_start"].shape == (2 * t["nbands"] + 1,) and t["band_start"][-1] == t["entry_img"].shape[0] >= 108
        assert (ms.first_numpy(reg, t, boxes, qpass) == want).all(), nb
    assert ms.band_tables(reg)["nbands"] == max(1, int(np.diff(reg["pass_start"]).max()) // 8) > 1
    with pytest.raises(ValueError):
        ms.band_tables(reg, 0)


# ---- the procedure ----

def outline(x_px):
    """The ring of an image whose left x_px columns are not blank."""
    return [(0, 0), (x_px, 0), (x_px, 1024), (0, 1024), (0, 0)]


def sweep(tmp_path, ring_2014=outline(158), status_2017=COMPLETE_STATS):
    """Three passes on one tile: six cages in a row at y = 500 in every year (pixel columns 99-109, 112-122, 124-134, 135-145, 147-157 and
    160-170), six more at y = 800 in 2011.  The 2014 image is partly blank (columns 0 .. 158 remain, so its own facility has five cages);
    2017's is complete (or what status_2017 says)."""
    row = lambda px, py: f"0 {px / 1024:g} {py / 1024:g} {10 / 1024:g} {10 / 1024:g} 0.9\n"
    labels, csv_path = synthetic_sweep(tmp_path, (2011, 2014, 2017), {2011: [row(105 + 12 * k, 800) for k in range(6)]})
    key = write_key(tmp_path / "key.csv", [(STEM.format(2011), COMPLETE_STATS), (STEM.format(2014), PARTLY_STATS), (STEM.format(2017), status_2017)])
    geom = write_geom(tmp_path / "geom.geojson", {STEM.format(2014): ring_2014})
    table = geocode.geocode_label_dir(labels, csv_path)
    res = dd.dedup_from_table(table, key, geom, None, cpu=True)
    fac = dd.cluster(table, res, labels_fn=facilities.dbscan_numpy)
    reg = ms.regions(dd.read_blank_key(key), dd.read_blank_geom(geom), geocode.load_wanted_bboxes(csv_path))
    return {"labels": labels, "bboxes": csv_path, "key": key, "geom": geom, "table": table, "fac": fac, "reg": reg}


MAP = {"2013-2015": "2010-2012", "2016-2018": "2010-2012", "2019-2021": "2010-2012", "2010-2012": "2013-2015"}


def check_against_literal(fac, table, reg, cmap):
    imp = ms.impute(fac, table, ms.make_first(reg, "numpy"), cmap)
    lit = ms.impute_literal(fac, table, ms.make_first(reg, "bruteforce"), cmap)
    for p in cmap:
        mine = [k for k in range(len(imp["pass"])) if imp["pass"][k] == p]
        own, added = [k for k in mine if imp["own"][k]], [k for k in mine if not imp["own"][k]]
        assert mine == own + added and mine == list(range(mine[0], mine[0] + len(mine))) if mine else True
        theirs_own = [k for k in range(lit[p]["total"]) if lit[p]["from_pass"][k] == p]
        theirs_added = [k for k in range(lit[p]["total"]) if lit[p]["from_pass"][k] != p]
        assert imp["counts"][p] == (len(own), len(added)) == (lit[p]["total"] - lit[p]["added"], lit[p]["added"])
        for a, b in ((own, theirs_own), (added, theirs_added)):
            assert [imp["facility_index"][k] for k in a] == [lit[p]["facility_index"][k] for k in b]
            assert [imp["from_pass"][k] for k in a] == [lit[p]["from_pass"][k] for k in b]
            for col in ms.CAGE_COLUMNS:
                assert [imp[col][k] for k in a] == [lit[p][col][k] for k in b], (p, col)
    assert [p for p in imp["pass"]] == sorted(imp["pass"])
    return imp, lit


def test_impute_is_the_reference_procedure(tmp_path):
    s = sweep(tmp_path)
    fac, table, reg = s["fac"], s["table"], s["reg"]
    assert sorted(zip(fac["pass"], map(len, fac["cage_ids"]))) == [("2010-2012", 6), ("2010-2012", 6), ("2013-2015", 5), ("2016-2018", 6)]
    assert reg["passes"] == ["2010-2012", "2013-2015", "2016-2018"] and reg["kind"].tolist() == [0, 1, 0]
    imp, lit = check_against_literal(fac, table, reg, MAP)
    # 2014 sees columns 0 .. 158: of both facilities of 2011 the cage at 160 is added, the others are covered (157 | 158: one is beside it)
    xmin = np.asarray(table["xmin"])
    assert imp["counts"] == {"2010-2012": (2, 0), "2013-2015": (1, 2), "2016-2018": (1, 0), "2019-2021": (0, 2)}
    for k in [k for k in range(len(imp["pass"])) if imp["pass"][k] == "2013-2015" and not imp["own"][k]]:
        assert xmin[imp["cage_ids"][k]].tolist() == [160] and imp["from_pass"][k] == "2010-2012"
    # 2019-2021 has no image at all: everything of the compare pass is added, as it is
    last = [k for k in range(len(imp["pass"])) if imp["pass"][k] == "2019-2021"]
    assert [imp["cage_ids"][k] for k in last] == [fac["cage_ids"][f] for f in range(4) if fac["pass"][f] == "2010-2012"]
    # complete images cover everything: nothing of 2011 is added to 2016-2018, nothing of 2014 to 2010-2012
    assert [a["kept"] for a in imp["added"] if a["to_pass"] == "2010-2012"] == [False]
    assert [a["kept"] for a in imp["added"] if a["to_pass"] == "2016-2018"] == [False, False]
    q = imp["queries"]
    assert list(zip(q["cage"], q["target"])) == sorted(set(zip(q["cage"], q["target"]))) and len(q["cage"]) == 12 * 3 + 5
    assert set(q["first"][[t == "2019-2021" for t in q["target"]]].tolist()) == {-1}
    # a facility whose cage_ids_min empties while cage_ids does not is dropped; one whose cage_ids empties while cage_ids_min does not stays
    f = [k for k in range(4) if fac["pass"][k] == "2010-2012"]
    fac2 = {k: (list(v) if isinstance(v, list) else v) for k, v in fac.items()}
    fac2["cage_ids_min"] = [list(v) for v in fac["cage_ids_min"]]
    fac2["cage_ids"] = [list(v) for v in fac["cage_ids"]]
    fac2["cage_ids_min"][f[0]] = [c for c in fac["cage_ids"][f[0]] if xmin[c] <= 147]
    fac2["cage_ids"][f[1]] = [c for c in fac["cage_ids"][f[1]] if xmin[c] <= 147]
    imp2, _ = check_against_literal(fac2, table, reg, MAP)
    rec = {(a["facility_index"], a["to_pass"]): a for a in imp2["added"]}
    a0, a1 = rec[(fac["facility_index"][f[0]], "2013-2015")], rec[(fac["facility_index"][f[1]], "2013-2015")]
    assert not a0["kept"] and a0["before"] == [6, 6, 5] and a0["after"] == [1, 1, 0] and a0["position"] == -1
    assert a1["kept"] and a1["before"] == [5, 6, 6] and a1["after"] == [0, 1, 1] and imp2["cage_ids"][a1["position"]] == []
    assert imp2["counts"]["2013-2015"] == (1, 1)
    with pytest.raises(ValueError, match="itself"):
        ms.impute(fac, table, ms.make_first(reg, "numpy"), {"2013-2015": "2013-2015"})


def test_map_option():
    assert ms.parse_map(None) == ms.parse_map("") == ms.DEFAULT_MAP and len(ms.DEFAULT_MAP) == 6 and ms.DEFAULT_MAP["2016-2018"] == "2010-2012"
    assert ms.parse_map("2013-2015=2010-2012, 2016-2018=2013-2015") == {"2013-2015": "2010-2012", "2016-2018": "2013-2015"}
    for bad in ("2013-2015", "a=a", "a=b,a=c", "=b", "a=b,"):
        with pytest.raises(ValueError):
            ms.parse_map(bad)


# ---- the simulation and the files ----

FACTORS = "pass,s_mean,s_sd,h_mean,h_sd\n2000-2004,9,3,0.8,0.1\n2005-2009,10,3,0.9,0.1\n2010-2012,11,3,0.8,0.1\n2013-2015,12,3,0.8,0.1\n2016-2018,13,3,0.7,0.1\n2019-2021,12,2,0.8,0.1\n"


def run_cli(s, tmp_path, name, *more, cpu=True):
    out = tmp_path / name
    argv = ["--labels", s["labels"], "--geocode-bboxes", s["bboxes"], "--tonnage-factors", str(tmp_path / "factors.csv"), "--tonnage-K", "64",
            "--tonnage-seed", "7", "--out", str(out), *(["--cpu"] if cpu else []), *more]
    assert tn.main(argv) == 0
    return out


def sites_csv(tmp_path, table):
    """One site whose box ends half a pixel before column 135 of the tile (the cages at 99, 112 and 124 meet it), and one far away."""
    k = int(np.nonzero(np.asarray(table["xmin"]) == 135)[0][0])
    x, y = float(table["xmin_3857"][k]) - 0.15 - 1000.0, float(table["ymin_3857"][k])
    lon, lat = geocode.mercator_to_lonlat(np.float64(x), np.float64(y))
    path = tmp_path / "sites.csv"
    path.write_text(f"id,lat,lon\n1,{float(lat)!r},{float(lon)!r}\n2,10.0,10.0\n")
    return str(path)


def test_files_through_the_command_line(tmp_path):
    s = sweep(tmp_path)
    (tmp_path / "factors.csv").write_text(FACTORS)
    dedup = ["--dedup-years", s["key"], s["geom"]]
    plain = run_cli(s, tmp_path, "plain", *dedup)
    sites = sites_csv(tmp_path, s["table"])
    full = run_cli(s, tmp_path, "full", *dedup, "--tonnage-missing", "--tonnage-near-sites", sites)
    a, b = (open(d / tn.ESTIMATES_FILE).read().splitlines() for d in (plain, full))
    assert b[:len(a)] == a and len(a) == 4 and all(r.startswith("Model,") for r in a[1:])
    for name in (tn.FACILITIES_FILE, dd.CAGES_FILE, dd.TILES_FILE, dd.JSON_FILE):
        assert open(plain / name, "rb").read() == open(full / name, "rb").read()
    doc, doc0 = json.load(open(full / tn.JSON_FILE)), json.load(open(plain / tn.JSON_FILE))
    assert {k: v for k, v in doc.items() if k not in ("missing", "near_sites")} == doc0 and "missing" not in doc0 and "near_sites" not in doc0
    assert not [f.name for f in plain.iterdir() if f.name in (ms.CAGES_FILE, ms.FACILITIES_FILE, ms.NEAR_FILE)]
    # the rows: the hand-built facility table through tonnage.estimate
    fac, table = s["fac"], s["table"]
    xmin = np.asarray(table["xmin"])
    of = lambda p: [f for f in range(4) if fac["pass"][f] == p]
    cut = lambda f: {col: [c for c in fac[col][f] if xmin[c] >= 160] for col in ms.CAGE_COLUMNS}
    asis = lambda f: {col: list(fac[col][f]) for col in ms.CAGE_COLUMNS}
    # the default map: 2005-2009 and 2019-2021 have no image, so 2010-2012's facilities are added as they are; 2010-2012 would take from
    # 2005-2009, which has none; 2017's complete image covers everything of 2010-2012; 2000-2004 has nothing at all and gets no row
    rows = [("2005-2009", f, asis(f)) for f in of("2010-2012")] + [("2010-2012", f, asis(f)) for f in of("2010-2012")] + \
           [("2013-2015", f, asis(f)) for f in of("2013-2015")] + [("2013-2015", f, cut(f)) for f in of("2010-2012")] + \
           [("2016-2018", f, asis(f)) for f in of("2016-2018")] + [("2019-2021", f, asis(f)) for f in of("2010-2012")]
    hand = {"facility_index": [fac["facility_index"][f] for _, f, _ in rows], "pass": [p for p, _, _ in rows], "_areas": fac["_areas"],
            **{col: [lists[col] for _, _, lists in rows] for col in ms.CAGE_COLUMNS}}
    est = tn.estimate(hand, None, table, tn.read_factors(str(tmp_path / "factors.csv")), K=64, seed=7, cpu=True)
    assert b[len(a):] == [f"Model + Estimate missing,{p},{m!r},{sd!r}" for p, m, sd in zip(est["pass"], est["tonnage"], est["tonnage_sd"])]
    assert est["pass"] == ["2005-2009", "2010-2012", "2013-2015", "2016-2018", "2019-2021"] and [r.split(",")[1] for r in a[1:]] == est["pass"][1:4]
    model = {r.split(",")[1]: float(r.split(",")[2]) for r in a[1:]}
    filled = {r.split(",")[1]: float(r.split(",")[2]) for r in b[len(a):]}
    assert filled["2013-2015"] > model["2013-2015"] and filled["2016-2018"] != model["2016-2018"] and filled["2005-2009"] > 0 and filled["2019-2021"] > 0
    assert doc["missing"]["map"] == ms.DEFAULT_MAP
    assert doc["missing"]["passes"]["2013-2015"] == {"compare": "2010-2012", "own": 1, "added": 2, "images": 1, "ring_vertices": 5}
    assert doc["missing"]["passes"]["2019-2021"] == {"compare": "2010-2012", "own": 0, "added": 2, "images": 0, "ring_vertices": 0}
    assert doc["missing"]["passes"]["2000-2004"] == {"compare": "2005-2009", "own": 0, "added": 0, "images": 0, "ring_vertices": 0}
    cages = open(full / ms.CAGES_FILE).read().splitlines()
    assert cages[0] == "row,image,pass,target_pass,first_image,kept" and len(cages) == 1 + 12 * 4
    k136 = int(np.nonzero((xmin == 160) & (np.asarray(table["year"]) == 2011))[0][0])
    assert f"{k136},{STEM.format(2011)}.jpeg,2010-2012,2013-2015,,1" in cages and f"{k136},{STEM.format(2011)}.jpeg,2010-2012,2016-2018,{STEM.format(2017)}.jpeg,0" in cages
    facs = open(full / ms.FACILITIES_FILE).read().splitlines()
    assert facs[0] == "facility_index,from_pass,to_pass,cage_ids_before,cage_ids_after,cage_ids_max_before,cage_ids_max_after,cage_ids_min_before,cage_ids_min_after,kept,tonnage,tonnage_sd"
    kept = [r.split(",") for r in facs[1:] if r.split(",")[9] == "1"]
    assert len(facs) == 1 + 2 * 4 and len(kept) == 6 and all(float(r[10]) > 0 for r in kept) and all(r.endswith(",0,,") for r in facs[1:] if r.split(",")[9] == "0")
    assert [r[3:9] for r in kept if r[2] == "2013-2015"] == [["6", "1"] * 3] * 2
    assert not [f.name for f in full.iterdir() if f.name.endswith(".tmp")]
    # near the sites: three cages of each of the four facilities lie in the first site's box
    near = open(full / ms.NEAR_FILE).read().splitlines()
    assert near[0] == "pass,tonnage,tonnage_sd,facilities,cages"
    assert [(r.split(",")[0], r.split(",")[3], r.split(",")[4]) for r in near[1:]] == [("2010-2012", "2", "6"), ("2013-2015", "1", "3"), ("2016-2018", "1", "3")]
    from aquaculture_amd import kfold
    cutn = ms.near(fac, table, "bruteforce", kfold.load_known_sites(sites))
    assert all(sorted(xmin[ids].tolist()) == [99, 112, 124] for ids in cutn["cage_ids"]) and cutn["pass"] == fac["pass"]
    est_n = tn.estimate(cutn, None, table, tn.read_factors(str(tmp_path / "factors.csv")), K=64, seed=7, cpu=True)
    assert [r.split(",")[1] for r in near[1:]] == [repr(v) for v in est_n["tonnage"]]
    assert doc["near_sites"] == {"sites": 2, "facilities": 4}
    # near the sites alone needs no --dedup-years; an explicit map; the file says which passes got a row
    only = run_cli(s, tmp_path, "only", "--tonnage-near-sites", sites)
    assert open(only / ms.NEAR_FILE).read().splitlines()[0] == near[0] and len(open(only / tn.ESTIMATES_FILE).read().splitlines()) == 4
    one = run_cli(s, tmp_path, "one", *dedup, "--tonnage-missing", "2016-2018=2013-2015")
    assert [r.split(",")[:2] for r in open(one / tn.ESTIMATES_FILE).read().splitlines()[4:]] == [["Model + Estimate missing", "2016-2018"]]


def test_refusals(tmp_path):
    from aquaculture_amd import detect
    base = ["--geocode-bboxes", "wb.csv", "--tonnage-factors", "f.csv"]
    opt = detect.parse_opt([*base, "--tonnage", "--dedup-years", "--tonnage-missing", "--tonnage-near-sites", "s.csv"])
    assert opt.tonnage_missing == "" and opt.tonnage_near_sites == "s.csv"
    assert detect.parse_opt([*base, "--tonnage", "--dedup-years", "--tonnage-missing", "2013-2015=2010-2012"]).tonnage_missing == "2013-2015=2010-2012"
    assert detect.parse_opt(base).tonnage_missing is None and detect.parse_opt(base).tonnage_near_sites is None
    for argv in ([*base, "--tonnage", "--tonnage-missing"], [*base, "--dedup-years", "--tonnage-missing"], [*base, "--tonnage-near-sites", "s.csv"],
                 [*base, "--tonnage", "--dedup-years", "--tonnage-missing", "a=a"]):
        with pytest.raises(SystemExit):
            detect.parse_opt(argv)
    with pytest.raises(ValueError, match="needs both"):
        detect.run("w.pt", "src", geocode_bboxes="wb.csv", tonnage="", tonnage_factors="f.csv", tonnage_missing="")
    with pytest.raises(ValueError, match="needs both"):
        detect.run("w.pt", "src", geocode_bboxes="wb.csv", dedup_years="", tonnage_missing="")
    with pytest.raises(ValueError, match="needs --tonnage"):
        detect.run("w.pt", "src", geocode_bboxes="wb.csv", tonnage_near_sites="s.csv")
    assert "--dedup-years" in detect.MISSING_NEEDS_TONNAGE_DEDUP and "--tonnage" in detect.NEAR_SITES_NEED_TONNAGE
    with pytest.raises(SystemExit):
        tn.main(["--labels", "l", "--geocode-bboxes", "wb.csv", "--tonnage-factors", "f.csv", "--tonnage-missing"])
    with pytest.raises(ValueError, match="needs --dedup-years"):
        tn.tonnage_from_table({}, str(tmp_path), "f.csv", missing={"map": {}})


def test_build_and_exports():
    from aquaculture_amd import build, engine
    assert ("coverage.hip", ["-ffp-contract=off"]) in build.SOURCES and "aq_coverage_first_i32" in engine.EXPORTS
    header = open(__file__.rsplit("/", 2)[0] + "/include/aq_engine.h").read()
    assert "int aq_coverage_first_i32(" in header
