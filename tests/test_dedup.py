"""--dedup-years on the host: the three restated kernels (dedup.fill_numpy / sets_numpy / select_numpy) against definitions written out here
and against dedup.selections_literal, the reference's per-permutation allocation; the sweep's files; the cage_ids_min / cage_ids_max
matching; the refusals.  tests/test_gpu_dedup.py holds the kernels to the restatement byte for byte."""
import functools
import itertools
import json
import os

import numpy as np
import pytest

from aquaculture_amd import blank as aqblank, blank_geom as bg, dedup as dd, facilities, geocode, tonnage as tn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = dd.SEL_MIN | dd.SEL_MAX | dd.SEL_RANDOM
FRAMES = ((40, 24), (64, 8))                                # w + 1 = 41 and 65: rows of 2 and 3 words


# ---- drawn masks and their rings ----

def drawn_masks(w, h):
    """name -> bool [h, w]; in every one the component with the largest exterior ring is the one the name describes."""
    out = {}
    m = np.zeros((h, w), bool)                              # a blob with a hole and an island in the hole
    m[1:h - 1, 2:w - 3] = True
    m[2:h - 2, 4:w - 5] = False
    m[3:h - 3, 7:w - 9] = True
    out["hole_island"] = m
    m = np.zeros((h, w), bool)                              # two diagonal pixels joined at one vertex, across the word boundary
    m[2, 31] = m[3, 32] = True
    out["diagonal"] = m
    m = np.zeros((h, w), bool)                              # a cross that touches all four borders: toggles in the extra column x = w
    m[:, 30:34] = True
    m[h // 2 - 1:h // 2 + 1, :] = True
    out["borders"] = m
    for name, (x, y) in (("pixel_corner", (w - 1, h - 1)), ("pixel_31", (31, 0)), ("pixel_32", (32, h - 1))):
        m = np.zeros((h, w), bool)
        m[y, x] = True
        out[name] = m
    return out


def ring_of(mask):
    c = bg.components_numpy(mask=mask)
    return bg.ring_from_edges(c["edges"], mask.shape[1]), c


def even_odd(ring, w, h):
    """The definition, pixel by pixel: (c, r) is inside iff an odd number of vertical unit edges of the ring in row r lie at x <= c."""
    out = np.zeros((h, w), bool)
    for r in range(h):
        for c in range(w):
            n = 0
            for (xa, ya), (xb, yb) in zip(ring[:-1], ring[1:]):
                if xa == xb and min(ya, yb) <= r < max(ya, yb) and xa <= c:
                    n += 1
            out[r, c] = n % 2 == 1
    return out


def enclosed(c):
    """The winner's pixels and everything it encloses, from the label maps: what is not the winner and cannot reach the frame's border
    through 4-connected steps over pixels that are not the winner's is enclosed."""
    from scipy import ndimage
    winner = c["fg"] == int(c["record"][2])
    free = np.ones((winner.shape[0] + 2, winner.shape[1] + 2), bool)
    free[1:-1, 1:-1] = ~winner
    lab, _ = ndimage.label(free)
    return ~(lab == lab[0, 0])[1:-1, 1:-1]


def unpack(words, w, h):
    """bitmap words of one frame -> (bool [h, w], the bits from column w on)."""
    rows = np.asarray(words, np.uint32).reshape(h, dd.pitch_words(w))
    bits = ((rows[:, :, None] >> np.arange(32, dtype=np.uint32)[None, None, :]) & 1).reshape(h, -1).astype(bool)
    return bits[:, :w], bits[:, w:]


def fill_problem():
    """One group per drawn mask and frame (a single BITMAP slot, no cages)."""
    ws, hs, slots, masks = [], [], [], []
    for w, h in FRAMES:
        for name, m in drawn_masks(w, h).items():
            ring, c = ring_of(m)
            ws.append(w); hs.append(h); slots.append([ring]); masks.append((name, m, ring, c))
    return dd.make_problem(ws, hs, slots, [], [], np.zeros((0, 4)), []), masks


def test_fill_is_the_even_odd_fill_of_the_exterior_ring():
    p, masks = fill_problem()
    t = dd.tables(p)
    assert t["bitmap_words"] == sum(h * dd.pitch_words(w) * 6 for w, h in FRAMES) and [dd.pitch_words(w) for w, _ in FRAMES] == [2, 3]
    bitmap = dd.fill_numpy(t["ring_xy"], t["ring_start"], t["ring_frame"], t["bitmap_words"])
    assert bitmap.dtype == np.uint32
    for (name, m, ring, c), (word0, w, h, _) in zip(masks, t["ring_frame"].tolist()):
        got, extra = unpack(bitmap[word0:word0 + h * dd.pitch_words(w)], w, h)
        assert not extra.any(), name                        # a closed ring toggles every row an even number of times
        assert (got == even_odd(ring, w, h)).all(), name
        assert (got == enclosed(c)).all(), name
        assert (got == dd.literal_mask(ring, w, h)).all(), name
        assert got[m & (c["fg"] == int(c["record"][2]))].all()
    by_name = {name: (m, ring) for name, m, ring, _ in masks[:6]}
    assert by_name["hole_island"][0].sum() < even_odd(by_name["hole_island"][1], 40, 24).sum()         # the hole is filled
    assert any(v[0] == 40 for v in by_name["borders"][1]) and any(v[0] == 40 for v in by_name["pixel_corner"][1])   # x = w is toggled
    assert len(by_name["diagonal"][1]) == 9                 # one walk through the shared vertex, visited twice


# ---- windows ----

def window_problem(w, h, px, py):
    """One group, one BITMAP slot whose mask is the pixel (px, py), and cages around it -> (problem, expected survival)."""
    m = np.zeros((h, w), bool)
    m[py, px] = True
    ring, _ = ring_of(m)
    far = 4
    cases = [((px - far, px, py, py), True),                # xmax == c: touches the pixel's left edge
             ((px - far, px - 1, py, py), False),
             ((px + 1, px + far, py, py), True),            # xmin == c + 1: touches its right edge
             ((px + 2, px + far, py, py), False),
             ((px, px, py - far, py), True),                # the same in y
             ((px, px, py - far, py - 1), False),
             ((px, px, py + 1, py + far), True),
             ((px, px, py + 2, py + far), False),
             ((px + 1, px + far, py + 1, py + far), True),  # the corner alone
             ((px, px, py, py), True),
             ((-9, w + 9, -9, h + 9), True),                # the whole frame and more
             ((w + 2, w + 9, py, py), False),               # wholly outside the frame, on every side
             ((-9, -2, py, py), False), ((px, px, h + 2, h + 9), False), ((px, px, -9, -2), False),
             ((px + far, px, py, py), False)]               # an empty box
    boxes = [b for b, _ in cases]
    p = dd.make_problem([w], [h], [[ring]], [0] * len(boxes), [0] * len(boxes), boxes, [1.0] * len(boxes))
    return p, np.asarray([s for _, s in cases])


WINDOW_PIXELS = [(w, h, px, py) for w, h in FRAMES for px, py in ((31, 3), (32, 3), (0, 0), (w - 1, h - 1), (0, h - 1), (w - 1, 0))]


@pytest.mark.parametrize("w,h,px,py", WINDOW_PIXELS)
def test_windows_touching_counts(w, h, px, py):
    p, want = window_problem(w, h, px, py)
    got = dd.selections_numpy(p)["bits"]
    assert ((got == ALL) == want).all() and set(got.tolist()) <= {0, ALL}, (got, want)
    assert (dd.selections_literal(p)["bits"] == got).all()


# ---- selections by hand ----

def halves(w, h, cut=20):
    return [(0, 0), (cut, 0), (cut, h), (0, h), (0, 0)], [(cut, 0), (w, 0), (w, h), (cut, h), (cut, 0)]


LEFT, RIGHT = (5, 8, 5, 8), (30, 33, 5, 8)                  # two boxes well inside the two halves of a 40 x 24 frame


def hand_problems():
    """name -> (problem, expected bits, expected (min, max) order numbers, expected sums)."""
    w, h = 40, 24
    left, right = halves(w, h)
    R, N, X = dd.SEL_RANDOM, dd.SEL_MIN, dd.SEL_MAX
    out = {}
    # 2019 complete, 2020 partly blank (its left half): order (0, 1) keeps A and B = 17, order (1, 0) keeps C and B = 11
    two = lambda areas, **kw: dd.make_problem([w], [h], [[None, left]], [0, 0, 0, 0], [0, 0, 1, 1], [LEFT, RIGHT, LEFT, RIGHT], areas, **kw)
    out["two_years"] = (two([10.0, 7.0, 4.0, 2.0]), [X | R, N | X | R, N, 0], (1, 0), [17.0, 11.0])
    out["two_years_random_10"] = (two([10.0, 7.0, 4.0, 2.0], random_order=[[1, 0, -1, -1, -1]]), [X, N | X | R, N | R, 0], (1, 0), [17.0, 11.0])
    # all areas equal: max is the last permutation, min the first
    out["equal"] = (dd.make_problem([w], [h], [[None, left]], [0, 0], [0, 1], [LEFT, LEFT], [3.0, 3.0]), [N | R, X], (0, 1), [3.0, 3.0])
    out["nan_area"] = (two([np.nan, 7.0, 4.0, 2.0]), [N | R, N | X | R, X, 0], (0, 1), [7.0, 11.0])
    out["no_cages"] = (dd.make_problem([w], [h], [[None, left]], [], [], np.zeros((0, 4)), []), [], (0, 1), [0.0, 0.0])
    # a cage on a blank image of the tile (slot -1) and one on an image of no group at all
    out["blank_image"] = (dd.make_problem([w], [h], [[None, left]], [0, 0, -1], [0, -1, -1], [LEFT, LEFT, LEFT], [1.0, 1.0, 1.0]), [X | R, 0, 0], (1, 0), [1.0, 0.0])
    out["one_year"] = (dd.make_problem([w], [h], [[right]], [0, 0], [0, 0], [LEFT, RIGHT], [1.0, 2.0]), [0, ALL], (0, 0), [2.0])
    # three years: left half, right half, complete; the sums of the six orders worked out by hand
    three = dd.make_problem([w], [h], [[left, right, None]], [0, 0, 0, 0], [0, 1, 2, 2], [LEFT, RIGHT, LEFT, RIGHT], [5.0, 3.0, 4.0, 1.0],
                            random_order=[[1, 2, 0, -1, -1]])
    out["three_years"] = (three, [X, X | R, N | R, N], (4, 2), [8.0, 6.0, 8.0, 7.0, 5.0, 5.0])
    # five complete years with one cage each: the first year of an order takes everything
    five = dd.make_problem([w], [h], [[None] * 5], [0] * 5, range(5), [LEFT] * 5, [1.0, 2.0, 4.0, 8.0, 16.0], random_order=[[2, 0, 4, 1, 3]])
    out["five_years"] = (five, [N, 0, R, 0, X], (0, 119), [float(1 << q[0]) for q in itertools.permutations(range(5))])
    return out


@pytest.mark.parametrize("name", sorted(hand_problems()))
def test_selections_by_hand(name):
    p, bits, (qmin, qmax), sums = hand_problems()[name]
    for res in (dd.selections_numpy(p), dd.selections_literal(p)):
        assert res["bits"].tolist() == bits
        assert res["chosen"][0, :2].tolist() == [qmin, qmax] and res["chosen"][0, 3] == len(sums)
        assert res["sums"][0, :len(sums)].tolist() == sums and not res["sums"][0, len(sums):].any()
        n = int(p["n"][0])
        assert list(itertools.permutations(range(n)))[res["chosen"][0, 2]] == tuple(p["random_order"][0, :n].tolist())


def test_survival_from_the_word_is_the_literal_allocation_for_every_order():
    """Bit S of a word says a pixel of the window lies in exactly the masks of S; for every order of three overlapping masks the rule
    "some S has the cage's slot first" gives what mask_i & ~(earlier masks) gives."""
    w, h = 40, 24
    rings = [[(0, 0), (25, 0), (25, 16), (0, 16), (0, 0)], [(10, 4), (40, 4), (40, 24), (10, 24), (10, 4)], [(18, 0), (30, 0), (30, 24), (18, 24), (18, 0)]]
    boxes = [(x, x + 3, y, y + 2) for x in range(0, 38, 5) for y in range(0, 22, 4)]
    for order in itertools.permutations(range(3)):
        p = dd.make_problem([w], [h], [rings], [0] * (3 * len(boxes)), np.repeat(np.arange(3), len(boxes)), boxes * 3, np.ones(3 * len(boxes)),
                            random_order=[list(order) + [-1, -1]])
        a, b = dd.selections_numpy(p), dd.selections_literal(p)
        assert (a["bits"] == b["bits"]).all() and (a["chosen"] == b["chosen"]).all()
        assert 0 < ((a["bits"] & dd.SEL_RANDOM) != 0).sum() < a["bits"].shape[0]


# ---- the seeded random case ----

def random_ring(rng, w, h):
    """One in eight: the exterior ring of the largest component of a few random rectangles, some cut out again (None if nothing is left).
    Else, made directly: one to six columns side by side, each from its own top to its own bottom, all of them crossing one common row."""
    if rng.random() < 0.125 and w * h < 10000:
        m = np.zeros((h, w), bool)
        for k in range(int(rng.integers(1, 4)) + int(rng.integers(0, 3))):
            x0, y0 = int(rng.integers(0, w - 1)), int(rng.integers(0, h - 1))
            m[y0:int(rng.integers(y0 + 1, h + 1)), x0:int(rng.integers(x0 + 1, w + 1))] = k < 3
        return ring_of(m)[0] if m.any() else None
    xs = np.unique(rng.integers(0, w + 1, int(rng.integers(2, 8)))).tolist()
    if len(xs) < 2:
        return None
    mid = int(rng.integers(0, h))
    tops, bottoms = rng.integers(0, mid + 1, len(xs) - 1).tolist(), rng.integers(mid + 1, h + 1, len(xs) - 1).tolist()
    ring = [(xs[0], tops[0])]
    for k in range(len(xs) - 1):                            # along the tops to the right, then along the bottoms back
        ring += [(xs[k], tops[k]), (xs[k + 1], tops[k])]
    for k in range(len(xs) - 2, -1, -1):
        ring += [(xs[k + 1], bottoms[k]), (xs[k], bottoms[k])]
    ring.append(ring[0])
    return [v for k, v in enumerate(ring) if k == 0 or v != ring[k - 1]]


def random_problem(seed, G, C, w=96, h=72, big=None):
    """G groups of 1 .. 5 images on w x h frames (a third complete, the others random blobs), C cages with boxes in and around the frame,
    some on blank images, areas with repeats, a NaN and zeros; big = (group, side): that group has five blob images on side x side."""
    rng = np.random.default_rng(seed)
    ws, hs, slots, order = [w] * G, [h] * G, [], []
    for g in range(G):
        n = 1 + g % 5 if g < 5 else int(rng.integers(1, 6))
        if big is not None and g == big[0]:
            n, ws[g], hs[g] = 5, big[1], big[1]
        s = []
        for _ in range(n):
            ring = None if rng.random() < 0.33 and not (big and g == big[0]) else random_ring(rng, ws[g], hs[g])
            s.append(ring)
        slots.append(s)
        order.append(list(rng.permutation(n)) + [-1] * (5 - n))
    cg = rng.integers(0, G, C)
    if big is not None:
        cg[:C // 50] = big[0]
    n_of = np.asarray([len(s) for s in slots])
    cs = np.where(rng.random(C) < 0.05, -1, rng.integers(0, 5, C) % n_of[cg])
    cg = np.where(rng.random(C) < 0.02, -1, cg)
    cs = np.where(cg < 0, -1, cs)
    fw, fh = np.asarray(ws)[np.maximum(cg, 0)], np.asarray(hs)[np.maximum(cg, 0)]
    x, y = (rng.random(C) * (fw + 8) - 5).astype(np.int64), (rng.random(C) * (fh + 8) - 5).astype(np.int64)
    box = np.stack([x, x + rng.integers(0, 14, C), y, y + rng.integers(0, 14, C)], 1)
    area = rng.choice([1.0, 2.5, 7.25, 0.0, 13.125, np.nan, 1e-3], C)
    return dd.make_problem(ws, hs, slots, cg, cs, box, area, order)


@functools.lru_cache(maxsize=None)
def random_case():
    p = random_problem(20260, 300, 3000)
    return p, dd.selections_numpy(p), dd.selections_literal(p)


def test_random_case_equals_the_literal_algorithm():
    p, a, b = random_case()
    assert sorted(set(p["n"].tolist())) == [1, 2, 3, 4, 5]
    for k in ("bits", "chosen", "sums"):
        assert a[k].dtype == b[k].dtype and (a[k] == b[k]).all(), k
    seen = set(a["bits"].tolist())
    assert {0, ALL, dd.SEL_MIN, dd.SEL_MAX} <= seen and len(seen) >= 7          # the selections do differ
    assert (a["chosen"][:, 0] != a["chosen"][:, 1]).any() and (a["chosen"][:, :3] >= 0).all()


def test_chunks_change_no_byte():
    p, a, _ = random_case()
    parts = dd.chunks(p, 40000)
    assert len(parts) > 5 and parts[0][0] == 0 and parts[-1][1] == 300 and all(x[1] == y[0] for x, y in zip(parts, parts[1:]))
    b = dd.selections_numpy(p, budget=40000)
    assert all((a[k] == b[k]).all() for k in a)
    t = dd.tables(p, 100, 200)                              # a slice: groups, offsets and cages are the chunk's own
    assert t["group"].shape == (100, 16) and t["cage_start"][0] == 0 and t["cage"].shape[0] == t["cage_start"][-1] == ((p["cage_group"] >= 100) & (p["cage_group"] < 200)).sum()
    assert (np.diff(t["rows"][t["cage_start"][3]:t["cage_start"][4]]) > 0).all()


# ---- the sweep's files ----

STEM = "ORTHOIMAGERY.ORTHOPHOTOS{}_3_0_0"
COMPLETE_STATS, BLANK_STATS, PARTLY_STATS = (0, 200, 0, 0, 1 << 20, 0, 0, 1023, 1023), (255, 255, 1024, 1024, 0, 1024, 1024, -1, -1), (0, 255, 10, 0, 1000, 0, 0, 1023, 1013)


def write_key(path, images):
    """images: [(stem, stats)] -> the key file as blank.merge_parts writes it."""
    names = [s + ".jpeg" for s, _ in images]
    rows = aqblank.key_rows(names, np.asarray([st for _, st in images], np.int64))
    with open(path, "w") as f:
        f.write(aqblank.HEADER + "".join(f"{i},{r}\n" for i, r in enumerate(rows)))
    return str(path)


def write_geom(path, rings):
    feats = [bg.feature(stem + ".jpeg", np.zeros(12, np.int32), ring) for stem, ring in rings.items()]
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "features": feats}, f)
    return str(path)


def synthetic_sweep(tmp_path, years=(2014, 2015, 2017), extra_rows=None):
    """Scene 3 is 1843.2 m wide (0.3 m per pixel).  Tile (0, 0) holds the same six circles 12 px apart in every year."""
    labels = tmp_path / "labels"
    labels.mkdir()
    x0, y0 = (float(v) for v in geocode.lonlat_to_mercator(np.float64(3.5), np.float64(43.3)))
    x1, y1 = x0 + 1843.2, y0 + 1843.2
    csv_path = tmp_path / "wanted_bboxes.csv"
    csv_path.write_text(f',geometry\n3,"POLYGON (({x1!r} {y0!r}, {x1!r} {y1!r}, {x0!r} {y1!r}, {x0!r} {y0!r}, {x1!r} {y0!r}))"\n')
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    for y in years:
        rows = [row(0, 105 + 12 * k, 500, 10, 0.9) for k in range(6)] + (extra_rows or {}).get(y, [])
        (labels / (STEM.format(y) + ".txt")).write_text("".join(rows))
    return str(labels), str(csv_path)


def test_two_years_of_a_pass_count_once(tmp_path):
    labels, csv_path = synthetic_sweep(tmp_path)
    key = write_key(tmp_path / "key.csv", [(STEM.format(y), COMPLETE_STATS) for y in (2014, 2015, 2017)])
    geom = write_geom(tmp_path / "geom.geojson", {})
    table = geocode.geocode_label_dir(labels, csv_path)
    plain = facilities.cluster(table, "pass", labels_fn=facilities.dbscan_numpy)
    assert sorted(zip(plain["pass"], map(len, plain["cage_ids"]))) == [("2013-2015", 12), ("2016-2018", 6)]
    res = dd.dedup_from_table(table, key, geom, str(tmp_path / "out"), cpu=True)
    assert dd.survivors(res).sum() == 12 and dd.survivors(res, "min").sum() == 12 and res["bits"].shape == (18,)
    fac = dd.cluster(table, res, labels_fn=facilities.dbscan_numpy)
    assert sorted(zip(fac["pass"], map(len, fac["cage_ids"]))) == [("2013-2015", 6), ("2016-2018", 6)]
    a, b = plain["pass"].index("2013-2015"), fac["pass"].index("2013-2015")
    assert fac["area"][b] == pytest.approx(plain["area"][a] / 2, rel=1e-13)
    o, q = plain["pass"].index("2016-2018"), fac["pass"].index("2016-2018")
    assert fac["cage_ids"][q] == plain["cage_ids"][o] == fac["cage_ids_min"][q] == fac["cage_ids_max"][q] and fac["area"][q] == plain["area"][o]
    # equal areas: min is the first order (2014 keeps the tile), max the last (2015 does); the facility's two columns are those clusterings'
    years = np.asarray(table["year"])
    assert set(years[fac["cage_ids_min"][b]]) == {2014} and set(years[fac["cage_ids_max"][b]]) == {2015} and len(fac["cage_ids_min"][b]) == 6
    assert fac["cage_ids"][b] in (fac["cage_ids_min"][b], fac["cage_ids_max"][b])
    # the bootstrap's table: the bounds are sums over six cages each, not twelve
    factors = {"2013-2015": (12.0, 3.0, 0.8, 0.1), "2016-2018": (12.0, 3.0, 0.8, 0.1)}
    t_plain, _ = tn.build_table(plain, None, table, factors)
    t_dd, _ = tn.build_table(fac, None, table, factors)
    ent = lambda t, f, bit: t["area"][t["entry_start"][f]:t["entry_start"][f + 1]][(t["flags"][t["entry_start"][f]:t["entry_start"][f + 1]] & bit) != 0]
    for bit in (tn.SEL_MIN, tn.SEL_MAX, tn.SEL_RANDOM):
        assert ent(t_plain, a, bit).shape == (12,) and ent(t_dd, b, bit).shape == (6,)
        assert ent(t_dd, b, bit).sum() == pytest.approx(ent(t_plain, a, bit).sum() / 2, rel=1e-13)
    # the files
    cages = open(tmp_path / "out" / dd.CAGES_FILE).read().splitlines()
    assert cages[0] == "row,image,pass,tile_key,random,min,max" and len(cages) == 19
    assert cages[1].startswith(f"0,{STEM.format(2014)}.jpeg,2013-2015,3-0-0,") and cages[1].endswith(",1,0")
    tiles = open(tmp_path / "out" / dd.TILES_FILE).read().splitlines()
    assert len(tiles) == 3 and tiles[1].startswith(f"2013-2015,3-0-0,{STEM.format(2014)} {STEM.format(2015)},") and ",0 1,1 0," in tiles[1]
    doc = json.load(open(tmp_path / "out" / dd.JSON_FILE))
    assert doc["cages"] == 18 and doc["groups"] == 2 and doc["survivors"] == {"random": 12, "min": 12, "max": 12} and doc["seed"] == 0 and doc["cpu"]
    assert not [f for f in os.listdir(tmp_path / "out") if f.endswith(".tmp")]
    # the command lines: the module's own writes the same files; tonnage's takes the two blank files
    assert dd.main(["--labels", labels, "--geocode-bboxes", csv_path, "--blank-key", key, "--blank-geom", geom, "--out", str(tmp_path / "cli"), "--cpu"]) == 0
    for f in (dd.CAGES_FILE, dd.TILES_FILE, dd.JSON_FILE):
        assert open(tmp_path / "cli" / f, "rb").read() == open(tmp_path / "out" / f, "rb").read()
    fpath = tmp_path / "factors.csv"
    fpath.write_text("pass,s_mean,s_sd,h_mean,h_sd\n2013-2015,12,3,0.8,0.1\n2016-2018,12,3,0.8,0.1\n")
    common = ["--labels", labels, "--geocode-bboxes", csv_path, "--tonnage-factors", str(fpath), "--tonnage-K", "64", "--cpu"]
    assert tn.main([*common, "--out", str(tmp_path / "t_plain")]) == 0
    assert tn.main([*common, "--out", str(tmp_path / "t_dd"), "--dedup-years", key, geom]) == 0
    ton = lambda d: {r.split(",")[1]: float(r.split(",")[3]) for r in open(tmp_path / d / tn.FACILITIES_FILE).read().splitlines()[1:]}
    assert ton("t_dd")["2016-2018"] == ton("t_plain")["2016-2018"] and 0.3 < ton("t_dd")["2013-2015"] / ton("t_plain")["2013-2015"] < 0.7
    assert json.load(open(tmp_path / "t_dd" / tn.JSON_FILE))["dedup_years"] == {"selection": "random"}
    assert "dedup_years" not in json.load(open(tmp_path / "t_plain" / tn.JSON_FILE))
    # the seed decides the random order and nothing else does
    picks = {tuple(dd.dedup_from_table(table, key, geom, None, seed=s, cpu=True)["result"]["chosen"][:, 2].tolist()) for s in range(8)}
    assert len(picks) > 1
    again = dd.dedup_from_table(table, key, geom, None, seed=3, cpu=True)
    assert (again["bits"] == dd.dedup_from_table(table, key, geom, None, seed=3, cpu=True)["bits"]).all()


def test_white_space_and_blank_images(tmp_path):
    """2014 is partly blank (its right half, from x = 512, is white), 2015 complete, 2013 blank: a cage detected in the white part of 2014
    is dropped under every selection, the cages of the blank year too; those in 2014's left half compete with 2015's."""
    row = lambda cls, px, py, w, conf: f"{cls} {px / 1024:g} {py / 1024:g} {w / 1024:g} {w / 1024:g} {conf:g}\n"
    labels, csv_path = synthetic_sweep(tmp_path, (2013, 2014, 2015), {2014: [row(0, 800, 500, 10, 0.9), row(1, 300, 300, 10, 0.2)]})
    key = write_key(tmp_path / "key.csv", [(STEM.format(2013), BLANK_STATS), (STEM.format(2014), PARTLY_STATS), (STEM.format(2015), COMPLETE_STATS),
                                           ("ORTHOIMAGERY.ORTHOPHOTOS2015_3_1024_0", PARTLY_STATS)])     # partly blank without a feature: "actually blank"
    geom = write_geom(tmp_path / "geom.geojson", {STEM.format(2014): [(0, 0), (512, 0), (512, 1024), (0, 1024), (0, 0)]})
    table = geocode.geocode_label_dir(labels, csv_path)
    for sel in ("min", "max", "random"):
        res = dd.dedup_from_table(table, key, geom, None, sel, cpu=True)
        p = res["problem"]
        assert len(p["slots"]) == 1 and p["n"].tolist() == [2] and p["images"] == [[STEM.format(2014), STEM.format(2015)]]
        years = np.asarray(table["year"])
        assert not res["take"][(years == 2014) & (np.asarray(table["det_conf"]) < 0.5)].any()           # below --facilities-conf: takes no part
        keep = dd.survivors(res)
        assert not keep[years == 2013].any()
        white = (years == 2014) & (np.asarray(table["xmin"]) > 700)
        assert white.sum() == 1 and res["bits"][white].tolist() == [0]
        assert keep.sum() == 6 and len(set(years[keep])) == 1
        lit = dd.selections_literal(p)
        assert (lit["bits"] == res["result"]["bits"]).all()
    assert dd.survivors(res, "min").sum() == dd.survivors(res, "max").sum() == 6


# ---- cage_ids_min / cage_ids_max ----

def test_matching_takes_the_largest_overlap_of_the_same_pass():
    boxes = [(0, 0, 10, 10), (10, 0, 20, 10),               # the facility: U has 200 m^2
             (5, 0, 12, 10),                                # 0: 70 / 200
             (8, 2, 20, 8),                                 # 1: 72 / 200
             (0, 0, 20, 10),                                # 2: all of it, but another pass
             (20, 0, 30, 10),                               # 3: touches only: a match with overlap 0
             (8, 2, 20, 8),                                 # 4: ties with 1
             (50, 50, 60, 60),                              # 5: apart
             (0, 0, 20, 10)]                                # 6: all of it, but a rectangle farm: not part of all_cages
    b = np.asarray(boxes, np.float64)
    table = {"xmin_3857": b[:, 0], "ymin_3857": b[:, 1], "xmax_3857": b[:, 2], "ymax_3857": b[:, 3], "cls": np.asarray([0, 1, 0, 1, 0, 0, 1, 0, 4])}
    fac = {"facility_index": [0], "pass": ["p"], "cage_ids": [[0, 1]]}
    other = lambda ids, passes: {"facility_index": list(range(len(ids))), "pass": passes, "cage_ids": [[i] for i in ids]}
    assert dd.union_overlap(b[:2], b[2:3]) == pytest.approx(0.35) and dd.union_overlap(b[:2], b[3:4]) == pytest.approx(0.36)
    assert dd.union_overlap(b[:2], b[5:6]) == 0.0 and dd.union_overlap(b[:2], b[7:8]) is None
    assert dd.union_overlap(b[:2], np.concatenate([b[2:4], b[2:4]])) == pytest.approx((70 + 72 - 4 * 6) / 200)     # a union, not a sum
    assert dd.match_cage_ids(table, fac, other([2, 3, 4, 5, 7], ["p", "p", "q", "p", "p"])) == [[3]]
    assert dd.match_cage_ids(table, fac, other([6, 3, 2], ["p", "p", "p"])) == [[6]]                    # a tie: the smallest facility_index
    assert dd.match_cage_ids(table, fac, other([5, 7], ["p", "p"])) == [[5]]
    assert dd.match_cage_ids(table, fac, other([7, 4, 8], ["p", "q", "p"])) == [None]
    assert dd.match_cage_ids(table, fac, other([], [])) == [None]


def test_no_match_gives_an_empty_min_and_the_own_cages_as_max(monkeypatch):
    fac = {"facility_index": [0], "pass": ["p"], "cage_ids": [[0, 1]]}
    empty = {"facility_index": [], "pass": [], "cage_ids": []}
    monkeypatch.setattr(facilities, "cluster", lambda table, by, *a, keep=None, **kw: dict(fac) if keep == "random" else dict(empty))
    monkeypatch.setattr(dd, "survivors", lambda d, sel=None: sel or d["selection"])
    z = np.asarray([0.0, 1.0])
    got = dd.cluster({"cls": np.zeros(2, np.int64), "xmin_3857": z, "ymin_3857": z, "xmax_3857": z + 1, "ymax_3857": z + 1}, {"selection": "random"})
    assert got["cage_ids_min"] == [[]] and got["cage_ids_max"] == [[0, 1]]


# ---- refusals ----

def test_refusals(tmp_path):
    w, h = 40, 24
    left, _ = halves(w, h)
    with pytest.raises(ValueError, match=r"tile 7 of the list has 6 images; a group takes 1 to 5"):
        dd.make_problem([w], [h], [[None] * 6], [], [], np.zeros((0, 4)), [], names=["tile 7 of the list"])
    for ring, match in (([(0, 0), (41, 0), (41, 5), (0, 5), (0, 0)], "outside the 40 x 24 frame"), ([(0, 0), (5, 5), (0, 5), (0, 0)], "not axis-parallel"),
                        ([(0, 0), (5, 0), (5, 5), (0, 5)], "not a closed walk"), ([(0, -1), (5, -1), (5, 5), (0, 5), (0, -1)], "outside")):
        with pytest.raises(ValueError, match=match):
            dd.make_problem([w], [h], [[ring]], [], [], np.zeros((0, 4)), [])
    with pytest.raises(ValueError, match="does not exist"):
        dd.make_problem([w], [h], [[None, left]], [0], [2], [LEFT], [1.0])
    with pytest.raises(ValueError, match="not a permutation"):
        dd.make_problem([w], [h], [[None, left]], [], [], np.zeros((0, 4)), [], random_order=[[0, 0, -1, -1, -1]])
    # six years of one tile in one "pass" cannot happen with the reference's passes; a year outside them all falls into "No group"
    labels, csv_path = synthetic_sweep(tmp_path, tuple(range(1990, 1996)))
    table = geocode.geocode_label_dir(labels, csv_path)
    key = write_key(tmp_path / "key.csv", [(STEM.format(y), COMPLETE_STATS) for y in range(1990, 1996)])
    geom = write_geom(tmp_path / "geom.geojson", {})
    with pytest.raises(ValueError, match=r"pass No group, tile 3-0-0 \(.*1990.*1995.*\) has 6 images"):
        dd.dedup_from_table(table, key, geom, None, cpu=True)
    # an image of the label directory that the key lacks
    short = write_key(tmp_path / "short.csv", [(STEM.format(y), COMPLETE_STATS) for y in (1990, 1992)])
    with pytest.raises(ValueError, match=rf"4 images of the label directory are not in the blank key: {STEM.format(1991)} {STEM.format(1993)} "):
        dd.dedup_from_table(table, short, geom, None, cpu=True)
    with pytest.raises(ValueError, match="selection"):
        dd.dedup_from_table(table, key, geom, None, "median", cpu=True)
    bad = tmp_path / "bad.geojson"
    bad.write_text(json.dumps({"type": "FeatureCollection", "features": [{"type": "Feature", "properties": {"image": "a.jpeg"}, "geometry": None}]}))
    with pytest.raises(ValueError, match="ring_px"):
        dd.read_blank_geom(str(bad))
    with pytest.raises(ValueError, match="by 'pass'"):
        facilities.facilities_from_table(table, str(tmp_path / "f.geojson"), "year", cpu=True, dedup={"selection": "random"})


def test_options_symbols_and_the_build(lib):
    from aquaculture_amd import build, detect, engine
    header = open(os.path.join(ROOT, "include", "aq_engine.h")).read()
    for name in ("aq_dedup_fill_u32", "aq_dedup_sets_u32", "aq_dedup_select_f64"):
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert any(src == "dedup.hip" for src, _ in build.SOURCES)
    guards = open(os.path.join(ROOT, "aquaculture_amd", "csrc", "size_guards.h")).read()
    assert "dedup_count_fits" in guards and "dedup_frame_fits" in guards and "kDedupMaxSlots = 5" in guards
    assert (dd.SEL_MIN, dd.SEL_MAX, dd.SEL_RANDOM) == (tn.SEL_MIN, tn.SEL_MAX, tn.SEL_RANDOM) == (4, 8, 16)
    assert (engine.DEDUP_ABSENT, engine.DEDUP_FULL, engine.DEDUP_BITMAP, engine.DEDUP_MAX_PERMS) == (dd.KIND_ABSENT, dd.KIND_FULL, dd.KIND_BITMAP, dd.MAX_PERMS)
    assert dd.MAX_SLOTS == max(b - a + 1 for a, b in facilities.IMAGE_PASSES) == 5 and dd.FRAME == bg.IM_SIZE == geocode.IM_WIDTH
    base = ["--weights", "w.pt", "--source", "src", "--geocode-bboxes", "wb.csv"]
    opt = detect.parse_opt([*base, "--dedup-years"])
    assert opt.dedup_years == "" and opt.dedup_selection == "random" and opt.dedup_seed == 0 and opt.blank_geom == "" and opt.blank_key == ""
    opt = detect.parse_opt([*base, "--dedup-years", "out", "--dedup-selection", "max", "--dedup-seed", "7", "--facilities", "--facilities-by", "pass"])
    assert (opt.dedup_years, opt.dedup_selection, opt.dedup_seed) == ("out", "max", 7)
    plain = detect.parse_opt(base)
    assert plain.dedup_years is None and plain.blank_geom is None and plain.blank_key is None
    for argv in (["--weights", "w.pt", "--source", "src", "--dedup-years"], [*base, "--dedup-years", "--facilities"],
                 [*base, "--dedup-years", "--facilities", "--facilities-by", "year"], [*base, "--dedup-years", "--dedup-selection", "median"]):
        with pytest.raises(SystemExit):
            detect.parse_opt(argv)
    with pytest.raises(ValueError, match="needs --geocode-bboxes"):
        detect.run("w.pt", "src", dedup_years="")
    with pytest.raises(ValueError, match="--facilities-by pass"):
        detect.run("w.pt", "src", dedup_years="", geocode_bboxes="wb.csv", facilities="", facilities_by="year")
    with pytest.raises(ValueError, match="random, min or max"):
        detect.run("w.pt", "src", dedup_years="", geocode_bboxes="wb.csv", dedup_selection="median")
    assert "dedup" not in str(detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True))
