"""Facilities outside a pass's imagery (``--tonnage-missing``) and near known sites (``--tonnage-near-sites``).

The reference's headline table (src/Results/tonnage_estimates.py:110-133) has two rows per image pass: ``Model``, the bootstrap over the
facilities seen in that pass, and ``Model + Estimate missing``, the same plus the facilities of a neighbouring pass that lie where this pass
has no imagery (compute_complete_period_tonnage_estimates, src/utils_tonnage.py:1139-1201).  Both it and the reference's other printed
result, the tonnage near Trujillo et al.'s locations (trujillo_comparison), rest on one primitive, modify_cage_list_using_geometry
(:1108-1136): does a cage's box intersect a union of regions?  The definitions (include/aq_engine.h):

    image region   an image takes part under the rule of dedup.build_problem -- status ``complete``, or ``partly blank`` with a ring in the
                   blank-geom file -- if its name parses to a bbox_ind the wanted-bboxes table lists.  Its rectangle is
                   blank_geom.tile_bounds(name, wanted) = (west, south, east, north) in EPSG:3857.  Complete image: the closed rectangle.
                   Partly blank image: the closed even-odd region of the ring blank_geom.to_bounds(ring_px, west, south, east, north),
                   computed here in numpy by that expression, so both ends of a vertical segment hold the same double.
    coverage of p  the union of the regions of the images whose year maps to pass p (facilities.image_pass).
    meets(B, i)    closed box B = (x0, y0, x1, y1).  Rectangle image: x0 <= east && x1 >= west && y0 <= north && y1 >= south.  Ring image:
                   some segment's closed bounding box overlaps B (the segments are axis-parallel: the segment meets B), or an odd number of
                   segments have (ay <= y0) != (by <= y0) and ax > x0 (the corner (x0, y0) strictly inside; it only decides when no
                   segment meets B).  A box with a NaN meets nothing.
    first[q]       for query q = (box, target pass): the smallest image number of that pass whose region meets the box, or -1; images are
                   numbered in the order of ``regions``: sorted by (pass, image name).  Covered = first >= 0.

The predicate has three forms: first_gpu (csrc/coverage.hip through engine.coverage_first), first_numpy (the kernel's steps restated, through
the same band tables: the same bytes) and first_bruteforce (every image of the pass, no bands, written independently: the yardstick).
"""
from __future__ import annotations

import json
import os
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import blank as aqblank
from . import blank_geom
from . import facilities as aqfac

KIND_RECT, KIND_RING = 0, 1
MAX_BANDS = 1024                                            # default band count: min(this, max(1, most images of a pass // 8))
CAGE_COLUMNS = ("cage_ids", "cage_ids_max", "cage_ids_min")  # the reference's order (:1171)
SITES_PASS = "known sites"                                  # the pseudo-pass of ``near``
# reference src/Results/tonnage_estimates.py:111-118 (period_comparison_dict): current pass -> the pass its missing facilities come from
DEFAULT_MAP = {"2000-2004": "2005-2009", "2005-2009": "2010-2012", "2010-2012": "2005-2009", "2013-2015": "2010-2012",
               "2016-2018": "2010-2012", "2019-2021": "2010-2012"}
SOURCE = "Model + Estimate missing"
CAGES_FILE, FACILITIES_FILE, NEAR_FILE = "tonnage_missing_cages.csv", "tonnage_missing_facilities.csv", "tonnage_near_sites.csv"


# ---- the image table ----

def _table(passes: List[str], pass_id, rect, rings: List[Optional[np.ndarray]], names: List[str]) -> dict:
    n = len(names)
    counts = np.asarray([0 if r is None else r.shape[0] for r in rings], np.int64)
    start = np.zeros(n + 1, np.int64)
    np.cumsum(counts, out=start[1:])
    if start[-1] >= 1 << 31:
        raise ValueError(f"coverage: {start[-1]} ring vertices (fewer than 2^31: the ring starts are 32-bit)")
    xy = np.concatenate([r for r in rings if r is not None], 0) if counts.any() else np.zeros((0, 2))
    pass_id = np.asarray(pass_id, np.int32).reshape(-1)
    return {"passes": list(passes), "pass_id": pass_id, "pass_start": np.searchsorted(pass_id, np.arange(len(passes) + 1)).astype(np.int32),
            "rect": np.ascontiguousarray(rect, dtype=np.float64).reshape(-1, 4), "kind": (counts > 0).astype(np.uint8),
            "ring_start": start.astype(np.int32), "xy": np.ascontiguousarray(xy, dtype=np.float64).reshape(-1, 2), "names": list(names)}


def ring_metres(ring_px, west: float, south: float, east: float, north: float) -> np.ndarray:
    """blank_geom.to_bounds in numpy -> float64 [n, 2], the walk closed if the file left it open."""
    r = np.asarray(ring_px, np.float64).reshape(-1, 2)
    if r.shape[0] and (r[0] != r[-1]).any():
        r = np.concatenate([r, r[:1]], 0)
    a, e = (east - west) / blank_geom.IM_SIZE, (south - north) / blank_geom.IM_SIZE
    return np.stack([a * r[:, 0] + west, e * r[:, 1] + north], 1)


def regions(key_rows: Sequence[dict], rings: Dict[str, list], wanted: Dict[int, Tuple[float, float, float, float]]) -> dict:
    """The image table of a sweep from dedup.read_blank_key's rows, dedup.read_blank_geom's rings and geocode.load_wanted_bboxes' table:
    ``passes`` (the names of the passes that have an image, sorted), and per image, sorted by (pass, image name): ``pass_id``, ``rect``
    float64 [I, 4] (west, south, east, north), ``kind`` (KIND_RECT / KIND_RING), ``ring_start`` int32 [I + 1] into ``xy`` float64 [V, 2]
    (the metre vertices; a rectangle image has none), ``names``; and ``pass_start`` int32 [P + 1]."""
    from .dedup import _stem
    status = {}
    for r in key_rows:
        status[_stem(r["image"])] = r["image_status"]
    items = []
    for stem, st in status.items():
        year, ind, _, _ = aqblank.name_fields(stem)
        if ind == "" or int(ind) not in wanted:
            continue
        if st == aqblank.COMPLETE or (st == aqblank.PARTLY_BLANK and stem in rings):
            items.append((aqfac.image_pass(int(year)), stem, st != aqblank.COMPLETE))
    items.sort()
    passes = sorted({p for p, _, _ in items})
    rect, walks = [], []
    for _, stem, partly in items:
        b = blank_geom.tile_bounds(stem, wanted)
        rect.append(b)
        walks.append(ring_metres(rings[stem], *b) if partly else None)
    return _table(passes, [passes.index(p) for p, _, _ in items], np.asarray(rect, np.float64).reshape(-1, 4), walks, [s for _, s, _ in items])


def rect_regions(rects, pass_name: str = SITES_PASS, names: Optional[Sequence[str]] = None) -> dict:
    """``regions``' table for closed rectangles (west, south, east, north) that form one pass."""
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    n = rects.shape[0]
    return _table([pass_name], np.zeros(n, np.int32), rects, [None] * n, [str(k) for k in range(n)] if names is None else list(names))


def site_regions(sites) -> dict:
    """The closed +-1000 m rectangles of kfold.load_known_sites' points, built in EPSG:3857 as kfold.in_known_area builds them."""
    from .kfold import SITE_HALF_SIDE
    s = np.asarray(sites, np.float64).reshape(-1, 2)
    return rect_regions(np.stack([s[:, 0] - SITE_HALF_SIDE, s[:, 1] - SITE_HALF_SIDE, s[:, 0] + SITE_HALF_SIDE, s[:, 1] + SITE_HALF_SIDE], 1))


# ---- the band structure ----

def _band(y, Y0, h, nbands: int) -> np.ndarray:
    """floor((y - Y0) / h) clamped to [0, nbands) as int64: the kernel's expression (what is not >= 0, a NaN included, is band 0)."""
    with np.errstate(all="ignore"):
        t = np.floor((np.asarray(y, np.float64) - Y0) / h)
        return np.where(t >= 0.0, np.where(t < float(nbands), t, float(nbands - 1)), 0.0).astype(np.int64)


def band_tables(reg: dict, nbands: Optional[int] = None) -> dict:
    """Per pass nbands horizontal bands from Y0 = the pass's smallest south, of height h = (largest north - Y0) / nbands (1 where that is
    not positive); image i is entered in every band from band(south) to band(north).  -> ``nbands``, ``band`` float64 [P, 2] (Y0, h),
    ``entry_img`` int32 [entries] pass by pass and band by band (by image inside a band), ``band_start`` int32 [P nbands + 1]."""
    P, ps = len(reg["passes"]), reg["pass_start"].astype(np.int64)
    if nbands is None:
        nbands = min(MAX_BANDS, max(1, int(np.diff(ps).max()) // 8)) if P else 1
    nbands = int(nbands)
    if nbands < 1 or P * nbands + 1 >= 1 << 31:
        raise ValueError(f"coverage: {nbands} bands for each of {P} passes")
    if not np.isfinite(reg["rect"]).all():
        raise ValueError("coverage: an image rectangle is not finite")
    band = np.zeros((P, 2))
    start, entry = np.zeros(P * nbands + 1, np.int64), []
    at = 0
    for p in range(P):
        i0, i1 = int(ps[p]), int(ps[p + 1])
        south, north = reg["rect"][i0:i1, 1], reg["rect"][i0:i1, 3]
        Y0 = float(south.min()) if i1 > i0 else 0.0
        h = (float(north.max()) - Y0) / nbands if i1 > i0 else 1.0
        if not h > 0:
            h = 1.0
        band[p] = (Y0, h)
        lo, hi = _band(south, Y0, h, nbands), _band(north, Y0, h, nbands)
        counts = np.maximum(hi - lo + 1, 0)
        img = np.repeat(np.arange(i0, i1, dtype=np.int64), counts)
        first = np.cumsum(counts) - counts
        band_of = np.repeat(lo, counts) + (np.arange(int(counts.sum())) - np.repeat(first, counts))
        order = np.argsort(band_of, kind="stable")
        entry.append(img[order])
        start[p * nbands:(p + 1) * nbands + 1] = at + np.searchsorted(band_of[order], np.arange(nbands + 1))
        at += img.shape[0]
    if at >= 1 << 31:
        raise ValueError(f"coverage: {at} band entries (fewer than 2^31 in one call): use fewer bands")
    return {"nbands": nbands, "band": band, "entry_img": (np.concatenate(entry) if entry else np.zeros(0, np.int64)).astype(np.int32),
            "band_start": start.astype(np.int32)}


# ---- the predicate ----

def _queries(boxes, qpass) -> Tuple[np.ndarray, np.ndarray]:
    boxes = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
    qpass = np.ascontiguousarray(np.asarray(qpass, np.int32).reshape(-1))
    if qpass.shape[0] != boxes.shape[0]:
        raise ValueError(f"coverage: {boxes.shape[0]} boxes and {qpass.shape[0]} target passes")
    return boxes, qpass


def first_numpy(reg: dict, bands: dict, boxes, qpass) -> np.ndarray:
    """The kernel's steps in numpy -> int32 [Q]: per query the run of entries of the bands band(y0) .. band(y1) of its target pass, the
    rectangle test on every entry, the images that pass it with a ring segment by segment."""
    boxes, qpass = _queries(boxes, qpass)
    P, I, nb = len(reg["passes"]), reg["rect"].shape[0], int(bands["nbands"])
    rect, rs, xy = reg["rect"], reg["ring_start"].astype(np.int64), reg["xy"]
    entry, bstart = bands["entry_img"].astype(np.int64), bands["band_start"].astype(np.int64)
    out = np.full(boxes.shape[0], -1, np.int32)
    for q in range(boxes.shape[0]):
        x0, y0, x1, y1 = boxes[q].tolist()
        tp = int(qpass[q])
        if not 0 <= tp < P or x0 != x0 or y0 != y0 or x1 != x1 or y1 != y1:
            continue
        Y0, h = bands["band"][tp].tolist()
        b0, b1 = int(_band(y0, Y0, h, nb)), int(_band(y1, Y0, h, nb))
        run0 = int(bstart[tp * nb + b0])
        run1 = int(bstart[tp * nb + b1 + 1]) if b1 >= b0 else run0
        img = entry[run0:run1]
        img = img[(img >= 0) & (img < I)]
        r = rect[img]
        img = img[(x0 <= r[:, 2]) & (x1 >= r[:, 0]) & (y0 <= r[:, 3]) & (y1 >= r[:, 1])]
        ring = rs[img + 1] > rs[img]
        best = int(img[~ring].min()) if (~ring).any() else I
        for i in np.unique(img[ring]).tolist():             # ascending: the first that meets is the smallest
            if i >= best:
                break
            a, c = xy[rs[i]:rs[i + 1] - 1], xy[rs[i] + 1:rs[i + 1]]
            hit = ((a[:, 0] <= x1) | (c[:, 0] <= x1)) & ((a[:, 0] >= x0) | (c[:, 0] >= x0)) & ((a[:, 1] <= y1) | (c[:, 1] <= y1)) & ((a[:, 1] >= y0) | (c[:, 1] >= y0))
            if hit.any() or int((((a[:, 1] <= y0) != (c[:, 1] <= y0)) & (a[:, 0] > x0)).sum()) & 1:
                best = i
                break
        if best < I:
            out[q] = best
    return out


def first_bruteforce(reg: dict, boxes, qpass, chunk_pairs: int = 1 << 22) -> np.ndarray:
    """The definition without a search structure -> int32 [Q]: every image of the target pass, from the last to the first; a rectangle by
    the overlap of two intervals per axis, a ring by its segments' bounding boxes and by counting the vertical segments to the right of the
    corner (x0, y0) that span its y.  No rectangle test before a ring."""
    boxes, qpass = _queries(boxes, qpass)
    out = np.full(boxes.shape[0], -1, np.int32)
    rs = reg["ring_start"].astype(np.int64)
    with np.errstate(all="ignore"):
        for p in range(len(reg["passes"])):
            qs = np.nonzero(qpass == p)[0]
            if qs.shape[0] == 0:
                continue
            for i in range(int(reg["pass_start"][p + 1]) - 1, int(reg["pass_start"][p]) - 1, -1):
                if reg["kind"][i] == KIND_RECT:
                    w, s, e, n = reg["rect"][i].tolist()
                    b = boxes[qs]
                    meets = (np.maximum(b[:, 0], w) <= np.minimum(b[:, 2], e)) & (np.maximum(b[:, 1], s) <= np.minimum(b[:, 3], n))
                    out[qs[meets]] = i
                    continue
                v = reg["xy"][rs[i]:rs[i + 1]]
                sx0, sx1 = np.minimum(v[:-1, 0], v[1:, 0])[None, :], np.maximum(v[:-1, 0], v[1:, 0])[None, :]
                sy0, sy1 = np.minimum(v[:-1, 1], v[1:, 1])[None, :], np.maximum(v[:-1, 1], v[1:, 1])[None, :]
                vertical = (v[:-1, 0] == v[1:, 0])[None, :]
                step = max(1, chunk_pairs // max(1, v.shape[0]))
                for at in range(0, qs.shape[0], step):
                    k = qs[at:at + step]
                    x0, y0, x1, y1 = (boxes[k, j, None] for j in range(4))
                    touch = ((sx0 <= x1) & (x0 <= sx1) & (sy0 <= y1) & (y0 <= sy1)).any(1)
                    right = (vertical & (sx0 > x0) & (sy0 <= y0) & (y0 < sy1)).sum(1) % 2 == 1
                    nan = np.isnan(boxes[k]).any(1)
                    out[k[(touch | right) & ~nan]] = i
    return out


def first_gpu(reg: dict, bands: dict, boxes, qpass, times: Optional[dict] = None) -> np.ndarray:
    """int32 [Q] from the GPU (engine.coverage_first: host arrays in, host array out).  Raises without the library or a GPU."""
    import torch
    from . import engine
    boxes, qpass = _queries(boxes, qpass)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    return engine.coverage_first(dev(reg["rect"]), dev(reg["ring_start"]), dev(reg["xy"]), dev(bands["entry_img"]), dev(bands["band_start"]),
                                 dev(bands["band"]), bands["nbands"], dev(boxes), dev(qpass), reg["ring_start"], bands["band_start"], bands["band"],
                                 times=times).cpu().numpy()


HOWS = ("gpu", "numpy", "bruteforce")


def make_first(reg: dict, how: str = "gpu", nbands: Optional[int] = None) -> Callable:
    """fn(boxes [Q, 4], pass names [Q]) -> first int32 [Q] over `reg`, by first_gpu, first_numpy or first_bruteforce; a pass that has no
    image is a pass with empty coverage.  The function carries ``reg``."""
    if how not in HOWS:
        raise ValueError(f"coverage: how = {how!r} ({', '.join(HOWS)})")
    bands = band_tables(reg, nbands) if how != "bruteforce" else None
    index = {p: k for k, p in enumerate(reg["passes"])}

    def fn(boxes, names):
        qpass = np.asarray([index.get(p, -1) for p in names], np.int32)
        if how == "bruteforce":
            return first_bruteforce(reg, boxes, qpass)
        return (first_gpu if how == "gpu" else first_numpy)(reg, bands, boxes, qpass)
    fn.reg = reg
    return fn


# ---- the imputation ----

def parse_map(text: Optional[str]) -> Dict[str, str]:
    """``cur=cmp[,cur=cmp...]`` -> {current pass: compare pass}; nothing: the reference's period_comparison_dict."""
    if not text:
        return dict(DEFAULT_MAP)
    out: Dict[str, str] = {}
    for part in text.split(","):
        cur, eq, cmp_ = part.partition("=")
        cur, cmp_ = cur.strip(), cmp_.strip()
        if not eq or not cur or not cmp_:
            raise ValueError(f"--tonnage-missing {text!r}: {part!r} is not CURRENT_PASS=COMPARE_PASS")
        if cur == cmp_:
            raise ValueError(f"--tonnage-missing {text!r}: pass {cur} cannot fill in for itself")
        if cur in out:
            raise ValueError(f"--tonnage-missing {text!r}: pass {cur} is listed twice")
        out[cur] = cmp_
    return out


def _column(fac: Dict[str, list], col: str, f: int) -> List[int]:
    return [int(c) for c in (fac[col][f] if col in fac else fac["cage_ids"][f])]


def _cut_table(fac, rows: List[Tuple[str, int, bool, Dict[str, List[int]]]]) -> Dict[str, list]:
    """(to pass, facility position in fac, own, the three lists) per kept facility -> the facility dict tonnage.build_table takes."""
    out = {"facility_index": [int(fac["facility_index"][f]) for _, f, _, _ in rows], "pass": [p for p, _, _, _ in rows],
           "from_pass": [fac["pass"][f] for _, f, _, _ in rows], "own": [own for _, _, own, _ in rows], "position": [f for _, f, _, _ in rows]}
    for col in CAGE_COLUMNS:
        out[col] = [lists[col] for _, _, _, lists in rows]
    if "_areas" in fac:
        out["_areas"] = fac["_areas"]
    return out


def impute(fac: Dict[str, list], table: Dict[str, np.ndarray], first_fn: Callable, compare_map: Dict[str, str]) -> dict:
    """For each current pass p of the map, in sorted order: the facilities of pass p as they are, in fac order, then the facilities of
    compare_map[p], in fac order, with each of cage_ids, cage_ids_max and cage_ids_min cut to the cages that p's coverage does NOT cover
    (a cage's box: its row of land.table_boxes(table)), those whose cut cage_ids_min is empty dropped (the reference's rule, :1177-1178),
    the rest re-labelled as pass p.  The queries are the unique (cage, target pass) pairs, sorted; first_fn (make_first's) answers them in
    one call.  -> the facility dict of tonnage.build_table (facility_index, pass, cage_ids*, _areas; beside them from_pass, own, position)
    with ``queries`` (cage, target, first), ``added`` (every facility of a compare pass, kept or not: facility_index, from_pass, to_pass,
    before and after lengths, kept, position in the table or -1) and ``counts`` {p: (own, added)}."""
    from . import land as aqland
    for p, c in compare_map.items():
        if p == c:
            raise ValueError(f"tonnage missing: pass {p} cannot fill in for itself")
    boxes = aqland.table_boxes(table)
    F = len(fac["facility_index"])
    of_pass: Dict[str, List[int]] = {}
    for f in range(F):
        of_pass.setdefault(fac["pass"][f], []).append(f)
    pairs = sorted({(c, p) for p, cmp_ in compare_map.items() for f in of_pass.get(cmp_, []) for col in CAGE_COLUMNS for c in _column(fac, col, f)})
    first = np.asarray(first_fn(boxes[[c for c, _ in pairs]].reshape(-1, 4), [p for _, p in pairs]), np.int32).reshape(-1) if pairs else np.zeros(0, np.int32)
    covered = {pair: int(v) >= 0 for pair, v in zip(pairs, first.tolist())}
    rows, added, counts = [], [], {}
    for p in sorted(compare_map):
        own = [(p, f, True, {col: _column(fac, col, f) for col in CAGE_COLUMNS}) for f in of_pass.get(p, [])]
        extra = []
        for f in of_pass.get(compare_map[p], []):
            before = {col: _column(fac, col, f) for col in CAGE_COLUMNS}
            after = {col: [c for c in before[col] if not covered[(c, p)]] for col in CAGE_COLUMNS}
            kept = len(after["cage_ids_min"]) > 0
            added.append({"facility_index": int(fac["facility_index"][f]), "from_pass": compare_map[p], "to_pass": p,
                          "before": [len(before[col]) for col in CAGE_COLUMNS], "after": [len(after[col]) for col in CAGE_COLUMNS], "kept": kept,
                          "position": len(rows) + len(own) + len(extra) if kept else -1})
            if kept:
                extra.append((p, f, False, after))
        counts[p] = (len(own), len(extra))
        rows += own + extra
    out = _cut_table(fac, rows)
    out.update(queries={"cage": [c for c, _ in pairs], "target": [p for _, p in pairs], "first": first}, added=added, counts=counts)
    return out


def impute_literal(fac: Dict[str, list], table: Dict[str, np.ndarray], first_fn: Callable, compare_map: Dict[str, str]) -> dict:
    """The reference's loops as they stand (:1162-1184), for the tests: per period, per column, per facility, per cage one question; the
    facilities of the two passes in fac order (``isin``), those without a cage in cage_ids_min dropped, all re-labelled.  -> per period
    {"facility_index", "from_pass", "cage_ids", "cage_ids_max", "cage_ids_min", "total", "added"}: the last two are the numbers the
    reference prints."""
    from . import land as aqland
    boxes = aqland.table_boxes(table)
    out = {}
    for current, compare in compare_map.items():
        take = [f for f in range(len(fac["facility_index"])) if fac["pass"][f] in (compare, current)]
        cols = {}
        for col in CAGE_COLUMNS:
            cols[col] = []
            for f in take:
                ids = _column(fac, col, f)
                if fac["pass"][f] != current:
                    new = []
                    for c in ids:
                        intersects = int(first_fn(boxes[c].reshape(1, 4), [current])[0]) >= 0
                        if not intersects:
                            new.append(c)
                    ids = new
                cols[col].append(ids)
        keep = [k for k in range(len(take)) if len(cols["cage_ids_min"][k]) > 0]
        out[current] = {"facility_index": [int(fac["facility_index"][take[k]]) for k in keep], "from_pass": [fac["pass"][take[k]] for k in keep],
                        **{col: [cols[col][k] for k in keep] for col in CAGE_COLUMNS}, "total": len(keep),
                        "added": sum(fac["pass"][take[k]] == compare for k in keep)}
    return out


def near(fac: Dict[str, list], table: Dict[str, np.ndarray], first_fn, sites) -> dict:
    """The ``inside`` form (the reference's trujillo_comparison): every facility keeps its pass, all three columns are cut to the cages
    whose box meets the closed +-1000 m rectangle of a site, and a facility whose cut cage_ids_min is empty is dropped.  first_fn: "gpu",
    "numpy" or "bruteforce", or make_first's function over site_regions(sites).  -> impute's facility dict with ``queries``."""
    from . import land as aqland
    if isinstance(first_fn, str):
        first_fn = make_first(site_regions(sites), first_fn)
    boxes = aqland.table_boxes(table)
    F = len(fac["facility_index"])
    cages = sorted({c for f in range(F) for col in CAGE_COLUMNS for c in _column(fac, col, f)})
    first = np.asarray(first_fn(boxes[cages].reshape(-1, 4), [SITES_PASS] * len(cages)), np.int32).reshape(-1) if cages else np.zeros(0, np.int32)
    covered = {c: int(v) >= 0 for c, v in zip(cages, first.tolist())}
    rows = []
    for f in range(F):
        cut = {col: [c for c in _column(fac, col, f) if covered[c]] for col in CAGE_COLUMNS}
        if cut["cage_ids_min"]:
            rows.append((fac["pass"][f], f, True, cut))
    out = _cut_table(fac, rows)
    out["queries"] = {"cage": cages, "target": [SITES_PASS] * len(cages), "first": first}
    return out


# ---- the step inside tonnage.tonnage_from_table ----

def settings(map_text: Optional[str], blank_key: str, blank_geom_path: str, bboxes_csv: str) -> dict:
    """What tonnage_from_table(missing=...) takes: the map and the sweep's three files."""
    return {"map": parse_map(map_text), "blank_key": blank_key, "blank_geom": blank_geom_path, "bboxes": bboxes_csv}


def _lines(out_dir: str, name: str, lines: List[str]) -> None:
    from .dedup import _durable
    os.makedirs(out_dir, exist_ok=True)
    _durable(os.path.join(out_dir, name), "".join(lines))


def missing_estimates(fac, table, opts: dict, estimate_fn: Callable, out_dir: str, cpu: bool = False) -> dict:
    """Image table, imputation, one simulation of the imputed table (estimate_fn(facility dict) = tonnage.estimate with the run's settings)
    and the two files.  -> {"rows": [(pass, tonnage, tonnage_sd)] sorted by pass, "json": tonnage.json's ``missing`` section}.  A pass of
    the map with neither own nor added facilities has nothing to simulate and gets no row."""
    from . import dedup as aqdedup
    from . import geocode
    reg = regions(aqdedup.read_blank_key(opts["blank_key"]), aqdedup.read_blank_geom(opts["blank_geom"]), geocode.load_wanted_bboxes(opts["bboxes"]))
    imp = impute(fac, table, make_first(reg, "numpy" if cpu else "gpu"), opts["map"])
    est = estimate_fn(imp) if imp["facility_index"] else None
    stems = [str(s) for s in table["stems"]]
    q = imp["queries"]
    lines = ["row,image,pass,target_pass,first_image,kept\n"]
    for c, target, v in zip(q["cage"], q["target"], q["first"].tolist()):
        lines.append(f"{c},{stems[int(table['image'][c])]}.jpeg,{aqfac.image_pass(int(table['year'][c]))},{target},"
                     f"{reg['names'][v] + '.jpeg' if v >= 0 else ''},{int(v < 0)}\n")
    _lines(out_dir, CAGES_FILE, lines)
    lines = ["facility_index,from_pass,to_pass," + ",".join(f"{col}_before,{col}_after" for col in CAGE_COLUMNS) + ",kept,tonnage,tonnage_sd\n"]
    for a in imp["added"]:
        ton = (repr(est["facility_tonnage"][a["position"]]), repr(est["facility_tonnage_sd"][a["position"]])) if a["kept"] else ("", "")
        lines.append(f"{a['facility_index']},{a['from_pass']},{a['to_pass']}," + ",".join(f"{b},{c}" for b, c in zip(a["before"], a["after"])) +
                     f",{int(a['kept'])},{ton[0]},{ton[1]}\n")
    _lines(out_dir, FACILITIES_FILE, lines)
    ps = reg["pass_start"].astype(np.int64)
    rs = reg["ring_start"].astype(np.int64)
    per_pass = {}
    for p in sorted(opts["map"]):
        k = reg["passes"].index(p) if p in reg["passes"] else -1
        per_pass[p] = {"compare": opts["map"][p], "own": imp["counts"][p][0], "added": imp["counts"][p][1],
                       "images": int(ps[k + 1] - ps[k]) if k >= 0 else 0, "ring_vertices": int(rs[ps[k + 1]] - rs[ps[k]]) if k >= 0 else 0}
    rows = list(zip(est["pass"], est["tonnage"], est["tonnage_sd"])) if est is not None else []
    return {"rows": rows, "json": {"map": dict(sorted(opts["map"].items())), "passes": per_pass}, "imputed": imp, "estimate": est}


def near_estimates(fac, table, sites_csv: str, estimate_fn: Callable, out_dir: str, cpu: bool = False) -> dict:
    """--tonnage-near-sites: a further simulation of the facilities cut to the cages near a known site -> tonnage_near_sites.csv, one row
    per pass: pass, tonnage, tonnage_sd, facilities, cages (the summed length of the cut cage_ids, the reference's num_cages)."""
    from .kfold import load_known_sites
    sites = load_known_sites(sites_csv)
    cut = near(fac, table, "numpy" if cpu else "gpu", sites)
    est = estimate_fn(cut) if cut["facility_index"] else None
    lines = ["pass,tonnage,tonnage_sd,facilities,cages\n"]
    for k, p in enumerate(est["pass"] if est is not None else []):
        of = [j for j in range(len(cut["pass"])) if cut["pass"][j] == p]
        lines.append(f"{p},{est['tonnage'][k]!r},{est['tonnage_sd'][k]!r},{len(of)},{sum(len(cut['cage_ids'][j]) for j in of)}\n")
    _lines(out_dir, NEAR_FILE, lines)
    return {"json": {"sites": int(sites.shape[0]), "facilities": len(cut["facility_index"])}, "cut": cut, "estimate": est}
