"""Images wholly on land (``detect.py --land-images``, ``python -m aquaculture_amd.land --images``, ``python -m aquaculture_amd.evaluate
--land-images``): land_images.csv and land_images.json from the images' rectangles and the land file.

reference src/utils.py:46-69 (mark_land_images): an image contains only land when its rectangle lies ``within`` the land polygons shrunk by
5 m (``buffer(-5)`` in EPSG:3857, dissolved).  The reference drops the detections of such images (``surely_land``), puts the images into the
stratum ``land`` (set_buckets) and takes them out of the image table before the hold-out and the folds are drawn
(src/get_kfold_cluster_performance.py:84-109, 495-503); ``--evaluate-kfold`` does the last two with this module's answer (kfold.py).

No polygon is buffered.  A rectangle R lies inside the erosion of a region L by r exactly when R lies in L and no point of the boundary of L
is nearer to R than r: one inside test for a corner and a minimum over rectangle-to-edge distances.  Two land features that share an edge each
retreat from it in the reference, and a rectangle across that edge is not ``within``; here the shared edge is at distance 0: the same answer.

THE RULE (csrc/land_images.hip states it too; the kernel and land_images_numpy evaluate these expressions in this order, without fused
multiply-adds).  N rectangles (x0, y0, x1, y1), x0 <= x1 and y0 <= y1; E segments (ax, ay, bx, by) as land.load_land_geojson gives them; an
indent r > 0; all fp64 EPSG:3857 metres.  max(u, v) below keeps a NaN of either side, as numpy.maximum does.
  psd(p; a, b)   point to segment, squared: ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay, L = ux ux + uy uy,
                 t = (wx ux + wy uy) / L, replaced by 0 by a selection when not L > 0 (the 0 / 0 of a segment of no length never gets
                 through), then t = 0 if t < 0 else (1 if t > 1 else t), ex = wx - t ux, ey = wy - t uy, result ex ex + ey ey
  prd(p; R)      point to rectangle, squared: dx = max(max(x0 - px, px - x1), 0), dy = max(max(y0 - py, py - y1), 0), result dx dx + dy dy
  d2(R, seg)     0 if the segment meets the closed rectangle, by the land filter's bit-0 predicate as it stands (land.py); else the minimum
                 of psd for the corners (x0, y0), (x1, y0), (x1, y1), (x0, y1), then prd(a; R), then prd(b; R): for a segment and a convex
                 polygon that do not meet, one of these six attains the distance
Every minimum is the selection ``v if v < m else m`` starting from m = +inf, so a NaN never enters.  Per rectangle one double and one byte:
  dist2    the minimum of d2 over the segments, capped: m if m < cap2 else cap2, cap2 = (2 r) (2 r)
  bit 0    dist2 < r r: a coast edge is nearer than the indent, an edge that meets the rectangle included
  bit 1    the land filter's corner parity as it stands: the even-odd rule for (x0, y0)
An image is on land iff the byte is 2; at distance r exactly it is on land, as ``within`` allows touching.  A rectangle with a coordinate
that is not a number gets byte 0 and dist2 = cap2, by a test of its own before anything else.  The GPU searches the segments
of the bands band(y0 - 3 r) .. band(y1 + 3 r) only; one outside them has a y-gap above 3 r (1 - 1e-9) and a computed d2 above cap2, so the cap
makes both outputs independent of the band height, and the restatement here, which has no bands and takes every segment, gives the same bytes
and the same doubles.

The detections need no filter of their own: a detection's box lies inside its image's rectangle, that rectangle inside the land, so the land
filter's byte for the box is not 0 and the ocean rows hold none of them (a property the tests check).

NOT pinned, and what differs from the reference:
  * GEOS draws the quarter circle of a buffer as 8 chords, so where its buffer(-r) goes round a vertex of the coast the retreat is
    between r cos(pi / 16) and r, not r.  Only an image whose distance lies within that 2 % of the indent -- r cos(pi / 16) <= dist <=
    r / cos(pi / 16), taken on both sides -- can be decided differently from the exact erosion; land_images.json counts them
    (``near_threshold``).
  * bit 1 is even-odd parity over all rings, where the reference has the union of per-polygon erosions: overlapping land polygons differ, as
    they already do for ``--land-filter``.
  * no shapely / geopandas on the machines this was written on: the comparison with ``within(buffer(-5))`` itself is not pinned; the rule
    is pinned against exact rational arithmetic (fractions.Fraction) away from |d2 - r^2| < 1e-6.
"""
from __future__ import annotations

import csv
import json
import math
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import land

INDENT = 5.0                                                # metres: the reference's buffer(-5)
CSV_FILE, JSON_FILE = "land_images.csv", "land_images.json"
CSV_COLUMNS = ("image", "on_land", "inside", "dist")
NEEDS_LAND = ("--land-images marks the images that lie within the land polygons: it needs --land-filter GEOJSON (the land file) and "
              "--geocode-bboxes CSV (the images' rectangles)")
SCENES_NEED_IMAGES = ("--land-images with --tile-scenes: the tiles cut from the scenes are not listed anywhere after the sweep, so the image list "
                      "needs --evaluate-kfold-images FILE (the tile names, one per line)")
ON_LAND = 2                                                 # the byte of an image wholly on land: corner inside, no edge nearer than the indent


# ---- the rule ----

def _check_indent(indent) -> float:
    r = float(indent)
    if not (r > 0 and math.isfinite(r)):
        raise ValueError(f"land images: indent = {indent} (it has to be positive and finite)")
    return r


def _psd(px, py, ax, ay, bx, by):
    ux, uy, wx, wy = bx - ax, by - ay, px - ax, py - ay
    L = ux * ux + uy * uy
    t = (wx * ux + wy * uy) / L
    t = np.where(L > 0.0, t, 0.0)
    t = np.where(t < 0.0, 0.0, np.where(t > 1.0, 1.0, t))
    ex, ey = wx - t * ux, wy - t * uy
    return ex * ex + ey * ey


def _prd(px, py, x0, y0, x1, y1):
    dx, dy = np.maximum(np.maximum(x0 - px, px - x1), 0.0), np.maximum(np.maximum(y0 - py, py - y1), 0.0)
    return dx * dx + dy * dy


def land_images_numpy(rects, segs, indent: float = INDENT, chunk_pairs: int = 1 << 20) -> Tuple[np.ndarray, np.ndarray]:
    """The rule of the module's docstring in numpy -> (flags uint8 [N], dist2 float64 [N]): every rectangle against every segment,
    `chunk_pairs` pairs at a time (about 400 bytes of temporaries per pair).  For ``--cpu`` and the tests; no bands: it takes every segment,
    which by the cap gives what engine.land_images gives."""
    r = _check_indent(indent)
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    segs = np.asarray(segs, np.float64).reshape(-1, 4)
    n, E = rects.shape[0], segs.shape[0]
    cap2, r2 = (2.0 * r) * (2.0 * r), r * r
    flags, dist2 = np.zeros(n, np.uint8), np.full(n, cap2, np.float64)
    if n == 0 or E == 0:
        return flags, dist2
    ax, ay, bx, by = (segs[None, :, k] for k in range(4))
    step = max(1, chunk_pairs // E)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        for i in range(0, n, step):
            x0, y0, x1, y1 = (rects[i:i + step, k, None] for k in range(4))
            o = land._orient(ax, ay, bx, by, x0, y0)
            up = ay <= y0
            cross = (up != (by <= y0)) & np.where(up, o > 0.0, o < 0.0)
            near = ((ax <= x1) | (bx <= x1)) & ((ax >= x0) | (bx >= x0)) & ((ay <= y1) | (by <= y1)) & ((ay >= y0) | (by >= y0))
            o1, o2, o3 = land._orient(ax, ay, bx, by, x1, y0), land._orient(ax, ay, bx, by, x1, y1), land._orient(ax, ay, bx, by, x0, y1)
            one_side = ((o > 0.0) & (o1 > 0.0) & (o2 > 0.0) & (o3 > 0.0)) | ((o < 0.0) & (o1 < 0.0) & (o2 < 0.0) & (o3 < 0.0))
            m = np.full(o.shape, np.inf)
            for v in (_psd(x0, y0, ax, ay, bx, by), _psd(x1, y0, ax, ay, bx, by), _psd(x1, y1, ax, ay, bx, by), _psd(x0, y1, ax, ay, bx, by),
                      _prd(ax, ay, x0, y0, x1, y1), _prd(bx, by, x0, y0, x1, y1)):
                m = np.where(v < m, v, m)
            d2 = np.where(near & ~one_side, 0.0, m)
            best = d2.min(1)                                # (m is never NaN, so neither is d2; the minimum of a set has no order)
            best = np.where(best < cap2, best, cap2)
            nan = np.isnan(rects[i:i + step]).any(1)
            best, cross = np.where(nan, cap2, best), cross & ~nan[:, None]
            dist2[i:i + step] = best
            flags[i:i + step] = (best < r2).astype(np.uint8) | ((cross.sum(1) & 1).astype(np.uint8) << 1)
    return flags, dist2


def land_images_literal(rects, segs, indent, number=float) -> Tuple[List[int], list]:
    """The definition in plain loops over one arithmetic type -> (bytes, dist2), both lists: ``float`` (IEEE doubles, each operation rounded
    once) or ``fractions.Fraction`` (exact; the inputs have to be finite then).  For the tests."""
    zero, one = number(0), number(1)
    r = number(indent)
    cap2, r2 = (2 * r) * (2 * r), r * r
    inf = float("inf")
    big = lambda u, v: u if (u > v or u != u) else v

    def psd(px, py, ax, ay, bx, by):
        ux, uy, wx, wy = bx - ax, by - ay, px - ax, py - ay
        L = ux * ux + uy * uy
        t = (wx * ux + wy * uy) / L if L > 0 else zero
        t = zero if t < 0 else (one if t > 1 else t)
        ex, ey = wx - t * ux, wy - t * uy
        return ex * ex + ey * ey

    def prd(px, py, x0, y0, x1, y1):
        dx, dy = big(big(x0 - px, px - x1), zero), big(big(y0 - py, py - y1), zero)
        return dx * dx + dy * dy

    orient = lambda ax, ay, bx, by, cx, cy: (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)
    segs = [tuple(number(v) for v in s) for s in np.asarray(segs, np.float64).reshape(-1, 4).tolist()]
    flags, dist2 = [], []
    for x0, y0, x1, y1 in (tuple(number(v) for v in b) for b in np.asarray(rects, np.float64).reshape(-1, 4).tolist()):
        m, crossings = inf, 0
        for ax, ay, bx, by in (segs if x0 == x0 and y0 == y0 and x1 == x1 and y1 == y1 else []):
            corners = ((x0, y0), (x1, y0), (x1, y1), (x0, y1))
            o = [orient(ax, ay, bx, by, cx, cy) for cx, cy in corners]
            if (ay <= y0) != (by <= y0) and ((o[0] > 0) if ay <= y0 else (o[0] < 0)):
                crossings += 1
            near = (ax <= x1 or bx <= x1) and (ax >= x0 or bx >= x0) and (ay <= y1 or by <= y1) and (ay >= y0 or by >= y0)
            if near and not (all(v > 0 for v in o) or all(v < 0 for v in o)):
                d2 = zero
            else:
                d2 = inf
                for v in [psd(cx, cy, ax, ay, bx, by) for cx, cy in corners] + [prd(ax, ay, x0, y0, x1, y1), prd(bx, by, x0, y0, x1, y1)]:
                    d2 = v if v < d2 else d2
            m = d2 if d2 < m else m
        m = m if m < cap2 else cap2
        dist2.append(m)
        flags.append(int(m < r2) | ((crossings & 1) << 1))
    return flags, dist2


def land_images_gpu(rects, segs, indent: float = INDENT, band_height: Optional[float] = None, times: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(flags, dist2) from the GPU (engine.land_images: host arrays in, host arrays out).  Raises without the library or a GPU: use
    land_images_numpy there."""
    import torch
    from . import engine
    rects = np.ascontiguousarray(np.asarray(rects, np.float64).reshape(-1, 4))
    segs = np.ascontiguousarray(np.asarray(segs, np.float64).reshape(-1, 4))
    f, d = engine.land_images(torch.from_numpy(rects).cuda(), torch.from_numpy(segs).cuda(), _check_indent(indent), band_height, times=times)
    return f.cpu().numpy(), d.cpu().numpy()


def on_land(rects, segs, indent: float = INDENT, cpu: bool = False) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(bool [N]: the image lies wholly on land, the bytes, dist2).  cpu = from land_images_numpy instead of the GPU."""
    flags, dist2 = land_images_numpy(rects, segs, indent) if cpu else land_images_gpu(rects, segs, indent)
    return flags == ON_LAND, flags, dist2


# ---- files ----

def near_threshold(dist2, indent: float) -> int:
    """How many images have r cos(pi / 16) <= dist <= r / cos(pi / 16): the ring in which GEOS's 8-chord quarter circles can decide
    differently from the exact erosion."""
    r, c = float(indent), math.cos(math.pi / 16)
    d = np.sqrt(np.asarray(dist2, np.float64))
    return int(((d >= r * c) & (d <= r / c)).sum())


def write_csv(path: str, stems: Sequence[str], flags, dist2) -> int:
    """land_images.csv: image, on_land (True / False), inside (bit 1: the rectangle's south-west corner is inside the land), dist =
    sqrt(dist2) as ``repr``: the distance in metres from the rectangle to the nearest land edge, capped at twice the indent."""
    flags, dist2 = np.asarray(flags, np.uint8), np.asarray(dist2, np.float64)
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(CSV_COLUMNS)
        for k, s in enumerate(stems):
            w.writerow([s, "True" if flags[k] == ON_LAND else "False", "True" if flags[k] & 2 else "False", repr(float(math.sqrt(dist2[k])))])
    return len(stems)


def read_csv(path: str) -> Dict[str, list]:
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    return {"image": [r["image"] for r in rows], "on_land": [r["on_land"] == "True" for r in rows], "inside": [r["inside"] == "True" for r in rows],
            "dist": [float(r["dist"]) for r in rows]}


def summary(flags, dist2, indent: float, edges: int, device: str) -> dict:
    """What land_images.json holds."""
    flags = np.asarray(flags, np.uint8)
    return {"indent": float(indent), "images": int(flags.shape[0]), "on_land": int((flags == ON_LAND).sum()),
            "by_byte": {str(b): int((flags == b).sum()) for b in range(4)}, "land_edges": int(edges),
            "near_threshold": near_threshold(dist2, indent), "device": device}


def land_images_from_names(names: Sequence[str], wanted_bboxes_csv: str, land_geojson, out_csv: str, indent: float = INDENT, cpu: bool = False,
                           device: Optional[str] = None) -> dict:
    """The step as the command lines run it: the rectangles of `names` (compared without directory and extension; kfold.tile_rects on the
    --geocode-bboxes file), the land file (a path, or its segments), the marks, and the two files: `out_csv` and land_images.json beside it
    -> {"stems": the names' stems, "on_land": bool per name, "flags", "dist2", "summary"}."""
    from . import evaluate, kfold
    indent = _check_indent(indent)
    stems = [evaluate._stem(s) for s in names]
    rect_of = kfold.tile_rects(wanted_bboxes_csv)
    rects = np.asarray([rect_of(s) for s in stems], np.float64).reshape(-1, 4)
    segs = land.load_land_geojson(land_geojson) if isinstance(land_geojson, (str, os.PathLike)) else np.asarray(land_geojson, np.float64).reshape(-1, 4)
    mark, flags, dist2 = on_land(rects, segs, indent, cpu=cpu)
    if device is None:
        if cpu:
            device = "cpu"
        else:
            import torch
            device = torch.cuda.get_device_name()
    os.makedirs(os.path.dirname(os.path.abspath(out_csv)), exist_ok=True)
    write_csv(out_csv, stems, flags, dist2)
    s = summary(flags, dist2, indent, segs.shape[0], device)
    with open(os.path.join(os.path.dirname(os.path.abspath(out_csv)), JSON_FILE), "w") as f:
        json.dump(s, f, indent=1)
    return {"stems": stems, "on_land": mark, "flags": flags, "dist2": dist2, "summary": s}


def describe(res: dict) -> str:
    s = res["summary"]
    return (f"{s['on_land']} of {s['images']} images wholly on land, {s['indent']:g} m or more from the coast ({s['land_edges']} land edges; "
            f"{s['near_threshold']} within 2 % of the indent)")


def add_options(p) -> None:
    """The options detect.py and the evaluate command line share."""
    p.add_argument("--land-images", nargs="?", const="", default=None, metavar="CSV",
                   help="after the land filter, mark the images whose rectangles lie wholly on land, at least --land-images-indent metres from the "
                        "coast (the reference's mark_land_images, src/utils.py:46-69: within the land shrunk by buffer(-5)), the rectangle-to-edge "
                        f"distances on the GPU, and write {CSV_FILE} (default beside the other outputs) and {JSON_FILE}; with --evaluate-kfold those "
                        "images leave the image table before the splits are drawn and form the stratum `land`; needs the land file and "
                        "--geocode-bboxes")
    p.add_argument("--land-images-indent", type=float, default=INDENT, metavar="R", help="how far the land is shrunk, in EPSG:3857 metres (the reference: 5)")
