"""The non-blank polygon of partly blank tiles (``detect.py --blank-geom``).

After its white-space key the reference makes a third pass over the imagery (reference src/utils.py:453-466): for every tile marked
``partly blank`` it calls ``correct_partly_blank_geom`` (:482-530), which decodes the tile again, builds the mask ``max(R, G, B) < 250``,
polygonises its 8-connected components (``rasterio.features.shapes(..., connectivity=8)``), keeps the polygon whose exterior ring encloses
the largest area, maps it to the tile's bounds and simplifies it by 0.5.  A tile without any polygon is dropped as "actually blank".
Here the components, the winner and its ring's edges come from the decoded tile while it lies in HBM (csrc/blank_geom.hip,
engine.blank_components / engine.blank_ring_edges); this module is the host half:

    components_numpy   the literal restatement of the kernels in numpy and a union-find over row runs (documentation, CPU tests)
    ring_from_edges    the winner's outer edges chained into one closed walk of pixel corners
    to_bounds          rasterio.transform.from_bounds(west, south, east, north, 1024, 1024) + affine_transform
    simplify_dp        Douglas-Peucker on the closed ring
    PartFile, merge_parts, feature ...   the GeoJSON file, per-rank parts appended batch by batch as blank.PartFile's

Definitions (all integer-exact).  m = max(R, G, B) < 250.  Foreground components are the 8-connected components of m, background regions
the 4-connected components of ~m; every background region that touches the frame's border belongs to one "outside" region, as if the frame
stood in a one-pixel background border.  A label is the row-major index y w + x of the component's first pixel (outside: -1).  A unit edge
between a pixel of m and the outside region (or the frame's border) is an outer edge, and

    E(C) = sum over pixels (x, y) of C: (x + 1) [right neighbour is outside] - x [left neighbour is outside]

is the area inside C's exterior ring (pixels + holes + islands) when no other component encloses C, and smaller than its encloser's E
otherwise, so arg max E is the reference's ``max_poly`` (``Polygon(shape[0]["coordinates"][0]).area``).  Ties go to the smallest label.

Not pinned (neither rasterio / GDAL nor shapely is available to test against): the reference's tie order is rasterio's emission order; the
ring's start vertex and direction (here: the lexicographically smallest (y, x) vertex first, foreground on the right of every edge, which
is clockwise on the screen with y down); how GDAL walks a vertex where two diagonal foreground pixels meet (here: they are connected, the
ring is one walk that visits such a vertex twice); and the simplification: shapely's ``simplify(0.5)`` is GEOS's topology-preserving
Douglas-Peucker, ``simplify_dp`` is the plain one.  The exact, unsimplified pixel ring is therefore always written as well (``ring_px``).
"""
from __future__ import annotations

import glob
import json
import os
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import blank as aqblank

RECORD_FIELDS = ("examined", "n_components", "label", "px", "area_px", "x0", "y0", "x1", "y1", "n_edges", "edge_px", "reserved")   # aq_blank_geom
SIDE_N, SIDE_E, SIDE_S, SIDE_W = 1, 2, 4, 8            # side mask of an edge pixel: which of its four sides are outer edges
GEOM_FILE = "image_boxes_partly_blank.geojson"
IM_SIZE = 1024                                          # reference src/utils.py:18-19 (IM_WIDTH, IM_HEIGHT)
NOT_FG, OUTSIDE, NOT_BG = -1, -1, -2                    # label maps: foreground map off the mask; background map: outside region, on the mask


def _label_runs(m: np.ndarray, diagonal: bool) -> np.ndarray:
    """Components of the boolean image m (8-connected if `diagonal`, else 4-connected) -> int64 [h, w]: the row-major index of the
    component's first pixel, -1 off m.  Runs of each row, then a union-find over the runs of neighbouring rows (the smaller run number is
    the parent, so a root is the component's first run in row-major order)."""
    h, w = m.shape
    padded = np.zeros((h, w + 2), np.int8)
    padded[:, 1:-1] = m
    d = np.diff(padded, axis=1)
    ys, starts = np.nonzero(d == 1)
    ends = np.nonzero(d == -1)[1]                       # exclusive; same order as the starts (row-major)
    n = starts.shape[0]
    parent = list(range(n))

    def find(a):
        while parent[a] != a:
            parent[a] = parent[parent[a]]
            a = parent[a]
        return a

    first = np.searchsorted(ys, np.arange(h + 1))       # runs of row y: first[y] .. first[y + 1]
    s_, e_ = starts.tolist(), ends.tolist()
    reach = 1 if diagonal else 0
    for y in range(1, h):
        a, a_end, b, b_end = first[y - 1], first[y], first[y], first[y + 1]
        while a < a_end and b < b_end:
            if s_[a] < e_[b] + reach and e_[a] + reach > s_[b]:
                ra, rb = find(a), find(b)
                if ra != rb:
                    parent[max(ra, rb)] = min(ra, rb)
            if e_[a] < e_[b]:                           # the run that ends first cannot touch anything further right
                a += 1
            else:
                b += 1
    roots = np.asarray([find(a) for a in range(n)], np.int64)
    run_label = (ys * w + starts)[roots] if n else np.zeros(0, np.int64)
    out = np.full((h, w), -1, np.int64)
    out[m] = np.repeat(run_label, ends - starts)        # the pixels of m in row-major order are the runs one after the other
    return out


def components_numpy(img: np.ndarray = None, mask: np.ndarray = None) -> Dict[str, object]:
    """One uint8 RGB image [h, w, 3] (or its mask, bool [h, w]) -> what the kernels compute for it:
    ``mask``; ``fg`` int32 [h, w] (component label, NOT_FG off the mask); ``bg`` int32 [h, w] (region label, OUTSIDE for the outside
    region, NOT_BG on the mask); ``labels`` and ``areas`` (every component's label, ascending, and its E); ``record`` int32 [12]
    (RECORD_FIELDS, examined = 1; no component: label -1, the empty box w, h, -1, -1); ``edges`` int32 [edge_px, 2]: (pixel index,
    side mask) of every winner pixel with an outer edge, ascending."""
    if mask is None:
        img = np.asarray(img)
        assert img.dtype == np.uint8 and img.ndim == 3 and img.shape[2] == 3
        mask = img.max(axis=2) < 250
    m = np.asarray(mask, bool)
    h, w = m.shape
    assert h > 0 and w > 0
    fg = _label_runs(m, True)
    comp = np.ones((h + 2, w + 2), bool)                # the complement inside a one-pixel background border
    comp[1:-1, 1:-1] = ~m
    lab = _label_runs(comp, False)                      # the border's region has label 0 (its first pixel)
    inner = lab[1:-1, 1:-1]
    outside = np.ones((h + 2, w + 2), bool)
    outside[1:-1, 1:-1] = inner == 0
    py, px = np.divmod(inner, w + 2)
    bg = np.where(m, NOT_BG, np.where(inner == 0, OUTSIDE, (py - 1) * w + (px - 1)))
    ys, xs = np.nonzero(m)
    right, left = outside[ys + 1, xs + 2], outside[ys + 1, xs]
    up, down = outside[ys, xs + 1], outside[ys + 2, xs + 1]
    labels, inverse = np.unique(fg[ys, xs], return_inverse=True)
    contrib = (xs + 1) * right.astype(np.int64) - xs * left.astype(np.int64)
    areas = np.zeros(labels.shape[0], np.int64)
    np.add.at(areas, inverse, contrib)
    rec = np.zeros(len(RECORD_FIELDS), np.int64)
    rec[0], rec[1] = 1, labels.shape[0]
    edges = np.zeros((0, 2), np.int32)
    if labels.shape[0]:
        k = int(np.argmax(areas))                       # the first of equal maxima: labels ascend, so the smallest label
        win = inverse == k
        sides = (SIDE_N * up + SIDE_E * right + SIDE_S * down + SIDE_W * left)[win]
        wy, wx = ys[win], xs[win]
        on = sides > 0
        edges = np.stack([(wy * w + wx)[on], sides[on]], axis=1).astype(np.int32)
        n_edges = int(up[win].sum() + right[win].sum() + down[win].sum() + left[win].sum())
        rec[2:] = (labels[k], int(win.sum()), areas[k], wx.min(), wy.min(), wx.max(), wy.max(), n_edges, int(on.sum()), 0)
    else:
        rec[2:] = (-1, 0, 0, w, h, -1, -1, 0, 0, 0)
    return {"mask": m, "fg": fg.astype(np.int32), "bg": bg.astype(np.int32), "labels": labels.astype(np.int64), "areas": np.asarray(areas, np.int64),
            "record": rec.astype(np.int32), "edges": edges}


_STEP = {SIDE_N: (0, 0, 1, 0), SIDE_E: (1, 0, 1, 1), SIDE_S: (1, 1, 0, 1), SIDE_W: (0, 1, 0, 0)}     # side -> its edge (x, y) -> (x, y), relative to the pixel


def ring_from_edges(edges, w: int) -> List[Tuple[int, int]]:
    """(pixel index, side mask) rows of one component's outer edges (any order), frame width w -> the closed walk of pixel-corner vertices
    [(x, y), ...], first vertex repeated at the end, collinear runs merged; [] for no edges.  x to the right, y down (rasterio's frame with
    the identity transform).  Every unit edge has the foreground on its right; where two edges leave a vertex (two diagonal foreground
    pixels meet there) the walk turns left, which treats the two pixels as connected, so the ring is one walk that visits the vertex twice.
    The walk starts at the lexicographically smallest (y, x) vertex, on the edge that leaves it to the right: the result does not depend on
    the order of the rows.  Raises ValueError if the edges are not one closed walk."""
    e = np.asarray(edges, np.int64).reshape(-1, 2)
    if e.shape[0] == 0:
        return []
    out_of: Dict[Tuple[int, int], List[Tuple[int, int]]] = {}
    n_edges = 0
    for idx, sides in e.tolist():
        y, x = divmod(idx, w)
        for s, (ax, ay, bx, by) in _STEP.items():
            if sides & s:
                out_of.setdefault((x + ax, y + ay), []).append((bx - ax, by - ay))
                n_edges += 1
    start = min(out_of, key=lambda v: (v[1], v[0]))
    # at the topmost-leftmost vertex only the top edge of the pixel below and right of it leaves: direction (1, 0)
    at, d = start, (1, 0)
    if d not in out_of[start]:
        raise ValueError("outer edges: no edge leaves the first vertex to the right")
    ring = [start]
    used = 0
    while True:
        out_of[at].remove(d)
        used += 1
        at = (at[0] + d[0], at[1] + d[1])
        if at == start and not out_of[at]:
            break
        cands = out_of.get(at)
        if not cands:
            raise ValueError(f"outer edges: the walk ends at {at}")
        # preference: left turn, straight on, right turn (y down: left of (dx, dy) is (dy, -dx))
        for nd in ((d[1], -d[0]), d, (-d[1], d[0])):
            if nd in cands:
                break
        else:
            raise ValueError(f"outer edges: the walk turns back at {at}")
        if nd != d:
            ring.append(at)
        d = nd
    if used != n_edges:
        raise ValueError(f"outer edges: {n_edges - used} edges are not on the first closed walk")
    if ring[0] != ring[-1]:
        ring.append(start)
    return ring


def ring_area(ring: Sequence[Tuple[float, float]]) -> float:
    """Shoelace area of a closed ring, positive for the orientation ring_from_edges gives (sum of x dy)."""
    return sum((x0 + x1) * (y1 - y0) for (x0, y0), (x1, y1) in zip(ring[:-1], ring[1:])) / 2


def to_bounds(ring, west: float, south: float, east: float, north: float) -> List[Tuple[float, float]]:
    """Pixel-corner ring -> metres: rasterio.transform.from_bounds(west, south, east, north, width=1024, height=1024) followed by shapely's
    affine_transform (reference :525-527): x_m = west + px (east - west) / 1024, y_m = north - py (north - south) / 1024, with the
    reference's fixed 1024 whatever the image's real size."""
    a, e = (east - west) / IM_SIZE, (south - north) / IM_SIZE      # Affine.translation(west, north) * Affine.scale(a, e)
    return [(a * x + west, e * y + north) for x, y in ring]


def tile_bounds(name: str, wanted_bboxes: Dict[int, Tuple[float, float, float, float]]) -> Tuple[float, float, float, float]:
    """(west, south, east, north) in EPSG:3857 of the 1024-px tile `name` (<prefix><year>_<bbox_ind>_<x_offset>_<y_offset>[.ext]) inside its
    6144-px parent scene, by the arithmetic of geocode.geocode_detections."""
    from .geocode import IM_HEIGHT, IM_WIDTH, LARGE_TIF_SIZE
    _, ind, xo, yo = aqblank.name_fields(name)
    if ind == "":
        raise ValueError(f"tile name {name!r}: expected <prefix><year>_<bbox_ind>_<x_offset>_<y_offset>")
    if int(ind) not in wanted_bboxes:
        raise KeyError(f"bbox_ind {ind} not in the wanted_bboxes table")
    bx0, by0, bx1, by1 = wanted_bboxes[int(ind)]
    sx, sy = (bx1 - bx0) / LARGE_TIF_SIZE, (by1 - by0) / LARGE_TIF_SIZE
    return (int(xo) * sx + bx0, by1 - (int(yo) + IM_HEIGHT) * sy, (int(xo) + IM_WIDTH) * sx + bx0, by1 - int(yo) * sy)


def _dist(p, a, b) -> float:
    """Distance of point p from the segment a b."""
    (px, py), (ax, ay), (bx, by) = p, a, b
    dx, dy = bx - ax, by - ay
    den = dx * dx + dy * dy
    t = 0.0 if den == 0 else min(1.0, max(0.0, ((px - ax) * dx + (py - ay) * dy) / den))
    return float(np.hypot(px - (ax + t * dx), py - (ay + t * dy)))


def simplify_dp(ring, tol: float) -> List[Tuple[float, float]]:
    """Douglas-Peucker on a closed ring (first vertex repeated at the end): the ring is cut at its first vertex and at the vertex farthest
    from it, each half is simplified between its kept end points, a vertex being dropped only if the whole run it lies in stays within
    `tol` of the chord that replaces it.  tol <= 0 returns the ring as it is.  (The plain algorithm, not GEOS's topology-preserving one.)"""
    pts = [tuple(p) for p in ring]
    if tol <= 0 or len(pts) <= 4:
        return pts
    body = pts[:-1]
    far = max(range(len(body)), key=lambda i: (body[i][0] - body[0][0]) ** 2 + (body[i][1] - body[0][1]) ** 2)
    if far == 0:
        return pts
    keep = [False] * len(pts)
    keep[0] = keep[far] = keep[-1] = True
    stack = [(0, far), (far, len(pts) - 1)]
    while stack:
        i, j = stack.pop()
        if j <= i + 1:
            continue
        worst, at = -1.0, -1
        for k in range(i + 1, j):
            dk = _dist(pts[k], pts[i], pts[j])
            if dk > worst:
                worst, at = dk, k
        if worst > tol:
            keep[at] = True
            stack += [(i, at), (at, j)]
    return [p for p, k in zip(pts, keep) if k]


# ---- the GeoJSON file: per-rank parts, merged by rank 0 ----

def feature(name: str, record, ring_px, wanted_bboxes: Optional[Dict[int, Tuple[float, float, float, float]]] = None, tol: float = 0.5) -> dict:
    """One feature of the file: the tile's name fields, the winner's record and exact pixel ring as properties; the geometry is the ring in
    EPSG:3857 metres simplified by `tol` when the bounds table is given, else the pixel ring."""
    rec = dict(zip(RECORD_FIELDS, (int(v) for v in np.asarray(record).tolist())))
    year, ind, xo, yo = aqblank.name_fields(name)
    ring_px = [[int(x), int(y)] for x, y in ring_px]
    if wanted_bboxes is not None:
        coords = [[float(x), float(y)] for x, y in simplify_dp(to_bounds(ring_px, *tile_bounds(name, wanted_bboxes)), tol)]
    else:
        coords = ring_px
    return {"type": "Feature",
            "properties": {"image": os.path.basename(name), "year": year, "bbox_ind": ind, "x_offset": xo, "y_offset": yo,
                           "n_components": rec["n_components"], "px": rec["px"], "area_px": rec["area_px"],
                           "x0": rec["x0"], "y0": rec["y0"], "x1": rec["x1"], "y1": rec["y1"], "ring_px": ring_px},
            "geometry": {"type": "Polygon", "coordinates": [coords]}}


def feature_numpy(name: str, img: np.ndarray, wanted_bboxes=None, tol: float = 0.5) -> Optional[dict]:
    """The feature of one decoded tile computed on the host (components_numpy); None when the tile has no component."""
    c = components_numpy(img)
    if c["record"][1] == 0:
        return None
    return feature(name, c["record"], ring_from_edges(c["edges"], img.shape[1]), wanted_bboxes, tol)


def part_path(directory: str, rank: int) -> str:
    return os.path.join(directory, f"blank_geom.rank{rank}.jsonl")


class PartFile(aqblank.PartFile):
    """A rank's part, ``blank_geom.rank<r>.jsonl`` in the run directory: one ``<order>,<json>`` line per partly blank tile, the json being
    its feature, or ``null`` for a tile without a component ("actually blank").  Appending and durability as blank.PartFile's: the line is
    in the file (fsync'd when durable) before the done-manifest records the tile."""

    def __init__(self, directory: str, rank: int = 0):
        super().__init__(directory, rank)
        self.path = part_path(directory, rank)


def part_rows(names: Sequence[str], features: Sequence[Optional[dict]]) -> List[str]:
    """The part lines (without order and newline) of tiles and their features: {"image": name, "feature": feature or null}, keys sorted."""
    return [json.dumps({"image": os.path.basename(n), "feature": f}, sort_keys=True, separators=(",", ":")) for n, f in zip(names, features)]


def read_parts(directory: str) -> Dict[str, Tuple[int, Optional[dict]]]:
    """Every ``blank_geom.rank*.jsonl`` of the directory -> {image: (order, feature or None)}; a last line without its newline is
    ignored, an image that appears twice keeps its first row (the bytes are equal)."""
    found: Dict[str, Tuple[int, Optional[dict]]] = {}
    for path in sorted(glob.glob(os.path.join(directory, "blank_geom.rank*.jsonl"))):
        with open(path, "rb") as f:
            data = f.read()
        end = data.rfind(b"\n")
        if end < 0:
            continue
        for line in data[:end].decode().split("\n"):
            if not line:
                continue
            order, row = line.split(",", 1)
            rec = json.loads(row)
            found.setdefault(rec["image"], (int(order), rec["feature"]))
    return found


def merge_parts(directory: str, out_path: str, listing: Optional[Sequence[str]] = None, crs: Optional[str] = None) -> Dict[str, object]:
    """The GeoJSON file from the directory's part files: features in the order of the source listing (as blank.merge_parts orders the
    key's rows), one per line, written to a temporary file and renamed.  crs = the CRS name of the geometry (EPSG:3857 when the rings are
    in metres; none for pixel rings).  Returns {"features": n, "actually_blank": [image, ...]}."""
    place = {os.path.basename(n): i for i, n in enumerate(listing)} if listing is not None else {}
    rows = sorted(read_parts(directory).items(), key=lambda kv: (place.get(kv[0], len(place)), kv[1][0], kv[0]))
    feats = [json.dumps(f, sort_keys=True, separators=(",", ":")) for _, (_, f) in rows if f is not None]
    head = '{"type":"FeatureCollection",'
    if crs:
        head += '"crs":' + json.dumps({"type": "name", "properties": {"name": crs}}, sort_keys=True, separators=(",", ":")) + ","
    tmp = out_path + ".tmp"
    with open(tmp, "w", newline="") as f:
        f.write(head + '"features":[\n' + ",\n".join(feats) + ("\n" if feats else "") + "]}\n")
        f.flush()
        os.fsync(f.fileno())
    os.replace(tmp, out_path)
    return {"features": len(feats), "actually_blank": [image for image, (_, f) in rows if f is None]}
