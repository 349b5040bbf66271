"""Overlapping download boxes (``detect.py --dedup-overlaps``, ``python -m aquaculture_amd.overlaps``): every cage once.

reference src/utils.py:241-322.  The 1200 m download boxes of data/wanted_bboxes.csv overlap; a cage in an overlap is photographed, tiled
and detected once per box.  ``deduplicate_download_boxes`` gives box i the part of its rectangle that no earlier box of the file covers
(``overlay(how='difference')`` against the dissolved earlier regions) and drops a box that has nothing left;
``deduplicate_gdf_with_bboxes`` replaces every detection's polygon by its intersection with the region of its own box and drops the
detections whose intersection ``is_empty``.  The reference runs the pair right after geocoding (geocode_results.py:256-262), on the human
labels before the tuning grid (get_kfold_cluster_performance.py:55,62) and before the model-error fit and the area caps
(utils_tonnage.py:159-160, :945).

Everything here is axis-parallel rectangles in EPSG:3857, so the overlay is a rule of comparisons, with no arithmetic on coordinates:

  region of box i   C_i = the earlier boxes j < i whose open interiors meet R_i's (x0_j < x1_i && x1_j > x0_i, likewise in y).  xs = the sorted
                    distinct values of {x0_i, x1_i} and the x0_j, x1_j of C_i clamped into [x0_i, x1_i]; ys likewise.  Cell (a, b) =
                    [xs[a], xs[a+1]] x [ys[b], ys[b+1]] is covered iff some j of C_i has x0_j <= xs[a] && xs[a+1] <= x1_j and the same in y.
                    The region is the union of the uncovered cells; a box without one is dropped.
  detection D of i  state 0 dropped   no uncovered cell meets the closed D (xs[a] <= D.x1 && D.x0 <= xs[a+1], same in y)
                    state 1 whole     every cell whose open interior meets D's is uncovered (C_i empty: the common case)
                    state 2 clipped   an uncovered and a covered cell both meet D's open interior
                    state 3 touching  no uncovered cell meets D's open interior, but one meets the closed D: shapely's intersection is a line
                                      or a point, not ``is_empty``, so the reference keeps the row.  A D without area can only be 0 or 3.
                    Survivors: states 1, 2 and 3.
  values            for states 1 - 3, over the pieces cell ^ D of the uncovered cells that meet the closed D: clip_bounds = the min / max of
                    their corners (selections), clip_area = the sum of (min(x1) - max(x0)) * (min(y1) - max(y0)).  For state 0: NaN bounds,
                    area 0.

The values are taken on the cells of D's OWN grid: the grid of box i built from P(D), the partners of C_i that meet the closed D, only.  A
partner that does not meet the closed D covers no point of it, so the states and the bounds are those of the full grid (clip_literal takes
its state from the full grid of C_i, found by brute force, and the tests compare); but its edges would cut D's pieces differently, and a sum
of fp64 products depends on the cut.  The area's one written order: the rows of D's grid bottom to top, inside a row the cells left to
right added to a row sum that starts at 0, the row sums added to the area in row order.  clip_numpy walks D's grid as the kernel does (the
next edge after v = the smallest clamped partner edge above v) and gives the kernel's bytes; clip_literal sorts the edges and loops.

The kernels: csrc/overlaps.hip through engine.overlap_partners (the lists C_i, ascending, through horizontal bands) and engine.overlap_clip.

Downstream, a survivor keeps its FULL box: centroids, areas and joins use the detection as geocoded even in state 2, where the reference
goes on with the clipped polygon.  dedup_overlaps.json counts the rows this concerns (``clipped``).

Checked on the CPU against the reference's shipped data/wanted_bboxes_dedup.csv (a GeoJSON): the boxes without a region are exactly the ones
missing from that file, and the regions' rings are the shipped rings vertex for vertex (tests/test_overlaps.py on the overlapping subset,
tests/golden/g15_*).  The vertex lists of clipped detections (``clipped_geometry``: row strips) are NOT pinned: same point set as the
reference's intersection, GEOS's own vertex order and merging not reproduced.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import geocode
from .land import BOX_COLUMNS, table_boxes

DROPPED, WHOLE, CLIPPED, TOUCHING = 0, 1, 2, 3
STATE_NAMES = ("dropped", "whole", "clipped", "touching")
MAX_BANDS = 65536
DETECTIONS_FILE, REGIONS_FILE, SUMMARY_FILE = "dedup_detections.geojson", "wanted_bboxes_dedup.geojson", "dedup_overlaps.json"
CRS3857 = {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}


# ---- the box table ----

def load_boxes(path: str) -> Tuple[np.ndarray, np.ndarray]:
    """data/wanted_bboxes.csv -> (ids int64 [n], boxes float64 [n, 4] as x0, y0, x1, y1) in FILE ORDER, which is the priority: a box yields
    to every box before it."""
    table = geocode.load_wanted_bboxes(path)
    ids = np.fromiter(table.keys(), np.int64, len(table))
    return ids, np.asarray(list(table.values()), np.float64).reshape(-1, 4)


def box_rows(ids: np.ndarray, bbox_ind: np.ndarray, names: Sequence[str]) -> np.ndarray:
    """Row of the box table for every bbox_ind -> int32 [m].  A bbox_ind that is not in the table raises, naming the image it came from."""
    ids = np.asarray(ids, np.int64)
    bbox_ind = np.asarray(bbox_ind, np.int64).reshape(-1)
    if ids.shape[0] == 0:
        if bbox_ind.shape[0]:
            raise KeyError(f"overlaps: image {names[0]!r}: bbox_ind {int(bbox_ind[0])} is not in the box table (it is empty)")
        return np.zeros(0, np.int32)
    order = np.argsort(ids, kind="stable")
    pos = np.clip(np.searchsorted(ids[order], bbox_ind), 0, ids.shape[0] - 1)
    bad = np.nonzero(ids[order][pos] != bbox_ind)[0]
    if bad.size:
        k = int(bad[0])
        raise KeyError(f"overlaps: image {names[k]!r}: bbox_ind {int(bbox_ind[k])} is not in the box table")
    return order[pos].astype(np.int32)


# ---- the partner lists ----

def partners_numpy(boxes) -> Tuple[np.ndarray, np.ndarray]:
    """C_i for every box -> (start int64 [n + 1], partner int32 [start[n]]): box i's partners are partner[start[i] : start[i + 1]], ascending."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = b.shape[0]
    lists = []
    for i in range(n):
        e = b[:i]
        lists.append(np.nonzero((e[:, 0] < b[i, 2]) & (e[:, 2] > b[i, 0]) & (e[:, 1] < b[i, 3]) & (e[:, 3] > b[i, 1]))[0].astype(np.int32))
    start = np.zeros(n + 1, np.int64)
    if n:
        start[1:] = np.cumsum([l.shape[0] for l in lists])
    return start, (np.concatenate(lists) if lists else np.zeros(0, np.int32)).astype(np.int32)


def _band(y, Y0: float, h: float, nbands: int) -> np.ndarray:
    """floor((y - Y0) / h) clamped to [0, nbands): the kernel's expression (a NaN lands in band 0 there and here)."""
    with np.errstate(invalid="ignore"):
        t = np.floor((np.asarray(y, np.float64) - Y0) / h)
    return np.where(t >= 0.0, np.minimum(t, float(nbands - 1)), 0.0).astype(np.int64)


def band_table(boxes, nbands: Optional[int] = None) -> Dict[str, object]:
    """The search structure aq_overlap_partners_f64 takes: nbands horizontal bands of height h from Y0 = the smallest y0; box j is entered in
    every band from band(y0_j) to band(y1_j); entry_box int32 [entries] lists the boxes band by band, ascending inside a band, band_start
    int32 [nbands + 1] the bands' first entries.  nbands = None: bands as high as the highest box (a box then lies in two or three), at most
    65536 of them; a given count divides the y-extent evenly."""
    b = np.asarray(boxes, np.float64).reshape(-1, 4)
    n = b.shape[0]
    if n == 0:
        return {"entry_box": np.zeros(0, np.int32), "band_start": np.zeros(2, np.int32), "nbands": 1, "Y0": 0.0, "h": 1.0}
    if not np.isfinite(b).all():
        raise ValueError("overlaps: a box coordinate is not finite")
    Y0, top = float(b[:, 1].min()), float(b[:, 3].max())
    if nbands is None:
        h = float((b[:, 3] - b[:, 1]).max())
        if not h > 0:
            h = 1.0
        while (top - Y0) / h >= MAX_BANDS:
            h *= 2.0
        nbands = int(math.floor((top - Y0) / h)) + 1
    else:
        nbands = int(nbands)
        if nbands < 1:
            raise ValueError(f"overlaps: {nbands} bands (at least 1)")
        h = (top - Y0) / nbands
        if not h > 0:
            h = 1.0
    lo, hi = _band(b[:, 1], Y0, h, nbands), _band(b[:, 3], Y0, h, nbands)
    counts = hi - lo + 1
    entries = int(counts.sum())
    if entries >= 2 ** 31:
        raise ValueError(f"overlaps: {entries} band entries (fewer than 2^31 in one call): use fewer bands")
    box_of = np.repeat(np.arange(n, dtype=np.int64), counts)
    first = np.cumsum(counts) - counts
    band_of = lo[box_of] + (np.arange(entries, dtype=np.int64) - first[box_of])
    order = np.argsort(band_of, kind="stable")
    band_start = np.searchsorted(band_of[order], np.arange(nbands + 1))
    return {"entry_box": box_of[order].astype(np.int32), "band_start": band_start.astype(np.int32), "nbands": nbands, "Y0": Y0, "h": float(h)}


def partners_gpu(boxes, nbands: Optional[int] = None, times: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """partners_numpy's arrays from the GPU (engine.overlap_partners: host arrays in, host arrays out).  Raises without the library or a GPU."""
    import torch
    from . import engine
    b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
    t = band_table(b, nbands)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    start, partner = engine.overlap_partners(dev(b), dev(t["entry_box"]), dev(t["band_start"]), t["nbands"], t["Y0"], t["h"], times=times)
    return start.cpu().numpy(), partner.cpu().numpy()


# ---- the clip ----

def _clamp(c: float, lo: float, hi: float) -> float:
    return lo if c < lo else hi if c > hi else c


def _next_edge(cur: float, lo: float, hi: float, P: Sequence[Sequence[float]], k0: int, k1: int) -> float:
    """The smallest of hi and the partners' edges (coordinates k0 and k1, clamped into [lo, hi]) above cur."""
    best = hi
    for p in P:
        for c in (_clamp(p[k0], lo, hi), _clamp(p[k1], lo, hi)):
            if c > cur and c < best:
                best = c
    return best


def _walk(D, R, P, strips: Optional[list] = None):
    """D's grid, as the kernel walks it: D and R = (x0, y0, x1, y1) of the detection and of its box, P = the partners that meet the closed D.
    -> (state, (bx0, by0, bx1, by1), area).  strips = a list that receives the uncovered pieces with area, merged along every row:
    (x0, y0, x1, y1)."""
    dx0, dy0, dx1, dy1 = D
    lx, ly, hx, hy = R
    u_closed = u_open = c_open = False
    bx0 = by0 = math.inf
    bx1 = by1 = -math.inf
    area = 0.0
    ya = ly
    while ya < hy:
        yb = _next_edge(ya, ly, hy, P, 1, 3)
        if ya <= dy1 and dy0 <= yb:
            row = 0.0
            run = None
            xa = lx
            while xa < hx:
                xb = _next_edge(xa, lx, hx, P, 0, 2)
                if xa <= dx1 and dx0 <= xb:
                    covered = False
                    for p in P:
                        if p[0] <= xa and xb <= p[2] and p[1] <= ya and yb <= p[3]:
                            covered = True
                            break
                    px0, px1 = (xa if xa > dx0 else dx0), (xb if xb < dx1 else dx1)
                    py0, py1 = (ya if ya > dy0 else dy0), (yb if yb < dy1 else dy1)
                    opens = px0 < px1 and py0 < py1
                    if covered:
                        c_open = c_open or opens
                    else:
                        u_closed = True
                        u_open = u_open or opens
                        bx0, by0 = (px0 if px0 < bx0 else bx0), (py0 if py0 < by0 else by0)
                        bx1, by1 = (px1 if px1 > bx1 else bx1), (py1 if py1 > by1 else by1)
                        row = row + (px1 - px0) * (py1 - py0)
                        if strips is not None and opens:
                            if run is not None and run[2] == px0:
                                run[2] = px1
                            else:
                                run = [px0, py0, px1, py1]
                                strips.append(run)
                xa = xb
            area = area + row
        ya = yb
    if not u_closed:
        return DROPPED, (math.nan,) * 4, 0.0
    state = CLIPPED if u_open and c_open else WHOLE if u_open else TOUCHING
    return state, (bx0, by0, bx1, by1), area


def _check_inputs(boxes, det_row, dets):
    b = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
    r = np.ascontiguousarray(np.asarray(det_row, np.int32).reshape(-1))
    d = np.ascontiguousarray(np.asarray(dets, np.float64).reshape(-1, 4))
    if r.shape[0] != d.shape[0]:
        raise ValueError(f"overlaps: {r.shape[0]} box rows for {d.shape[0]} detections")
    if r.size and (r.min() < 0 or r.max() >= b.shape[0]):
        raise ValueError(f"overlaps: a detection's box row is outside the {b.shape[0]} boxes")
    return b, r, d


def clip_numpy(boxes, start, partner, det_row, dets) -> Dict[str, np.ndarray]:
    """The kernel's steps on the host -> {"state" uint8 [m], "clip_bounds" float64 [m, 4], "clip_area" float64 [m], "has_region" uint8 [n]}:
    the same bytes as engine.overlap_clip.  boxes [n, 4], (start, partner) the partner lists, det_row int32 [m] the detections' box rows,
    dets [m, 4] their boxes.  A detection none of whose box's partners meets it closed is settled against the one cell of its box, all at
    once; the others walk their grid one by one."""
    b, r, d = _check_inputs(boxes, det_row, dets)
    start, partner = np.asarray(start, np.int64), np.asarray(partner, np.int64)
    n, m = b.shape[0], d.shape[0]
    has = np.zeros(n, np.uint8)
    for i in range(n):
        P = b[partner[start[i]:start[i + 1]]].tolist()
        has[i] = _walk(b[i].tolist(), b[i].tolist(), P)[0] != DROPPED
    state = np.zeros(m, np.uint8)
    bounds = np.full((m, 4), np.nan)
    area = np.zeros(m, np.float64)
    if m == 0:
        return {"state": state, "clip_bounds": bounds, "clip_area": area, "has_region": has}
    R = b[r]
    lonely = (start[r.astype(np.int64) + 1] - start[r]) == 0
    # the one cell of a box without partners: the walk's comparisons on whole arrays
    px0, px1 = np.where(R[:, 0] > d[:, 0], R[:, 0], d[:, 0]), np.where(R[:, 2] < d[:, 2], R[:, 2], d[:, 2])
    py0, py1 = np.where(R[:, 1] > d[:, 1], R[:, 1], d[:, 1]), np.where(R[:, 3] < d[:, 3], R[:, 3], d[:, 3])
    closed = (R[:, 0] < R[:, 2]) & (R[:, 1] < R[:, 3]) & (R[:, 0] <= d[:, 2]) & (d[:, 0] <= R[:, 2]) & (R[:, 1] <= d[:, 3]) & (d[:, 1] <= R[:, 3])
    opens = (px0 < px1) & (py0 < py1)
    one = lonely & closed
    state[one] = np.where(opens[one], WHOLE, TOUCHING)
    bounds[one] = np.stack([px0, py0, px1, py1], 1)[one]
    with np.errstate(invalid="ignore"):
        area[one] = (0.0 + (px1 - px0) * (py1 - py0))[one]
    for k in np.nonzero(~lonely)[0].tolist():
        i = int(r[k])
        D = d[k].tolist()
        P = [p for p in b[partner[start[i]:start[i + 1]]].tolist() if p[0] <= D[2] and D[0] <= p[2] and p[1] <= D[3] and D[1] <= p[3]]
        state[k], bounds[k], area[k] = _walk(D, b[i].tolist(), P)
    return {"state": state, "clip_bounds": bounds, "clip_area": area, "has_region": has}


def _grid(R, C):
    xs = sorted({R[0], R[2]} | {_clamp(c, R[0], R[2]) for p in C for c in (p[0], p[2])})
    ys = sorted({R[1], R[3]} | {_clamp(c, R[1], R[3]) for p in C for c in (p[1], p[3])})
    return xs, ys


def _cells(R, C):
    """Every cell of box R's grid over the boxes C: (x0, y0, x1, y1, covered), b outer, a inner."""
    xs, ys = _grid(R, C)
    for b_ in range(len(ys) - 1):
        for a in range(len(xs) - 1):
            x0, x1, y0, y1 = xs[a], xs[a + 1], ys[b_], ys[b_ + 1]
            yield x0, y0, x1, y1, any(p[0] <= x0 and x1 <= p[2] and p[1] <= y0 and y1 <= p[3] for p in C)


def _state(cells, D) -> int:
    u_closed = u_open = c_open = False
    for x0, y0, x1, y1, covered in cells:
        closed = x0 <= D[2] and D[0] <= x1 and y0 <= D[3] and D[1] <= y1
        opens = max(x0, D[0]) < min(x1, D[2]) and max(y0, D[1]) < min(y1, D[3])
        u_closed |= closed and not covered
        u_open |= opens and not covered
        c_open |= opens and covered
    return DROPPED if not u_closed else CLIPPED if u_open and c_open else WHOLE if u_open else TOUCHING


def clip_literal(boxes, det_row, dets) -> Dict[str, np.ndarray]:
    """The rule of the module's docstring in plain loops, one detection at a time, with nothing shared with clip_numpy: C_i by comparing with
    every earlier box, the grids by sorting, the state on the FULL grid of C_i, the values on D's own grid (and the state there has to be
    the same one: asserted).  Same dictionary as clip_numpy."""
    b, r, d = _check_inputs(boxes, det_row, dets)
    B = b.tolist()
    n, m = len(B), d.shape[0]
    C = [[B[j] for j in range(i) if B[j][0] < B[i][2] and B[j][2] > B[i][0] and B[j][1] < B[i][3] and B[j][3] > B[i][1]] for i in range(n)]
    has = np.asarray([any(not c[4] for c in _cells(B[i], C[i])) for i in range(n)], np.uint8).reshape(n)
    state = np.zeros(m, np.uint8)
    bounds = np.full((m, 4), np.nan)
    area = np.zeros(m, np.float64)
    for k in range(m):
        i, D = int(r[k]), d[k].tolist()
        s = _state(_cells(B[i], C[i]), D)
        if not has[i]:
            assert s == DROPPED
        P = [p for p in C[i] if p[0] <= D[2] and D[0] <= p[2] and p[1] <= D[3] and D[1] <= p[3]]
        own = list(_cells(B[i], P))
        assert _state(own, D) == s, "the state on D's own grid is not the state on the box's grid"
        state[k] = s
        if s == DROPPED:
            continue
        pieces = [(max(x0, D[0]), max(y0, D[1]), min(x1, D[2]), min(y1, D[3])) for x0, y0, x1, y1, covered in own
                  if not covered and x0 <= D[2] and D[0] <= x1 and y0 <= D[3] and D[1] <= y1]
        rows: Dict[float, float] = {}
        for x0, y0, x1, y1, covered in own:                 # a row that meets the closed D adds its sum, were it 0
            if y0 <= D[3] and D[1] <= y1:
                rows.setdefault(y0, 0.0)
                if not covered and x0 <= D[2] and D[0] <= x1:
                    rows[y0] = rows[y0] + (min(x1, D[2]) - max(x0, D[0])) * (min(y1, D[3]) - max(y0, D[1]))
        total = 0.0
        for y0 in sorted(rows):
            total = total + rows[y0]
        bounds[k] = (min(p[0] for p in pieces), min(p[1] for p in pieces), max(p[2] for p in pieces), max(p[3] for p in pieces))
        area[k] = total
    return {"state": state, "clip_bounds": bounds, "clip_area": area, "has_region": has}


def clip_gpu(boxes, start, partner, det_row, dets, times: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """clip_numpy's dictionary from the GPU (engine.overlap_clip).  Raises without the library or a GPU."""
    import torch
    from . import engine
    b, r, d = _check_inputs(boxes, det_row, dets)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    out = engine.overlap_clip(dev(b), dev(np.asarray(start, np.int64)), dev(np.asarray(partner, np.int32)), dev(r), dev(d), times=times)
    return {k: v.cpu().numpy() for k, v in zip(("state", "clip_bounds", "clip_area", "has_region"), out)}


def clip(boxes, det_row, dets, cpu: bool = False, times: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """Partner lists and clip in one call, on the GPU or (cpu) in numpy -> clip_numpy's dictionary plus "start" and "partner"."""
    start, partner = partners_numpy(boxes) if cpu else partners_gpu(boxes, times=times)
    out = (clip_numpy if cpu else clip_gpu)(boxes, start, partner, det_row, dets, **({} if cpu else {"times": times}))
    out["start"], out["partner"] = start, partner
    return out


def survivors(state) -> np.ndarray:
    """bool [m]: the rows the reference keeps (states 1, 2 and 3)."""
    return np.asarray(state) != DROPPED


# ---- the regions ----

def _rings(U: np.ndarray, xs: List[float], ys: List[float]) -> List[List[List[List[float]]]]:
    """The polygons of the uncovered cells U[b][a]: the cells' boundary edges, directed with the region on their left, chained into rings
    (at a vertex where two cells meet diagonally the walk turns left, so such cells stay separate polygons), collinear vertices removed.
    -> a list of polygons, each [exterior (counter-clockwise), holes (clockwise) ...], rings closed."""
    nb, na = U.shape
    comp = -np.ones((nb, na), np.int64)
    ncomp = 0
    for b0 in range(nb):
        for a0 in range(na):
            if U[b0, a0] and comp[b0, a0] < 0:
                stack = [(b0, a0)]
                comp[b0, a0] = ncomp
                while stack:
                    b_, a = stack.pop()
                    for bb, aa in ((b_ + 1, a), (b_ - 1, a), (b_, a + 1), (b_, a - 1)):
                        if 0 <= bb < nb and 0 <= aa < na and U[bb, aa] and comp[bb, aa] < 0:
                            comp[bb, aa] = ncomp
                            stack.append((bb, aa))
                ncomp += 1
    inside = lambda b_, a: 0 <= b_ < nb and 0 <= a < na and bool(U[b_, a])
    edges: Dict[Tuple[int, int], List[Tuple[int, int, int]]] = {}      # from vertex (a, b) -> [(to a, to b, component)]
    for b_ in range(nb):
        for a in range(na):
            if not U[b_, a]:
                continue
            c = int(comp[b_, a])
            if not inside(b_ - 1, a):
                edges.setdefault((a, b_), []).append((a + 1, b_, c))                # bottom, eastwards
            if not inside(b_, a + 1):
                edges.setdefault((a + 1, b_), []).append((a + 1, b_ + 1, c))        # right, northwards
            if not inside(b_ + 1, a):
                edges.setdefault((a + 1, b_ + 1), []).append((a, b_ + 1, c))        # top, westwards
            if not inside(b_, a - 1):
                edges.setdefault((a, b_ + 1), []).append((a, b_, c))                # left, southwards
    polys: List[List[List[List[float]]]] = [[] for _ in range(ncomp)]
    for v0 in sorted(edges):
        while edges.get(v0):
            ta, tb, c = edges[v0].pop()
            ring, prev, cur = [v0], v0, (ta, tb)
            while cur != v0:
                ring.append(cur)
                outs = edges[cur]
                din = (cur[0] - prev[0], cur[1] - prev[1])
                left = (-din[1], din[0])
                pick = max(range(len(outs)), key=lambda q: ((outs[q][0] - cur[0], outs[q][1] - cur[1]) == left, outs[q][2] == c))
                na_, nb_, _ = outs.pop(pick)
                prev, cur = cur, (na_, nb_)
            k = len(ring)
            keep = [q for q in range(k) if (ring[q][0] - ring[q - 1][0], ring[q][1] - ring[q - 1][1]) !=
                    (ring[(q + 1) % k][0] - ring[q][0], ring[(q + 1) % k][1] - ring[q][1])]
            pts = [[xs[ring[q][0]], ys[ring[q][1]]] for q in keep]
            twice = sum(p[0] * q[1] - q[0] * p[1] for p, q in zip(ring, ring[1:] + ring[:1]))       # on the cell indices: exact
            pts.append(list(pts[0]))
            if twice > 0:
                polys[c].insert(0, pts)
            else:
                polys[c].append(pts)
    return polys


def regions(boxes) -> List[Optional[dict]]:
    """The reference's de-duplicated box polygons: for every box its region as a GeoJSON geometry in EPSG:3857 -- a Polygon, a MultiPolygon
    where the uncovered cells fall apart (cells that meet only at a corner are separate polygons), or None for a box that is dropped.
    Exterior rings run counter-clockwise, holes clockwise, without collinear vertices."""
    B = np.asarray(boxes, np.float64).reshape(-1, 4).tolist()
    start, partner = partners_numpy(B)
    out: List[Optional[dict]] = []
    for i, R in enumerate(B):
        C = [B[j] for j in partner[start[i]:start[i + 1]].tolist()]
        xs, ys = _grid(R, C)
        if len(xs) < 2 or len(ys) < 2:
            out.append(None)
            continue
        U = np.asarray([not c[4] for c in _cells(R, C)], bool).reshape(len(ys) - 1, len(xs) - 1)
        polys = _rings(U, xs, ys)
        out.append(None if not polys else {"type": "Polygon", "coordinates": polys[0]} if len(polys) == 1 else
                   {"type": "MultiPolygon", "coordinates": polys})
    return out


def region_area(boxes, i: int) -> float:
    """Area of box i's region as a plain sum over its uncovered cells, row by row."""
    B = np.asarray(boxes, np.float64).reshape(-1, 4).tolist()
    C = [p for p in B[:i] if p[0] < B[i][2] and p[2] > B[i][0] and p[1] < B[i][3] and p[3] > B[i][1]]
    return float(sum((x1 - x0) * (y1 - y0) for x0, y0, x1, y1, covered in _cells(B[i], C) if not covered))


def clipped_geometry(D, R, P) -> dict:
    """A clipped detection's survivors' geometry in EPSG:3857: the uncovered pieces with area, merged along each row of D's grid into strips.
    The same point set as the reference's intersection up to its lines and points; the vertex lists are this module's own."""
    strips: List[List[float]] = []
    _walk(list(D), list(R), [list(p) for p in P], strips)
    rings = [[[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]] for x0, y0, x1, y1 in strips]
    return {"type": "Polygon", "coordinates": rings[0]} if len(rings) == 1 else {"type": "MultiPolygon", "coordinates": rings}


# ---- tables and files ----

def table_rows(table: Dict[str, np.ndarray], ids: np.ndarray) -> np.ndarray:
    """The box rows of a geocoded table's detections (bbox_ind from geocode.parse_stems of the image names)."""
    stems = [str(s) for s in table["stems"]]
    ind = geocode.parse_stems(stems)[0] if stems else np.zeros(0, np.int64)
    img = np.asarray(table["image"], np.int64)
    return box_rows(ids, ind[img], [stems[int(k)] + ".jpeg" for k in img])


def clip_table(table: Dict[str, np.ndarray], bboxes_csv: str, cpu: bool = False) -> Dict[str, object]:
    """The whole step for a geocoded table -> clip()'s dictionary plus "ids", "boxes", "det_row", "device" and "times" (seconds)."""
    ids, boxes = load_boxes(bboxes_csv)
    rows = table_rows(table, ids)
    times: Dict[str, float] = {}
    t0 = time.perf_counter()
    out: Dict[str, object] = dict(clip(boxes, rows, table_boxes(table), cpu=cpu, times=times))
    times["clip_s"] = time.perf_counter() - t0
    out.update(ids=ids, boxes=boxes, det_row=rows, device="cpu" if cpu else "gpu", times=times)
    return out


def _label_stem(name: str) -> str:
    base, ext = os.path.splitext(os.path.basename(str(name)))
    return base if ext.lower() in (".jpeg", ".jpg", ".png", ".tif", ".tiff") else base + ext


def truth_rows(truth: Dict[str, np.ndarray], bboxes_csv: str, cpu: bool = False) -> np.ndarray:
    """bool [L]: the labels the reference keeps (get_kfold_cluster_performance.py:55,62; utils_tonnage.py:159-160): their
    xmin_3857 .. ymax_3857 rectangles through the same clip, the bbox_ind from the label's image name.  truth:
    evaluate.load_truth_geojson's columns."""
    ids, boxes = load_boxes(bboxes_csv)
    names = [str(s) for s in truth["image"]]
    ind = geocode.parse_stems([_label_stem(s) for s in names])[0] if names else np.zeros(0, np.int64)
    return survivors(clip(boxes, box_rows(ids, ind, names), table_boxes(truth), cpu=cpu)["state"])


def filter_truth(truth: Dict[str, np.ndarray], bboxes_csv: Optional[str], cpu: bool = False) -> Dict[str, np.ndarray]:
    """The label columns without the labels in state 0 (bboxes_csv = None: as they are).  What --evaluate, --evaluate-kfold and
    --model-errors do to their truth boxes under --dedup-overlaps."""
    if bboxes_csv is None:
        return truth
    keep = truth_rows(truth, bboxes_csv, cpu=cpu)
    n = keep.shape[0]
    return {k: (np.asarray(v)[keep] if isinstance(v, np.ndarray) and v.shape[:1] == (n,) else v) for k, v in truth.items()}


def summary(res: Dict[str, object]) -> dict:
    state = np.asarray(res["state"])
    start = np.asarray(res["start"])
    counts = np.bincount(state, minlength=4)
    return {"detections": int(state.shape[0]), "survivors": int(survivors(state).sum()),
            "states": {name: int(counts[k]) for k, name in enumerate(STATE_NAMES)},
            "clipped_rows_keep_full_box": int(counts[CLIPPED]),
            "boxes": int(np.asarray(res["boxes"]).shape[0]), "boxes_dropped": int((np.asarray(res["has_region"]) == 0).sum()),
            "boxes_with_partners": int((np.diff(start) > 0).sum()), "partners_max": int(np.diff(start).max()) if start.shape[0] > 1 else 0,
            "device": res["device"], "times": {k: float(v) for k, v in dict(res["times"]).items()}}


def write_files(out_dir: str, table: Dict[str, np.ndarray], res: Dict[str, object]) -> dict:
    """dedup_detections.geojson (the survivors as geocode.write_geojson writes them, each with ``index`` = its row in detections.geojson,
    ``clip_state`` and ``clip_area``; a clipped one with its strips as geometry, in longitude / latitude like the rest),
    wanted_bboxes_dedup.geojson (bbox_ind + region in EPSG:3857: what the reference's scripts read as wanted_bboxes_dedup.csv) and
    dedup_overlaps.json.  Returns the summary."""
    os.makedirs(out_dir, exist_ok=True)
    stems = table["stems"]
    state, area, boxes = np.asarray(res["state"]), np.asarray(res["clip_area"]), np.asarray(res["boxes"])
    start, partner, rows = np.asarray(res["start"]), np.asarray(res["partner"]), np.asarray(res["det_row"])
    dets = table_boxes(table)
    feats = []
    for k in np.nonzero(survivors(state))[0].tolist():
        f = geocode.feature(stems, table, k)
        f["properties"] = {"index": k, **f["properties"], "clip_state": int(state[k]), "clip_area": float(area[k])}
        if state[k] == CLIPPED:
            i, D = int(rows[k]), dets[k].tolist()
            P = [p for p in boxes[partner[start[i]:start[i + 1]]].tolist() if p[0] <= D[2] and D[0] <= p[2] and p[1] <= D[3] and D[1] <= p[3]]
            g = clipped_geometry(D, boxes[i].tolist(), P)
            lonlat = lambda ring: [[float(v) for v in geocode.mercator_to_lonlat(np.float64(x), np.float64(y))] for x, y in ring]
            g["coordinates"] = ([lonlat(r_) for r_ in g["coordinates"]] if g["type"] == "Polygon" else
                                [[lonlat(r_) for r_ in poly] for poly in g["coordinates"]])
            f["geometry"] = g
        feats.append(f)
    with open(os.path.join(out_dir, DETECTIONS_FILE), "w") as f:
        json.dump({"type": "FeatureCollection", "crs": geocode.CRS84, "features": feats}, f)
    reg = regions(boxes)
    with open(os.path.join(out_dir, REGIONS_FILE), "w") as f:
        json.dump({"type": "FeatureCollection", "crs": CRS3857,
                   "features": [{"type": "Feature", "properties": {"bbox_ind": int(i)}, "geometry": g} for i, g in zip(res["ids"], reg) if g is not None]}, f)
    s = summary(res)
    with open(os.path.join(out_dir, SUMMARY_FILE), "w") as f:
        json.dump(s, f, indent=1)
    return s


def describe(s: dict) -> str:
    st = s["states"]
    return (f"{s['survivors']} of {s['detections']} detections kept ({st['whole']} whole, {st['clipped']} clipped, {st['touching']} touching, "
            f"{st['dropped']} dropped); {s['boxes_dropped']} of {s['boxes']} boxes have no region, at most {s['partners_max']} earlier partners")


def dedup_from_table(table: Dict[str, np.ndarray], bboxes_csv: str, out_dir: str, cpu: bool = False) -> Dict[str, object]:
    """detect.py's step: clip, write the three files -> {"keep" bool [n], "summary", "result"}."""
    res = clip_table(table, bboxes_csv, cpu=cpu)
    s = write_files(out_dir, table, res)
    return {"keep": survivors(res["state"]), "summary": s, "result": res}


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.overlaps",
                                description="Count every cage of an existing label directory once where the download boxes overlap, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv (file order is the priority)")
    p.add_argument("--out", default=None, metavar="DIR", help="default <labels>/..")
    p.add_argument("--cpu", action="store_true", help="partner lists and clip from the numpy restatement instead of the GPU")
    opt = p.parse_args(argv)
    out = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    dd = dedup_from_table(table, opt.geocode_bboxes, out, cpu=opt.cpu)
    print(f"{describe(dd['summary'])} in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
