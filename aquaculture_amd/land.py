"""The land filter (``detect.py --land-filter``, ``python -m aquaculture_amd.land``): ocean_detections.geojson from detections.geojson.
(``python -m aquaculture_amd.land --images FILE`` is the images' counterpart, land_images.py: which images lie wholly on land.)

reference src/process_yolo/geocode_results.py:200-218 (remove_land_detections): ``detections.sjoin(french_land, how='inner')`` with the
default predicate ``intersects`` drops every detection whose box intersects the land polygon; what is left is saved with ``index=True`` as
ocean_detections.geojson, which every later step of the reference reads (calc_net_areas.py:164-170, utils_tonnage.py:952,
Results/tonnage_estimates.py:47).  Here the test runs in EPSG:3857 on the table's xmin_3857 .. ymax_3857 boxes against the segments
(ax, ay, bx, by) of all rings of the land, exterior and holes alike, and gives one byte per box:

  bit 0    some segment meets the closed box: the two bounding boxes overlap (closed comparisons) and the box's four corners are not all
           strictly on one side of the segment's line.  The side is the sign of orient(a, b, c) = (bx - ax) (cy - ay) - (by - ay) (cx - ax),
           evaluated in fp64 in exactly that form; a segment of no length is then a point-in-box test, with no special case.
  bit 1    the corner (x0, y0) is inside the land under the even-odd rule over all rings: the parity of the segments with
           (ay <= y0) != (by <= y0) (half-open in y) that have the corner strictly on their left if they go up, strictly on their right
           if they go down, again by the sign of orient.

A box that no ring edge meets lies wholly inside or wholly outside the land, so ``byte != 0`` is ``intersects``, and touching counts as
intersecting.  The bytes come from the GPU (csrc/land_filter.hip through engine.land_flags) or, without one, from land_flags_numpy; both
evaluate the same expressions and give the same bytes.

NOT pinned, for want of GEOS / shapely / geopandas on the machines this was written on:
  * the comparison with shapely's ``intersects`` itself.  Agreement is claimed where exact arithmetic is away from determinant ties (the
    tests compare with a definition written as a double loop and, for polygons without holes, with matplotlib's Path.intersects_bbox), and
    at exact ties only with the touch rule above.  GEOS's robust predicates may decide differently from fp64 for a box edge within rounding
    of a coastline vertex.
  * the size of the real land shapefile (france_final_land_filter.shp is not here): the band table's defaults are sized for 1e5 to 1e6
    vertices by estimate, not by measurement.
  * the reference joins in the detections' CRS at that point of its main (EPSG:4326 after to_crs); boxes are axis-parallel in both, the
    land's edges are straight in the CRS they are tested in, here EPSG:3857.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import geocode

BOX_COLUMNS = ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857")
_LONLAT = ("urn:ogc:def:crs:OGC:1.3:CRS84", "urn:ogc:def:crs:OGC::CRS84", "urn:ogc:def:crs:EPSG::4326", "EPSG:4326", "OGC:CRS84", "CRS84", "WGS84")
_MERCATOR = ("urn:ogc:def:crs:EPSG::3857", "EPSG:3857", "urn:ogc:def:crs:EPSG::900913", "EPSG:900913")


# ---- the land file ----

def _polygons(obj, path: str) -> List[list]:
    """The coordinate arrays of all polygons of a GeoJSON object, in file order."""
    t = obj.get("type") if isinstance(obj, dict) else None
    if t == "Polygon":
        return [obj["coordinates"]]
    if t == "MultiPolygon":
        return list(obj["coordinates"])
    if t == "Feature":
        return _polygons(obj["geometry"], path) if obj.get("geometry") is not None else []
    if t == "FeatureCollection":
        return [p for f in obj["features"] for p in _polygons(f, path)]
    if t == "GeometryCollection":
        return [p for g in obj["geometries"] for p in _polygons(g, path)]
    if t in ("Point", "MultiPoint", "LineString", "MultiLineString"):
        return []                                           # no area: nothing a box can be inside of (the reference's file holds polygons only)
    raise ValueError(f"{path}: not a GeoJSON geometry, Feature or collection (type {t!r})")


def load_land_geojson(path: str) -> np.ndarray:
    """The land polygons of a GeoJSON file -> float64 [E, 4] segments (ax, ay, bx, by) in EPSG:3857: every edge of every ring (holes
    included) of every Polygon / MultiPolygon, bare or inside Features, a FeatureCollection or GeometryCollections.  Without a ``crs`` member,
    or with CRS84 / EPSG:4326, the vertices are longitude, latitude and go through geocode.lonlat_to_mercator one by one, as
    GeoDataFrame.to_crs does; EPSG:3857 is taken as it is; any other CRS raises, by name.  A ring the file left open is closed.
    (A shapefile: ``ogr2ogr -f GeoJSON land.geojson france_final_land_filter.shp`` first; there is no .shp reader here.)"""
    with open(path) as f:
        doc = json.load(f)
    crs = doc.get("crs") if isinstance(doc, dict) else None
    name = None
    if crs is not None:
        name = (crs.get("properties") or {}).get("name") if isinstance(crs, dict) else None
        if name is None:
            raise ValueError(f"{path}: a crs member without a name: {crs!r}")
    if name is None or name in _LONLAT:
        project = True
    elif name in _MERCATOR:
        project = False
    else:
        raise ValueError(f"{path}: CRS {name} is neither longitude / latitude (CRS84, EPSG:4326) nor EPSG:3857; re-project the file first")
    segs = []
    for poly in _polygons(doc, path):
        for ring in poly:
            r = np.asarray(ring, np.float64)
            if r.size == 0:
                continue
            if r.ndim != 2 or r.shape[1] < 2:
                raise ValueError(f"{path}: a ring is not a list of positions")
            r = r[:, :2]
            if not np.array_equal(r[0], r[-1]):
                r = np.concatenate([r, r[:1]], 0)
            if project:
                x, y = geocode.lonlat_to_mercator(r[:, 0], r[:, 1])
                r = np.stack([x, y], 1)
            segs.append(np.concatenate([r[:-1], r[1:]], 1))
    out = np.concatenate(segs, 0) if segs else np.zeros((0, 4), np.float64)
    if not np.isfinite(out).all():
        raise ValueError(f"{path}: a vertex is not finite in EPSG:3857 (a latitude of +-90?)")
    return np.ascontiguousarray(out)


# ---- the flags ----

def _orient(ax, ay, bx, by, cx, cy):
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax)


def land_flags_numpy(boxes, segs, chunk_pairs: int = 1 << 21) -> np.ndarray:
    """The rule set of the module's docstring in numpy -> uint8 [N]: every box against every segment, `chunk_pairs` pairs at a time (about
    150 bytes of temporaries per pair).  For ``--cpu`` and the tests; the GPU path has a search structure, this has none."""
    boxes = np.asarray(boxes, np.float64).reshape(-1, 4)
    segs = np.asarray(segs, np.float64).reshape(-1, 4)
    n, E = boxes.shape[0], segs.shape[0]
    out = np.zeros(n, np.uint8)
    if n == 0 or E == 0:
        return out
    ax, ay, bx, by = (segs[None, :, k] for k in range(4))
    step = max(1, chunk_pairs // E)
    for i in range(0, n, step):
        x0, y0, x1, y1 = (boxes[i:i + step, k, None] for k in range(4))
        o = _orient(ax, ay, bx, by, x0, y0)
        up = ay <= y0
        cross = (up != (by <= y0)) & np.where(up, o > 0.0, o < 0.0)
        near = ((ax <= x1) | (bx <= x1)) & ((ax >= x0) | (bx >= x0)) & ((ay <= y1) | (by <= y1)) & ((ay >= y0) | (by >= y0))
        o1, o2, o3 = _orient(ax, ay, bx, by, x1, y0), _orient(ax, ay, bx, by, x1, y1), _orient(ax, ay, bx, by, x0, y1)
        one_side = ((o > 0.0) & (o1 > 0.0) & (o2 > 0.0) & (o3 > 0.0)) | ((o < 0.0) & (o1 < 0.0) & (o2 < 0.0) & (o3 < 0.0))
        hit = (near & ~one_side).any(1)
        out[i:i + step] = hit.astype(np.uint8) | ((cross.sum(1) & 1).astype(np.uint8) << 1)
    return out


def land_flags(boxes, segs, band_height: Optional[float] = None, times: Optional[dict] = None) -> np.ndarray:
    """uint8 [N] from the GPU (engine.land_flags: host arrays in, host array out).  Raises without the library or a GPU: use
    land_flags_numpy there."""
    import torch
    from . import engine
    boxes = np.ascontiguousarray(np.asarray(boxes, np.float64).reshape(-1, 4))
    segs = np.ascontiguousarray(np.asarray(segs, np.float64).reshape(-1, 4))
    return engine.land_flags(torch.from_numpy(boxes).cuda(), torch.from_numpy(segs).cuda(), band_height, times=times).cpu().numpy()


def table_boxes(table: Dict[str, np.ndarray]) -> np.ndarray:
    """float64 [n, 4] (x0, y0, x1, y1) of the detections' EPSG:3857 boxes."""
    return np.stack([np.asarray(table[c], np.float64) for c in BOX_COLUMNS], 1).reshape(-1, 4)


def ocean_rows(table: Dict[str, np.ndarray], segs, cpu: bool = False) -> np.ndarray:
    """bool [n]: True for a detection whose (xmin_3857, ymin_3857, xmax_3857, ymax_3857) box is not on land.  cpu = the flags from
    land_flags_numpy instead of the GPU."""
    boxes = table_boxes(table)
    return (land_flags_numpy(boxes, segs) if cpu else land_flags(boxes, segs)) == 0


# ---- files ----

def write_ocean_geojson(path: str, stems: Sequence[str], table: Dict[str, np.ndarray], keep) -> int:
    """The features geocode.write_geojson writes for the rows with keep[k], in table order, each with the property ``index``: its row number
    in the full table (the reference saves with ``index=True``; facilities' cage_ids refer to it).  Returns the number of features."""
    keep = np.asarray(keep, bool)
    if keep.shape != (table["image"].shape[0],):
        raise ValueError(f"land filter: {keep.shape[0] if keep.ndim else 0} keep flags for {table['image'].shape[0]} detections")
    feats = []
    for k in np.nonzero(keep)[0].tolist():
        f = geocode.feature(stems, table, k)
        f["properties"] = {"index": k, **f["properties"]}
        feats.append(f)
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": geocode.CRS84, "features": feats}, f)
    return len(feats)


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.land",
                                description="Drop the detections of an existing label directory whose boxes touch land, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--land", required=True, metavar="GEOJSON", help="the land polygons (the reference's france_final_land_filter.shp as GeoJSON)")
    p.add_argument("--out", default=None, metavar="GEOJSON", help="default <labels>/../ocean_detections.geojson; with --images the directory of its two files")
    p.add_argument("--cpu", action="store_true", help="flags from the numpy restatement instead of the GPU")
    p.add_argument("--images", default=None, metavar="FILE",
                   help="instead of the detections: mark the images of FILE (names, one per line) whose rectangles lie wholly on land, at least "
                        "--land-images-indent metres from the coast (detect.py --land-images), and write land_images.csv and land_images.json")
    p.add_argument("--land-images-indent", type=float, default=5.0, metavar="R", help="how far the land is shrunk, in EPSG:3857 metres (the reference: 5)")
    opt = p.parse_args(argv)
    if opt.images is not None:
        from . import evaluate, land_images
        out_dir = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
        try:
            res = land_images.land_images_from_names(evaluate.read_image_list(opt.images), opt.geocode_bboxes, opt.land,
                                                     os.path.join(out_dir, land_images.CSV_FILE), opt.land_images_indent, cpu=opt.cpu)
        except ValueError as e:
            p.error(str(e))
        print(f"{land_images.describe(res)} in {out_dir}")
        return 0
    out = opt.out or os.path.join(os.path.dirname(os.path.abspath(opt.labels.rstrip("/"))), "ocean_detections.geojson")
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    segs = load_land_geojson(opt.land)
    keep = ocean_rows(table, segs, cpu=opt.cpu)
    n = write_ocean_geojson(out, table["stems"], table, keep)
    print(f"{n} of {keep.shape[0]} detections at sea ({segs.shape[0]} land edges) in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
