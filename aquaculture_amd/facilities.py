"""Candidate facilities from geocoded detections (``detect.py --facilities``, ``python -m aquaculture_amd.facilities``).

The reference's last two steps before its headline result, on the table geocode.geocode_detections returns:

  * net_areas        reference src/process_yolo/calc_net_areas.py (calc_all_areas with get_circle_area_from_bbox and
                     get_square_area_from_bbox): per-cage area estimate, its variance and bounds, from the EPSG:3035 box and, for circles,
                     whether the pixel box touches the image's border.  The same operations in the same order, on whole columns.
  * cluster          reference src/cluster_facilities.py (predictions_cluster -> DBSCAN_cluster): detections with det_conf >= conf_thresh,
                     per year or image pass, sklearn.cluster.DBSCAN(eps = 10 m, min_samples = 5) on the cages' centroids in EPSG:3035; every
                     cluster is a facility.  The labels come from the GPU (csrc/facilities.hip through engine.facility_dbscan) or, without
                     one, from dbscan_numpy; both compute exactly sklearn's labels:

                       core     at least min_samples points of the group within eps, the point itself included, dx dx + dy dy <= eps eps
                       root     of a core point: the smallest core index of its connected component of the core-core graph;
                                of any other point with a core neighbour: the smallest root among those neighbours (sklearn grows its
                                clusters in label order, so that cluster reaches the point first); else -1, noise
                       label    the rank of the root among the distinct roots of the group, -1 for noise

Pinned against scikit-learn (labels and core flags, exactly) and against recorded results of the reference's two area functions
(tests/golden/g11_net_areas.json).  NOT pinned, for want of geopandas / pyproj / shapely on the machines this was written on -- the same
status as the EPSG:3035 columns of geocode.py: the centroid chain (the reference takes shapely's ``centroid`` of the EPSG:3857 box
re-projected vertex by vertex to EPSG:3035; here the four corners go through geocode's published IOGP formulas and the quadrilateral's
area-weighted centroid is taken), the inverse projection that delivers the facility point in EPSG:3857, and the text form of the WKT
numbers (``repr``).  The ``*_farm_geoms`` columns hold the detections' original EPSG:3857 boxes; the reference's have been to EPSG:3035 and
back, which differs by rounding only.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import geocode

AREA_COLUMNS = ("area", "area_var", "min_area", "max_area")
FARM_TYPES = ("square", "circle", "rectangle")            # the reference's num_<t>_farms / <t>_farm_geoms columns, in its order
CLS_OF = {name: c for c, name in geocode.REVERSE_CLASS_MAPPING.items()}
IMAGE_PASSES = ((2000, 2004), (2005, 2009), (2010, 2012), (2013, 2015), (2016, 2018), (2019, 2021))
"""reference src/utils.py:116-130 (map_year_to_image_pass_opt2)"""


def image_pass(year: int) -> str:
    for a, b in IMAGE_PASSES:
        if a <= year <= b:
            return f"{a}-{b}"
    return "No group"


# ---- areas ----

def net_areas(table: Dict[str, np.ndarray], widths, heights) -> Dict[str, np.ndarray]:
    """The columns area, area_var, min_area, max_area (m^2) of the reference's calc_all_areas for every detection of `table`.
    widths, heights = the pixel size of each detection's image (scalars or one entry per detection).  Box width = e_max_3035 - e_min_3035,
    height = n_max_3035 - n_min_3035.  circle_farm: an ellipse; a box on the left / right border (pixel xmin == 0 or xmax == width) or on
    the top / bottom border (ymin == 0 or ymax == height) lies between a triangle and a half ellipse, on both between a triangle and a
    quarter ellipse.  square_farm: between half the box and the box.  Every other class: NaN (the reference leaves them undefined)."""
    w = np.asarray(table["e_max_3035"], np.float64) - np.asarray(table["e_min_3035"], np.float64)
    h = np.asarray(table["n_max_3035"], np.float64) - np.asarray(table["n_min_3035"], np.float64)
    cls = np.asarray(table["cls"])
    xb = (np.asarray(table["xmin"]) == 0) | (np.asarray(table["xmax"]) == np.asarray(widths))
    yb = (np.asarray(table["ymin"]) == 0) | (np.asarray(table["ymax"]) == np.asarray(heights))
    return _areas(w, h, cls == CLS_OF["circle_farm"], cls == CLS_OF["square_farm"], xb, yb)


def _areas(w, h, circle, square, xb, yb) -> Dict[str, np.ndarray]:
    """The reference's two functions, branch by branch, each expression in its operation order (calc_net_areas.py:38-58 and :76-80)."""
    w, h = np.asarray(w, np.float64), np.asarray(h, np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        tri = h * w / 2
        mx = np.where(xb & yb, np.pi * h * w / 4, np.where(xb, np.pi * (h / 2) * w / 2, np.pi * h * (w / 2) / 2))
        border = xb | yb
        full = np.pi * (w / 2) * (h / 2)
        sq_min, sq_max = w * h * (1 / 2), w * h
        lo = np.where(circle, np.where(border, tri, full), sq_min)
        hi = np.where(circle, np.where(border, mx, full), sq_max)
        est = np.where(circle & ~border, full, (lo + hi) / 2)
        var = np.where(circle & ~border, 0.0, ((hi - lo) * (hi - lo)) / 12)
    nan = ~(np.asarray(circle) | np.asarray(square))
    out = {"area": est, "area_var": var, "min_area": lo, "max_area": hi}
    for v in out.values():
        v[nan] = np.nan
    return out


# ---- centroids ----

def centroids_3035(table: Dict[str, np.ndarray]) -> np.ndarray:
    """float64 [n, 2] (easting, northing): the area-weighted centroid of each detection's EPSG:3857 box carried corner by corner to EPSG:3035
    (mercator_to_lonlat, lonlat_to_laea_europe).  Coordinates are taken relative to the first corner, so the shoelace sums work on box-sized
    numbers, not on 4e6 m."""
    x0, x1 = np.asarray(table["xmin_3857"], np.float64), np.asarray(table["xmax_3857"], np.float64)
    y0, y1 = np.asarray(table["ymin_3857"], np.float64), np.asarray(table["ymax_3857"], np.float64)
    corners = ((x1, y0), (x1, y1), (x0, y1), (x0, y0))      # shapely.geometry.box's ring
    en = [geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(x, y)) for x, y in corners]
    e = np.stack([c[0] for c in en], 1)
    n = np.stack([c[1] for c in en], 1)
    if e.shape[0] == 0:
        return np.zeros((0, 2), np.float64)
    de, dn = e - e[:, :1], n - n[:, :1]
    de2, dn2 = np.roll(de, -1, 1), np.roll(dn, -1, 1)
    cross = de * dn2 - de2 * dn
    a2 = cross.sum(1)                                       # twice the signed area
    with np.errstate(invalid="ignore", divide="ignore"):
        ce = ((de + de2) * cross).sum(1) / (3.0 * a2)
        cn = ((dn + dn2) * cross).sum(1) / (3.0 * a2)
    flat = ~(np.abs(a2) > 0)                                # a box without area: the mean of its corners
    ce[flat], cn[flat] = de[flat].mean(1), dn[flat].mean(1)
    return np.stack([e[:, 0] + ce, n[:, 0] + cn], 1)


# ---- DBSCAN ----

def roots_to_labels(root: np.ndarray, group: np.ndarray) -> np.ndarray:
    """sklearn's labels per group (each group's start at 0): the rank of a point's root among the distinct roots of its group; -1 stays."""
    root, group = np.asarray(root, np.int64), np.asarray(group, np.int64)
    labels = np.full(root.shape[0], -1, np.int64)
    has = root >= 0
    if not has.any():
        return labels
    u = np.unique(root[has])                                # ascending; a root is a point, so it has one group
    gu = group[u]
    order = np.lexsort((u, gu))
    first = np.searchsorted(gu[order], gu[order], side="left")
    rank = np.empty(u.shape[0], np.int64)
    rank[order] = np.arange(u.shape[0]) - first
    labels[has] = rank[np.searchsorted(u, root[has])]
    return labels


def dbscan_numpy(xy, group=None, eps: float = 10.0, min_samples: int = 5) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The rule set of the module's docstring without a GPU -> (labels int64 [n], core bool [n], root int64 [n]).  Candidate pairs come from
    a k-d tree at a slightly larger radius; the decision is the exact fp64 expression dx dx + dy dy <= eps eps, as on the GPU."""
    from scipy.sparse import coo_matrix
    from scipy.sparse.csgraph import connected_components
    from scipy.spatial import cKDTree
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    group = np.zeros(n, np.int64) if group is None else np.asarray(group, np.int64)
    if not eps > 0 or min_samples < 1:
        raise ValueError(f"facilities: eps = {eps}, min_samples = {min_samples} (eps > 0 and min_samples >= 1)")
    pairs = []
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        pr = cKDTree(xy[idx]).query_pairs(eps * (1 + 1e-9), output_type="ndarray")
        pairs.append(idx[pr])
    pr = np.concatenate(pairs, 0) if pairs else np.zeros((0, 2), np.int64)
    d = xy[pr[:, 0]] - xy[pr[:, 1]]
    pr = pr[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= eps * eps]
    a, b = pr[:, 0], pr[:, 1]
    count = 1 + np.bincount(a, minlength=n) + np.bincount(b, minlength=n)
    core = count >= min_samples
    root = np.full(n, -1, np.int64)
    cc = core[a] & core[b]
    _, comp = connected_components(coo_matrix((np.ones(int(cc.sum()), np.int8), (a[cc], b[cc])), shape=(n, n)), directed=False)
    first = np.full(n, n, np.int64)
    ci = np.nonzero(core)[0]
    np.minimum.at(first, comp[ci], ci)
    root[ci] = first[comp[ci]]
    best = np.full(n, n, np.int64)
    for s, t in ((a, b), (b, a)):                           # s a core point, t not: t may take s's root
        m = core[s] & ~core[t]
        np.minimum.at(best, t[m], root[s[m]])
    border = ~core & (best < n)
    root[border] = best[border]
    return roots_to_labels(root, group), core, root


def dbscan_labels(xy, group=None, eps: float = 10.0, min_samples: int = 5, times: Optional[dict] = None) -> Tuple[np.ndarray, np.ndarray]:
    """(labels int64 [n], core bool [n]) from the GPU: sklearn.cluster.DBSCAN(eps, min_samples).fit(xy[group == g]).labels_ of every group g
    (dense int ids; default one group) at the group's points.  Raises without the library or a GPU: use dbscan_numpy there."""
    import torch
    from . import engine
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    group = np.zeros(xy.shape[0], np.int32) if group is None else np.ascontiguousarray(group, dtype=np.int32)
    core, root = engine.facility_dbscan(torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda(), eps, min_samples, times=times)
    core_h, root_h = core.cpu().numpy(), root.cpu().numpy()
    return roots_to_labels(root_h, group), core_h.astype(bool)


# ---- the facility table ----

def _wkt_multipolygon(table, members: np.ndarray) -> str:
    if members.shape[0] == 0:
        return "MULTIPOLYGON EMPTY"
    parts = []
    for k in members.tolist():
        x0, y0, x1, y1 = (repr(float(table[c][k])) for c in ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857"))
        parts.append(f"(({x1} {y0}, {x1} {y1}, {x0} {y1}, {x0} {y0}, {x1} {y0}))")
    return "MULTIPOLYGON (" + ", ".join(parts) + ")"


def cluster(table: Dict[str, np.ndarray], by: str = "year", conf_thresh: float = 0.5, eps: float = 10.0, min_cages: int = 5,
            widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT, labels_fn: Optional[Callable] = None, keep=None) -> Dict[str, list]:
    """The reference's facility table (predictions_cluster) as columns: num_square_farms, num_circle_farms, num_rectangle_farms, `by`
    (``year`` or ``pass``: the image pass of the year), noise_points (of the facility's group), square_/circle_/rectangle_farm_geoms
    (MULTIPOLYGON WKT, EPSG:3857), cage_ids (row numbers in `table`: the reference's ``index``), area, area_var, min_area, max_area
    (sums over the members, NaN skipped as pandas skips them), facility_index, x_3857 / y_3857 (the Point: the mean of the members'
    EPSG:3035 centroids, delivered in EPSG:3857) and, beside the reference's, x_3035 / y_3035.  Facilities are ordered by group in
    order of first appearance, then by label.  Detections with det_conf >= conf_thresh take part; with keep (bool per detection: the
    land filter's ocean rows) only those of them with keep[k] -- cage_ids and ``_members`` stay row numbers of the full table.
    labels_fn(xy, group, eps, min_samples) -> (labels, core[, ...]); default dbscan_labels (the GPU).  The result also carries ``_members``: per detection of
    `table` its facility_index or -1, and ``_areas``: net_areas of the whole table."""
    if by not in ("year", "pass"):
        raise ValueError(f"facilities: cluster by 'year' or 'pass', not {by!r}")
    n_all = np.asarray(table["det_conf"]).shape[0]
    take = np.asarray(table["det_conf"], np.float64) >= conf_thresh
    if keep is not None:
        if np.asarray(keep).shape != (n_all,):
            raise ValueError(f"facilities: keep has shape {np.asarray(keep).shape}, the table {n_all} detections")
        take &= np.asarray(keep, bool)
    keep = np.nonzero(take)[0]
    years = np.asarray(table["year"], np.int64)[keep]
    values = [int(y) for y in years] if by == "year" else [image_pass(int(y)) for y in years]
    order: Dict[object, int] = {}
    group = np.asarray([order.setdefault(v, len(order)) for v in values], np.int32)
    xy = centroids_3035({c: np.asarray(table[c])[keep] for c in ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857")})
    labels = np.asarray((labels_fn or dbscan_labels)(xy, group, float(eps), int(min_cages))[0], np.int64) if keep.shape[0] else np.zeros(0, np.int64)
    areas = net_areas(table, widths, heights)
    cls = np.asarray(table["cls"], np.int64)[keep]
    out: Dict[str, list] = {k: [] for k in ("num_square_farms", "num_circle_farms", "num_rectangle_farms", by, "noise_points", "square_farm_geoms",
                                            "circle_farm_geoms", "rectangle_farm_geoms", "cage_ids", *AREA_COLUMNS, "facility_index",
                                            "x_3857", "y_3857", "x_3035", "y_3035")}
    members = np.full(n_all, -1, np.int64)
    for value, g in order.items():
        in_g = group == g
        noise = int((labels[in_g] == -1).sum())
        for l in np.unique(labels[in_g]):
            if l == -1:
                continue
            m = np.nonzero(in_g & (labels == l))[0]         # positions among the kept detections, in table order
            ids = keep[m]
            fi = len(out["facility_index"])
            for t in FARM_TYPES:
                of_t = cls[m] == CLS_OF.get(t + "_farm", -1)
                out[f"num_{t}_farms"].append(int(of_t.sum()))
                out[f"{t}_farm_geoms"].append(_wkt_multipolygon(table, ids[of_t]))
            out["cage_ids"].append([int(i) for i in ids])
            for c in AREA_COLUMNS:
                out[c].append(float(np.nansum(areas[c][ids])))
            out[by].append(value)
            out["noise_points"].append(noise)
            out["facility_index"].append(fi)
            e, nn = float(xy[m, 0].mean()), float(xy[m, 1].mean())
            x, y = geocode.lonlat_to_mercator(*geocode.laea_europe_to_lonlat(np.float64(e), np.float64(nn)))
            out["x_3857"].append(float(x)); out["y_3857"].append(float(y)); out["x_3035"].append(e); out["y_3035"].append(nn)
            members[ids] = fi
    out["_members"] = members
    out["_areas"] = areas
    return out


# ---- files ----

_CRS_3857 = {"type": "name", "properties": {"name": "urn:ogc:def:crs:EPSG::3857"}}


def _num(v: float):
    return None if v != v else v                            # NaN is not JSON


def detections_path(out_geojson: str) -> str:
    """reference cluster_facilities.py:169"""
    return out_geojson.replace(".geojson", "_detections.geojson")


def write_facilities_geojson(path: str, fac: Dict[str, list]) -> int:
    """The facility table as a FeatureCollection of Points in EPSG:3857 (the reference's ``df.to_file(facilities_path)``)."""
    cols = [c for c in fac if not c.startswith("_") and c not in ("x_3857", "y_3857")]
    feats = [{"type": "Feature", "properties": {c: fac[c][k] for c in cols},
              "geometry": {"type": "Point", "coordinates": [fac["x_3857"][k], fac["y_3857"][k]]}} for k in range(len(fac["facility_index"]))]
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": _CRS_3857, "features": feats}, f)
    return len(feats)


def write_facility_detections_geojson(path: str, table: Dict[str, np.ndarray], fac: Dict[str, list], stems: Optional[Sequence[str]] = None) -> int:
    """The detections that belong to any facility, in EPSG:3857, with ``index`` (the cage id of the facilities' cage_ids), the area
    columns and their facility_index (the reference's ``facility_detections``)."""
    feats = []
    stems = table.get("stems") if stems is None else stems
    for k in np.nonzero(fac["_members"] >= 0)[0].tolist():
        x0, y0, x1, y1 = (float(table[c][k]) for c in ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857"))
        props = {"index": k, "xmin": int(table["xmin"][k]), "xmax": int(table["xmax"][k]), "ymin": int(table["ymin"][k]), "ymax": int(table["ymax"][k]),
                 "type": geocode.REVERSE_CLASS_MAPPING[int(table["cls"][k])], "year": int(table["year"][k]), "det_conf": float(table["det_conf"][k]),
                 **{c: _num(float(fac["_areas"][c][k])) for c in AREA_COLUMNS}, "facility_index": int(fac["_members"][k])}
        if stems is not None:
            props["image"] = str(stems[int(table["image"][k])]) + ".jpeg"
        feats.append({"type": "Feature", "properties": props,
                      "geometry": {"type": "Polygon", "coordinates": [[[x1, y0], [x1, y1], [x0, y1], [x0, y0], [x1, y0]]]}})
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": _CRS_3857, "features": feats}, f)
    return len(feats)


def facilities_from_table(table: Dict[str, np.ndarray], out_geojson: str, by: str = "year", conf_thresh: float = 0.5, eps: float = 10.0,
                          min_cages: int = 5, widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT, cpu: bool = False, keep=None,
                          bathymetry: Optional[dict] = None, dedup: Optional[dict] = None) -> Dict[str, list]:
    """cluster() and both files: `out_geojson` and <out>_detections.geojson.  cpu = labels from dbscan_numpy instead of the GPU; keep =
    cluster()'s (the land filter's ocean rows).  bathymetry (bathymetry.settings' result): the facilities also get the reference's
    add_facility_depth columns bathy_depth, cage_depth, bathy_min, bathy_max, bathy_mean (null without a valid cell).  dedup
    (dedup.dedup_from_table's result, made with the same conf_thresh and keep; by = "pass" only): the survivors of its selection are
    clustered and the facilities get cage_ids_min and cage_ids_max."""
    if dedup is not None:
        if by != "pass":
            raise ValueError("facilities: the years of a pass are de-duplicated, so --dedup-years clusters by 'pass', not by 'year'")
        from . import dedup as aqdedup
        fac = aqdedup.cluster(table, dedup, conf_thresh, eps, min_cages, widths, heights, labels_fn=dbscan_numpy if cpu else None)
    else:
        fac = cluster(table, by, conf_thresh, eps, min_cages, widths, heights, labels_fn=dbscan_numpy if cpu else None, keep=keep)
    if bathymetry is not None:
        from . import bathymetry as aqbathy
        cols = aqbathy.depths_of(fac, table, bathymetry, cpu=cpu)
        fac.update({c: cols[c] for c in aqbathy.DEPTH_COLUMNS})
    write_facilities_geojson(out_geojson, fac)
    write_facility_detections_geojson(detections_path(out_geojson), table, fac)
    return fac


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--facilities-conf", type=float, default=0.5, metavar="CONF", help="detections with det_conf >= CONF take part (reference conf_thresh)")
    p.add_argument("--facilities-eps", type=float, default=10.0, metavar="M", help="DBSCAN eps in metres (reference distance_threshold)")
    p.add_argument("--facilities-min-cages", type=int, default=5, metavar="N", help="DBSCAN min_samples (reference amnt_min_clusters)")
    p.add_argument("--facilities-by", choices=("year", "pass"), default="year", help="cluster per year or per image pass (reference cluster_variable)")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.facilities",
                                description="Cluster the detections of an existing label directory into facilities, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--out", default=None, metavar="GEOJSON", help="default <labels>/../facilities.geojson")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the circle areas)")
    p.add_argument("--cpu", action="store_true", help="labels from the numpy / scipy restatement instead of the GPU")
    add_options(p)
    opt = p.parse_args(argv)
    out = opt.out or os.path.join(os.path.dirname(os.path.abspath(opt.labels.rstrip("/"))), "facilities.geojson")
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    fac = facilities_from_table(table, out, opt.facilities_by, opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages,
                                opt.image_size[0], opt.image_size[1], cpu=opt.cpu)
    print(f"{len(fac['facility_index'])} facilities of {int((fac['_members'] >= 0).sum())} cages in {out}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
