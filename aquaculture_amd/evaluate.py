"""Cage-level precision and recall of the facility detections over the tuning grid (``detect.py --evaluate``, ``python -m aquaculture_amd.evaluate``).

The reference chooses the three numbers behind its facility list -- the confidence threshold, the DBSCAN distance and the minimum cluster
size -- in src/get_kfold_cluster_performance.py: for every combination of 82 x 8 x 10 values (get_fold_performance) it keeps the detections
of at least that confidence, clusters them per year (predictions_cluster), keeps the members of any cluster and joins them with the human
labels both ways (get_stats_total / get_tp: a query is a true positive when its box intersects a key of the same year and type):

    precision = true-positive member detections / member detections          recall = labels met by a member detection / labels

Here the whole grid comes from one neighbour search per distance instead of one DBSCAN run per combination.  With c_i the confidence of
detection i and N[i] its closed eps-neighbourhood within its year (i included):

    core     i is a core point at (c, m)  iff  c <= T(i, m) = min(c_i, m-th largest confidence in N[i])        (-inf: N[i] has fewer than m points)
    member   sklearn labels i >= 0 at (c, m)  iff  c <= M(i, m) = min(c_i, max over j in N[i] of T(j, m))
    rows     whether a detection meets a label does not depend on the grid (tp_i); a label is met iff a matching detection is a member,
             so with R(l, m) = max of M(j, m) over the detections j matching label l:
             n_pred = #{i : M(i, m) >= c}     n_pred_tp = #{i : M(i, m) >= c and tp_i}     n_label_tp = #{l : R(l, m) >= c}

Every M and R is one of the input confidences, unchanged, so each >= is the reference's own fp64 comparison and the counts are exact.  M comes
from the GPU (csrc/evaluate.hip through engine.eval_member_conf), tp and R from its box join (engine.box_match), the counts from torch's
sort and searchsorted; ``cpu=True`` / ``--cpu`` restates every step in numpy / scipy (member_conf_numpy, box_match_numpy), with the same
bytes and counts.

operating_point() reports one combination as the reference's test_set_performance does: the cage-level numbers above, and facility-level
ones -- detections and labels (confidence 1, threshold 0) clustered per year (facilities.dbscan_labels), every cluster the bounding box of its
members' EPSG:3857 boxes, matched per year.

Pinned against scikit-learn's DBSCAN per combination plus a brute-force join (the four counts, exactly).  NOT pinned, and what differs:
  * the centroid chain (facilities.centroids_3035) has the status facilities.py describes: no pyproj / shapely to compare with;
  * the reference's overlap de-duplication (deduplicate_gdf_with_bboxes) of labels and detections is applied under ``--dedup-overlaps``
    only (overlaps.py: the detections through ``keep``, the labels through overlaps.filter_truth, ``dedup_overlaps`` = the box file); a
    clipped survivor keeps its full box here, where the reference goes on with the clipped polygon;
  * the reference's get_tp tests ``r['index_key']`` for truth, so a match with row 0 of the key table never counts; that slip is not
    reproduced: row 0 matches like any other;
  * the reference drops the detections of images that lie wholly on land ("surely_land"); here the land filter's ocean rows are used when
    given (``keep``), box by box, and they hold no detection of such an image: its box lies inside the image's rectangle, that inside the
    land (``--land-images``, land_images.py, marks those images);
  * ``images`` (``--evaluate-images``) restricts detections and labels to a list of images, which is how the reference applies a fold; its
    stratified folds themselves -- the image table, the hold-out, the folds, the winners on the test images -- are ``--evaluate-kfold``
    (kfold.py, whose docstring lists what is not reproduced there); with ``--land-images`` the images wholly on land leave its image table
    before the splits are drawn and form the stratum ``land``, as in the reference.
"""
from __future__ import annotations

import argparse
import itertools
import json
import os
import sys
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import facilities, geocode

TRUTH_TYPES = {"circle_cage": "circle_farm", "square_cage": "square_farm"}       # reference load_datasets_for_model_evaluation
CAGE_CLASSES = tuple(facilities.CLS_OF[t] for t in ("circle_farm", "square_farm"))
DEFAULT_CONF = np.arange(0.6, 1.01, 0.005)                  # reference src/get_kfold_cluster_performance_cfg.py
DEFAULT_EPS = np.arange(10, 151, 20)
DEFAULT_MIN = np.arange(1, 11)
MAX_K = 16                                                  # engine.EVAL_MAX_K: the largest minimum cluster size of a grid
COLUMNS = ("conf_thresh", "distance_threshold", "min_cluster_size", "precision", "recall", "product", "f_score",
           "n_pred", "n_pred_tp", "n_label", "n_label_tp")
BOX_COLUMNS = ("xmin_3857", "ymin_3857", "xmax_3857", "ymax_3857")
CSV_FILE, JSON_FILE = "cluster_performance.csv", "evaluation.json"


# ---- inputs ----

def load_truth_geojson(path: str) -> Dict[str, np.ndarray]:
    """The human labels (reference output/humanlabels.geojson: polygons in EPSG:3857 with ``type``, ``year`` and ``image``) as columns:
    xmin_3857 .. ymax_3857 (the polygon's bounds; the reference's labels are axis-aligned rectangles), cls (circle_cage -> circle_farm,
    square_cage -> square_farm; every other type is dropped), year, image (the file name, object array)."""
    with open(path) as f:
        obj = json.load(f)
    crs = ((obj.get("crs") or {}).get("properties") or {}).get("name", "")
    if crs and not crs.replace("::", ":").endswith(":3857"):
        raise ValueError(f"{path}: the labels have to be in EPSG:3857, not {crs}")
    rows = []
    for k, feat in enumerate(obj.get("features", [])):
        props, geom = feat.get("properties") or {}, feat.get("geometry") or {}
        kind = TRUTH_TYPES.get(props.get("type"))
        if kind is None:
            continue
        if geom.get("type") == "Polygon":
            rings = [geom["coordinates"][0]]
        elif geom.get("type") == "MultiPolygon":
            rings = [poly[0] for poly in geom["coordinates"]]
        else:
            raise ValueError(f"{path}: feature {k} is a {geom.get('type')}, not a polygon")
        pts = np.asarray([p[:2] for ring in rings for p in ring], np.float64)
        rows.append((pts[:, 0].min(), pts[:, 1].min(), pts[:, 0].max(), pts[:, 1].max(), facilities.CLS_OF[kind], int(props["year"]),
                     str(props.get("image", ""))))
    out = {c: np.asarray([r[i] for r in rows], np.float64) for i, c in enumerate(BOX_COLUMNS)}
    out["cls"] = np.asarray([r[4] for r in rows], np.int64)
    out["year"] = np.asarray([r[5] for r in rows], np.int64)
    out["image"] = np.asarray([r[6] for r in rows], dtype=object)
    return out


def read_image_list(path: str) -> List[str]:
    """Image names, one per line (empty lines skipped)."""
    with open(path) as f:
        return [l.strip() for l in f if l.strip()]


def _stem(name: str) -> str:
    """The name without directory and image extension (the names themselves hold dots: ORTHOIMAGERY.ORTHOPHOTOS2015_3_0_0)."""
    base, ext = os.path.splitext(os.path.basename(str(name)))
    return base if ext.lower() in (".jpeg", ".jpg", ".png", ".tif", ".tiff") else base + ext


def _sample(cols: Dict[str, np.ndarray], rows: np.ndarray, conf: np.ndarray) -> Dict[str, np.ndarray]:
    sub = {c: np.asarray(cols[c], np.float64)[rows] for c in BOX_COLUMNS}
    return {"box": np.ascontiguousarray(np.stack([sub[c] for c in BOX_COLUMNS], 1)) if rows.shape[0] else np.zeros((0, 4), np.float64),
            "xy": facilities.centroids_3035(sub), "conf": np.ascontiguousarray(conf, dtype=np.float64),
            "year": np.asarray(cols["year"], np.int64)[rows], "cls": np.asarray(cols["cls"], np.int64)[rows], "rows": rows}


def inputs(table: Dict[str, np.ndarray], truth: Dict[str, np.ndarray], keep=None, images: Optional[Sequence[str]] = None) -> Dict[str, dict]:
    """What the grid works on, from geocode's detection table and load_truth_geojson's labels -> {"det": ..., "lab": ..., "years": ...}; each
    sample holds box [n, 4] (EPSG:3857), xy [n, 2] (EPSG:3035 centroids), conf, year, cls, rows (row numbers of its source), and after this
    call year_id (dense) and group (year_id * 2 + square: what a match requires to agree).  Only circle and square detections take part;
    keep = bool per detection (the land filter's ocean rows); images = names (compared without directory and extension): detections and
    labels of other images are left out.  Labels have confidence 1."""
    cls = np.asarray(table["cls"], np.int64)
    take = np.isin(cls, CAGE_CLASSES)
    if keep is not None:
        if np.asarray(keep).shape != take.shape:
            raise ValueError(f"evaluate: keep has shape {np.asarray(keep).shape}, the table {take.shape[0]} detections")
        take &= np.asarray(keep, bool)
    take_l = np.ones(truth["cls"].shape[0], bool)
    if images is not None:
        wanted = {_stem(s) for s in images}
        stems = np.asarray([_stem(s) in wanted for s in table["stems"]], bool).reshape(-1)
        take &= stems[np.asarray(table["image"], np.int64)] if take.shape[0] else take
        take_l &= np.asarray([_stem(s) in wanted for s in truth["image"]], bool).reshape(-1)
    d_rows, l_rows = np.nonzero(take)[0], np.nonzero(take_l)[0]
    det = _sample(table, d_rows, np.asarray(table["det_conf"], np.float64)[d_rows])
    lab = _sample(truth, l_rows, np.ones(l_rows.shape[0], np.float64))
    years = np.unique(np.concatenate([det["year"], lab["year"]]))
    for s in (det, lab):
        s["year_id"] = np.searchsorted(years, s["year"]).astype(np.int32)
        s["group"] = (s["year_id"] * 2 + (s["cls"] == facilities.CLS_OF["square_farm"])).astype(np.int32)
    return {"det": det, "lab": lab, "years": years}


def parse_grid(text: str, integer: bool = False) -> np.ndarray:
    """``start:stop:step`` (numpy.arange) or a comma list.  integer = whole numbers required (the minimum cluster sizes)."""
    try:
        if ":" in text:
            parts = [p.strip() for p in text.split(":")]
            if len(parts) != 3:
                raise ValueError
            vals = np.arange(*[int(p) for p in parts]) if all(_is_int(p) for p in parts) else np.arange(*[float(p) for p in parts])
        else:
            parts = [p.strip() for p in text.split(",") if p.strip()]
            vals = np.asarray([int(p) for p in parts]) if all(_is_int(p) for p in parts) else np.asarray([float(p) for p in parts])
    except (ValueError, ZeroDivisionError):
        raise ValueError(f"evaluate: {text!r} is neither start:stop:step nor a comma list of numbers") from None
    if vals.shape[0] == 0:
        raise ValueError(f"evaluate: {text!r} names no value")
    if integer and vals.dtype.kind != "i":
        raise ValueError(f"evaluate: {text!r} has to name whole numbers")
    return vals


def _is_int(p: str) -> bool:
    try:
        int(p)
        return True
    except ValueError:
        return False


# ---- the numpy restatement of the two kernels ----

def member_conf_numpy(xy, group, conf, eps: float, K: int) -> np.ndarray:
    """M float64 [n, K] of the module's docstring without a GPU (engine.eval_member_conf gives the same bytes).  Candidate pairs come from a
    k-d tree at a slightly larger radius; the decision is the exact fp64 expression dx dx + dy dy <= eps eps, as on the GPU."""
    from scipy.spatial import cKDTree
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    group, conf = np.asarray(group, np.int64), np.asarray(conf, np.float64)
    if not eps > 0 or not 1 <= int(K) <= MAX_K:
        raise ValueError(f"evaluate: eps = {eps}, K = {K} (eps > 0 and 1 <= K <= {MAX_K})")
    if n == 0:
        return np.zeros((0, K), np.float64)
    pairs = []
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        pairs.append(idx[cKDTree(xy[idx]).query_pairs(eps * (1 + 1e-9), output_type="ndarray")])
    pr = np.concatenate(pairs, 0)
    d = xy[pr[:, 0]] - xy[pr[:, 1]]
    pr = pr[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= eps * eps]
    me = np.arange(n)
    row = np.concatenate([pr[:, 0], pr[:, 1], me])         # the closed neighbourhoods as (row, col) pairs, the point itself included
    col = np.concatenate([pr[:, 1], pr[:, 0], me])
    order = np.lexsort((-conf[col], row))                   # by row, confidences descending
    row, col = row[order], col[order]
    start = np.searchsorted(row, me)
    count = np.bincount(row, minlength=n)
    M = np.empty((n, K), np.float64)
    for m in range(K):
        kth = np.where(count > m, conf[col[np.minimum(start + m, row.shape[0] - 1)]], -np.inf)
        T = np.minimum(conf, kth)
        M[:, m] = np.minimum(conf, np.maximum.reduceat(T[col], start))
    return M


def box_match_numpy(qbox, qgroup, kbox, kgroup, payload=None, chunk: int = 256) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(hit bool [Q], out float64 [Q, K] or None): the closed-box join within equal group ids (engine.box_match gives the same).  Every
    pair of a block of `chunk` queries (in x order) and the keys whose x0 can reach the block is tested by brute force; boxes with a NaN
    match nothing."""
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int64), np.asarray(kgroup, np.int64)
    hit = np.zeros(qbox.shape[0], bool)
    out = None if payload is None else np.full((qbox.shape[0], np.asarray(payload).shape[1]), -np.inf)
    pay = None if payload is None else np.asarray(payload, np.float64)
    q_ok, k_ok = ~np.isnan(qbox).any(1), ~np.isnan(kbox).any(1)
    for g in np.unique(qgroup[q_ok]):
        qi, ki = np.nonzero((qgroup == g) & q_ok)[0], np.nonzero((kgroup == g) & k_ok)[0]
        if ki.shape[0] == 0:
            continue
        qi, ki = qi[np.argsort(qbox[qi, 0], kind="stable")], ki[np.argsort(kbox[ki, 0], kind="stable")]
        kx0 = kbox[ki, 0]
        widest = float((kbox[ki, 2] - kx0).max())
        for at in range(0, qi.shape[0], chunk):
            q = qi[at:at + chunk]
            lo = np.searchsorted(kx0, qbox[q, 0].min() - widest, side="left")      # a key further left ends before the block begins
            hi = np.searchsorted(kx0, qbox[q, 2].max(), side="right")              # a key further right begins after the block ends
            kk = ki[lo:hi]
            if kk.shape[0] == 0:
                continue
            kb, qb = kbox[kk], qbox[q][:, None, :]
            meet = (kb[None, :, 0] <= qb[:, :, 2]) & (qb[:, :, 0] <= kb[None, :, 2]) & (kb[None, :, 1] <= qb[:, :, 3]) & (qb[:, :, 1] <= kb[None, :, 3])
            hit[q] = meet.any(1)
            if out is not None:
                a, b = np.nonzero(meet)
                np.maximum.at(out, q[a], pay[kk[b]])
    return hit, out


# ---- the grid ----

def _check_grids(conf_grid, eps_grid, min_grid):
    conf_grid, eps_grid, min_grid = (np.atleast_1d(np.asarray(v)) for v in (conf_grid, eps_grid, min_grid))
    if min_grid.dtype.kind not in "iu" or min_grid.shape[0] == 0 or min_grid.min() < 1 or min_grid.max() > MAX_K:
        raise ValueError(f"evaluate: minimum cluster sizes have to be whole numbers in 1 .. {MAX_K}")
    if conf_grid.shape[0] == 0 or eps_grid.shape[0] == 0 or not (np.asarray(eps_grid, np.float64) > 0).all() or np.isnan(np.asarray(conf_grid, np.float64)).any():
        raise ValueError("evaluate: the grid needs at least one confidence threshold and one positive distance")
    return conf_grid, eps_grid, min_grid


def _counts_numpy(values: np.ndarray, thresholds: np.ndarray) -> np.ndarray:
    """int64 [K, C]: how many rows of values [n, K] are >= each threshold, per column."""
    n = values.shape[0]
    return np.stack([n - np.searchsorted(np.sort(values[:, m]), thresholds, side="left") for m in range(values.shape[1])]).astype(np.int64)


def _counts_torch(values, thresholds):
    import torch
    n, K = values.shape
    s = torch.sort(values.t().contiguous(), dim=1).values
    return (n - torch.searchsorted(s, thresholds.expand(K, -1).contiguous(), right=False)).cpu().numpy().astype(np.int64)


def grid(data: Dict[str, dict], conf_grid=DEFAULT_CONF, eps_grid=DEFAULT_EPS, min_grid=DEFAULT_MIN, cpu: bool = False,
         times: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """The table of the module's docstring for inputs() `data`: one row per element of itertools.product(conf_grid, eps_grid, min_grid), in
    that order (the reference's), as a dict of columns COLUMNS.  precision is NaN where n_pred is 0, recall where there are no labels.
    cpu = the numpy restatement instead of the GPU.  times = a dict that receives "sort_ms", "kernel_ms" (GPU: HIP events around the sorts
    and the kernels) and "count_ms" (wall clock)."""
    conf_grid, eps_grid, min_grid = _check_grids(conf_grid, eps_grid, min_grid)
    det, lab = data["det"], data["lab"]
    n, L, K = det["conf"].shape[0], lab["conf"].shape[0], int(min_grid.max())
    G = 2 * max(1, data["years"].shape[0])
    C, E, S = conf_grid.shape[0], eps_grid.shape[0], min_grid.shape[0]
    thr = np.asarray(conf_grid, np.float64)
    cols = min_grid.astype(np.int64) - 1
    n_pred, n_pred_tp, n_label_tp = (np.zeros((C, E, S), np.int64) for _ in range(3))
    t = {"sort_ms": 0.0, "kernel_ms": 0.0, "count_ms": 0.0}

    def timed(tm):
        t["sort_ms"] += tm.get("sort_ms", 0.0)
        t["kernel_ms"] += tm.get("kernel_ms", 0.0)

    if cpu:
        tp = box_match_numpy(det["box"], det["group"], lab["box"], lab["group"])[0]
        for e, eps in enumerate(eps_grid):
            M = member_conf_numpy(det["xy"], det["year_id"], det["conf"], float(eps), K)
            R = box_match_numpy(lab["box"], lab["group"], det["box"], det["group"], payload=M)[1]
            t0 = time.perf_counter()
            n_pred[:, e, :] = _counts_numpy(M, thr)[cols].T
            n_pred_tp[:, e, :] = _counts_numpy(M[tp], thr)[cols].T
            n_label_tp[:, e, :] = _counts_numpy(R, thr)[cols].T
            t["count_ms"] += (time.perf_counter() - t0) * 1e3
    else:
        import torch
        from . import engine
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        dbox, dgroup, dxy, dyear, dconf = (dev(det[c]) for c in ("box", "group", "xy", "year_id", "conf"))
        lbox, lgroup = dev(lab["box"]), dev(lab["group"])
        thr_d = dev(thr)
        tm = {} if times is not None else None
        tp = engine.box_match(dbox, dgroup, lbox, lgroup, G, times=tm)[0].bool()
        timed(tm or {})
        for e, eps in enumerate(eps_grid):
            M = engine.eval_member_conf(dxy, dyear, dconf, float(eps), K, times=tm)
            timed(tm or {})
            R = engine.box_match(lbox, lgroup, dbox, dgroup, G, payload=M, times=tm)[1]
            timed(tm or {})
            t0 = time.perf_counter()
            n_pred[:, e, :] = _counts_torch(M, thr_d)[cols].T
            n_pred_tp[:, e, :] = _counts_torch(M[tp], thr_d)[cols].T
            n_label_tp[:, e, :] = _counts_torch(R, thr_d)[cols].T
            t["count_ms"] += (time.perf_counter() - t0) * 1e3
    if times is not None:
        times.update(t)
    prod = list(itertools.product(conf_grid.tolist(), eps_grid.tolist(), min_grid.tolist()))
    out = {"conf_thresh": np.asarray([p[0] for p in prod], conf_grid.dtype), "distance_threshold": np.asarray([p[1] for p in prod], eps_grid.dtype),
           "min_cluster_size": np.asarray([p[2] for p in prod], np.int64)}
    out.update(rates(n_pred.reshape(-1), n_pred_tp.reshape(-1), np.full(C * E * S, L, np.int64), n_label_tp.reshape(-1)))
    return out


def rates(n_pred, n_pred_tp, n_label, n_label_tp) -> Dict[str, np.ndarray]:
    """precision, recall, product and f_score as the reference forms them (means of booleans; 2 (p r / (p + r))), and the four counts."""
    n_pred, n_pred_tp, n_label, n_label_tp = (np.asarray(v, np.int64) for v in (n_pred, n_pred_tp, n_label, n_label_tp))
    with np.errstate(invalid="ignore", divide="ignore"):
        precision = np.where(n_pred > 0, n_pred_tp / n_pred.astype(np.float64), np.nan)
        recall = np.where(n_label > 0, n_label_tp / n_label.astype(np.float64), np.nan)
        product = precision * recall
        f_score = 2 * (product / (precision + recall))
    return {"precision": precision, "recall": recall, "product": product, "f_score": f_score,
            "n_pred": n_pred, "n_pred_tp": n_pred_tp, "n_label": n_label, "n_label_tp": n_label_tp}


def idxmax(values) -> Optional[int]:
    """pandas' Series.idxmax: the first maximum, NaN skipped; None when every value is NaN (or there is none)."""
    v = np.asarray(values, np.float64)
    ok = ~np.isnan(v)
    if not ok.any():
        return None
    return int(np.nonzero(ok & (v == v[ok].max()))[0][0])


# ---- one combination, as the reference's test_set_performance ----

def _cluster_boxes(sample: Dict[str, np.ndarray], take: np.ndarray, eps: float, min_cages: int, cpu: bool):
    """DBSCAN per year of the rows `take` of a sample -> (member bool [n], boxes [F, 4]: the bounds of every cluster's boxes, year_id int32 [F])."""
    idx = np.nonzero(take)[0]
    member = np.zeros(take.shape[0], bool)
    if idx.shape[0] == 0:
        return member, np.zeros((0, 4), np.float64), np.zeros(0, np.int32)
    fn = facilities.dbscan_numpy if cpu else facilities.dbscan_labels
    labels = np.asarray(fn(sample["xy"][idx], sample["year_id"][idx], float(eps), int(min_cages))[0], np.int64)
    member[idx[labels >= 0]] = True
    m = idx[labels >= 0]
    if m.shape[0] == 0:
        return member, np.zeros((0, 4), np.float64), np.zeros(0, np.int32)
    key = sample["year_id"][m].astype(np.int64) * (int(labels.max()) + 1) + labels[labels >= 0]
    order = np.argsort(key, kind="stable")
    first = np.nonzero(np.concatenate([[True], key[order][1:] != key[order][:-1]]))[0]
    b = sample["box"][m[order]]
    boxes = np.stack([np.minimum.reduceat(b[:, 0], first), np.minimum.reduceat(b[:, 1], first),
                      np.maximum.reduceat(b[:, 2], first), np.maximum.reduceat(b[:, 3], first)], 1)
    return member, np.ascontiguousarray(boxes), sample["year_id"][m[order][first]].astype(np.int32)


def _hits(qbox, qgroup, kbox, kgroup, G: int, cpu: bool) -> np.ndarray:
    if cpu:
        return box_match_numpy(qbox, qgroup, kbox, kgroup)[0]
    import torch
    from . import engine
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()
    return engine.box_match(dev(qbox, np.float64), dev(qgroup, np.int32), dev(kbox, np.float64), dev(kgroup, np.int32), G)[0].cpu().numpy().astype(bool)


def operating_point(data: Dict[str, dict], conf: float, eps: float, min_cages: int, cpu: bool = False) -> Dict[str, dict]:
    """{"cage": ..., "facility": ...} at one combination: each the precision, recall, product, f_score and four counts of rates().  cage:
    the detections of confidence >= conf that DBSCAN(eps, min_cages) per year puts into a cluster, against the labels (year and type have
    to agree).  facility: those clusters against the clusters of the labels (all of them: confidence 1, threshold 0), each cluster the
    bounding box of its members' EPSG:3857 boxes, matched per year."""
    det, lab = data["det"], data["lab"]
    G = 2 * max(1, data["years"].shape[0])
    member, fbox, fyear = _cluster_boxes(det, det["conf"] >= conf, eps, min_cages, cpu)
    _, lfbox, lfyear = _cluster_boxes(lab, lab["conf"] >= 0, eps, min_cages, cpu)
    mbox, mgroup = det["box"][member], det["group"][member]
    cage = rates(int(member.sum()), int(_hits(mbox, mgroup, lab["box"], lab["group"], G, cpu).sum()),
                 lab["conf"].shape[0], int(_hits(lab["box"], lab["group"], mbox, mgroup, G, cpu).sum()))
    fac = rates(fbox.shape[0], int(_hits(fbox, fyear, lfbox, lfyear, G, cpu).sum()),
                lfbox.shape[0], int(_hits(lfbox, lfyear, fbox, fyear, G, cpu).sum()))
    scalar = lambda r: {k: (int(v) if v.dtype.kind == "i" else float(v)) for k, v in r.items()}
    return {"conf_thresh": float(conf), "distance_threshold": float(eps), "min_cluster_size": int(min_cages), "cage": scalar(cage), "facility": scalar(fac)}


# ---- files ----

def _fmt(v) -> str:
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    return "" if v != v else repr(float(v))


def write_performance_csv(path: str, table: Dict[str, np.ndarray]) -> int:
    """The grid as CSV: a header, one line per row; whole-number columns as integers, the others as ``repr`` of the double, NaN empty."""
    n = table["n_pred"].shape[0]
    with open(path, "w") as f:
        f.write(",".join(COLUMNS) + "\n")
        cols = [table[c].tolist() for c in COLUMNS]
        for k in range(n):
            f.write(",".join(_fmt(c[k]) for c in cols) + "\n")
    return n


def read_performance_csv(path: str) -> Dict[str, np.ndarray]:
    """write_performance_csv's file back: the count columns and min_cluster_size as int64, the others as float64 (empty: NaN)."""
    with open(path) as f:
        header = f.readline().strip().split(",")
        rows = [l.rstrip("\n").split(",") for l in f if l.strip()]
    ints = {"min_cluster_size", "n_pred", "n_pred_tp", "n_label", "n_label_tp"}
    return {c: np.asarray([int(r[i]) for r in rows], np.int64) if c in ints
            else np.asarray([float(r[i]) if r[i] else np.nan for r in rows], np.float64) for i, c in enumerate(header)}


def _json_num(v):
    v = v.item() if isinstance(v, np.generic) else v
    return None if isinstance(v, float) and v != v else v      # NaN is not JSON


def _json_row(table: Dict[str, np.ndarray], k: Optional[int]):
    return None if k is None else {"row": k, **{c: _json_num(table[c][k]) for c in COLUMNS}}


def summary(data: Dict[str, dict], table: Dict[str, np.ndarray], op: Dict[str, dict]) -> dict:
    """What evaluation.json holds: the sizes, the grid's best row by ``product`` and by ``f_score`` (idxmax) and the operating point."""
    clean = lambda d: {k: (clean(v) if isinstance(v, dict) else _json_num(v)) for k, v in d.items()}
    return {"n_detections": int(data["det"]["conf"].shape[0]), "n_labels": int(data["lab"]["conf"].shape[0]),
            "years": [int(y) for y in data["years"]], "grid_rows": int(table["n_pred"].shape[0]),
            "best_product": _json_row(table, idxmax(table["product"])), "best_f_score": _json_row(table, idxmax(table["f_score"])),
            "operating_point": clean(op)}


def evaluate_table(table: Dict[str, np.ndarray], truth_path: str, out_dir: str, conf_grid=DEFAULT_CONF, eps_grid=DEFAULT_EPS, min_grid=DEFAULT_MIN,
                   op: Tuple[float, float, int] = (0.5, 10.0, 5), keep=None, images: Optional[Sequence[str]] = None, cpu: bool = False,
                   times: Optional[dict] = None, dedup_overlaps: Optional[str] = None) -> dict:
    """inputs(), grid(), operating_point(*op) and both files in out_dir: cluster_performance.csv and evaluation.json -> summary().
    dedup_overlaps = the download-box file: the labels pass through overlaps.filter_truth first."""
    from . import overlaps
    data = inputs(table, overlaps.filter_truth(load_truth_geojson(truth_path), dedup_overlaps, cpu=cpu), keep, images)
    perf = grid(data, conf_grid, eps_grid, min_grid, cpu=cpu, times=times)
    point = operating_point(data, float(op[0]), float(op[1]), int(op[2]), cpu=cpu)
    t0 = time.perf_counter()
    os.makedirs(out_dir, exist_ok=True)
    write_performance_csv(os.path.join(out_dir, CSV_FILE), perf)
    s = summary(data, perf, point)
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump(s, f, indent=1)
    if times is not None:
        times["files_ms"] = (time.perf_counter() - t0) * 1e3
    return s


def describe(s: dict) -> str:
    best = s["best_f_score"]
    cage = s["operating_point"]["cage"]
    at = (f"best f_score {best['f_score']:.4f} at conf {best['conf_thresh']:g}, eps {best['distance_threshold']:g}, min {best['min_cluster_size']}"
          if best else "no row with an f_score")
    num = lambda v: "nan" if v is None else f"{v:.4f}"
    return (f"evaluated {s['n_detections']} detections against {s['n_labels']} labels over {s['grid_rows']} combinations: {at}; "
            f"operating point precision {num(cage['precision'])}, recall {num(cage['recall'])}")


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--evaluate-out", default=None, metavar="DIR", help=f"where {CSV_FILE} and {JSON_FILE} go")
    p.add_argument("--evaluate-conf", default=None, metavar="GRID", help="confidence thresholds: start:stop:step (numpy arange) or a comma list (default 0.6:1.01:0.005)")
    p.add_argument("--evaluate-eps", default=None, metavar="GRID", help="DBSCAN distances in metres, the same forms (default 10:151:20)")
    p.add_argument("--evaluate-min-cages", default=None, metavar="GRID", help=f"minimum cluster sizes, the same forms, whole numbers up to {MAX_K} (default 1:11:1)")
    p.add_argument("--evaluate-images", default=None, metavar="FILE", help="image names, one per line: detections and labels of other images are left out (a fold)")
    p.add_argument("--evaluate-kfold", nargs="?", const=5, default=None, type=int, metavar="N",
                   help="cross-validate the tuning as the reference does (src/get_kfold_cluster_performance.py): a stratified image table, a hold-out, "
                        "N stratified folds (a bare flag: 5), the grid on every fold's train images -- all folds in one GPU call per distance --, "
                        f"the winners on its test images; writes {KFOLD_FILES[0]}, {KFOLD_FILES[1]} and {KFOLD_FILES[2]} beside the other two files; 2 to 15")
    p.add_argument("--evaluate-kfold-images", default=None, metavar="FILE",
                   help="the images of the cross-validation's table, one name per line, in this order (default: every image of the sweep, or of the "
                        "label directory and the truth, sorted by name; required with --tile-scenes, whose tiles are listed nowhere)")
    p.add_argument("--evaluate-known-sites", default=None, metavar="CSV",
                   help="known sites (columns lat, lon; the reference's data/aquaculture_med_dedupe.csv): images without a detection are stratified by "
                        "whether they meet the +-1000 m box of one")
    p.add_argument("--evaluate-kfold-seed", default=1, type=int, metavar="SEED", help="random_state of the hold-out and of the folds (default 1, the reference's)")
    p.add_argument("--evaluate-kfold-test", default=0.1, type=float, metavar="FRACTION", help="share of the images set aside before the folds (default 0.1; 0: none)")


KFOLD_FILES = ("kfold_results.csv", "kfold_images.csv", "kfold.json")      # kfold.RESULTS_FILE, IMAGES_FILE, JSON_FILE


def check_kfold_options(n_splits, test_frac) -> None:
    """What the command lines refuse before any work: a fold count outside 2 .. 15 (2 N + 2 subset bits in a 32-bit word) and a hold-out
    fraction outside [0, 1)."""
    if n_splits is not None and not 2 <= int(n_splits) <= 15:
        raise ValueError(f"--evaluate-kfold {n_splits}: 2 to 15 folds")
    if not 0 <= float(test_frac) < 1:
        raise ValueError(f"--evaluate-kfold-test {test_frac}: a fraction in [0, 1)")


def kfold_from_options(table, truth_path: str, out_dir: str, grids, op, keep, images, n_splits: int, kfold_images: Optional[str], known_sites: Optional[str],
                       seed: int, test_frac: float, wanted_bboxes_csv: Optional[str], names: Optional[Sequence[str]] = None, cpu: bool = False,
                       dedup_overlaps: Optional[str] = None, land: Optional[Sequence[str]] = None) -> dict:
    """The cross-validation as both command lines run it: names = the images of the table when --evaluate-kfold-images gives none (None: those
    with a detection or a label).  dedup_overlaps = the download-box file: the labels pass through overlaps.filter_truth first.  land = the
    images wholly on land (--land-images), which kfold.kfold takes out of the table."""
    from . import kfold as aqkfold
    from . import overlaps
    if kfold_images:
        names = read_image_list(kfold_images)
    sites = aqkfold.load_known_sites(known_sites) if known_sites else None
    if sites is not None and not wanted_bboxes_csv:
        raise ValueError("--evaluate-known-sites needs the images' rectangles: --geocode-bboxes CSV")
    rects = aqkfold.tile_rects(wanted_bboxes_csv) if sites is not None else None
    return aqkfold.kfold(table, overlaps.filter_truth(load_truth_geojson(truth_path), dedup_overlaps, cpu=cpu), out_dir, n_splits, names=names, rects=rects, sites=sites, seed=seed, test_frac=test_frac,
                         conf_grid=grids[0], eps_grid=grids[1], min_grid=grids[2], op=op, keep=keep, images=images, cpu=cpu, land=land)


def land_image_names(table, truth_path: Optional[str], kfold_images: Optional[str], names: Optional[Sequence[str]] = None) -> List[str]:
    """The image list of --land-images, which is the one --evaluate-kfold makes its table of: --evaluate-kfold-images when given, else
    `names` (the sweep's listing), else the images of the detection table and of the truth, sorted by stem."""
    if kfold_images:
        return read_image_list(kfold_images)
    if names is not None:
        return list(names)
    truth = load_truth_geojson(truth_path)["image"] if truth_path else []
    return sorted({_stem(s) for s in table["stems"]} | {_stem(s) for s in truth})


def grids_from_options(conf: Optional[str], eps: Optional[str], min_cages: Optional[str]):
    return (DEFAULT_CONF if conf is None else parse_grid(conf), DEFAULT_EPS if eps is None else parse_grid(eps),
            DEFAULT_MIN if min_cages is None else parse_grid(min_cages, integer=True))


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.evaluate",
                                description="Score the detections of an existing label directory against human labels over the tuning grid, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--truth", required=True, metavar="GEOJSON", help="the human labels (reference output/humanlabels.geojson)")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea take part (the land filter)")
    p.add_argument("--cpu", action="store_true", help="the numpy / scipy restatement instead of the GPU")
    add_options(p)
    facilities.add_options(p)
    from . import land_images
    land_images.add_options(p)
    opt = p.parse_args(argv)
    if opt.land_images is not None and opt.land is None:
        p.error(land_images.NEEDS_LAND.replace("--land-filter", "--land"))
    try:
        land_images._check_indent(opt.land_images_indent)
        grids = grids_from_options(opt.evaluate_conf, opt.evaluate_eps, opt.evaluate_min_cages)
        check_kfold_options(opt.evaluate_kfold, opt.evaluate_kfold_test)
    except ValueError as e:
        p.error(str(e))
    out_dir = opt.evaluate_out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land is not None:
        from . import land
        keep = land.ocean_rows(table, land.load_land_geojson(opt.land), cpu=opt.cpu)
    images = read_image_list(opt.evaluate_images) if opt.evaluate_images else None
    s = evaluate_table(table, opt.truth, out_dir, *grids, op=(opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages),
                       keep=keep, images=images, cpu=opt.cpu)
    print(describe(s) + f" in {out_dir}")
    on_land = None
    if opt.land_images is not None:
        li = land_images.land_images_from_names(land_image_names(table, opt.truth, opt.evaluate_kfold_images), opt.geocode_bboxes, opt.land,
                                                opt.land_images or os.path.join(out_dir, land_images.CSV_FILE), opt.land_images_indent, cpu=opt.cpu)
        on_land = [s_ for s_, l in zip(li["stems"], li["on_land"]) if l]
        print(f"{land_images.describe(li)} in {opt.land_images or os.path.join(out_dir, land_images.CSV_FILE)}")
    if opt.evaluate_kfold is not None:
        from . import kfold as aqkfold
        k = kfold_from_options(table, opt.truth, out_dir, grids, (opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages), keep, images,
                               opt.evaluate_kfold, opt.evaluate_kfold_images, opt.evaluate_known_sites, opt.evaluate_kfold_seed, opt.evaluate_kfold_test,
                               opt.geocode_bboxes, cpu=opt.cpu, land=on_land)
        print(aqkfold.describe(k) + f" in {out_dir}")
    return 0


from .kfold import box_match_subsets_numpy, cross_validate, kfold, member_conf_subsets_numpy      # noqa: E402  (kfold.py reads this module's names when called)


if __name__ == "__main__":
    sys.exit(main())
