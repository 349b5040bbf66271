"""The model's cage-area error per image pass and cage type (``detect.py --model-errors``, ``python -m aquaculture_amd.model_errors``).

The table the bootstrap of tonnage.py takes as ``--tonnage-errors``: mean and sd of (label area - detection area) per (pass, type).  The
reference computes it in src/utils_tonnage.py:130-203 (define_model_error_distributions) with :284-327 (get_cage_area_errors_from_labels):
detections above a confidence threshold are joined to the human labels of the same year and type, each detection keeps the label it
overlaps most, error = label area - detection area, and scipy.stats.norm.fit gives one normal per (pass, type).  The definition here:

Samples (evaluate.inputs).  Queries: detections of class circle_farm / square_farm with det_conf > conf -- strictly, as the reference
filters here (``--facilities-conf`` keeps det_conf >= conf); with the land filter only its ocean rows (``keep``).  Keys: labels of type
circle_cage / square_cage.  group = year_id * 2 + square, the grouping of evaluate.inputs.

Areas (facilities._areas on both sides).  Detections: the ``area`` column of facilities.net_areas.  Labels: the EPSG:3857 bounds carried
corner by corner to EPSG:3035 (geocode.mercator_to_lonlat, lonlat_to_laea_europe), width and height from the bounds of that quadrilateral,
as the reference's ``row['geometry'].bounds`` after ``to_crs``; the border flags from the label's own xmin, ymin, xmax, ymax, jpeg_width,
jpeg_height properties (load_truth_geojson below returns them and refuses a file without them).

Match.  Label k is a candidate of detection q iff their groups are equal and their closed EPSG:3857 boxes intersect (evaluate's box_match
predicate).  inter(q, k) = (min(q.x1, k.x1) - max(q.x0, k.x0)) * (min(q.y1, k.y1) - max(q.y0, k.y0)): two subtractions and one product in
fp64, as written.  The match is the candidate of the largest inter; among equal inter the smallest label row wins; a NaN inter never wins
over a number.  Per query: match (int32 label row, -1 without a candidate), overlap = 100 * inter / ((q.x1 - q.x0) * (q.y1 - q.y0)) as
computed (inf or NaN for a query without area), error = area_label[match] - area_det[q]; overlap and error are NaN without a match.
Every NaN is stored as the canonical quiet NaN, whatever operation made it.

Moments.  mgroup = pass_id * 2 + square; the passes are the sorted distinct facilities.image_pass(year) of the labels (the reference's
period_passes).  A query is a member when match >= 0, its pass is one of the labels' and its error is finite.  Per group n, mean = S / n,
sd = sqrt(D / n) -- scipy.stats.norm.fit: the population sd -- with S = sum of error and D = sum of (error - mean)^2 in one written order:
lane l of 64 adds the values of the rows q = l (mod 64) in increasing q, +0.0 for a non-member (exact); the 64 partials then fold as
v[i] + v[i + 32], + 16, ... + 1.  A group with n = 0 is left out of the files (the bootstrap then uses its (0, 0) default) and
model_errors.json lists it under "empty".

The match and the moments come from the GPU (csrc/model_errors.hip through engine.model_error_match / model_error_moments) or, with
cpu=True / ``--cpu``, from match_numpy / moments_numpy; both give the same bytes.  literal_numpy is the reference's procedure pair by
pair, for the tests.

Pinned against literal_numpy and scipy.stats.norm.fit (tests/test_model_errors.py).  NOT pinned, and what differs from the reference:
  * the overlap is measured on the EPSG:3857 rectangles, not on the EPSG:3035 quadrilaterals the reference intersects.  The ratio of two
    areas a few metres apart survives the re-projection: over the labels of tests/golden/g12 the 3035 / 3857 area scale varies by 2.4e-4
    relative, and only the part of that within one query's reach could change which label wins -- where two candidates' overlaps agree
    to within that local distortion.  tests/test_model_errors.py compares the choice with a polygon clip in EPSG:3035 on its fixture;
  * ties: the reference sorts with pandas' unstable quicksort and keeps the first, which is not reproducible; here the smallest label row;
  * the reference's overlap de-duplication (deduplicate_gdf_with_bboxes) is applied under ``--dedup-overlaps`` only -- the status
    evaluate.py gives it: the detections through ``keep``, the labels through overlaps.filter_truth (``dedup_overlaps`` = the box file);
    the reference itself notes that it "isn't really needed" for the detections;
  * areas, centroids and the EPSG:3035 chain have the status facilities.py and geocode.py describe (no pyproj / shapely to compare with).
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from typing import Dict, List, Optional, Tuple

import numpy as np

from . import evaluate, facilities, geocode

PIXEL_COLUMNS = ("xmin", "ymin", "xmax", "ymax", "jpeg_width", "jpeg_height")
FARM_TYPES = ("circle_farm", "square_farm")                  # the type of moment group pass_id * 2 + square
CSV_FILE, CAGES_FILE, JSON_FILE = "model_errors.csv", "model_error_cages.csv", "model_errors.json"
LANES = 64


# ---- inputs ----

def load_truth_geojson(path: str) -> Dict[str, np.ndarray]:
    """evaluate.load_truth_geojson's columns and, per label, the six PIXEL_COLUMNS (float64: the label's box in the pixels of its image and
    that image's size) and ``feature`` (its number among the file's features).  A label without one of the six is refused."""
    out = evaluate.load_truth_geojson(path)
    with open(path) as f:
        obj = json.load(f)
    rows, numbers = [], []
    for k, feat in enumerate(obj.get("features", [])):
        props = feat.get("properties") or {}
        if evaluate.TRUTH_TYPES.get(props.get("type")) is None:
            continue
        lacking = [c for c in PIXEL_COLUMNS if not isinstance(props.get(c), (int, float)) or isinstance(props.get(c), bool)]
        if lacking:
            raise ValueError(f"{path}: feature {k} lacks {', '.join(lacking)}: the label areas need the labels' pixel boxes and image sizes "
                             f"({', '.join(PIXEL_COLUMNS)}, as the reference's output/humanlabels.geojson carries them)")
        rows.append([float(props[c]) for c in PIXEL_COLUMNS])
        numbers.append(k)
    px = np.asarray(rows, np.float64).reshape(-1, len(PIXEL_COLUMNS))
    out.update({c: np.ascontiguousarray(px[:, i]) for i, c in enumerate(PIXEL_COLUMNS)})
    out["feature"] = np.asarray(numbers, np.int64)
    return out


def label_areas(truth: Dict[str, np.ndarray]) -> np.ndarray:
    """float64 [L]: the reference's compute_cage_area_estimates_gdf ``area`` of every label (the module's docstring, "Areas")."""
    x0, y0, x1, y1 = (np.asarray(truth[c], np.float64) for c in evaluate.BOX_COLUMNS)
    en = [geocode.lonlat_to_laea_europe(*geocode.mercator_to_lonlat(x, y)) for x, y in ((x1, y0), (x1, y1), (x0, y1), (x0, y0))]
    e, n = np.stack([c[0] for c in en], 1).reshape(-1, 4), np.stack([c[1] for c in en], 1).reshape(-1, 4)
    w, h = e.max(1) - e.min(1), n.max(1) - n.min(1)
    cls = np.asarray(truth["cls"], np.int64)
    xb = (np.asarray(truth["xmin"]) == 0) | (np.asarray(truth["xmax"]) == np.asarray(truth["jpeg_width"]))
    yb = (np.asarray(truth["ymin"]) == 0) | (np.asarray(truth["ymax"]) == np.asarray(truth["jpeg_height"]))
    return facilities._areas(w, h, cls == facilities.CLS_OF["circle_farm"], cls == facilities.CLS_OF["square_farm"], xb, yb)["area"]


def samples(table: Dict[str, np.ndarray], truth: Dict[str, np.ndarray], conf: float, keep=None, widths=geocode.IM_WIDTH,
            heights=geocode.IM_HEIGHT) -> Dict[str, object]:
    """What the two steps work on -> {"q": queries, "k": keys, "passes": [...], "G": groups of the match}.  Each side holds box [n, 4], group
    int32, area, rows (row numbers of its source) and square (bool); the queries also mgroup int32 (-1: the pass has no labels)."""
    data = evaluate.inputs(table, truth, keep)
    det, lab = data["det"], data["lab"]
    take = det["conf"] > conf                                # strictly: the reference's detections_df['det_conf'] > confidence_threshold
    square = facilities.CLS_OF["square_farm"]
    area_det = np.asarray(facilities.net_areas(table, widths, heights)["area"], np.float64)
    q = {"box": np.ascontiguousarray(det["box"][take]), "group": np.ascontiguousarray(det["group"][take]), "rows": det["rows"][take],
         "square": det["cls"][take] == square, "year": det["year"][take]}
    q["area"] = np.ascontiguousarray(area_det[q["rows"]])
    k = {"box": lab["box"], "group": lab["group"], "rows": lab["rows"], "square": lab["cls"] == square, "year": lab["year"],
         "area": np.ascontiguousarray(label_areas(truth)[lab["rows"]])}
    passes = sorted({facilities.image_pass(int(y)) for y in k["year"]})
    pid = np.asarray([passes.index(p) if p in passes else -1 for p in (facilities.image_pass(int(y)) for y in q["year"])], np.int64)
    q["mgroup"] = np.where(pid >= 0, pid * 2 + q["square"], -1).astype(np.int32)
    return {"q": q, "k": k, "passes": passes, "G": 2 * max(1, data["years"].shape[0])}


# ---- the numpy restatement of the two kernels ----

def _canonical(v: np.ndarray) -> np.ndarray:
    v[np.isnan(v)] = np.nan                                 # one NaN, whatever made it
    return v


def match_numpy(qbox, qgroup, qarea, kbox, kgroup, karea, chunk: int = 256) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(match int32 [Q], overlap float64 [Q], error float64 [Q]) of the module's docstring without a GPU (engine.model_error_match gives
    the same bytes): every pair of a block of `chunk` queries (in x order) and the keys of their group whose x0 can reach the block, by
    brute force, as evaluate.box_match_numpy; the rule is a total order, so the result does not depend on the order of the pairs."""
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int64), np.asarray(kgroup, np.int64)
    qarea, karea = np.asarray(qarea, np.float64), np.asarray(karea, np.float64)
    Q = qbox.shape[0]
    match = np.full(Q, -1, np.int32)
    inter_w = np.full(Q, np.nan)
    with np.errstate(all="ignore"):
        for g in np.unique(qgroup):
            qi, ki = np.nonzero(qgroup == g)[0], np.nonzero(kgroup == g)[0]
            if ki.shape[0] == 0:
                continue
            qi, ki = qi[np.argsort(qbox[qi, 0], kind="stable")], ki[np.argsort(kbox[ki, 0], kind="stable")]     # (NaN last)
            kx0 = kbox[ki, 0]
            widths = kbox[ki, 2] - kx0
            widest = float(np.nanmax(widths)) if not np.isnan(widths).all() else 0.0
            group_keys = ki
            for at in range(0, qi.shape[0], chunk):
                q = qi[at:at + chunk]
                x_lo, x_hi = np.nanmin(qbox[q, 0]) if not np.isnan(qbox[q, 0]).all() else np.nan, qbox[q, 2]
                x_hi = np.nanmax(x_hi) if not np.isnan(x_hi).all() else np.nan
                if np.isnan(x_lo) or np.isnan(x_hi):
                    continue                                # a block of NaN queries matches nothing
                lo = np.searchsorted(kx0, x_lo - widest, side="left")           # a key further left ends before the block begins
                hi = np.searchsorted(kx0, x_hi, side="right")                   # a key further right begins after the block ends
                ki = group_keys[lo:hi]
                if ki.shape[0] == 0:
                    continue
                kb = kbox[ki][None, :, :]
                qb = qbox[q][:, None, :]
                meet = (kb[:, :, 0] <= qb[:, :, 2]) & (qb[:, :, 0] <= kb[:, :, 2]) & (kb[:, :, 1] <= qb[:, :, 3]) & (qb[:, :, 1] <= kb[:, :, 3])
                inter = (np.minimum(qb[:, :, 2], kb[:, :, 2]) - np.maximum(qb[:, :, 0], kb[:, :, 0])) * \
                        (np.minimum(qb[:, :, 3], kb[:, :, 3]) - np.maximum(qb[:, :, 1], kb[:, :, 1]))
                number = meet & ~np.isnan(inter)
                cand = np.where(number.any(1)[:, None], number, meet)            # NaN candidates count only where there is no number
                best = np.where(cand & number, inter, -np.inf).max(1)
                cand &= ~number | (inter == best[:, None])
                row = np.where(cand, ki[None, :], np.iinfo(np.int64).max)
                at_k = row.argmin(1)
                has = cand.any(1)
                match[q[has]] = ki[at_k[has]]
                inter_w[q[has]] = inter[np.nonzero(has)[0], at_k[has]]
        has = match >= 0
        overlap, error = np.full(Q, np.nan), np.full(Q, np.nan)
        b = qbox[has]
        overlap[has] = 100.0 * inter_w[has] / ((b[:, 2] - b[:, 0]) * (b[:, 3] - b[:, 1]))
        error[has] = karea[match[has]] - qarea[has]
    return match, _canonical(overlap), _canonical(error)


def _lane_sums(values: np.ndarray) -> np.ndarray:
    """values [G, Q] -> [G]: per row, lane l adds the entries q = l (mod 64) in increasing q, then the 64 partials fold by halves."""
    G, Q = values.shape
    pad = -Q % LANES
    v = np.concatenate([values, np.zeros((G, pad))], 1).reshape(G, -1, LANES)     # (a lane's missing last row: + 0.0, which changes nothing)
    s = np.zeros((G, LANES))
    for r in range(v.shape[1]):
        s = s + v[:, r, :]
    h = LANES // 2
    while h >= 1:
        s = s[:, :h] + s[:, h:2 * h]
        h //= 2
    return s[:, 0]


def moments_numpy(error, match, mgroup, G: int) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """(n int64 [G], mean float64 [G], sd float64 [G]) of the module's docstring without a GPU (engine.model_error_moments gives the same
    bytes); mean and sd are NaN where n = 0."""
    error, match, mgroup = np.asarray(error, np.float64), np.asarray(match, np.int64), np.asarray(mgroup, np.int64)
    G = int(G)
    member = (mgroup[None, :] == np.arange(G)[:, None]) & ((match >= 0) & np.isfinite(error))[None, :]
    n = member.sum(1).astype(np.int64)
    with np.errstate(all="ignore"):
        S = _lane_sums(np.where(member, error[None, :], 0.0))
        mean = S / n.astype(np.float64)
        d = error[None, :] - mean[:, None]
        D = _lane_sums(np.where(member, d * d, 0.0))
        sd = np.sqrt(D / n.astype(np.float64))
    mean[n == 0], sd[n == 0] = np.nan, np.nan
    return n, _canonical(mean), _canonical(sd)


def literal_numpy(q: Dict[str, np.ndarray], k: Dict[str, np.ndarray], passes: List[str]) -> Dict[str, object]:
    """The reference's procedure, pair by pair in plain Python: per (pass, type) the queries and keys of that pass and type
    (define_model_error_distributions' loop); a pair joins when the years agree and the closed boxes intersect; spatial_overlap =
    intersection area / query area * 100; the pairs of a query are sorted by it, descending (equal: the smaller key row), the first is kept
    and area_dif = key area - query area.  -> {"match" [Q], "error" [Q], "errors": {(pass, type): [area_dif, ...]}}."""
    Q = q["box"].shape[0]
    match, error = np.full(Q, -1, np.int64), np.full(Q, np.nan)
    errors: Dict[Tuple[str, str], List[float]] = {}
    q_pass = [facilities.image_pass(int(y)) for y in q["year"]]
    k_pass = [facilities.image_pass(int(y)) for y in k["year"]]
    for p in passes:
        for square, kind in enumerate(FARM_TYPES):
            keys = [j for j in range(k["box"].shape[0]) if k_pass[j] == p and bool(k["square"][j]) == bool(square)]
            difs = errors.setdefault((p, kind), [])
            for i in range(Q):
                if q_pass[i] != p or bool(q["square"][i]) != bool(square):
                    continue
                x0, y0, x1, y1 = (float(v) for v in q["box"][i])
                joined = []
                for j in keys:
                    a0, b0, a1, b1 = (float(v) for v in k["box"][j])
                    if int(k["year"][j]) != int(q["year"][i]) or not (a0 <= x1 and x0 <= a1 and b0 <= y1 and y0 <= b1):
                        continue
                    inter = (min(x1, a1) - max(x0, a0)) * (min(y1, b1) - max(y0, b0))
                    joined.append((-(inter / ((x1 - x0) * (y1 - y0)) * 100), j))
                if not joined:
                    continue
                joined.sort()
                j = joined[0][1]
                match[i], error[i] = j, float(k["area"][j]) - float(q["area"][i])
                difs.append(error[i])
    return {"match": match, "error": error, "errors": errors}


# ---- the table ----

def distributions(table: Dict[str, np.ndarray], truth: Dict[str, np.ndarray], conf: float, keep=None, cpu: bool = False,
                  widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT, times: Optional[dict] = None) -> Dict[str, object]:
    """The error table of geocode's detection `table` against load_truth_geojson's `truth` at threshold `conf` (the module's docstring).
    -> passes, groups [(pass, farm_type)] with n, mean, sd per group; errors {(pass, farm_type): (mean, sd)} of the groups with n > 0 (what
    tonnage.build_table takes); empty [(pass, farm_type)]; and per query rows (row numbers of `table`), match (row numbers of `truth`),
    overlap, error, area, area_label.  cpu = the numpy restatement instead of the GPU.  times = a dict that receives "sort_ms" and
    "kernel_ms" (GPU: HIP events)."""
    s = samples(table, truth, float(conf), keep, widths, heights)
    q, k, passes = s["q"], s["k"], s["passes"]
    M = 2 * len(passes)
    if cpu:
        match, overlap, error = match_numpy(q["box"], q["group"], q["area"], k["box"], k["group"], k["area"])
        n, mean, sd = moments_numpy(error, match, q["mgroup"], M)
    else:
        import torch
        from . import engine
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
        tm = {} if times is not None else None
        m_d, o_d, e_d = engine.model_error_match(dev(q["box"]), dev(q["group"]), dev(q["area"]), dev(k["box"]), dev(k["group"]), dev(k["area"]),
                                                 s["G"], times=tm)
        tm2 = {} if times is not None else None
        n_d, mean_d, sd_d = engine.model_error_moments(e_d, m_d, dev(q["mgroup"]), M, times=tm2)
        if times is not None:
            times["sort_ms"] = tm.get("sort_ms", 0.0)
            times["kernel_ms"] = tm.get("kernel_ms", 0.0) + tm2.get("kernel_ms", 0.0)
        match, overlap, error = m_d.cpu().numpy(), o_d.cpu().numpy(), e_d.cpu().numpy()
        n, mean, sd = n_d.cpu().numpy(), mean_d.cpu().numpy(), sd_d.cpu().numpy()
    groups = [(p, t) for p in passes for t in FARM_TYPES]
    has = match >= 0
    lab_rows = np.where(has, k["rows"][np.maximum(match, 0)] if k["rows"].shape[0] else -1, -1).astype(np.int64)
    area_label = np.where(has, k["area"][np.maximum(match, 0)] if k["area"].shape[0] else np.nan, np.nan)
    return {"conf": float(conf), "passes": passes, "groups": groups, "n": n, "mean": mean, "sd": sd,
            "errors": {g: (float(mean[i]), float(sd[i])) for i, g in enumerate(groups) if n[i] > 0},
            "empty": [g for i, g in enumerate(groups) if n[i] == 0],
            "rows": q["rows"], "match": lab_rows, "overlap": overlap, "error": error, "area": q["area"], "area_label": area_label,
            "feature": np.asarray(truth["feature"], np.int64) if "feature" in truth else np.arange(np.asarray(truth["cls"]).shape[0]),
            "n_queries": int(match.shape[0]), "n_labels": int(k["area"].shape[0]), "n_matched": int(has.sum()), "n_members": int(n.sum())}


# ---- files ----

def write_errors_csv(path: str, res: Dict[str, object]) -> int:
    """model_errors.csv: pass, farm_type, model_error_mean, model_error_sd (the columns tonnage.read_errors takes as --tonnage-errors) and n;
    the doubles as ``repr``; groups with n = 0 are left out."""
    rows = 0
    with open(path, "w") as f:
        f.write("pass,farm_type,model_error_mean,model_error_sd,n\n")
        for i, (p, t) in enumerate(res["groups"]):
            if res["n"][i] > 0:
                f.write(f"{p},{t},{float(res['mean'][i])!r},{float(res['sd'][i])!r},{int(res['n'][i])}\n")
                rows += 1
    return rows


def write_cages_csv(path: str, res: Dict[str, object]) -> int:
    """model_error_cages.csv, the matched detections: index (row of detections.geojson), label (feature number of the truth file), overlap,
    area, area_label, error; the doubles as ``repr``, NaN empty."""
    num = lambda v: "" if v != v else repr(float(v))
    at = np.nonzero(res["match"] >= 0)[0]
    with open(path, "w") as f:
        f.write("index,label,overlap,area,area_label,error\n")
        for i in at.tolist():
            f.write(f"{int(res['rows'][i])},{int(res['feature'][res['match'][i]])},{num(res['overlap'][i])},{num(res['area'][i])},"
                    f"{num(res['area_label'][i])},{num(res['error'][i])}\n")
    return int(at.shape[0])


def summary(res: Dict[str, object], truth_path: Optional[str], cpu: bool) -> dict:
    """What model_errors.json holds: the parameters, the counts, the groups and the empty ones, the device."""
    device = "cpu"
    if not cpu:
        import torch
        device = torch.cuda.get_device_name(0)
    num = lambda v: None if v != v else float(v)
    return {"conf": res["conf"], "truth": os.path.basename(truth_path) if truth_path else None, "device": device, "cpu": bool(cpu),
            "n_detections": res["n_queries"], "n_labels": res["n_labels"], "n_matched": res["n_matched"], "n_members": res["n_members"],
            "passes": list(res["passes"]),
            "groups": [{"pass": p, "farm_type": t, "n": int(res["n"][i]), "model_error_mean": num(res["mean"][i]), "model_error_sd": num(res["sd"][i])}
                       for i, (p, t) in enumerate(res["groups"]) if res["n"][i] > 0],
            "empty": [list(g) for g in res["empty"]]}


def model_errors_from_table(table: Dict[str, np.ndarray], truth_path: str, out_dir: str, conf: float = 0.5, keep=None, cpu: bool = False,
                            widths=geocode.IM_WIDTH, heights=geocode.IM_HEIGHT, times: Optional[dict] = None,
                            dedup_overlaps: Optional[str] = None) -> Dict[str, object]:
    """load_truth_geojson, distributions() and the three files in out_dir -> distributions()' result.  dedup_overlaps = the download-box
    file: the labels pass through overlaps.filter_truth first."""
    from . import overlaps
    res = distributions(table, overlaps.filter_truth(load_truth_geojson(truth_path), dedup_overlaps, cpu=cpu), conf, keep, cpu, widths, heights, times)
    t0 = time.perf_counter()
    os.makedirs(out_dir, exist_ok=True)
    write_errors_csv(os.path.join(out_dir, CSV_FILE), res)
    write_cages_csv(os.path.join(out_dir, CAGES_FILE), res)
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump(summary(res, truth_path, cpu), f, indent=1)
        f.write("\n")
    if times is not None:
        times["files_ms"] = (time.perf_counter() - t0) * 1e3
    return res


def describe(res: Dict[str, object]) -> str:
    parts = [f"{p} {t} {float(res['mean'][i]):.1f} m2 (sd {float(res['sd'][i]):.1f}, n {int(res['n'][i])})"
             for i, (p, t) in enumerate(res["groups"]) if res["n"][i] > 0]
    return (f"model errors: {res['n_matched']} of {res['n_queries']} detections above {res['conf']:g} matched to {res['n_labels']} labels, "
            f"{len(parts)} groups" + (": " + ", ".join(parts) if parts else "") + (f"; {len(res['empty'])} empty" if res["empty"] else ""))


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--model-errors-conf", type=float, default=None, metavar="CONF",
                   help="detections with det_conf > CONF take part, strictly (reference confidence_threshold; default --facilities-conf)")
    p.add_argument("--model-errors-out", default=None, metavar="DIR", help=f"where {CSV_FILE}, {CAGES_FILE} and {JSON_FILE} go")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.model_errors",
                                description="The model's cage-area error per image pass and cage type, from the detections of an existing label "
                                            "directory and human labels, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--truth", required=True, metavar="GEOJSON", help="the human labels (reference output/humanlabels.geojson)")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea take part (the land filter)")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the detections' circle areas)")
    p.add_argument("--cpu", action="store_true", help="the numpy restatement instead of the GPU (the same bytes)")
    add_options(p)
    facilities.add_options(p)
    opt = p.parse_args(argv)
    out_dir = opt.model_errors_out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land is not None:
        from . import land
        keep = land.ocean_rows(table, land.load_land_geojson(opt.land), cpu=opt.cpu)
    conf = opt.facilities_conf if opt.model_errors_conf is None else opt.model_errors_conf
    try:
        res = model_errors_from_table(table, opt.truth, out_dir, conf, keep, opt.cpu, opt.image_size[0], opt.image_size[1])
    except ValueError as e:
        p.error(str(e))
    print(describe(res) + f" in {out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
