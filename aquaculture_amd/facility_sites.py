"""Known and additional facilities (``detect.py --facility-sites``, ``python -m aquaculture_amd.facility_sites``).

The data behind the reference's map of production locations (src/Results/FacilitiesMaps.py: get_true_facilities :64-94,
classify_our_facilities :117-188, count_unique_locations :97-114): which facilities lie within 1 km of a site the literature already knew
(Trujillo et al.), which are additional production locations, and how many distinct additional locations there are once a site seen in
several years or passes is counted once.  The plots and basemaps are not made here.  The definitions (DESIGN.md section 25,
include/aq_engine.h):

All boxes are closed, (x0, y0, x1, y1), fp64, EPSG:3857.  meet(a, b) = a.x0 <= b.x1 and b.x0 <= a.x1 and a.y0 <= b.y1 and b.y0 <= a.y1
(csrc/box_join.h's boxes_meet): touching counts, a NaN meets nothing.

1. Bounds.  bounds[f] = the minimum of xmin_3857 and ymin_3857 and the maximum of xmax_3857 and ymax_3857 over the facility's cage_ids whose
   class is circle_farm or square_farm (the reference boxes square_farm_geoms U circle_farm_geoms, :84-86: rectangle cages do not enter).
   Minima and maxima are selections ``v < m ? v : m`` from +inf and ``v > m ? v : m`` from -inf: a NaN coordinate is never selected.  A
   facility without such a cage, or one of whose selections is not finite, gets four NaNs and state ``no_bounds``.
2. Pass.  The facility's ``pass`` column, or facilities.image_pass(year) when the table is by year.  EARLY = 2000-2004, 2005-2009,
   2010-2012 (:145); LATE = 2013-2015, 2016-2018, 2019-2021 (:170); any other pass: state ``no_period``.
3. True facilities, only with a truth file.  The labels come from evaluate.load_truth_geojson, which keeps circle_cage and square_cage
   labels; the reference does not filter the types, and the file it ships holds only these two.  A label's group is the pass of its year,
   a facility's its pass.  label_hits[f] = the labels of f's group that bounds[f] meets, first_label[f] = the smallest such label row, or
   -1.  label_hits = 0: state ``not_true`` (the reference's sjoin, ``pass == cf_pass`` and drop_duplicates, :88-92).  Without a truth file
   every bounded facility of a period goes on and the two label columns are empty.
4. Sites.  The rows of the site file are grouped by distinct (lat, lon) in ascending order (pandas' groupby order, :50-52); num_cages is
   summed with min_count = 1: null only for a site without a parseable value, and for every site if the column is absent.  Only the sites
   whose EPSG:3857 point lies inside the closed total bounds of the wanted-bboxes table are used (:46-48); their number in that order is
   site_index.  The site box is missing.site_regions' rectangle: +-kfold.SITE_HALF_SIDE in EPSG:3857.  site_hits[f] and first_site[f] as in
   3, with one group.
5. Type.  Early pass: site_hits = 0 gives ``additional``, site_hits > 0 gives ``known_early``, which is not in the combined table, because
   the reference shows the sites themselves for those passes.  Late pass: ``known`` if site_hits > 0, else ``additional`` (:171-175).
6. Unique locations, separately for the early additional set and the late additional set.  N(i) = the j of the set with meet(bounds[i],
   bounds[j]); the pass is not compared, as in the reference's self-sjoin (:103); i is in N(i).  In ascending facility_index: an unmarked i is
   ``unique`` and every member of N(i) is marked.  location[i] = i if unique, else the smallest unique g < i with i in N(g).  The two
   counts of unique facilities are the numbers the reference prints (:152-153, :177-179).  The walk is sequential and runs on the host over
   the neighbour lists the device wrote.

Every step exists in three forms: the kernels (csrc/facility_sites.hip through engine.facility_bounds, box_join_count, box_join_list), their
numpy restatements (bounds_numpy, join_count_numpy, join_list_numpy: the same bytes; what cpu=True / ``--cpu`` runs) and classify_literal, the
reference's procedure in plain loops and pandas, written independently: the yardstick of the tests.

What differs from the reference:
  * the site box is the +-1000 m rectangle in EPSG:3857 this project has used since --evaluate-kfold; the reference builds its 1 km box in
    EPSG:3035 and reprojects the quadrilateral (a few metres at these latitudes, and the box is then some 1.37 km wide on the ground);
  * the late table is written in ascending facility_index; the reference sorts it by the site index, descending, with an unstable sort;
  * num_cages of a site without a parseable value is null, where the reference's ``sum()`` gives 0; cage_bin is null outside the bins,
    where the reference writes the string "nan";
  * the combined table also carries facility_index, first_site, unique and location, and the per-facility table is a file of its own.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time
from typing import Callable, Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import evaluate, facilities, geocode

EARLY = ("2000-2004", "2005-2009", "2010-2012")             # the study period of the known sites (reference :145)
LATE = ("2013-2015", "2016-2018", "2019-2021")              # (:170)
PASSES = EARLY + LATE
STATES = ("no_bounds", "no_period", "not_true", "additional", "known", "known_early")
TYPE_NAMES = {"additional": "Additional facility", "known": "Known facility"}
CAGE_BINS = np.asarray([0.0, 50.0, 100.0, 500.0])          # reference plot_map: pandas.cut(num_cages, [0, 50, 100, 500])
CAGE_BIN_NAMES = ("(0, 50]", "(50, 100]", "(100, 500]")
GEOJSON_FILE, CSV_FILE, JSON_FILE = "facility_sites.geojson", "facility_sites.csv", "facility_sites.json"
CSV_COLUMNS = ("facility_index", "pass", "state", "x0", "y0", "x1", "y1", "num_cages", "label_hits", "first_label", "site_hits", "first_site",
               "unique", "location")
LANES = 64


# ---- inputs ----

def facility_passes(fac: Dict[str, list]) -> List[str]:
    """The pass of every facility: its ``pass`` column, or image_pass(year) of a table clustered by year."""
    if "pass" in fac:
        return [str(p) for p in fac["pass"]]
    return [facilities.image_pass(int(y)) for y in fac["year"]]


def entries(fac: Dict[str, list], table: Dict[str, np.ndarray]) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """The facilities' cages as aq_facility_bounds_f64 takes them -> (entry_start int32 [F + 1], entry_box float64 [E, 4], entry_use uint8 [E]:
    1 for a circle or square cage).  A cage id outside the table is an entry that does not take part."""
    ids = [np.asarray(c, np.int64).reshape(-1) for c in fac["cage_ids"]]
    start = np.zeros(len(ids) + 1, np.int64)
    np.cumsum([c.shape[0] for c in ids], out=start[1:])
    if start[-1] >= 1 << 31:
        raise ValueError(f"facility sites: {start[-1]} cage entries (fewer than 2^31)")
    flat = np.concatenate(ids) if ids else np.zeros(0, np.int64)
    box = np.stack([np.asarray(table[c], np.float64) for c in evaluate.BOX_COLUMNS], 1).reshape(-1, 4)
    n = box.shape[0]
    inside = (flat >= 0) & (flat < n)
    at = np.where(inside, flat, 0)
    use = inside & np.isin(np.asarray(table["cls"], np.int64)[at] if n else np.zeros(flat.shape[0], np.int64), evaluate.CAGE_CLASSES)
    entry_box = box[at] if n else np.full((flat.shape[0], 4), np.nan)
    return start.astype(np.int32), np.ascontiguousarray(entry_box, dtype=np.float64).reshape(-1, 4), np.ascontiguousarray(use, dtype=np.uint8)


def read_sites(path: str) -> Dict[str, np.ndarray]:
    """The site file (reference data/aquaculture_med_dedupe.csv: lat, lon in degrees and num_cages, other columns ignored), its rows grouped by
    distinct (lat, lon) in ascending order -> lat, lon, num_cages (float64, the sum of the group's parseable values, NaN without one or
    without the column), xy float64 [n, 2] in EPSG:3857, and rows: the number of rows read.  A row without lat or lon is skipped."""
    with open(path, newline="") as f:
        r = csv.reader(f)
        header = [h.strip() for h in next(r)]
        if "lat" not in header or "lon" not in header:
            raise ValueError(f"{path}: the known sites need columns lat and lon")
        a, o = header.index("lat"), header.index("lon")
        c = header.index("num_cages") if "num_cages" in header else -1
        rows = []
        for row in r:
            if len(row) <= max(a, o) or not row[a].strip() or not row[o].strip():
                continue
            try:
                v = float(row[c]) if 0 <= c < len(row) and row[c].strip() else float("nan")
            except ValueError:
                v = float("nan")
            rows.append((float(row[a]), float(row[o]), v))
    t = np.asarray(rows, np.float64).reshape(-1, 3)
    keys, inverse = np.unique(t[:, :2], axis=0, return_inverse=True)             # sorted by lat, then lon
    inverse = np.asarray(inverse).reshape(-1)
    num = np.full(keys.shape[0], np.nan)
    for k, v in zip(inverse.tolist(), t[:, 2].tolist()):                          # in file order; min_count = 1: a NaN adds nothing
        if v == v:
            num[k] = v if num[k] != num[k] else num[k] + v
    x, y = geocode.lonlat_to_mercator(keys[:, 1], keys[:, 0])
    return {"lat": keys[:, 0].copy(), "lon": keys[:, 1].copy(), "num_cages": num, "rows": int(t.shape[0]),
            "xy": np.ascontiguousarray(np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1)).reshape(-1, 2)}


def total_bounds(wanted: Dict[int, Tuple[float, float, float, float]]) -> Tuple[float, float, float, float]:
    """The rectangle around every box of geocode.load_wanted_bboxes' table (geopandas' total_bounds)."""
    b = np.asarray(list(wanted.values()), np.float64).reshape(-1, 4)
    if b.shape[0] == 0:
        return (float("nan"),) * 4
    return float(b[:, 0].min()), float(b[:, 1].min()), float(b[:, 2].max()), float(b[:, 3].max())


def site_table(sites_csv: str, wanted: Dict[int, Tuple[float, float, float, float]]) -> Dict[str, object]:
    """read_sites cut to the sites inside the closed total bounds of `wanted`, in their order (the position is site_index), with ``box`` float64
    [n, 4] (missing.site_regions' rectangles), ``read`` (the distinct sites of the file) and ``rows``."""
    from . import missing
    s = read_sites(sites_csv)
    x0, y0, x1, y1 = total_bounds(wanted)
    xy = s["xy"]
    inside = (xy[:, 0] >= x0) & (xy[:, 0] <= x1) & (xy[:, 1] >= y0) & (xy[:, 1] <= y1)
    out = {k: v[inside] for k, v in s.items() if k != "rows"}
    out["box"] = np.ascontiguousarray(missing.site_regions(out["xy"])["rect"], dtype=np.float64).reshape(-1, 4)
    out["read"], out["rows"], out["bounds"] = int(xy.shape[0]), s["rows"], [x0, y0, x1, y1]
    return out


def cage_bin(num_cages) -> List[Optional[str]]:
    """pandas.cut(num_cages, [0, 50, 100, 500]) as strings: "(0, 50]", "(50, 100]", "(100, 500]", None outside the bins and for NaN."""
    c = np.asarray(num_cages, np.float64).reshape(-1)
    k = np.searchsorted(CAGE_BINS, c, side="left")          # pandas' own step: bins.searchsorted(x, side="left"); 0 and len(bins) are NaN
    none = (k == 0) | (k == CAGE_BINS.shape[0]) | np.isnan(c)
    return [None if n else CAGE_BIN_NAMES[i - 1] for i, n in zip(k.tolist(), none.tolist())]


# ---- the numpy restatements of the three kernels ----

def _fold(m: np.ndarray, smaller: bool) -> np.ndarray:
    """[n, 64] -> [n]: lane 0's view of the six exchange steps: m[i] = m[i + h] < m[i] ? m[i + h] : m[i] for h = 32, 16, ... 1 (> for a maximum)."""
    h = LANES // 2
    while h >= 1:
        lo, hi = m[:, :h], m[:, h:2 * h]
        m = np.where(hi < lo if smaller else hi > lo, hi, lo)
        h //= 2
    return m[:, 0]


def bounds_numpy(entry_start, entry_box, entry_use, chunk: int = 4096) -> np.ndarray:
    """float64 [F, 4] of definition 1 without a GPU, in the kernel's order (engine.facility_bounds gives the same bytes): lane l of 64 walks
    the entries start + l, start + l + 64, ... keeping ``v < m ? v : m`` / ``v > m ? v : m``, the 64 partials fold by halves."""
    start = np.asarray(entry_start, np.int64).reshape(-1)
    box = np.asarray(entry_box, np.float64).reshape(-1, 4)
    use = np.asarray(entry_use).reshape(-1) != 0
    F, E = start.shape[0] - 1, box.shape[0]
    out = np.full((F, 4), np.nan)
    if E == 0:
        return out
    lanes = np.arange(LANES, dtype=np.int64)
    with np.errstate(invalid="ignore"):
        for at in range(0, F, chunk):
            to = min(at + chunk, F)
            a = np.minimum(np.maximum(start[at:to], 0), E)
            b = np.minimum(np.maximum(start[at + 1:to + 1], a), E)
            m = np.empty((a.shape[0], LANES, 4))
            m[:, :, :2], m[:, :, 2:] = np.inf, -np.inf
            for r in range(int(-(-(b - a).max() // LANES)) if a.shape[0] else 0):
                e = a[:, None] + (r * LANES + lanes)[None, :]
                part = e < b[:, None]
                e = np.minimum(e, E - 1)
                part &= use[e]
                c = box[e]
                for j in range(4):
                    take = part & (c[:, :, j] < m[:, :, j] if j < 2 else c[:, :, j] > m[:, :, j])
                    m[:, :, j] = np.where(take, c[:, :, j], m[:, :, j])
            res = np.stack([_fold(m[:, :, j], j < 2) for j in range(4)], 1)
            res[~np.isfinite(res).all(1)] = np.nan
            out[at:to] = res
    return out


def key_order(kbox, kgroup) -> np.ndarray:
    """engine.box_match_sort's order in numpy: by (group, x0), stable, a NaN x0 last in its group."""
    kbox = np.asarray(kbox, np.float64).reshape(-1, 4)
    by_x = np.argsort(kbox[:, 0], kind="stable")
    return by_x[np.argsort(np.asarray(kgroup, np.int64)[by_x], kind="stable")]


def _pairs(qbox, qgroup, kbox, kgroup, G: int, chunk: int = 256) -> Tuple[np.ndarray, np.ndarray]:
    """(query, key row) of every meeting pair of equal group in [0, G), ordered by query and, within a query, by the key's position in
    key_order.  A block of queries (in x order) is tested against the keys of its group that can reach it: those from the first whose
    running maximum of x1 reaches the block's smallest x0 up to the last with x0 <= the block's largest x1."""
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int64).reshape(-1), np.asarray(kgroup, np.int64).reshape(-1)
    order = key_order(kbox, kgroup)
    kg = kgroup[order]
    qs, ks = [], []
    ok = ~np.isnan(qbox).any(1) & (qgroup >= 0) & (qgroup < int(G))
    for g in np.unique(qgroup[ok]):
        ki = order[np.searchsorted(kg, g, side="left"):np.searchsorted(kg, g, side="right")]
        if ki.shape[0] == 0:
            continue
        qi = np.nonzero(ok & (qgroup == g))[0]
        qi = qi[np.argsort(qbox[qi, 0], kind="stable")]
        kb = kbox[ki]
        kx0 = kb[:, 0]
        reach = np.maximum.accumulate(np.where(np.isnan(kb[:, 2]), -np.inf, kb[:, 2]))
        for at in range(0, qi.shape[0], chunk):
            q = qi[at:at + chunk]
            lo = int(np.searchsorted(reach, qbox[q, 0].min(), side="left"))
            hi = int(np.searchsorted(kx0, qbox[q, 2].max(), side="right"))     # (NaN x0 sort last and are beyond every number)
            if hi <= lo:
                continue
            a, b = qbox[q][:, None, :], kb[lo:hi][None, :, :]
            with np.errstate(invalid="ignore"):
                meet = (a[..., 0] <= b[..., 2]) & (b[..., 0] <= a[..., 2]) & (a[..., 1] <= b[..., 3]) & (b[..., 1] <= a[..., 3])
            r, c = np.nonzero(meet)
            qs.append(q[r])
            ks.append(ki[lo + c])
    if not qs:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    qs, ks = np.concatenate(qs), np.concatenate(ks)
    by_q = np.argsort(qs, kind="stable")
    return qs[by_q], ks[by_q]


def join_count_numpy(qbox, qgroup, kbox, kgroup, G: int) -> Tuple[np.ndarray, np.ndarray]:
    """(count int32 [Q], first int32 [Q]) without a GPU (engine.box_join_count gives the same bytes): the keys of the query's group whose
    closed box meets the query's, and the smallest row among them, -1 without one."""
    Q = np.asarray(qbox).reshape(-1, 4).shape[0]
    qs, ks = _pairs(qbox, qgroup, kbox, kgroup, G)
    count = np.bincount(qs, minlength=Q).astype(np.int32)
    first = np.full(Q, np.iinfo(np.int64).max, np.int64)
    np.minimum.at(first, qs, ks)
    return count, np.where(count > 0, first, -1).astype(np.int32)


def join_list_numpy(qbox, qgroup, kbox, kgroup, G: int) -> Tuple[np.ndarray, np.ndarray]:
    """(offset int64 [Q + 1], list int32 [offset[Q]]) without a GPU (engine.box_join_list gives the same arrays): the rows of the keys that
    meet query q at list[offset[q] : offset[q + 1]], in the order of the sorted keys."""
    Q = np.asarray(qbox).reshape(-1, 4).shape[0]
    qs, ks = _pairs(qbox, qgroup, kbox, kgroup, G)
    offset = np.zeros(Q + 1, np.int64)
    np.cumsum(np.bincount(qs, minlength=Q), out=offset[1:])
    return offset, ks.astype(np.int32)


def _kernels(cpu: bool, times: Optional[dict]) -> Tuple[Callable, Callable, Callable]:
    """The three steps on numpy arrays -> (bounds, count, lists): the restatements, or the kernels with the copies to and from the device."""
    if cpu:
        return bounds_numpy, join_count_numpy, join_list_numpy
    import torch
    from . import engine
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a, dtype=dt)).cuda()

    def timed(fn, *args):
        tm = {} if times is not None else None
        out = fn(*args, times=tm)
        if times is not None:
            for k, v in tm.items():
                times[k] = times.get(k, 0.0) + v
        return out

    def bounds(entry_start, entry_box, entry_use):
        es = np.ascontiguousarray(entry_start, dtype=np.int32)
        return timed(engine.facility_bounds, dev(es, np.int32), dev(np.asarray(entry_box).reshape(-1, 4), np.float64),
                     dev(entry_use, np.uint8), es).cpu().numpy()

    def count(qbox, qgroup, kbox, kgroup, G):
        c, f = timed(engine.box_join_count, dev(np.asarray(qbox).reshape(-1, 4), np.float64), dev(qgroup, np.int32),
                     dev(np.asarray(kbox).reshape(-1, 4), np.float64), dev(kgroup, np.int32), int(G))
        return c.cpu().numpy(), f.cpu().numpy()

    def lists(qbox, qgroup, kbox, kgroup, G):
        off, lst = timed(engine.box_join_list, dev(np.asarray(qbox).reshape(-1, 4), np.float64), dev(qgroup, np.int32),
                         dev(np.asarray(kbox).reshape(-1, 4), np.float64), dev(kgroup, np.int32), int(G))
        return off, lst.cpu().numpy()

    return bounds, count, lists


# ---- the classification ----

def walk_unique(members: Sequence[int], offset, lst) -> Tuple[Dict[int, bool], Dict[int, int]]:
    """Definition 6 over one set: members = its facility indices in ascending order, (offset, lst) the neighbour lists as positions in
    `members` -> ({facility: unique}, {facility: location})."""
    n = len(members)
    marked = [False] * n
    unique, location = {}, {}
    for i in range(n):
        if marked[i]:
            unique[members[i]] = False
            continue
        unique[members[i]], location[members[i]] = True, members[i]
        for j in np.asarray(lst[int(offset[i]):int(offset[i + 1])]).tolist():
            if not marked[j]:
                marked[j] = True
                if j != i:
                    location[members[j]] = members[i]
    return unique, location


def _period(p: str) -> Optional[str]:
    return "early" if p in EARLY else "late" if p in LATE else None


def _result(fac, passes, bounds, state, label, site, unique, location, sites, truth_given: bool) -> Dict[str, object]:
    F = len(passes)
    counts: Dict[str, Dict[str, int]] = {}
    for p, s in zip(passes, state):
        counts.setdefault(p, {})[s] = counts.setdefault(p, {}).get(s, 0) + 1
    n_unique = {per: sum(1 for f in range(F) if state[f] == "additional" and _period(passes[f]) == per and unique.get(f)) for per in ("early", "late")}
    return {"facility_index": [int(v) for v in fac["facility_index"]], "pass": list(passes), "state": list(state),
            "bounds": np.asarray(bounds, np.float64).reshape(-1, 4), "num_cages": [len(c) for c in fac["cage_ids"]],
            "label_hits": None if not truth_given else np.asarray(label[0], np.int64), "first_label": None if not truth_given else np.asarray(label[1], np.int64),
            "site_hits": np.asarray(site[0], np.int64), "first_site": np.asarray(site[1], np.int64),
            "unique": [unique.get(f) for f in range(F)], "location": [location.get(f) for f in range(F)],
            "sites": sites, "counts": {p: dict(sorted(c.items())) for p, c in sorted(counts.items())},
            "unique_additional_early": n_unique["early"], "unique_additional_late": n_unique["late"]}


def label_groups(truth: Dict[str, np.ndarray]) -> np.ndarray:
    """int64 [L]: the position in PASSES of the pass of every label's year, -1 for a year outside every pass."""
    return np.asarray([PASSES.index(p) if p in PASSES else -1 for p in (facilities.image_pass(int(y)) for y in truth["year"])], np.int64).reshape(-1)


def classify(fac: Dict[str, list], table: Dict[str, np.ndarray], sites: Dict[str, object], truth: Optional[Dict[str, np.ndarray]] = None,
             cpu: bool = False, times: Optional[dict] = None) -> Dict[str, object]:
    """The six definitions of the module's docstring for the facility table `fac` (facilities.cluster's or dedup.cluster's) over geocode's
    detection `table`, site_table's `sites` and, optionally, evaluate.load_truth_geojson's `truth` -> per facility facility_index, pass,
    state, bounds [F, 4], num_cages, label_hits and first_label (None without truth), site_hits, first_site, unique and location (None
    outside the additional sets); ``sites``, ``counts`` {pass: {state: n}}, unique_additional_early and unique_additional_late.  cpu = the
    numpy restatements instead of the GPU.  times = a dict that receives "bounds_ms", "count_ms" and "list_ms" (GPU: HIP events, summed over
    the calls)."""
    bounds_fn, count_fn, lists_fn = _kernels(cpu, times)
    passes = facility_passes(fac)
    F = len(passes)
    bounds = bounds_fn(*entries(fac, table))
    group = np.asarray([PASSES.index(p) if p in PASSES else -1 for p in passes], np.int32).reshape(-1)
    label = None
    if truth is not None:
        lg = label_groups(truth)
        rows = np.nonzero(lg >= 0)[0]
        lbox = np.stack([np.asarray(truth[c], np.float64) for c in evaluate.BOX_COLUMNS], 1).reshape(-1, 4)[rows]
        hits, first = count_fn(bounds, group, lbox, lg[rows].astype(np.int32), len(PASSES))
        label = (hits.astype(np.int64), np.where(first >= 0, rows[np.maximum(first, 0)] if rows.shape[0] else -1, -1).astype(np.int64))
    site = count_fn(bounds, np.zeros(F, np.int32), sites["box"], np.zeros(sites["box"].shape[0], np.int32), 1)
    state = []
    for f in range(F):
        if np.isnan(bounds[f]).any():
            state.append("no_bounds")
        elif group[f] < 0:
            state.append("no_period")
        elif label is not None and label[0][f] == 0:
            state.append("not_true")
        elif passes[f] in EARLY:
            state.append("known_early" if site[0][f] > 0 else "additional")
        else:
            state.append("known" if site[0][f] > 0 else "additional")
    unique, location = {}, {}
    for per in ("early", "late"):
        members = [f for f in range(F) if state[f] == "additional" and _period(passes[f]) == per]
        if not members:
            continue
        b = np.ascontiguousarray(bounds[members])
        zero = np.zeros(len(members), np.int32)
        off, lst = lists_fn(b, zero, b, zero, 1)
        u, l = walk_unique(members, off, lst)
        unique.update(u)
        location.update(l)
    return _result(fac, passes, bounds, state, label, site, unique, location, sites, truth is not None)


def classify_literal(fac: Dict[str, list], table: Dict[str, np.ndarray], sites_csv: str, wanted: Dict[int, Tuple[float, float, float, float]],
                     truth: Optional[Dict[str, np.ndarray]] = None) -> Dict[str, object]:
    """The reference's procedure done literally, pair by pair in plain loops and pandas (the yardstick of the tests; it shares no step with
    classify): boxes from Python's comparisons, every spatial join a brute-force pair test and a left join, ``pass == cf_pass``,
    drop_duplicates, sort_values(ascending=False), and count_unique_locations' two lists as they stand.  -> classify's result."""
    import pandas as pd
    from .kfold import SITE_HALF_SIDE
    meet = lambda a, b: bool(a[0] <= b[2] and b[0] <= a[2] and a[1] <= b[3] and b[1] <= a[3])
    frame = lambda rows, cols: pd.DataFrame(np.asarray(rows, np.int64).reshape(-1, len(cols)), columns=cols)      # (int64 also when empty)
    passes = facility_passes(fac)
    F = len(passes)
    cls = np.asarray(table["cls"], np.int64)
    # get_true_facilities: box(*all_cages.bounds) of the square and circle cages
    bounds = []
    for f in range(F):
        x0, y0, x1, y1 = float("inf"), float("inf"), float("-inf"), float("-inf")
        for c in fac["cage_ids"][f]:
            if int(cls[c]) not in evaluate.CAGE_CLASSES:
                continue
            a0, b0, a1, b1 = (float(table[col][c]) for col in evaluate.BOX_COLUMNS)
            x0, y0 = (a0 if a0 < x0 else x0), (b0 if b0 < y0 else y0)
            x1, y1 = (a1 if a1 > x1 else x1), (b1 if b1 > y1 else y1)
        finite = all(np.isfinite(v) for v in (x0, y0, x1, y1))
        bounds.append((x0, y0, x1, y1) if finite else (float("nan"),) * 4)
    df = pd.DataFrame({"facility_index": list(range(F)), "pass": passes, "bounds": bounds, "cage_ids": list(fac["cage_ids"])})
    bounded = df[[not np.isnan(b[0]) for b in bounds]] if F else df
    label_hits = first_label = None
    if truth is not None:
        # .sjoin(cf_labels, how='left'); cf_pass; pass == cf_pass; drop_duplicates('facility_index')
        lbox = np.stack([np.asarray(truth[c], np.float64) for c in evaluate.BOX_COLUMNS], 1).reshape(-1, 4)
        right = [(int(r["facility_index"]), j, int(truth["year"][j])) for _, r in bounded.iterrows() for j in range(lbox.shape[0])
                 if meet(r["bounds"], lbox[j])]
        joined = bounded.merge(frame(right, ["facility_index", "label", "year"]), how="left", on="facility_index")
        joined["cf_pass"] = joined["year"].map(lambda y: None if pd.isnull(y) else facilities.image_pass(int(y)))
        joined = joined.loc[joined["pass"] == joined["cf_pass"]].copy()
        label_hits = np.asarray([int((joined["facility_index"] == f).sum()) for f in range(F)], np.int64)
        first_label = np.asarray([int(joined.loc[joined["facility_index"] == f, "label"].min()) if label_hits[f] else -1 for f in range(F)], np.int64)
        true = joined.drop_duplicates("facility_index")[["facility_index", "pass", "bounds", "cage_ids"]]
    else:
        true = bounded
    # define_Trujillo_locations: the rows inside the total bounds, grouped by (lat, lon)
    raw = pd.read_csv(sites_csv, float_precision="round_trip")
    if "num_cages" not in raw.columns:
        raw["num_cages"] = np.nan
    raw["num_cages"] = pd.to_numeric(raw["num_cages"], errors="coerce")
    raw = raw.dropna(subset=["lat", "lon"])
    x, y = geocode.lonlat_to_mercator(raw["lon"].to_numpy(np.float64), raw["lat"].to_numpy(np.float64))
    wb = np.asarray(list(wanted.values()), np.float64).reshape(-1, 4)
    xmin, ymin, xmax, ymax = wb[:, 0].min(), wb[:, 1].min(), wb[:, 2].max(), wb[:, 3].max()
    n_read = int(raw.groupby(["lat", "lon"]).ngroups)
    france = raw.loc[(x >= xmin) & (x <= xmax) & (y >= ymin) & (y <= ymax)]
    grouped = france.groupby(["lat", "lon"])["num_cages"].sum(min_count=1).reset_index()
    grouped["trujillo_facility_index"] = grouped.index
    sx, sy = geocode.lonlat_to_mercator(grouped["lon"].to_numpy(np.float64), grouped["lat"].to_numpy(np.float64))
    sx, sy = np.asarray(sx, np.float64).reshape(-1), np.asarray(sy, np.float64).reshape(-1)
    boxes = [(float(a) - SITE_HALF_SIDE, float(b) - SITE_HALF_SIDE, float(a) + SITE_HALF_SIDE, float(b) + SITE_HALF_SIDE) for a, b in zip(sx, sy)]

    def sjoin_sites(left):                                   # .sjoin(Trujillo_facility_boxes, how='left', predicate='intersects')
        right = [(int(r["facility_index"]), s) for _, r in left.iterrows() for s in range(len(boxes)) if meet(r["bounds"], boxes[s])]
        return left.merge(frame(right, ["facility_index", "trujillo_facility_index"]), how="left", on="facility_index")

    def count_unique_locations(fac_df):                      # :97-114, the bounds' self-join by brute force
        rows = [(int(a["facility_index"]), int(b["facility_index"])) for _, a in fac_df.iterrows() for _, b in fac_df.iterrows()
                if meet(a["bounds"], b["bounds"])]
        unique_facs = frame(rows, ["facility_index_left", "facility_index_right"])
        unique_facs = unique_facs.groupby("facility_index_left")["facility_index_right"].apply(lambda v: list(np.unique(v))).reset_index()
        unique_facilities, nonunique_facilities = [], []
        owner = {}
        for i in range(len(unique_facs)):
            row = unique_facs.iloc[i]
            if row["facility_index_left"] not in nonunique_facilities:
                unique_facilities.append(row["facility_index_left"])
                for j in row["facility_index_right"]:
                    if j not in nonunique_facilities:
                        owner[int(j)] = int(row["facility_index_left"])
                nonunique_facilities.extend(row["facility_index_right"])
        return [int(v) for v in unique_facilities], owner

    early = true.loc[true["pass"].isin(list(EARLY))].copy()
    early_joined = sjoin_sites(early)
    add_early = early_joined.loc[early_joined["trujillo_facility_index"].isna()].drop_duplicates("facility_index")
    late = true.loc[true["pass"].isin(list(LATE))].copy()
    late_joined = sjoin_sites(late)
    late_first = late_joined.sort_values("trujillo_facility_index", ascending=False).drop_duplicates("facility_index")
    add_late = late_first.loc[late_first["trujillo_facility_index"].isnull()].sort_values("facility_index")
    state = ["no_bounds" if np.isnan(bounds[f][0]) else "no_period" if passes[f] not in PASSES else "not_true" for f in range(F)]
    for f in true["facility_index"].tolist():
        if passes[f] in PASSES:
            state[f] = "known_early" if passes[f] in EARLY else "known"
    for f in add_early["facility_index"].tolist() + add_late["facility_index"].tolist():
        state[f] = "additional"
    site_hits, first_site = np.zeros(F, np.int64), np.full(F, -1, np.int64)
    for f in range(F):
        hit = [s for s in range(len(boxes)) if meet(bounds[f], boxes[s])]
        site_hits[f], first_site[f] = len(hit), min(hit) if hit else -1
    unique, location = {}, {}
    for add in (add_early, add_late):
        uniq, owner = count_unique_locations(add)
        for f in add["facility_index"].tolist():
            unique[f], location[f] = f in uniq, owner[f]
    sites = {"lat": grouped["lat"].to_numpy(np.float64), "lon": grouped["lon"].to_numpy(np.float64), "num_cages": grouped["num_cages"].to_numpy(np.float64),
             "xy": np.stack([sx, sy], 1).reshape(-1, 2), "box": np.asarray(boxes, np.float64).reshape(-1, 4), "read": n_read, "rows": int(raw.shape[0]),
             "bounds": [float(xmin), float(ymin), float(xmax), float(ymax)]}
    return _result(fac, passes, np.asarray(bounds, np.float64).reshape(-1, 4), state, (label_hits, first_label), (site_hits, first_site),
                   unique, location, sites, truth is not None)


# ---- files ----

def _num(v):
    return None if v is None or v != v else (int(v) if float(v).is_integer() else float(v))


def combined_features(res: Dict[str, object]) -> List[dict]:
    """The combined table (reference :158-187) as GeoJSON features: the early additional facilities, the sites once per early pass, the late
    known and additional facilities; facilities in ascending facility_index."""
    b = res["bounds"]
    sites = res["sites"]

    def facility(f):
        n = res["num_cages"][f]
        return {"type": "Feature", "properties": {"type": TYPE_NAMES[res["state"][f]], "pass": res["pass"][f], "num_cages": n, "cage_bin": cage_bin([n])[0],
                                                  "facility_index": res["facility_index"][f], "first_site": int(res["first_site"][f]),
                                                  "unique": res["unique"][f], "location": res["location"][f]},
                "geometry": {"type": "Point", "coordinates": [0.5 * (float(b[f, 0]) + float(b[f, 2])), 0.5 * (float(b[f, 1]) + float(b[f, 3]))]}}

    F = len(res["pass"])
    feats = [facility(f) for f in range(F) if res["state"][f] == "additional" and res["pass"][f] in EARLY]
    bins = cage_bin(sites["num_cages"])
    for p in EARLY:
        for s in range(sites["box"].shape[0]):
            feats.append({"type": "Feature", "properties": {"type": TYPE_NAMES["known"], "pass": p, "num_cages": _num(sites["num_cages"][s]),
                                                            "cage_bin": bins[s], "site_index": s},
                          "geometry": {"type": "Point", "coordinates": [float(sites["xy"][s, 0]), float(sites["xy"][s, 1])]}})
    feats += [facility(f) for f in range(F) if res["state"][f] in TYPE_NAMES and res["pass"][f] in LATE]
    return feats


def write_geojson(path: str, res: Dict[str, object]) -> int:
    feats = combined_features(res)
    with open(path, "w") as f:
        json.dump({"type": "FeatureCollection", "crs": facilities._CRS_3857, "features": feats}, f)
        f.write("\n")
    return len(feats)


def write_csv(path: str, res: Dict[str, object]) -> int:
    """facility_sites.csv: one row per facility, CSV_COLUMNS; the doubles as ``repr``, what is not defined empty, unique as 0 / 1."""
    num = lambda v: "" if v != v else repr(float(v))
    opt = lambda v: "" if v is None else str(int(v))
    F = len(res["pass"])
    with open(path, "w") as f:
        f.write(",".join(CSV_COLUMNS) + "\n")
        for k in range(F):
            lab = ("", "") if res["label_hits"] is None else (str(int(res["label_hits"][k])), str(int(res["first_label"][k])))
            f.write(f"{res['facility_index'][k]},{res['pass'][k]},{res['state'][k]}," + ",".join(num(v) for v in res["bounds"][k]) +
                    f",{res['num_cages'][k]},{lab[0]},{lab[1]},{int(res['site_hits'][k])},{int(res['first_site'][k])},"
                    f"{opt(res['unique'][k])},{opt(res['location'][k])}\n")
    return F


def summary(res: Dict[str, object], opts: dict, cpu: bool) -> dict:
    """What facility_sites.json holds: the parameters and the files read, the sites read and in bounds, the counts per pass and state, the
    two unique counts, the device."""
    device = "cpu"
    if not cpu:
        import torch
        device = torch.cuda.get_device_name(0)
    from .kfold import SITE_HALF_SIDE
    base = lambda p: os.path.basename(p) if p else None
    return {"sites": base(opts.get("sites")), "bboxes": base(opts.get("bboxes")), "truth": base(opts.get("truth")),
            "site_half_side": float(SITE_HALF_SIDE),
            "early": list(EARLY), "late": list(LATE), "total_bounds": res["sites"]["bounds"],
            "site_rows": res["sites"]["rows"], "sites_read": res["sites"]["read"], "sites_in_bounds": int(res["sites"]["box"].shape[0]),
            "facilities": len(res["pass"]), "counts": res["counts"],
            "unique_additional_early": res["unique_additional_early"], "unique_additional_late": res["unique_additional_late"],
            "device": device, "cpu": bool(cpu)}


def facility_sites_from_table(fac: Dict[str, list], table: Dict[str, np.ndarray], sites_csv: str, bboxes_csv: str, out_dir: str,
                              truth_path: Optional[str] = None, cpu: bool = False, times: Optional[dict] = None) -> Dict[str, object]:
    """site_table, classify() and the three files in out_dir -> classify's result."""
    sites = site_table(sites_csv, geocode.load_wanted_bboxes(bboxes_csv))
    truth = evaluate.load_truth_geojson(truth_path) if truth_path else None
    res = classify(fac, table, sites, truth, cpu, times)
    t0 = time.perf_counter()
    os.makedirs(out_dir, exist_ok=True)
    write_geojson(os.path.join(out_dir, GEOJSON_FILE), res)
    write_csv(os.path.join(out_dir, CSV_FILE), res)
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump(summary(res, {"sites": sites_csv, "bboxes": bboxes_csv, "truth": truth_path}, cpu), f, indent=1)
        f.write("\n")
    if times is not None:
        times["files_ms"] = (time.perf_counter() - t0) * 1e3
    return res


def describe(res: Dict[str, object]) -> str:
    n = {s: sum(1 for v in res["state"] if v == s) for s in STATES}
    return (f"facility sites: {len(res['pass'])} facilities against {res['sites']['box'].shape[0]} of {res['sites']['read']} known sites: "
            f"{n['known']} known, {n['known_early']} at a known site in its study period, {n['additional']} additional "
            f"({res['unique_additional_early']} unique locations early, {res['unique_additional_late']} late)"
            + "".join(f", {n[s]} {s}" for s in ("not_true", "no_period", "no_bounds") if n[s]))


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--facility-sites-truth", default=None, metavar="GEOJSON",
                   help="human labels (reference output/humanlabels.geojson): only the facilities whose rectangle meets a label of their pass take part")
    p.add_argument("--facility-sites-out", default=None, metavar="DIR", help=f"where {GEOJSON_FILE}, {CSV_FILE} and {JSON_FILE} go")


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.facility_sites",
                                description="Which facilities of an existing label directory lie at a known site and which are additional "
                                            "production locations, without running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--sites", required=True, metavar="CSV", help="the known sites (reference data/aquaculture_med_dedupe.csv: lat, lon, num_cages)")
    p.add_argument("--truth", default=None, metavar="GEOJSON", help="the human labels (reference output/humanlabels.geojson)")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: only the detections at sea are clustered (the land filter)")
    p.add_argument("--out", default=None, metavar="DIR", help="default <labels>/..")
    p.add_argument("--image-size", nargs=2, type=int, default=[geocode.IM_WIDTH, geocode.IM_HEIGHT], metavar=("W", "H"),
                   help="pixel size of the images (the border test of the circle areas)")
    p.add_argument("--cpu", action="store_true", help="the numpy restatements instead of the GPU (the same bytes)")
    facilities.add_options(p)
    opt = p.parse_args(argv)
    out_dir = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.land is not None:
        from . import land
        keep = land.ocean_rows(table, land.load_land_geojson(opt.land), cpu=opt.cpu)
    fac = facilities.cluster(table, opt.facilities_by, opt.facilities_conf, opt.facilities_eps, opt.facilities_min_cages, opt.image_size[0],
                             opt.image_size[1], labels_fn=facilities.dbscan_numpy if opt.cpu else None, keep=keep)
    try:
        res = facility_sites_from_table(fac, table, opt.sites, opt.geocode_bboxes, out_dir, opt.truth, opt.cpu)
    except ValueError as e:
        p.error(str(e))
    print(describe(res) + f" in {out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
