"""The numbers behind the reference's accuracy section (``detect.py --performance``, ``python -m aquaculture_amd.performance``): the stage curves
of its Figure 3, the strata table, and the upper bound on the cage population.

1. The curves (reference src/Results/ModelPerformance.py:108-167).  Precision and recall against the confidence threshold for three nested
   sets of the sampled images' circle and square detections -- ``all``, ``ocean`` (the image is not wholly on land: the reference's
   ``bucket != 'land'``, a rule per image, not the box-level land filter) and ``ocean + clustered`` (DBSCAN label >= 0, clustered ONCE per
   year at one distance and size over every ocean detection whatever its confidence, then thresholded; ``--evaluate`` thresholds first and
   clusters afterwards, over a grid) -- against ALL labels, as get_stats_total does.  With g = year_id * 2 + square (evaluate.inputs):

       tp_i        detection i meets a label of its group (one engine.box_match; independent of threshold and domain)
       R[l, d]     the largest confidence among the detections of domain d that meet label l (one engine.box_match, labels as queries,
                   payload [n, 3]: the confidence where the detection is in the domain, -inf elsewhere)
       at t        n_pred = #{i in d : c_i >= t}   n_pred_tp = #{i in d : c_i >= t and tp_i}   n_label_tp = #{l : R[l, d] >= t}
                   precision = n_pred_tp / n_pred (empty where n_pred = 0: pandas' mean of nothing is NaN)   recall = n_label_tp / n_label

   Every comparison is the reference's own fp64 >= on an unchanged input confidence, so the counts are exact.  The counts come from the sort
   and searchsorted of evaluate.py.  Also: ``fp_share_raw`` = 100 - 100 sum(tp) / n over ``all`` and ``land_fp_dropped`` = 100 - 100 (false
   positives in ocean) / (false positives in all), the two lines the reference prints first, and the rows it prints last (reported_rows).

2. The strata table (get_bucket_info_table, src/get_kfold_cluster_performance.py:225-256) over kfold.image_table: images, detections and
   labels per stratum for the whole image list and for the labelled sample, and estimated_num_labels_bucket = num_labels_sample /
   num_images_sample * num_images_bucket in that order in fp64 (empty where the stratum has no sampled image).  The images wholly on land
   form the row ``land`` and count as sampled, as the reference appends them to its sample (:88-92).  Labels of images outside the sample do
   not count (set_image_stats blanks them).

3. The population bound (reference src/Results/upper_bound_calculation.R).  For each rate r: if a fraction r of the images of the stratum "No
   detection, outside known area" held cages, how many positives would a sample of S of them hold?  K samples of S Bernoulli draws; the
   int(K / 2)-th smallest count (``all_zeros_50``); the smallest rate where that is not zero gives round(r I) cages_per_image + the labels
   of all other strata (``land`` excluded), with I and S the stratum's images and sampled images (the R script hard-codes 783355, 10518 and
   4010).  The draws come from the GPU (csrc/population.hip through engine.bernoulli_counts; include/aq_engine.h states the draw),
   counts_numpy restates them with tonnage.philox4x32, and the order statistic is torch's sort on the device.  ``zero_share`` = the share of
   samples without a positive is what the R comment talks about ("with 50% probability a sample of all zeros") and is reported beside it.

   ONE DELIBERATE DIFFERENCE from the R script: all rates are tested against the SAME uniforms (common random numbers).  The draw is made
   once and compared with every rate, so every simulation's counts are non-decreasing in the rate and the reported curve is monotone, at a
   tenth of the work; the R script draws afresh per rate.  (And the generator is Philox with a seed, not R's Mersenne twister.)

``cpu=True`` / ``--cpu`` runs the numpy restatements (evaluate.box_match_numpy, the numpy counts, facilities.dbscan_numpy, counts_numpy) and
writes the same bytes.

NOT reproduced (evaluate.py's list applies): get_tp's ``index_key`` row-0 slip (row 0 matches like any other here); under ``--dedup-overlaps`` a
clipped survivor keeps its full box where the reference goes on with the clipped polygon; the centroid chain has the status facilities.py
describes; the land images come from land_images.py's rule (no polygon buffer); ``sort_values('precision').head(1)`` is an unstable sort in
pandas: here a tie goes to the smaller threshold and an empty precision sorts last.
"""
from __future__ import annotations

import argparse
import csv
import json
import os
import sys
import time
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import evaluate, facilities, geocode, kfold
from .tonnage import philox4x32, uniform_from_words

DOMAINS = ("all", "ocean", "ocean + clustered")
CURVES_FILE, STRATA_FILE, JSON_FILE = "performance_curves.csv", "performance_strata.csv", "performance.json"
CURVE_COLUMNS = ("domain", "threshold", "precision", "recall", "n_pred", "n_pred_tp", "n_label", "n_label_tp")
STRATA_COLUMNS = ("bucket", "num_images_bucket", "num_images_sample", "num_detections_bucket", "num_detections_sample", "num_labels_sample",
                  "estimated_num_labels_bucket")
DEFAULT_THRESHOLDS = 100                                    # np.linspace(0, 1, 100), ModelPerformance.py:129
DEFAULT_EPS, DEFAULT_MIN_CAGES = 50.0, 5                    # ModelPerformance.py:94-95
DEFAULT_RATES = tuple(k * 1e-5 for k in range(1, 11))       # the R script's seq(0.00001, 0.0001, 0.00001)
DEFAULT_K, DEFAULT_SEED, DEFAULT_CAGES_PER_IMAGE = 10000, 0, 5.0
MAX_RATES = 16                                              # engine.BERNOULLI_MAX_RATES
SLOT = 16                                                   # the counter's third word: outside tonnage's slots 0 .. 6
MAX_DRAWS = 1 << 32                                         # of one launch
BOUND_STRATUM = kfold.NO_DET_OUT
NEEDS_EVALUATE = ("--performance scores geocoded detections against the human labels: it needs --evaluate TRUTH_GEOJSON and --geocode-bboxes CSV "
                  "(and --save-txt --save-conf)")
SCENES_NEED_IMAGES = ("--performance with --tile-scenes: the tiles cut from the scenes are not listed anywhere after the sweep, so the image list "
                      "needs --evaluate-kfold-images FILE (the tile names, one per line)")


# ---- options ----

def check_options(thresholds, eps, min_cages, rates, K) -> np.ndarray:
    """What the command lines refuse before any work -> the rates as float64 [R].  rates = the option's text (evaluate.parse_grid), a
    sequence, or None (the defaults)."""
    if int(thresholds) < 2:
        raise ValueError(f"--performance-thresholds {thresholds}: at least 2 (np.linspace(0, 1, N))")
    if not float(eps) > 0 or int(min_cages) < 1:
        raise ValueError(f"--performance-eps {eps}, --performance-min-cages {min_cages}: a positive distance and a size of at least 1")
    if int(K) < 2:
        raise ValueError(f"--performance-K {K}: at least 2 simulations")
    r = np.asarray(DEFAULT_RATES if rates is None else evaluate.parse_grid(rates) if isinstance(rates, str) else rates, np.float64).reshape(-1)
    if not 1 <= r.shape[0] <= MAX_RATES or not ((r >= 0) & (r <= 1)).all():
        raise ValueError(f"--performance-rates: 1 to {MAX_RATES} rates in [0, 1], not {r.tolist()}")
    return r


def read_sample(path: str) -> List[str]:
    """The labelled images (the reference's output/cf_images.csv): a CSV with a header line that has a column ``image``, or a plain list with
    one name per line."""
    with open(path, newline="") as f:
        lines = [l for l in f.read().splitlines() if l.strip()]
    if not lines:
        return []
    header = [h.strip() for h in next(csv.reader([lines[0]]))]
    if "image" in header:
        at = header.index("image")
        return [row[at].strip() for row in csv.reader(lines[1:]) if len(row) > at and row[at].strip()]
    return [l.strip() for l in lines]


# ---- 1. the curves ----

def domain_masks(det: Dict[str, np.ndarray], on_land: np.ndarray, eps: float, min_cages: int, cpu: bool = False) -> np.ndarray:
    """bool [n, 3], a column per domain, for the sampled detections `det` (an evaluate.inputs sample): all of them; those whose image is not
    wholly on land (on_land bool [n]); of those the ones DBSCAN(eps, min_cages) per year puts into a cluster."""
    n = det["conf"].shape[0]
    ocean = ~np.asarray(on_land, bool).reshape(-1)
    clustered = np.zeros(n, bool)
    idx = np.nonzero(ocean)[0]
    if idx.shape[0]:
        fn = facilities.dbscan_numpy if cpu else facilities.dbscan_labels
        labels = np.asarray(fn(det["xy"][idx], det["year_id"][idx], float(eps), int(min_cages))[0], np.int64)
        clustered[idx[labels >= 0]] = True
    return np.stack([np.ones(n, bool), ocean, clustered], 1)


def curve_counts(data: Dict[str, dict], masks: np.ndarray, thresholds: np.ndarray, cpu: bool = False, times: Optional[dict] = None) -> Dict[str, np.ndarray]:
    """{"tp": bool [n], "n_pred", "n_pred_tp", "n_label_tp": int64 [3, N]} of the module's docstring for evaluate.inputs() `data` (the sampled
    detections, all labels) and domain_masks() `masks`.  times receives "sort_ms" and "kernel_ms" of the two joins (GPU)."""
    det, lab = data["det"], data["lab"]
    n, L = det["conf"].shape[0], lab["conf"].shape[0]
    G = 2 * max(1, data["years"].shape[0])
    thr = np.ascontiguousarray(thresholds, dtype=np.float64)
    vals = np.where(masks, det["conf"][:, None], -np.inf)
    if cpu or n == 0 or L == 0:
        if n and L:
            tp = evaluate.box_match_numpy(det["box"], det["group"], lab["box"], lab["group"])[0]
            R = evaluate.box_match_numpy(lab["box"], lab["group"], det["box"], det["group"], payload=vals)[1]
        else:
            tp, R = np.zeros(n, bool), np.full((L, len(DOMAINS)), -np.inf)
        a, b, c = (evaluate._counts_numpy(v, thr) for v in (vals, np.where(tp[:, None], vals, -np.inf), R))
    else:
        import torch
        from . import engine
        dev = lambda x: torch.from_numpy(np.ascontiguousarray(x)).cuda()
        dbox, dgroup, lbox, lgroup, vals_d, thr_d = (dev(x) for x in (det["box"], det["group"], lab["box"], lab["group"], vals, thr))
        t = {"sort_ms": 0.0, "kernel_ms": 0.0}
        tm = {} if times is not None else None
        tp_d = engine.box_match(dbox, dgroup, lbox, lgroup, G, times=tm)[0].bool()
        for k in t:
            t[k] += (tm or {}).get(k, 0.0)
        R = engine.box_match(lbox, lgroup, dbox, dgroup, G, payload=vals_d, times=tm)[1]
        for k in t:
            t[k] += (tm or {}).get(k, 0.0)
        neg = torch.tensor(float("-inf"), dtype=torch.float64, device="cuda")
        a, b, c = (evaluate._counts_torch(v, thr_d) for v in (vals_d, torch.where(tp_d.unsqueeze(1), vals_d, neg), R))
        tp = tp_d.cpu().numpy()
        if times is not None:
            times.update(t)
    return {"tp": tp, "n_pred": a, "n_pred_tp": b, "n_label_tp": c}


def curve_table(counts: Dict[str, np.ndarray], thresholds: np.ndarray, n_label: int) -> Dict[str, np.ndarray]:
    """The 3 N rows of performance_curves.csv as columns, in DOMAINS' order."""
    N = thresholds.shape[0]
    out = {"domain": np.asarray([d for d in DOMAINS for _ in range(N)], dtype=object), "threshold": np.tile(np.asarray(thresholds, np.float64), len(DOMAINS))}
    out.update(evaluate.rates(counts["n_pred"].reshape(-1), counts["n_pred_tp"].reshape(-1), np.full(len(DOMAINS) * N, int(n_label), np.int64),
                              counts["n_label_tp"].reshape(-1)))
    return out


def _lowest_precision(table: Dict[str, np.ndarray], domain: str, at_least: float) -> Optional[int]:
    rows = np.nonzero((table["domain"] == domain) & (table["threshold"] >= at_least))[0]
    if rows.shape[0] == 0:
        return None
    p = table["precision"][rows]
    return int(rows[np.lexsort((table["threshold"][rows], np.where(np.isnan(p), np.inf, p)))[0]])      # NaN last, a tie to the smaller threshold


def reported_rows(table: Dict[str, np.ndarray]) -> List[dict]:
    """The rows ModelPerformance.py:157-167 prints: the row of lowest precision of ``all`` at t >= 0, 0.5 and 0.8 and of ``ocean`` and ``ocean +
    clustered`` at t >= 0.8, and the first ``ocean`` row with t >= 0.75."""
    out = []

    def add(rule, domain, at_least, k):
        row = None if k is None else {c: (table[c][k] if c == "domain" else evaluate._json_num(table[c][k])) for c in CURVE_COLUMNS}
        out.append({"rule": rule, "domain": domain, "min_threshold": at_least, "row": row})

    for domain, at_least in (("all", 0.0), ("all", 0.5), ("all", 0.8), ("ocean", 0.8), ("ocean + clustered", 0.8)):
        add("lowest precision", domain, at_least, _lowest_precision(table, domain, at_least))
    first = np.nonzero((table["domain"] == "ocean") & (table["threshold"] >= 0.75))[0]
    add("first row", "ocean", 0.75, int(first[0]) if first.shape[0] else None)
    return out


# ---- 2. the strata table ----

def strata_rows(images: Dict[str, np.ndarray], in_sample: np.ndarray, land: Optional[Dict[str, np.ndarray]] = None) -> List[dict]:
    """One row per stratum in kfold.STRATA's order, then ``land`` (when given: its images all count as sampled), with STRATA_COLUMNS as keys;
    estimated_num_labels_bucket is None where the stratum has no sampled image."""
    def row(name, n_det, n_lab, sampled):
        s_img, s_lab, n_img = int(sampled.sum()), int(n_lab[sampled].sum()), int(sampled.shape[0])
        est = None if s_img == 0 else float(np.float64(s_lab) / np.float64(s_img) * np.float64(n_img))
        return {"bucket": name, "num_images_bucket": n_img, "num_images_sample": s_img, "num_detections_bucket": int(n_det.sum()),
                "num_detections_sample": int(n_det[sampled].sum()), "num_labels_sample": s_lab, "estimated_num_labels_bucket": est}
    in_sample = np.asarray(in_sample, bool).reshape(-1)
    rows = []
    for k, name in enumerate(kfold.STRATA):
        take = images["bucket"] == k
        rows.append(row(name, images["n_detections"][take], images["n_labels"][take], in_sample[take]))
    if land is not None:
        rows.append(row(kfold.LAND, land["n_detections"], land["n_labels"], np.ones(land["image"].shape[0], bool)))
    return rows


# ---- 3. the population bound ----

def counts_numpy(seed: int, k0: int, K: int, S: int, rates, block: int = 1 << 21) -> np.ndarray:
    """int32 [K, R]: engine.bernoulli_counts without a GPU, the same bytes.  count[k][i] = #{j < S : u(k0 + k, j) < rates[i]}; u(k, j) from
    Philox4x32-10 at counter (k, j >> 1, 16, 0) under the seed's two halves: of its four words an even j takes (w1 : w0), an odd j
    (w3 : w2), each through tonnage.uniform_from_words.  `block` Philox calls at a time."""
    rates = np.asarray(rates, np.float64).reshape(-1)
    K, S, k0, seed = int(K), int(S), int(k0), int(seed)
    if not 1 <= rates.shape[0] <= MAX_RATES or not ((rates >= 0) & (rates <= 1)).all():
        raise ValueError(f"population: 1 to {MAX_RATES} rates in [0, 1], not {rates.tolist()}")
    if not 1 <= S < 1 << 31 or K < 0 or k0 < 0 or k0 + K > 1 << 32:
        raise ValueError(f"population: {K} simulations from {k0} of {S} draws (S in 1 .. 2^31 - 1, k0 + K <= 2^32)")
    calls = (S + 1) // 2
    out = np.zeros((K, rates.shape[0]), np.int32)
    rows = max(1, block // calls)
    for r0 in range(0, K, rows):
        k = np.arange(k0 + r0, k0 + min(K, r0 + rows), dtype=np.uint64)
        for c0 in range(0, calls, block):                   # (one pass unless a single simulation has more than `block` calls)
            c = np.arange(c0, min(calls, c0 + block), dtype=np.uint64)
            w0, w1, w2, w3 = philox4x32(k[:, None], c[None, :], SLOT, 0, seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF)
            u_even, u_odd = uniform_from_words(w0, w1), uniform_from_words(w2, w3)
            if S & 1 and c[-1] == calls - 1:
                u_odd[:, -1] = 2.0                          # the draw of j = S does not exist: below no rate
            for i, r in enumerate(rates.tolist()):
                out[r0:r0 + k.shape[0], i] += ((u_even < r).sum(1) + (u_odd < r).sum(1)).astype(np.int32)
    return out


def chunk_sizes(K: int, S: int) -> List[int]:
    """The simulations of each launch: at most MAX_DRAWS draws in one (the reference's 1.05e8 are one launch)."""
    per = max(1, MAX_DRAWS // int(S))
    return [min(per, int(K) - at) for at in range(0, int(K), per)]


def simulate(K: int, S: int, rates, seed: int = 0, cpu: bool = False, times: Optional[dict] = None) -> Dict[str, list]:
    """{"all_zeros_50": the K // 2-th smallest count per rate (R's sort(labels)[as.integer(K / 2)]), "zero_share": the share of the K samples
    without a positive, "zeros": their number}.  GPU: the draws, the sort and the select on the device; HIP events into times
    ("kernel_ms", "select_ms")."""
    K, S = int(K), int(S)
    if K < 2:
        raise ValueError(f"population: {K} simulations (at least 2)")
    rates = np.asarray(rates, np.float64).reshape(-1)
    if cpu:
        counts = np.concatenate([counts_numpy(seed, at, n, S, rates) for at, n in _chunks(K, S)], 0)
        kth = np.sort(counts, 0)[K // 2 - 1]
        zeros = (counts == 0).sum(0)
    else:
        import torch
        from . import engine
        counts = torch.empty((K, rates.shape[0]), dtype=torch.int32, device="cuda")
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(3)]
        ev[0].record()
        for at, n in _chunks(K, S):
            engine.bernoulli_counts(seed, at, n, S, rates, out=counts[at:at + n])
        ev[1].record()
        kth = torch.sort(counts, 0).values[K // 2 - 1].cpu().numpy()
        zeros = (counts == 0).sum(0).cpu().numpy()
        ev[2].record()
        if times is not None:
            torch.cuda.synchronize()
            times.update(kernel_ms=ev[0].elapsed_time(ev[1]), select_ms=ev[1].elapsed_time(ev[2]))
    return {"all_zeros_50": [int(v) for v in kth], "zero_share": [int(z) / K for z in zeros], "zeros": [int(z) for z in zeros]}


def _chunks(K: int, S: int):
    at = 0
    for n in chunk_sizes(K, S):
        yield at, n
        at += n


def population_bound(rates, all_zeros_50, zero_share, images_stratum: int, sample_stratum: int, labels_other_strata: int,
                     cages_per_image: float = DEFAULT_CAGES_PER_IMAGE, K: int = DEFAULT_K, seed: int = DEFAULT_SEED) -> dict:
    """The ``population_bound`` block of performance.json from the simulation's two curves: final_rate = the smallest rate whose order
    statistic is not zero (None without one: then no bound), images_with_cages = round(final_rate I) (Python's round: half to even, as R's),
    stratum_estimate = images_with_cages cages_per_image, upper_bound = stratum_estimate + labels_other_strata."""
    rates = [float(r) for r in np.asarray(rates, np.float64).reshape(-1)]
    hit = [r for r, z in zip(rates, all_zeros_50) if int(z) != 0]
    final = min(hit) if hit else None
    with_cages = None if final is None else int(round(final * int(images_stratum)))
    estimate = None if final is None else with_cages * float(cages_per_image)
    return {"rates": rates, "all_zeros_50": [int(z) for z in all_zeros_50], "zero_share": [float(z) for z in zero_share], "final_rate": final,
            "images_stratum": int(images_stratum), "sample_stratum": int(sample_stratum), "images_with_cages": with_cages,
            "cages_per_image": float(cages_per_image), "stratum_estimate": estimate, "labels_other_strata": int(labels_other_strata),
            "upper_bound": None if final is None else estimate + int(labels_other_strata), "K": int(K), "seed": int(seed)}


def bound_from_strata(rows: Sequence[dict], rates, K: int = DEFAULT_K, seed: int = DEFAULT_SEED, cages_per_image: float = DEFAULT_CAGES_PER_IMAGE,
                      cpu: bool = False, times: Optional[dict] = None) -> dict:
    """simulate() and population_bound() with I, S and the other strata's labels taken from strata_rows(); {"skipped": reason} when the
    stratum has no sampled image (there is no sample to be all zeros)."""
    mine = next(r for r in rows if r["bucket"] == BOUND_STRATUM)
    if mine["num_images_sample"] == 0:
        return {"skipped": f"no sampled image in the stratum '{BOUND_STRATUM}'"}
    other = sum(r["num_labels_sample"] for r in rows if r["bucket"] not in (BOUND_STRATUM, kfold.LAND))
    sim = simulate(K, mine["num_images_sample"], rates, seed, cpu=cpu, times=times)
    return population_bound(rates, sim["all_zeros_50"], sim["zero_share"], mine["num_images_bucket"], mine["num_images_sample"], other, cages_per_image, K, seed)


# ---- files ----

def write_curves_csv(path: str, table: Dict[str, np.ndarray]) -> int:
    """performance_curves.csv: whole-number columns as integers, the others as ``repr`` of the double, NaN empty."""
    n = table["n_pred"].shape[0]
    cols = [table[c].tolist() for c in CURVE_COLUMNS]
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(CURVE_COLUMNS)
        for k in range(n):
            w.writerow([kfold._cell(c[k]) for c in cols])
    return n


def read_curves_csv(path: str) -> Dict[str, np.ndarray]:
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {"domain": np.asarray([r["domain"] for r in rows], dtype=object)}
    for c in CURVE_COLUMNS[1:]:
        out[c] = (np.asarray([float(r[c]) if r[c] else np.nan for r in rows], np.float64) if c in ("threshold", "precision", "recall")
                  else np.asarray([int(r[c]) for r in rows], np.int64))
    return out


def write_strata_csv(path: str, rows: Sequence[dict]) -> int:
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(STRATA_COLUMNS)
        for r in rows:
            w.writerow([kfold._cell(r[c]) for c in STRATA_COLUMNS])
    return len(rows)


def read_strata_csv(path: str) -> List[dict]:
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    return [{c: r[c] if c == "bucket" else (None if r[c] == "" else float(r[c])) if c == "estimated_num_labels_bucket" else int(r[c])
             for c in STRATA_COLUMNS} for r in rows]


# ---- the whole step ----

def performance(table: Dict[str, np.ndarray], truth: Dict[str, np.ndarray], out_dir: str, names: Optional[Sequence[str]] = None,
                sample: Optional[Sequence[str]] = None, land: Optional[Sequence[str]] = None, keep=None, rects=None, sites=None,
                thresholds: int = DEFAULT_THRESHOLDS, eps: float = DEFAULT_EPS, min_cages: int = DEFAULT_MIN_CAGES, rates=None, K: int = DEFAULT_K,
                seed: int = DEFAULT_SEED, cages_per_image: float = DEFAULT_CAGES_PER_IMAGE, cpu: bool = False, device: Optional[str] = None,
                times: Optional[dict] = None) -> dict:
    """The three results for geocode's detection table and evaluate.load_truth_geojson's labels, and the three files in out_dir -> what
    performance.json holds.  names = the image list (default: the images of the table and of the truth, sorted by stem); sample = the labelled
    images (default: every image of the list); land = the images wholly on land (land_images.py), None without ``--land-images``: they count
    as sampled, leave the ``ocean`` domain and form the strata table's row ``land``; keep = bool per detection (--dedup-overlaps' survivors;
    NOT the land filter's rows); rects (an array per name, or a function of the stem) and sites as kfold.kfold takes them.  device = what the
    JSON records (default "cpu" with cpu, the GPU's name otherwise)."""
    rates = check_options(thresholds, eps, min_cages, rates, K)
    thr = np.linspace(0, 1, int(thresholds))
    every = evaluate.inputs(table, truth, keep)
    det_image = [evaluate._stem(table["stems"][i]) for i in np.asarray(table["image"], np.int64)[every["det"]["rows"]]]
    lab_image = [evaluate._stem(s) for s in np.asarray(truth["image"], dtype=object)[every["lab"]["rows"]]]
    if names is None:
        names = sorted({evaluate._stem(s) for s in table["stems"]} | {evaluate._stem(s) for s in truth["image"]})
    names = [evaluate._stem(s) for s in names]
    on = set() if land is None else {evaluate._stem(s) for s in land} & set(names)
    sampled = (set(names) if sample is None else {evaluate._stem(s) for s in sample} & set(names)) | on

    # 1. the curves: the sampled images' detections, every label
    det_sampled = np.asarray([s in sampled for s in det_image], bool).reshape(-1)
    data = kfold._subset(every, det_sampled, np.ones(len(lab_image), bool))
    det_on_land = np.asarray([s in on for s, t in zip(det_image, det_sampled) if t], bool).reshape(-1)
    masks = domain_masks(data["det"], det_on_land, eps, min_cages, cpu=cpu)
    counts = curve_counts(data, masks, thr, cpu=cpu, times=times)
    curves = curve_table(counts, thr, data["lab"]["conf"].shape[0])
    n, tp = int(masks.shape[0]), counts["tp"]
    fp_all, fp_ocean = int((~tp).sum()), int((~tp & masks[:, 1]).sum())

    # 2. the strata table: every image of the list, all cage detections
    is_land = np.asarray([s in on for s in names], bool).reshape(-1)
    rect_of = rects if callable(rects) else None
    if rect_of is not None:
        rects = np.asarray([rect_of(s) for s in names], np.float64).reshape(-1, 4)
    elif rects is not None:
        rects = np.asarray(rects, np.float64).reshape(-1, 4)
        if rects.shape[0] != len(names):
            raise ValueError(f"performance: {rects.shape[0]} rectangles for {len(names)} images")
    ocean_names = [s for s, l in zip(names, is_land) if not l]
    imgs = kfold.image_table(ocean_names, det_image, every["det"]["conf"], lab_image, None if rects is None else rects[~is_land], sites)
    land_imgs = None
    if land is not None:
        land_imgs = kfold.image_table([s for s, l in zip(names, is_land) if l], det_image, every["det"]["conf"], lab_image,
                                      None if rects is None else rects[is_land], sites)
    strata = strata_rows(imgs, np.asarray([s in sampled for s in ocean_names], bool), land_imgs)

    # 3. the population bound
    tb = {} if times is not None else None
    bound = bound_from_strata(strata, rates, K, seed, cages_per_image, cpu=cpu, times=tb)
    if times is not None:
        times.update({"population_" + k: v for k, v in tb.items()})

    if device is None:
        if cpu:
            device = "cpu"
        else:
            import torch
            device = torch.cuda.get_device_name()
    s = {"parameters": {"thresholds": int(thresholds), "eps": float(eps), "min_cages": int(min_cages), "rates": [float(r) for r in rates], "K": int(K),
                        "seed": int(seed), "cages_per_image": float(cages_per_image), "known_sites": 0 if sites is None else int(np.asarray(sites).shape[0])},
         "device": device, "land_images": land is not None, "n_images": len(names), "n_sampled_images": len(sampled), "n_land_images": len(on),
         "n_detections": n, "n_labels": int(data["lab"]["conf"].shape[0]),
         "fp_share_raw": None if n == 0 else 100 - 100 * int(tp.sum()) / n,
         "land_fp_dropped": None if fp_all == 0 else 100 - 100 * fp_ocean / fp_all,
         "reported_rows": reported_rows(curves), "strata": strata, "population_bound": bound}
    t0 = time.perf_counter()
    os.makedirs(out_dir, exist_ok=True)
    write_curves_csv(os.path.join(out_dir, CURVES_FILE), curves)
    write_strata_csv(os.path.join(out_dir, STRATA_FILE), strata)
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump(s, f, indent=1)
    if times is not None:
        times["files_ms"] = (time.perf_counter() - t0) * 1e3
    return s


def performance_from_options(table, truth_path: str, out_dir: str, wanted_bboxes_csv: str, names: Optional[Sequence[str]] = None,
                             kfold_images: Optional[str] = None, sample_file: Optional[str] = None, known_sites: Optional[str] = None,
                             land: Optional[Sequence[str]] = None, keep=None, dedup_overlaps: Optional[str] = None, cpu: bool = False,
                             device: Optional[str] = None, **settings) -> dict:
    """The step as both command lines run it: the image list of --land-images and --evaluate-kfold (evaluate.land_image_names), the labels
    through overlaps.filter_truth under --dedup-overlaps (dedup_overlaps = the download-box file), the rectangles from the --geocode-bboxes
    file when there are known sites."""
    from . import overlaps
    truth = overlaps.filter_truth(evaluate.load_truth_geojson(truth_path), dedup_overlaps, cpu=cpu)
    sites = kfold.load_known_sites(known_sites) if known_sites else None
    return performance(table, truth, out_dir, names=evaluate.land_image_names(table, truth_path, kfold_images, names),
                       sample=read_sample(sample_file) if sample_file else None, land=land, keep=keep,
                       rects=kfold.tile_rects(wanted_bboxes_csv) if sites is not None else None, sites=sites, cpu=cpu, device=device, **settings)


def describe(s: dict) -> str:
    b = s["population_bound"]
    bound = (b["skipped"] if "skipped" in b else "no rate with a non-zero median" if b["final_rate"] is None
             else f"rate {b['final_rate']:g}, upper bound {b['upper_bound']:g} cages")
    num = lambda v: "nan" if v is None else f"{v:.2f}"
    return (f"performance of {s['n_detections']} detections of {s['n_sampled_images']} sampled images against {s['n_labels']} labels: "
            f"{num(s['fp_share_raw'])} % false positives, {num(s['land_fp_dropped'])} % of them in images on land; population bound: {bound}")


def add_options(p: argparse.ArgumentParser) -> None:
    """The options detect.py and this module's command line share."""
    p.add_argument("--performance-sample", default=None, metavar="FILE",
                   help="the images that were labelled (the reference's output/cf_images.csv): a CSV with a column `image`, or one name per line "
                        "(default: every image of the list)")
    p.add_argument("--performance-thresholds", type=int, default=DEFAULT_THRESHOLDS, metavar="N", help="np.linspace(0, 1, N) (default 100; at least 2)")
    p.add_argument("--performance-eps", type=float, default=DEFAULT_EPS, metavar="METRES", help="DBSCAN distance of the third curve (default 50)")
    p.add_argument("--performance-min-cages", type=int, default=DEFAULT_MIN_CAGES, metavar="N", help="minimum cluster size of the third curve (default 5)")
    p.add_argument("--performance-rates", default=None, metavar="LIST",
                   help=f"up to {MAX_RATES} rates in [0, 1] for the population bound: start:stop:step or a comma list (default 1e-5 .. 1e-4 in steps of 1e-5)")
    p.add_argument("--performance-K", type=int, default=DEFAULT_K, metavar="K", help="simulations per rate (default 10000; at least 2)")
    p.add_argument("--performance-seed", type=int, default=DEFAULT_SEED, metavar="SEED", help="key of the generator (default 0)")
    p.add_argument("--performance-cages-per-image", type=float, default=DEFAULT_CAGES_PER_IMAGE, metavar="CAGES",
                   help="cages in an image that holds any, for the bound (default 5, the reference's)")


def settings_from_options(thresholds, eps, min_cages, rates, K, seed, cages_per_image) -> dict:
    """performance()'s keyword settings from the options' values, checked."""
    return {"thresholds": int(thresholds), "eps": float(eps), "min_cages": int(min_cages), "rates": check_options(thresholds, eps, min_cages, rates, K),
            "K": int(K), "seed": int(seed), "cages_per_image": float(cages_per_image)}


def main(argv: Optional[List[str]] = None) -> int:
    p = argparse.ArgumentParser(prog="python -m aquaculture_amd.performance",
                                description="Stage curves, strata table and population bound for the detections of an existing label directory, without "
                                            "running inference again.")
    p.add_argument("--labels", required=True, metavar="DIR", help="label files written by detect.py --save-txt --save-conf")
    p.add_argument("--geocode-bboxes", required=True, metavar="CSV", help="reference data/wanted_bboxes.csv")
    p.add_argument("--truth", required=True, metavar="GEOJSON", help="the human labels (reference output/humanlabels.geojson)")
    p.add_argument("--land", default=None, metavar="GEOJSON", help="land polygons: the images wholly on land are marked (land_images.py) and leave the ocean domain")
    p.add_argument("--land-images-indent", type=float, default=5.0, metavar="METRES", help="how far inside the land such an image lies (default 5)")
    p.add_argument("--out", default=None, metavar="DIR", help="where the three files go (default: beside the label directory)")
    p.add_argument("--evaluate-kfold-images", default=None, metavar="FILE", help="the image list, one name per line (default: the images of the labels and the truth)")
    p.add_argument("--evaluate-known-sites", default=None, metavar="CSV", help="known sites (columns lat, lon) for the two strata without a detection")
    p.add_argument("--dedup-overlaps", action="store_true", help="count each cage once where the download boxes overlap (overlaps.py), detections and labels")
    p.add_argument("--cpu", action="store_true", help="the numpy / scipy restatement instead of the GPU")
    add_options(p)
    opt = p.parse_args(argv)
    try:
        settings = settings_from_options(opt.performance_thresholds, opt.performance_eps, opt.performance_min_cages, opt.performance_rates,
                                         opt.performance_K, opt.performance_seed, opt.performance_cages_per_image)
    except ValueError as e:
        p.error(str(e))
    out_dir = opt.out or os.path.dirname(os.path.abspath(opt.labels.rstrip("/")))
    table = geocode.geocode_label_dir(opt.labels, opt.geocode_bboxes)
    keep = None
    if opt.dedup_overlaps:
        from . import overlaps
        keep = overlaps.survivors(overlaps.clip_table(table, opt.geocode_bboxes, cpu=opt.cpu)["state"])
    on_land = None
    if opt.land is not None:
        from . import land, land_images
        stems = [evaluate._stem(s) for s in evaluate.land_image_names(table, opt.truth, opt.evaluate_kfold_images)]
        rect_of = kfold.tile_rects(opt.geocode_bboxes)
        flags = land_images.on_land(np.asarray([rect_of(s) for s in stems], np.float64).reshape(-1, 4), land.load_land_geojson(opt.land),
                                    opt.land_images_indent, cpu=opt.cpu)[0]
        on_land = [s for s, l in zip(stems, flags) if l]
    s = performance_from_options(table, opt.truth, out_dir, opt.geocode_bboxes, kfold_images=opt.evaluate_kfold_images, sample_file=opt.performance_sample,
                                 known_sites=opt.evaluate_known_sites, land=on_land, keep=keep,
                                 dedup_overlaps=opt.geocode_bboxes if opt.dedup_overlaps else None, cpu=opt.cpu, **settings)
    print(describe(s) + f" in {out_dir}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
