"""Cross-validated tuning of the three facility numbers (``detect.py --evaluate ... --evaluate-kfold [N]``, ``python -m aquaculture_amd.evaluate
--evaluate-kfold [N]``): the rest of the reference's src/get_kfold_cluster_performance.py around the grid of evaluate.py.

The reference builds a table of images with strata (set_image_stats, set_buckets), sets a tenth of the images aside (train_test_split), runs
StratifiedKFold(5, shuffle=True, random_state=1) over the others, searches the 82 x 8 x 10 grid on every fold's train images, scores the
winner by ``product`` and the winner by ``f_score`` on the fold's test images (get_fold_performance), and reports one combination on the
images set aside (test_set_performance).  Here:

  image table   one row per image (image_table): n_detections and det_conf (the maximum) from the detections the grid uses, n_labels from the
                truth, in_known_area = the image's EPSG:3857 rectangle meets (touching counts) the +-1000 m box around a known site
                (load_known_sites: columns ``lat``, ``lon`` of a CSV, through geocode.lonlat_to_mercator); strata as set_buckets forms them
                (buckets: pandas.cut(det_conf, [0, 0.3, 0.5, 0.8, 1]) restated with one searchsorted, and the two "No detection" strata)
  splits        holdout_split and stratified_folds restate scikit-learn's train_test_split and StratifiedKFold(shuffle=True) on
                numpy.random.RandomState(seed): the same index arrays.  The reference hands the stratum codes to train_test_split as a second
                array to split, not as ``stratify=``, so its hold-out is a plain shuffle; that is kept.  (n_train is n - n_test, which is
                what scikit-learn computes when only test_size is given.)
  subsets       every detection and label carries one uint32 word (subset_words): bit f = in the train images of fold f, bit N + f = in its
                test images, bit 2 N = set aside, bit 2 N + 1 = any train image; 2 N + 2 <= 32
  grid phase    per distance ONE call for all folds: M [N][n][K] over the train bits (engine.eval_member_conf_subsets), R [N][L][K] from the
                join with M as payload (engine.box_match_subsets), the true-positive words from one join without payload (once, it does not
                depend on the distance); the counts by the batched sort / searchsorted of evaluate.py.  A join respects the subsets: a
                detection of a train image that meets only a label of a test image is no true positive, as in the reference, which filters
                detections and labels by image before it joins them
  winners       per fold the first maximum of ``product`` and of ``f_score`` (evaluate.idxmax: pandas' idxmax, NaN skipped)
  test phase    per distinct winning distance one more pair of calls over the test bits; the four counts at the winning (c, m): member iff M >= c
  hold-out      evaluate.operating_point on the detections and labels of the images set aside, at --facilities-conf / -eps / -min-cages

``cpu=True`` / ``--cpu`` runs the numpy restatements (member_conf_subsets_numpy, box_match_subsets_numpy), with the same bytes and counts.

Pinned against scikit-learn's splitters (index for index), pandas.cut, and the reference's procedure done literally per fold (scikit-learn's
DBSCAN per combination and year, brute-force joins restricted to the fold).  NOT pinned, and what differs (see also evaluate.py's list):
  * the land stratum is formed only with ``--land-images`` (land_images.py: the images whose rectangles lie within the land shrunk by 5 m,
    by rectangle-to-edge distances, no polygon buffer): kfold(land=...) takes those images out of the image table before the splits are drawn,
    in the order of the rest, as the reference does, and lists them with bucket and split ``land``; without the flag no image is taken out
    and ``--evaluate-kfold-images`` (a list without them) is how such images are left out.  What that rule does not pin is in land_images.py;
  * the reference filters the f_score winner's test members by the PRODUCT winner's confidence (get_fold_performance, last get_stats_total
    call); here each metric uses its own threshold;
  * the ``index_key`` row-0 slip of get_tp stays unreproduced and the overlap de-duplication unapplied, as in evaluate.py;
  * the standard deviations in kfold.json are pandas' default (ddof = 1) over the folds that have a value; the reference reports none.
"""
from __future__ import annotations

import csv
import json
import math
import os
import time
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import geocode

CONF_BINS = np.array([0.0, 0.3, 0.5, 0.8, 1.0])
INTERVALS = tuple(f"({a}, {b}]" for a, b in zip(CONF_BINS[:-1].tolist(), CONF_BINS[1:].tolist()))     # as pandas prints them: "(0.0, 0.3]"
NO_DET_IN, NO_DET_OUT = "No detection, in known area", "No detection, outside known area"
STRATA = INTERVALS + (NO_DET_IN, NO_DET_OUT)
LAND = "land"                                               # bucket and split of an image wholly on land (kfold(land=...)): in no split
SITE_HALF_SIDE = 1000.0                                     # metres in EPSG:3857, as the reference's '1km_box'
MAX_SUBSETS = 32
RESULTS_FILE, IMAGES_FILE, JSON_FILE = "kfold_results.csv", "kfold_images.csv", "kfold.json"
RESULT_COLUMNS = ("test_precision", "test_recall", "train_best_conf_thresh", "train_best_distance_threshold", "train_best_min_cluster_size", "metric",
                  "fold_id", "test_n_pred", "test_n_pred_tp", "test_n_label", "test_n_label_tp", "train_score")
IMAGE_COLUMNS = ("image", "year", "n_detections", "det_conf", "n_labels", "in_known_area", "bucket", "split")
METRICS = ("product", "f_score")


def _ev():
    from . import evaluate                                  # (evaluate.py imports this module's names at its end)
    return evaluate


# ---- the image table and its strata ----

def load_known_sites(path: str) -> np.ndarray:
    """The known sites (reference data/aquaculture_med_dedupe.csv): columns ``lat`` and ``lon`` in degrees, any others ignored -> float64 [n, 2]
    (x, y) in EPSG:3857."""
    with open(path, newline="") as f:
        r = csv.reader(f)
        header = [h.strip() for h in next(r)]
        if "lat" not in header or "lon" not in header:
            raise ValueError(f"{path}: the known sites need columns lat and lon")
        a, o = header.index("lat"), header.index("lon")
        rows = [(float(row[o]), float(row[a])) for row in r if len(row) > max(a, o) and row[a].strip() and row[o].strip()]
    ll = np.asarray(rows, np.float64).reshape(-1, 2)
    x, y = geocode.lonlat_to_mercator(ll[:, 0], ll[:, 1])
    return np.ascontiguousarray(np.stack([np.asarray(x, np.float64), np.asarray(y, np.float64)], 1))


def in_known_area(rects: np.ndarray, sites: Optional[np.ndarray], chunk: int = 4096) -> np.ndarray:
    """bool per image rectangle (west, south, east, north): it meets, touching included, the closed box [x - 1000, x + 1000] x [y - 1000, y + 1000]
    of a site (the box's corners are those four sums in fp64, as shapely.geometry.box holds them)."""
    rects = np.asarray(rects, np.float64).reshape(-1, 4)
    out = np.zeros(rects.shape[0], bool)
    if sites is None or np.asarray(sites).shape[0] == 0:
        return out
    s = np.asarray(sites, np.float64).reshape(-1, 2)
    x0, x1, y0, y1 = s[:, 0] - SITE_HALF_SIDE, s[:, 0] + SITE_HALF_SIDE, s[:, 1] - SITE_HALF_SIDE, s[:, 1] + SITE_HALF_SIDE
    for at in range(0, rects.shape[0], chunk):
        r = rects[at:at + chunk, None, :]
        out[at:at + chunk] = ((r[:, :, 0] <= x1) & (x0 <= r[:, :, 2]) & (r[:, :, 1] <= y1) & (y0 <= r[:, :, 3])).any(1)
    return out


def buckets(det_conf, known) -> np.ndarray:
    """The stratum of every image as an index into STRATA: pandas.cut(det_conf, [0, 0.3, 0.5, 0.8, 1]) (right-closed; 0, a value above 1 and NaN
    fall into no interval, which the reference then calls "No detection"), and for those the known-area flag."""
    c = np.asarray(det_conf, np.float64)
    k = np.searchsorted(CONF_BINS, c, side="left")          # pandas' own step: bins.searchsorted(x, side="left"), 0 and len(bins) are NaN
    none = (k == 0) | (k == CONF_BINS.shape[0]) | np.isnan(c)
    return np.where(none, np.where(np.asarray(known, bool), len(INTERVALS), len(INTERVALS) + 1), k - 1).astype(np.int64)


def _year_of(stem: str) -> Optional[int]:
    head = stem.split("_")[0][-4:]
    return int(head) if head.isdigit() else None


def image_table(names: Sequence[str], det_image: Sequence[str], det_conf, lab_image: Sequence[str], rects=None, sites=None) -> Dict[str, np.ndarray]:
    """One row per name of `names` (compared without directory and extension; the order is kept): image (the stem), year (from the name, -1
    without one), n_detections, det_conf (the maximum, NaN without a detection), n_labels, in_known_area, bucket (index into STRATA); and
    det_row / lab_row: the table row of every detection and label, -1 for an image that is not in the table.  rects = float64 [len(names), 4]
    (west, south, east, north in EPSG:3857), needed with sites."""
    ev = _ev()
    stems = [ev._stem(s) for s in names]
    row = {}
    for k, s in enumerate(stems):
        if s in row:
            raise ValueError(f"kfold: image {s} is listed twice")
        row[s] = k
    n = len(stems)
    det_row = np.asarray([row.get(ev._stem(s), -1) for s in det_image], np.int64).reshape(-1)
    lab_row = np.asarray([row.get(ev._stem(s), -1) for s in lab_image], np.int64).reshape(-1)
    conf = np.asarray(det_conf, np.float64).reshape(-1)
    top = np.full(n, -np.inf)
    np.maximum.at(top, det_row[det_row >= 0], conf[det_row >= 0])
    n_det = np.bincount(det_row[det_row >= 0], minlength=n).astype(np.int64)
    top = np.where(n_det > 0, top, np.nan)
    if sites is not None and rects is None:
        raise ValueError("kfold: the known sites need the images' rectangles")
    known = in_known_area(rects, sites) if rects is not None else np.zeros(n, bool)
    if known.shape[0] != n:
        raise ValueError(f"kfold: {known.shape[0]} rectangles for {n} images")
    years = [_year_of(s) for s in stems]
    return {"image": np.asarray(stems, dtype=object), "year": np.asarray([-1 if y is None else y for y in years], np.int64), "n_detections": n_det,
            "det_conf": top, "n_labels": np.bincount(lab_row[lab_row >= 0], minlength=n).astype(np.int64), "in_known_area": known,
            "bucket": buckets(top, known), "det_row": det_row, "lab_row": lab_row}


def strata_table(images: Dict[str, np.ndarray], land: Optional[Dict[str, np.ndarray]] = None) -> List[dict]:
    """Per stratum, in STRATA's order: images, detections, labels (the reference's get_bucket_info_table, whose sample is every image here).
    land = the image table of the images wholly on land: one more row, ``land``."""
    b = images["bucket"]
    rows = [{"bucket": name, "images": int((b == k).sum()), "detections": int(images["n_detections"][b == k].sum()),
             "labels": int(images["n_labels"][b == k].sum())} for k, name in enumerate(STRATA)]
    if land is not None:
        rows.append({"bucket": LAND, "images": int(land["image"].shape[0]), "detections": int(land["n_detections"].sum()), "labels": int(land["n_labels"].sum())})
    return rows


# ---- scikit-learn's two splitters ----

def holdout_split(n: int, frac: float, seed: int) -> Tuple[np.ndarray, np.ndarray]:
    """(train, test) index arrays of sklearn.model_selection.train_test_split(test_size=frac, random_state=seed) on n rows (no ``stratify``):
    n_test = ceil(frac n), n_train = n - n_test, one permutation of RandomState(seed), its first n_test entries the test rows.  frac = 0: no
    hold-out (every row trains, in order)."""
    if frac == 0:
        return np.arange(n), np.zeros(0, np.int64)
    if not 0 < frac < 1:
        raise ValueError(f"kfold: the hold-out fraction {frac} has to lie in [0, 1)")
    n_test = int(math.ceil(frac * n))
    n_train = n - n_test
    if n_train <= 0 or n_test <= 0:
        raise ValueError(f"kfold: a hold-out of {frac} leaves {max(n_train, 0)} of {n} images to train on")
    perm = np.random.RandomState(seed).permutation(n)
    return perm[n_test:n_test + n_train], perm[:n_test]


def stratified_folds(y, n_splits: int, seed: int) -> np.ndarray:
    """test_fold int64 [len(y)]: the fold whose test set holds each row, as StratifiedKFold(n_splits, shuffle=True, random_state=seed) assigns
    it (its split() yields, for k = 0 .. n_splits - 1, the rows with test_fold != k and those with test_fold == k, both ascending).  Refused:
    fewer than 2 folds, and more folds than the largest class has members (scikit-learn raises there too; a smaller class only makes it warn)."""
    y = np.asarray(y).reshape(-1)
    n_splits = int(n_splits)
    if n_splits < 2:
        raise ValueError(f"kfold: {n_splits} folds (at least 2)")
    _, first, inv = np.unique(y, return_index=True, return_inverse=True)
    enc = np.unique(first, return_inverse=True)[1][inv.reshape(-1)]         # classes numbered by first appearance
    counts = np.bincount(enc)
    if counts.shape[0] == 0 or n_splits > counts.max():
        raise ValueError(f"kfold: {n_splits} folds cannot be more than the {int(counts.max()) if counts.shape[0] else 0} images of the largest stratum")
    order = np.sort(enc)
    alloc = np.asarray([np.bincount(order[i::n_splits], minlength=counts.shape[0]) for i in range(n_splits)])
    rng = np.random.RandomState(seed)
    test_fold = np.empty(y.shape[0], np.int64)
    for c in range(counts.shape[0]):
        f = np.arange(n_splits).repeat(alloc[:, c])
        rng.shuffle(f)
        test_fold[enc == c] = f
    return test_fold


def split_images(bucket, n_splits: int, seed: int = 1, test_frac: float = 0.1) -> np.ndarray:
    """int64 per image: -1 = set aside (the hold-out), k = in the test set of fold k.  The hold-out first, then the folds over the train images
    in their (shuffled) order, stratified by `bucket`, both on a fresh RandomState(seed), as the reference does with one random_state."""
    n_splits = int(n_splits)
    if n_splits < 2:
        raise ValueError(f"kfold: {n_splits} folds (at least 2)")
    if 2 * n_splits + 2 > MAX_SUBSETS:
        raise ValueError(f"kfold: {n_splits} folds need {2 * n_splits + 2} subsets, more than the {MAX_SUBSETS} bits of a mask word (at most {(MAX_SUBSETS - 2) // 2} folds)")
    bucket = np.asarray(bucket).reshape(-1)
    train, _ = holdout_split(bucket.shape[0], float(test_frac), seed)
    split = np.full(bucket.shape[0], -1, np.int64)
    split[train] = stratified_folds(bucket[train], n_splits, seed)
    return split


def subset_words(split, n_splits: int) -> np.ndarray:
    """The uint32 word of every image: bit f (f < N) = trains in fold f, bit N + f = tested in fold f, bit 2 N = set aside, bit 2 N + 1 = any
    train image."""
    split, N = np.asarray(split, np.int64), int(n_splits)
    low = np.uint32((1 << N) - 1)
    held = split < 0
    fold = np.where(held, 0, split).astype(np.uint32)
    one = np.uint32(1)
    w = (low & ~(one << fold)) | (one << (fold + np.uint32(N))) | (one << np.uint32(2 * N + 1))
    return np.where(held, one << np.uint32(2 * N), w).astype(np.uint32)


# ---- the numpy restatement of the two kernels ----

def _neighbour_pairs(xy, group, eps):
    """(row, col) of every ordered pair within eps inside a group, the point itself included: evaluate.member_conf_numpy's pairs."""
    from scipy.spatial import cKDTree
    n = xy.shape[0]
    pairs = [np.zeros((0, 2), np.int64)]
    for g in np.unique(group):
        idx = np.nonzero(group == g)[0]
        pairs.append(idx[cKDTree(xy[idx]).query_pairs(eps * (1 + 1e-9), output_type="ndarray")].reshape(-1, 2))
    pr = np.concatenate(pairs, 0)
    d = xy[pr[:, 0]] - xy[pr[:, 1]]
    pr = pr[d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1] <= eps * eps]
    me = np.arange(n)
    return np.concatenate([pr[:, 0], pr[:, 1], me]), np.concatenate([pr[:, 1], pr[:, 0], me])


def member_conf_subsets_numpy(xy, group, conf, mask, eps: float, K: int, S: int) -> np.ndarray:
    """M float64 [S, n, K] without a GPU (engine.eval_member_conf_subsets gives the same bytes): per subset s (bit s of mask) the
    evaluate.member_conf_numpy of its points alone, -inf in the rows of the others.  The pairs within eps are found once; every subset keeps
    those whose two ends it holds."""
    ev = _ev()
    xy = np.asarray(xy, np.float64).reshape(-1, 2)
    n = xy.shape[0]
    group, conf, mask = np.asarray(group, np.int64), np.asarray(conf, np.float64), np.asarray(mask).astype(np.uint32)
    if not eps > 0 or not 1 <= int(K) <= ev.MAX_K or not 1 <= int(S) <= MAX_SUBSETS:
        raise ValueError(f"evaluate subsets: eps = {eps}, K = {K}, S = {S} (eps > 0, 1 <= K <= {ev.MAX_K} and 1 <= S <= {MAX_SUBSETS})")
    M = np.full((S, n, K), -np.inf)
    if n == 0:
        return M
    row_all, col_all = _neighbour_pairs(xy, group, float(eps))
    for s in range(S):
        bit = ((mask >> np.uint32(s)) & np.uint32(1)).astype(bool)
        keep = bit[row_all] & bit[col_all]
        row, col = row_all[keep], col_all[keep]
        if row.shape[0] == 0:
            continue
        order = np.lexsort((-conf[col], row))               # by row, confidences descending
        row, col = row[order], col[order]
        pts = np.nonzero(bit)[0]                            # every one of them has at least the pair with itself
        start = np.searchsorted(row, pts)
        count = np.bincount(row, minlength=n)[pts]
        for m in range(K):
            kth = np.where(count > m, conf[col[np.minimum(start + m, row.shape[0] - 1)]], -np.inf)
            T = np.full(n, -np.inf)
            T[pts] = np.minimum(conf[pts], kth)
            M[s, pts, m] = np.minimum(conf[pts], np.maximum.reduceat(T[col], start))
    return M


def _matching_pairs(qbox, qgroup, kbox, kgroup, chunk: int = 256):
    """(q, k) of every pair of a query and a key of its group whose closed boxes meet: evaluate.box_match_numpy's blocks, the pairs kept."""
    q_ok, k_ok = ~np.isnan(qbox).any(1), ~np.isnan(kbox).any(1)
    qs, ks = [np.zeros(0, np.int64)], [np.zeros(0, np.int64)]
    for g in np.unique(qgroup[q_ok]):
        qi, ki = np.nonzero((qgroup == g) & q_ok)[0], np.nonzero((kgroup == g) & k_ok)[0]
        if ki.shape[0] == 0:
            continue
        qi, ki = qi[np.argsort(qbox[qi, 0], kind="stable")], ki[np.argsort(kbox[ki, 0], kind="stable")]
        kx0 = kbox[ki, 0]
        widest = float((kbox[ki, 2] - kx0).max())
        for at in range(0, qi.shape[0], chunk):
            q = qi[at:at + chunk]
            lo = np.searchsorted(kx0, qbox[q, 0].min() - widest, side="left")
            hi = np.searchsorted(kx0, qbox[q, 2].max(), side="right")
            kk = ki[lo:hi]
            if kk.shape[0] == 0:
                continue
            kb, qb = kbox[kk], qbox[q][:, None, :]
            meet = (kb[None, :, 0] <= qb[:, :, 2]) & (qb[:, :, 0] <= kb[None, :, 2]) & (kb[None, :, 1] <= qb[:, :, 3]) & (qb[:, :, 1] <= kb[None, :, 3])
            a, b = np.nonzero(meet)
            qs.append(q[a])
            ks.append(kk[b])
    return np.concatenate(qs), np.concatenate(ks)


def box_match_subsets_numpy(qbox, qgroup, qmask, kbox, kgroup, kmask, S: int, payload=None) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """(hitmask uint32 [Q], out float64 [S, Q, K] or None) without a GPU (engine.box_match_subsets gives the same bytes): hitmask = qmask & the
    OR of kmask over the keys of the query's group whose closed boxes meet the query's; out[s] = the maximum of payload[s] over those of them
    that have bit s, for the queries that have it; -inf elsewhere.  Bits at and above S are dropped."""
    if not 1 <= int(S) <= MAX_SUBSETS:
        raise ValueError(f"box match subsets: S = {S} subsets (1 to {MAX_SUBSETS})")
    qbox, kbox = np.asarray(qbox, np.float64).reshape(-1, 4), np.asarray(kbox, np.float64).reshape(-1, 4)
    qgroup, kgroup = np.asarray(qgroup, np.int64), np.asarray(kgroup, np.int64)
    low = np.uint32((1 << int(S)) - 1)
    qmask, kmask = np.asarray(qmask).astype(np.uint32) & low, np.asarray(kmask).astype(np.uint32) & low
    q, k = _matching_pairs(qbox, qgroup, kbox, kgroup)
    met = np.zeros(qbox.shape[0], np.uint32)
    np.bitwise_or.at(met, q, kmask[k])
    hit = qmask & met
    if payload is None:
        return hit, None
    pay = np.asarray(payload, np.float64)
    assert pay.ndim == 3 and pay.shape[:2] == (int(S), kbox.shape[0])
    out = np.full((int(S), qbox.shape[0], pay.shape[2]), -np.inf)
    both = qmask[q] & kmask[k]
    for s in range(int(S)):
        take = ((both >> np.uint32(s)) & np.uint32(1)).astype(bool)
        np.maximum.at(out[s], q[take], pay[s][k[take]])
    return hit, out


# ---- the cross-validation ----

def _counts_numpy(values: np.ndarray, thresholds: np.ndarray) -> np.ndarray:
    """int64 [S, K, C]: how many rows of values [S, n, K] are >= each threshold, per subset and column."""
    ev = _ev()
    return np.stack([ev._counts_numpy(values[s], thresholds) for s in range(values.shape[0])])


def _counts_torch(values, thresholds):
    import torch
    S, n, K = values.shape
    srt = torch.sort(values.permute(0, 2, 1).contiguous(), dim=2).values
    at = torch.searchsorted(srt, thresholds.expand(S, K, -1).contiguous(), right=False)
    return (n - at).cpu().numpy().astype(np.int64)


def _bits(words: np.ndarray, first: int, count: int) -> np.ndarray:
    """The `count` bits from `first` on of every word, moved down to bit 0."""
    return ((np.asarray(words).astype(np.uint32) >> np.uint32(first)) & np.uint32((1 << count) - 1)).astype(np.uint32)


def _bit_rows(words: np.ndarray, count: int) -> np.ndarray:
    """bool [count, n]: bit s of every word."""
    w = np.asarray(words).astype(np.uint32)
    return np.stack([((w >> np.uint32(s)) & np.uint32(1)).astype(bool) for s in range(count)]) if count else np.zeros((0, w.shape[0]), bool)


class _Steps:
    """The three device steps over one pair of mask columns (the train bits or the test bits), on the GPU or restated."""

    def __init__(self, data, dmask, lmask, S, K, cpu, timed):
        self.det, self.lab, self.S, self.K, self.cpu, self.timed = data["det"], data["lab"], int(S), int(K), cpu, timed
        self.G = 2 * max(1, data["years"].shape[0])
        self.dmask, self.lmask = dmask.astype(np.uint32), lmask.astype(np.uint32)
        if not cpu:
            import torch
            dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
            d, l = self.det, self.lab
            self.t = {c: dev(d[c]) for c in ("box", "group", "xy", "year_id", "conf")}
            self.t.update(lbox=dev(l["box"]), lgroup=dev(l["group"]), dmask=dev(self.dmask.astype(np.int64)), lmask=dev(self.lmask.astype(np.int64)))

    def tp(self):
        """bool [S, n]: the detection is in subset s and meets a label of subset s."""
        d, l = self.det, self.lab
        if self.cpu:
            w = box_match_subsets_numpy(d["box"], d["group"], self.dmask, l["box"], l["group"], self.lmask, self.S)[0]
            return _bit_rows(w, self.S)
        import torch
        from . import engine
        t, tm = self.t, ({} if self.timed is not None else None)
        w = engine.box_match_subsets(t["box"], t["group"], t["dmask"], t["lbox"], t["lgroup"], t["lmask"], self.G, self.S, times=tm)[0]
        self._time(tm)
        return ((w.unsqueeze(0) >> torch.arange(self.S, device=w.device, dtype=torch.int32).unsqueeze(1)) & 1).bool()

    def member_and_recall(self, eps: float):
        """(M [S, n, K], R [S, L, K]) at one distance: numpy arrays with cpu, CUDA tensors otherwise."""
        d, l = self.det, self.lab
        if self.cpu:
            M = member_conf_subsets_numpy(d["xy"], d["year_id"], d["conf"], self.dmask, eps, self.K, self.S)
            return M, box_match_subsets_numpy(l["box"], l["group"], self.lmask, d["box"], d["group"], self.dmask, self.S, payload=M)[1]
        from . import engine
        t, tm = self.t, ({} if self.timed is not None else None)
        M = engine.eval_member_conf_subsets(t["xy"], t["year_id"], t["conf"], t["dmask"], eps, self.K, self.S, times=tm)
        self._time(tm)
        R = engine.box_match_subsets(t["lbox"], t["lgroup"], t["lmask"], t["box"], t["group"], t["dmask"], self.G, self.S, payload=M, times=tm)[1]
        self._time(tm)
        return M, R

    def _time(self, tm):
        if tm:
            self.timed["sort_ms"] += tm.get("sort_ms", 0.0)
            self.timed["kernel_ms"] += tm.get("kernel_ms", 0.0)


def fold_grids(data: Dict[str, dict], dwords, lwords, n_splits: int, conf_grid, eps_grid, min_grid, cpu: bool = False,
               times: Optional[dict] = None) -> List[Dict[str, np.ndarray]]:
    """The grid phase: per fold the table evaluate.grid gives for the fold's train detections and labels (the same columns, the same row
    order), all folds from one pair of calls per distance.  dwords / lwords = the subset words of the detections and the labels."""
    import itertools
    ev = _ev()
    conf_grid, eps_grid, min_grid = ev._check_grids(conf_grid, eps_grid, min_grid)
    N, K = int(n_splits), int(min_grid.max())
    C, E, Sm = conf_grid.shape[0], eps_grid.shape[0], min_grid.shape[0]
    thr = np.asarray(conf_grid, np.float64)
    cols = min_grid.astype(np.int64) - 1
    t = {"sort_ms": 0.0, "kernel_ms": 0.0, "count_ms": 0.0}
    steps = _Steps(data, _bits(dwords, 0, N), _bits(lwords, 0, N), N, K, cpu, t if times is not None else None)
    n_pred, n_pred_tp, n_label_tp = (np.zeros((N, C, E, Sm), np.int64) for _ in range(3))
    tp = steps.tp()
    if not cpu:
        import torch
        thr_d = torch.from_numpy(thr).cuda()
        neg = torch.tensor(float("-inf"), dtype=torch.float64, device="cuda")
    for e, eps in enumerate(eps_grid):
        M, R = steps.member_and_recall(float(eps))          # one distance's M at a time
        t0 = time.perf_counter()
        if cpu:
            a, b, c = _counts_numpy(M, thr), _counts_numpy(np.where(tp[:, :, None], M, -np.inf), thr), _counts_numpy(R, thr)
        else:
            a, b, c = _counts_torch(M, thr_d), _counts_torch(torch.where(tp.unsqueeze(2), M, neg), thr_d), _counts_torch(R, thr_d)
        n_pred[:, :, e, :] = a[:, cols, :].transpose(0, 2, 1)
        n_pred_tp[:, :, e, :] = b[:, cols, :].transpose(0, 2, 1)
        n_label_tp[:, :, e, :] = c[:, cols, :].transpose(0, 2, 1)
        del M, R
        t["count_ms"] += (time.perf_counter() - t0) * 1e3
    if times is not None:
        times.update(t)
    prod = list(itertools.product(conf_grid.tolist(), eps_grid.tolist(), min_grid.tolist()))
    head = {"conf_thresh": np.asarray([p[0] for p in prod], conf_grid.dtype), "distance_threshold": np.asarray([p[1] for p in prod], eps_grid.dtype),
            "min_cluster_size": np.asarray([p[2] for p in prod], np.int64)}
    n_label = _bit_rows(_bits(lwords, 0, N), N).sum(1)
    out = []
    for f in range(N):
        table = dict(head)
        table.update(ev.rates(n_pred[f].reshape(-1), n_pred_tp[f].reshape(-1), np.full(C * E * Sm, int(n_label[f]), np.int64), n_label_tp[f].reshape(-1)))
        out.append(table)
    return out


def fold_tests(data: Dict[str, dict], dwords, lwords, n_splits: int, winners: Sequence[Optional[Tuple[float, float, int]]], K: int,
               cpu: bool = False, times: Optional[dict] = None) -> List[Optional[Tuple[int, int, int, int]]]:
    """The test phase: winners[j] = (conf, eps, min size) of fold j // len(METRICS) or None -> its (n_pred, n_pred_tp, n_label, n_label_tp) on
    the fold's test detections and labels.  One pair of calls per distinct distance among the winners."""
    N = int(n_splits)
    t = {"sort_ms": 0.0, "kernel_ms": 0.0}
    out: List[Optional[Tuple[int, int, int, int]]] = [None] * len(winners)
    distances = sorted({float(w[1]) for w in winners if w is not None})
    if distances:
        steps = _Steps(data, _bits(dwords, N, N), _bits(lwords, N, N), N, K, cpu, t if times is not None else None)
        tp = steps.tp()
        tp = tp if cpu else tp.cpu().numpy()
        n_label = _bit_rows(_bits(lwords, N, N), N).sum(1)
        for eps in distances:
            M, R = steps.member_and_recall(eps)
            for j, w in enumerate(winners):
                if w is None or float(w[1]) != eps:
                    continue
                f, col = j // len(METRICS), int(w[2]) - 1
                member, met = M[f, :, col] >= float(w[0]), R[f, :, col] >= float(w[0])
                member, met = (member, met) if cpu else (member.cpu().numpy(), met.cpu().numpy())
                out[j] = (int(member.sum()), int((member & tp[f]).sum()), int(n_label[f]), int(met.sum()))
    if times is not None:
        times["sort_ms"] = times.get("sort_ms", 0.0) + t["sort_ms"]
        times["kernel_ms"] = times.get("kernel_ms", 0.0) + t["kernel_ms"]
    return out


def _subset(data: Dict[str, dict], dtake: np.ndarray, ltake: np.ndarray) -> Dict[str, dict]:
    cut = lambda s, take: {k: (v[take] if isinstance(v, np.ndarray) and v.shape[:1] == take.shape else v) for k, v in s.items()}
    return {"det": cut(data["det"], dtake), "lab": cut(data["lab"], ltake), "years": data["years"]}


def cross_validate(data: Dict[str, dict], images: Dict[str, np.ndarray], split, n_splits: int, conf_grid, eps_grid, min_grid,
                   op: Optional[Tuple[float, float, int]] = None, cpu: bool = False, times: Optional[dict] = None) -> dict:
    """The whole procedure for evaluate.inputs() `data`, image_table() `images` and split_images() `split` -> {"rows": two per fold (product,
    then f_score) with RESULT_COLUMNS as keys (None where a fold has no winner), "holdout": evaluate.operating_point(*op) on the images set
    aside (None without a hold-out or without op), "words": (detections', labels')}."""
    ev = _ev()
    N = int(n_splits)
    conf_grid, eps_grid, min_grid = ev._check_grids(conf_grid, eps_grid, min_grid)
    words = subset_words(split, N)
    dwords = np.where(images["det_row"] >= 0, words[np.maximum(images["det_row"], 0)], np.uint32(0)).astype(np.uint32)
    lwords = np.where(images["lab_row"] >= 0, words[np.maximum(images["lab_row"], 0)], np.uint32(0)).astype(np.uint32)
    tables = fold_grids(data, dwords, lwords, N, conf_grid, eps_grid, min_grid, cpu=cpu, times=times)
    best, winners = [], []
    for f in range(N):
        for metric in METRICS:
            k = ev.idxmax(tables[f][metric])
            best.append(k)
            winners.append(None if k is None else (float(tables[f]["conf_thresh"][k]), float(tables[f]["distance_threshold"][k]),
                                                   int(tables[f]["min_cluster_size"][k])))
    counts = fold_tests(data, dwords, lwords, N, winners, int(min_grid.max()), cpu=cpu, times=times)
    rows = []
    for j, (k, w, c) in enumerate(zip(best, winners, counts)):
        f, metric = j // len(METRICS), METRICS[j % len(METRICS)]
        row = {c_: None for c_ in RESULT_COLUMNS}
        row.update(metric=metric, fold_id=f)
        if w is not None:
            r = ev.rates(*c)
            row.update(test_precision=float(r["precision"]), test_recall=float(r["recall"]), train_best_conf_thresh=tables[f]["conf_thresh"][k].item(),
                       train_best_distance_threshold=tables[f]["distance_threshold"][k].item(), train_best_min_cluster_size=int(w[2]),
                       test_n_pred=c[0], test_n_pred_tp=c[1], test_n_label=c[2], test_n_label_tp=c[3], train_score=float(tables[f][metric][k]))
        rows.append(row)
    held = (words >> np.uint32(2 * N)) & np.uint32(1)
    holdout = None
    if op is not None and held.any():
        hd, hl = ((dwords >> np.uint32(2 * N)) & np.uint32(1)).astype(bool), ((lwords >> np.uint32(2 * N)) & np.uint32(1)).astype(bool)
        holdout = ev.operating_point(_subset(data, hd, hl), float(op[0]), float(op[1]), int(op[2]), cpu=cpu)
    return {"rows": rows, "holdout": holdout, "words": (dwords, lwords), "tables": tables}


# ---- files ----

def _cell(v) -> str:
    if v is None:
        return ""
    if isinstance(v, (bool, np.bool_)):
        return "True" if v else "False"
    if isinstance(v, (int, np.integer)):
        return str(int(v))
    if isinstance(v, str):
        return v
    return "" if v != v else repr(float(v))


def write_results_csv(path: str, rows: Sequence[dict]) -> int:
    """kfold_results.csv: the reference's columns, the four test counts and the train score; two lines per fold; doubles as ``repr``, NaN and
    the cells of a fold without a winner empty."""
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(RESULT_COLUMNS)
        for r in rows:
            w.writerow([_cell(r[c]) for c in RESULT_COLUMNS])
    return len(rows)


def read_results_csv(path: str) -> List[dict]:
    ints = {"train_best_min_cluster_size", "fold_id", "test_n_pred", "test_n_pred_tp", "test_n_label", "test_n_label_tp"}
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    conv = lambda c, v: v if c == "metric" else (None if v == "" else int(v)) if c in ints else (None if v == "" else float(v))
    return [{c: conv(c, r[c]) for c in RESULT_COLUMNS} for r in rows]


def split_names(split) -> List[str]:
    return ["test" if s < 0 else f"fold{int(s)}" for s in np.asarray(split).tolist()]


def _image_line(images: Dict[str, np.ndarray], k: int, bucket: str, split: str) -> list:
    y = int(images["year"][k])
    return [images["image"][k], "" if y < 0 else str(y), _cell(images["n_detections"][k]), _cell(float(images["det_conf"][k])),
            _cell(images["n_labels"][k]), _cell(bool(images["in_known_area"][k])), bucket, split]


def write_images_csv(path: str, images: Dict[str, np.ndarray], split, land: Optional[Dict[str, np.ndarray]] = None) -> int:
    """kfold_images.csv: one line per image of the table, in its order; split = ``test`` (set aside) or ``fold<k>`` (tested in fold k).
    land = the image table of the images wholly on land, with ``at``: the line each of them comes before (their place in the list of all
    images); their bucket and split are ``land``."""
    names = split_names(split)
    at = np.asarray(land["at"], np.int64) if land is not None else np.zeros(0, np.int64)
    j = 0
    with open(path, "w", newline="") as f:
        w = csv.writer(f, lineterminator="\n")
        w.writerow(IMAGE_COLUMNS)
        for k in range(len(names) + 1):
            while j < at.shape[0] and at[j] == k:
                w.writerow(_image_line(land, j, LAND, LAND))
                j += 1
            if k < len(names):
                w.writerow(_image_line(images, k, STRATA[int(images["bucket"][k])], names[k]))
    return len(names) + int(at.shape[0])


def read_images_csv(path: str) -> Dict[str, list]:
    with open(path, newline="") as f:
        rows = list(csv.DictReader(f))
    out = {c: [r[c] for r in rows] for c in IMAGE_COLUMNS}
    out["year"] = [int(v) if v else -1 for v in out["year"]]
    out["n_detections"], out["n_labels"] = [int(v) for v in out["n_detections"]], [int(v) for v in out["n_labels"]]
    out["det_conf"] = [float(v) if v else float("nan") for v in out["det_conf"]]
    out["in_known_area"] = [v == "True" for v in out["in_known_area"]]
    return out


def summary(images: Dict[str, np.ndarray], split, result: dict, params: dict, device: str, land: Optional[Dict[str, np.ndarray]] = None) -> dict:
    """What kfold.json holds: the parameters, the strata, mean and sd (ddof = 1) of the test precision and recall per metric over the folds that
    have a value, the hold-out operating point, the device.  land = the image table of the images wholly on land (kfold(land=...)): a ``land``
    row in the strata and their number as ``land_images``; n_images stays the number of images the splits were drawn over."""
    ev = _ev()
    clean = lambda d: {k: (clean(v) if isinstance(v, dict) else ev._json_num(v)) for k, v in d.items()}
    stats = {}
    for metric in METRICS:
        stats[metric] = {}
        for c in ("test_precision", "test_recall"):
            v = np.asarray([r[c] for r in result["rows"] if r["metric"] == metric and r[c] is not None and r[c] == r[c]], np.float64)
            stats[metric][c] = {"folds": int(v.shape[0]), "mean": float(v.mean()) if v.shape[0] else None,
                                "sd": float(v.std(ddof=1)) if v.shape[0] > 1 else None}
    split = np.asarray(split)
    out = {"parameters": params, "n_images": int(split.shape[0]), "n_train_images": int((split >= 0).sum()), "n_test_images": int((split < 0).sum()),
           "strata": strata_table(images, land), "folds": stats, "holdout": None if result["holdout"] is None else clean(result["holdout"]), "device": device}
    if land is not None:
        out["land_images"] = int(land["image"].shape[0])
    return out


def kfold(table: Dict[str, np.ndarray], truth: Dict[str, np.ndarray], out_dir: str, n_splits: int = 5, names: Optional[Sequence[str]] = None,
          rects=None, sites=None, seed: int = 1, test_frac: float = 0.1, conf_grid=None, eps_grid=None, min_grid=None,
          op: Tuple[float, float, int] = (0.5, 10.0, 5), keep=None, images: Optional[Sequence[str]] = None, cpu: bool = False,
          device: Optional[str] = None, times: Optional[dict] = None, land: Optional[Sequence[str]] = None) -> dict:
    """evaluate.inputs(table, truth, keep, images), the image table over `names` (default: the images of the detection table -- those with a
    label file -- and of the truth, sorted by stem; `images` restricts either; rects = their rectangles, or a function of the stem, needed
    with sites), the splits, cross_validate() and the three files in
    out_dir: kfold_results.csv, kfold_images.csv, kfold.json -> summary().  device = what kfold.json records as the device (default: "cpu" with
    cpu, the GPU's name otherwise).  land = the images wholly on land (names or stems; land_images.py), None without ``--land-images``: they
    leave `names` before the image table is made, the order of the rest kept, so the hold-out permutation and the folds run over the ocean
    images only, as the reference's do; kfold_images.csv lists them where they stood, with bucket and split ``land``."""
    ev = _ev()
    conf_grid = ev.DEFAULT_CONF if conf_grid is None else conf_grid
    eps_grid = ev.DEFAULT_EPS if eps_grid is None else eps_grid
    min_grid = ev.DEFAULT_MIN if min_grid is None else min_grid
    data = ev.inputs(table, truth, keep, images)
    det_image = [str(table["stems"][i]) for i in np.asarray(table["image"], np.int64)[data["det"]["rows"]]]
    lab_image = [str(s) for s in np.asarray(truth["image"], dtype=object)[data["lab"]["rows"]]]
    if names is None:
        names = sorted({ev._stem(s) for s in table["stems"]} | {ev._stem(s) for s in truth["image"]})
    if images is not None:
        wanted = {ev._stem(s) for s in images}
        names = [s for s in names if ev._stem(s) in wanted]
    rect_of = rects if callable(rects) else None
    if rect_of is None and rects is not None:
        rects = np.asarray(rects, np.float64).reshape(-1, 4)
        if rects.shape[0] != len(names):
            raise ValueError(f"kfold: {rects.shape[0]} rectangles for {len(names)} images")
    land_imgs = None
    if land is not None:
        # Their detections and labels get no table row and so no subset word: they take part in no fold and not in the hold-out.  (Under
        # --land-filter they were gone already: a detection's box lies inside its image's rectangle, that inside the land, so the land
        # filter's byte for it is not 0 and the ocean rows hold none of them.)
        on = {ev._stem(s) for s in land}
        is_land = np.asarray([ev._stem(s) in on for s in names], bool).reshape(-1)
        land_names = [s for s, l in zip(names, is_land) if l]
        names = [s for s, l in zip(names, is_land) if not l]
        land_rects = None
        if rect_of is None and rects is not None:
            land_rects, rects = rects[is_land], rects[~is_land]
        elif rect_of is not None:
            land_rects = np.asarray([rect_of(ev._stem(s)) for s in land_names], np.float64).reshape(-1, 4)
        land_imgs = image_table(land_names, det_image, data["det"]["conf"], lab_image, land_rects, sites)
        land_imgs["at"] = (np.nonzero(is_land)[0] - np.arange(len(land_names))).astype(np.int64)      # the ocean image each one stood before
    if rect_of is not None:
        rects = np.asarray([rect_of(ev._stem(s)) for s in names], np.float64).reshape(-1, 4)
    imgs = image_table(names, det_image, data["det"]["conf"], lab_image, rects, sites)
    split = split_images(imgs["bucket"], n_splits, seed, test_frac)
    result = cross_validate(data, imgs, split, n_splits, conf_grid, eps_grid, min_grid, op=op, cpu=cpu, times=times)
    if device is None:
        if cpu:
            device = "cpu"
        else:
            import torch
            device = torch.cuda.get_device_name()
    params = {"n_splits": int(n_splits), "seed": int(seed), "test_fraction": float(test_frac), "known_sites": 0 if sites is None else int(np.asarray(sites).shape[0]),
              "conf_thresholds": int(np.atleast_1d(conf_grid).shape[0]), "distance_thresholds": [float(v) for v in np.atleast_1d(eps_grid)],
              "min_cluster_sizes": [int(v) for v in np.atleast_1d(min_grid)], "operating_point": [float(op[0]), float(op[1]), int(op[2])]}
    t0 = time.perf_counter()
    os.makedirs(out_dir, exist_ok=True)
    write_results_csv(os.path.join(out_dir, RESULTS_FILE), result["rows"])
    write_images_csv(os.path.join(out_dir, IMAGES_FILE), imgs, split, land_imgs)
    s = summary(imgs, split, result, params, device, land_imgs)
    with open(os.path.join(out_dir, JSON_FILE), "w") as f:
        json.dump(s, f, indent=1)
    if times is not None:
        times["kfold_files_ms"] = (time.perf_counter() - t0) * 1e3
    return s


def describe(s: dict) -> str:
    num = lambda v: "nan" if v is None else f"{v:.4f}"
    f = s["folds"]["f_score"]
    return (f"{s['parameters']['n_splits']}-fold cross-validation over {s['n_train_images']} images ({s['n_test_images']} set aside): by f_score, "
            f"test precision {num(f['test_precision']['mean'])} +- {num(f['test_precision']['sd'])}, recall {num(f['test_recall']['mean'])} +- "
            f"{num(f['test_recall']['sd'])}")


def tile_rects(wanted_bboxes_csv: str):
    """stem -> (west, south, east, north) of a tile inside its scene, from the reference's data/wanted_bboxes.csv (blank_geom.tile_bounds)."""
    from . import blank_geom
    boxes = geocode.load_wanted_bboxes(wanted_bboxes_csv)
    return lambda stem: blank_geom.tile_bounds(stem, boxes)
