"""``yolov5/val.py`` on the HIP engine: P, R, mAP@0.5 and mAP@0.5:0.95 of a set of weights on a split of a YOLO dataset yaml.

    python yolov5/val.py --data DATA.yaml --weights W.pt [--half | --precision P] [--task val]

What upstream does ([UPSTREAM val.py run(), process_batch; utils/metrics.py ap_per_class, compute_ap, smooth, box_iou; utils/general.py
non_max_suppression(conf_thres=0.001, iou_thres=0.6, multi_label=True, max_det=300); utils/dataloaders.py img2label_paths,
verify_image_label]) and what is here:

  * the images go through detect.py's loader and device letterbox, not upstream's rect / pad 0.5 / INTER_AREA loader;
  * ``multi_label`` is a row expansion in front of the engine's NMS (aq_val_expand_rows_f32);
  * detections are matched to labels on the GPU (aq_val_match), in original-image pixels, fp32, without a host round trip;
  * after the sweep the GPU computes ap_per_class's scans, interpolations and sums (aq_val_scores_f64) on the stably sorted detections;
  * with ``--confusion-matrix`` the same detections and labels also go through upstream's ConfusionMatrix.process_batch on the GPU
    (aq_val_confusion): val_confusion.csv, val_confusion_norm.csv, val_images.csv and a ``confusion`` object in val.json;
  * with ``--plots [N]`` the first N batches (3) also become upstream's mosaics, val_batch{i}_labels.jpg and val_batch{i}_pred.jpg, pasted,
    resized, drawn and JPEG-transformed on the GPU (val_plots.py: aq_val_mosaic_u8, aq_annotate_u8, aq_image_jpeg_coefs_q).

Every device step has a numpy restatement here (expand_rows_numpy, match_numpy, confusion_numpy, scores_numpy) that gives the same bytes; ``--cpu`` runs
them on detections read back from label files: ``python -m aquaculture_amd.val --data DATA.yaml --labels DIR --cpu``.
"""
from __future__ import annotations

import argparse
import json
import os
import sys
import time
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

F32 = np.float32
IOUV = np.linspace(0.5, 0.95, 10).astype(F32)          # [UPSTREAM val.py] torch.linspace(0.5, 0.95, 10): the same ten fp32 values
AP_X = np.linspace(0, 1, 101)                          # [UPSTREAM compute_ap] the 101-point COCO integration grid
PX = np.linspace(0, 1, 1000)                           # [UPSTREAM ap_per_class] the confidence axis of the curves
EPS = 1e-16
CLASS_OFFSET = 7680                                    # [UPSTREAM non_max_suppression] max_wh: the per-class box offset
ROWS_BUDGET = 1 << 30                                  # bytes of expanded rows [b, M, 5 + nc] per NMS call: the batch is cut to stay under it
TASKS = ("val", "test", "train")
REFUSED_TASKS = {"speed": "--task speed is not part of this val.py: time the sweep with bench.py",
                 "study": "--task study is not part of this val.py: run it once per --imgsz"}
REFUSED_FLAGS = {"augment": "--augment is not part of this val.py (yolov5/detect.py runs augmented inference)",
                 "save_hybrid": "--save-hybrid is not part of this val.py: labels are never mixed into the predictions",
                 "save_json": "--save-json is not part of this val.py: no COCO json is written"}
DEPARTURES = (
    "images are loaded and letterboxed as yolov5/detect.py loads them (INTER_LINEAR, auto pad to a stride multiple), not by upstream's "
    "rect / pad 0.5 / INTER_AREA loader",
    "a best-label tie between more than one label of equal IoU goes to the higher label index (upstream leaves larger tie sets to numpy's sort)",
    "the trapezoid sum of compute_ap is added in ascending x one term at a time (numpy adds in pairwise blocks)",
    "dataset paths in the yaml that are relative resolve against the yaml file's directory",
    "a split entry that is a file with an image extension is that one image (upstream reads every file entry as a list of paths)",
    "the sort of the detections by confidence is stable: equal confidences stay in sweep order (upstream's np.argsort(-conf) is not stable)",
    "mAP50-95 of the all row is ap.mean(1).mean(), the mean over classes of each class's mean over the ten thresholds, as upstream computes it",
    "per-class rows are printed when (--verbose or nc < 50) and nc > 1, upstream's full condition",
)
CONFUSION_CONF, CONFUSION_IOU = 0.25, 0.45             # [UPSTREAM ConfusionMatrix.__init__] conf, iou_thres
CONFUSION_TIE_NOTE = ("confusion matrix: among equal IoUs a detection's best label is the one of higher index and a label keeps the detection of "
                      "higher index (upstream's argsort is not stable and leaves equal IoUs to numpy's sort)")
CONFUSION_QUIRK_NOTE = ("confusion matrix: in an image without a kept (label, detection) pair the detections add no background counts (upstream's "
                        "`if n:`), and an image without labels adds nothing whatever was detected on it (upstream's val.py calls process_batch only "
                        "for images with labels)")
TABLE_HEADER = ("%22s" + "%11s" * 6) % ("Class", "Images", "Instances", "P", "R", "mAP50", "mAP50-95")
TABLE_ROW = "%22s" + "%11i" * 2 + "%11.3g" * 4
NO_LABELS = "WARNING ⚠️ no labels found in %s set, can not compute metrics without labels"
IMG_FORMATS = ("bmp", "dng", "jpeg", "jpg", "mpo", "png", "tif", "tiff", "webp", "pfm")


# ------------------------------------------------------------------ data ------------------------------------------------------------------
def load_data_yaml(path: str) -> dict:
    """The dataset yaml: optional ``path``, ``train`` / ``val`` / ``test`` (a directory, a .txt list, or a list of either), ``names`` (a list
    or an {id: name} dict), optional ``nc``.  -> {"path", "train", "val", "test" (lists of absolute paths, or None), "names" {id: name}, "nc"}."""
    import yaml
    with open(path, errors="ignore") as f:
        data = yaml.safe_load(f)
    if not isinstance(data, dict):
        raise ValueError(f"{path}: not a dataset yaml (a mapping with val / names)")
    if "names" not in data:
        raise ValueError(f"{path}: 'names' is missing")
    names = data["names"]
    if isinstance(names, (list, tuple)):
        names = dict(enumerate(names))
    names = {int(k): str(v) for k, v in names.items()}
    nc = int(data.get("nc", len(names)))
    if nc != len(names) or sorted(names) != list(range(nc)):
        raise ValueError(f"{path}: {len(names)} names for nc = {nc} (the ids have to be 0 .. nc - 1)")
    root = Path(data.get("path") or "")
    if not root.is_absolute():
        root = (Path(path).resolve().parent / root).resolve()
    out = {"path": str(root), "names": names, "nc": nc}
    for k in TASKS:
        v = data.get(k)
        if v is None:
            out[k] = None
            continue
        entries = []
        for x in (v if isinstance(v, (list, tuple)) else [v]):
            p = (root / str(x)).resolve()
            if not p.exists() and str(x).startswith("../"):          # [UPSTREAM check_dataset]
                p = (root / str(x)[3:]).resolve()
            entries.append(str(p))
        out[k] = entries
    return out


def list_split_images(entries: Sequence[str]) -> List[str]:
    """[UPSTREAM LoadImagesAndLabels.__init__]: every entry a directory (searched recursively) or a .txt list of image paths (a leading ./
    stands for the list's directory); the image files of all entries, sorted."""
    import glob
    found: List[str] = []
    for e in entries:
        p = Path(e)
        if p.is_dir():
            found += glob.glob(str(p / "**" / "*.*"), recursive=True)
        elif p.is_file() and p.suffix[1:].lower() in IMG_FORMATS:                # (one image, named directly)
            found.append(str(p))
        elif p.is_file():
            parent = str(p.parent) + os.sep
            with open(p) as f:
                found += [x.replace("./", parent, 1) if x.startswith("./") else x for x in f.read().strip().splitlines() if x.strip()]
        else:
            raise FileNotFoundError(f"{e} does not exist")
    files = sorted(x for x in found if x.split(".")[-1].lower() in IMG_FORMATS)
    if not files:
        raise FileNotFoundError(f"no images found in {list(entries)}")
    return files


def img2label_path(image_path: str) -> str:
    """[UPSTREAM img2label_paths]: the LAST /images/ of the path becomes /labels/, the extension .txt."""
    sa, sb = f"{os.sep}images{os.sep}", f"{os.sep}labels{os.sep}"
    return sb.join(image_path.rsplit(sa, 1)).rsplit(".", 1)[0] + ".txt"


def read_label_file(path: str) -> Tuple[Optional[np.ndarray], int]:
    """[UPSTREAM verify_image_label] -> (rows float32 [n, 5] = cls xc yc w h, duplicate rows dropped).  A missing file: no labels.  A row
    whose column count is not five, a negative value or a coordinate above 1: (None, 0) -- the image is corrupt and is skipped.  Exact
    duplicate rows are dropped as upstream drops them (np.unique(axis=0): the rows that are left come in sorted order)."""
    if not os.path.isfile(path):
        return np.zeros((0, 5), F32), 0
    with open(path) as f:
        rows = [x.split() for x in f.read().strip().splitlines() if len(x)]
    if not rows:
        return np.zeros((0, 5), F32), 0
    if any(len(r) != 5 for r in rows):
        return None, 0
    try:
        lb = np.array(rows, dtype=F32)
    except ValueError:
        return None, 0
    if not (lb >= 0).all() or not (lb[:, 1:] <= 1).all():
        return None, 0
    _, i = np.unique(lb, axis=0, return_index=True)
    dup = lb.shape[0] - len(i)
    if dup:
        lb = lb[i]
    return lb, dup


def label_boxes(lb: np.ndarray, h0: int, w0: int) -> np.ndarray:
    """Label rows (cls xc yc w h, normalised) -> fp32 pixel boxes [n, 4]: x1 = (xc - w / 2) * w0, x2 = (xc + w / 2) * w0, likewise y with h0;
    one fp32 rounding per operation, in that order."""
    lb = np.asarray(lb, dtype=F32).reshape(-1, 5)
    hw, hh = lb[:, 3] / F32(2), lb[:, 4] / F32(2)
    return np.stack([(lb[:, 1] - hw) * F32(w0), (lb[:, 2] - hh) * F32(h0), (lb[:, 1] + hw) * F32(w0), (lb[:, 2] + hh) * F32(h0)], 1).astype(F32)


def letterbox_geom(img1_shape, img0_shape) -> np.ndarray:
    """(pad x, pad y, gain, w0, h0) as fp32: the constants of postprocess.scale_boxes for one image."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = ((img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2)
    return np.array([pad[0], pad[1], gain, img0_shape[1], img0_shape[0]], dtype=F32)


def scale_boxes_geom(boxes: np.ndarray, geom: np.ndarray) -> np.ndarray:
    """postprocess.scale_boxes from a letterbox_geom row: subtract the pad, divide by the gain, clip to the original image (no rounding)."""
    b = np.array(boxes, dtype=F32, copy=True).reshape(-1, 4)
    b[:, [0, 2]] -= geom[0]
    b[:, [1, 3]] -= geom[1]
    b /= geom[2]
    b[:, [0, 2]] = np.clip(b[:, [0, 2]], F32(0), geom[3])
    b[:, [1, 3]] = np.clip(b[:, [1, 3]], F32(0), geom[4])
    return b


# ------------------------------------------------------------ numpy restatements ----------------------------------------------------------
def expand_rows_numpy(pred: np.ndarray, conf_thres: float, M: int, rows: Optional[np.ndarray] = None) -> Tuple[np.ndarray, np.ndarray]:
    """aq_val_expand_rows_f32: pred float32 [B, N, 5 + nc] -> (rows [B, M, 5 + nc], counts int32 [B]).  ``rows`` = the buffer's bytes
    before the call (zeros when not given): what the kernel does not write stays."""
    pred = np.asarray(pred, dtype=F32)
    B, N, no = pred.shape
    conf = F32(conf_thres)
    rows = np.zeros((B, M, no), F32) if rows is None else rows
    counts = np.zeros(B, np.int32)
    picks = []
    for b in range(B):
        obj = pred[b, :, 4:5]
        ok = (obj > conf) & (obj * pred[b, :, 5:] > conf)                       # one fp32 product
        r, j = np.nonzero(ok)                                                   # (row, class) ascending
        counts[b] = r.shape[0]
        picks.append((r, j))
    if (counts > M).any():
        return rows, counts
    for b, (r, j) in enumerate(picks):
        k = r.shape[0]
        out = np.zeros((k, no), F32)
        out[:, :5] = pred[b, r, :5]
        out[np.arange(k), 5 + j] = pred[b, r, 5 + j]
        rows[b, :k] = out
        rows[b, k:, 4] = 0
    return rows, counts


def box_iou_numpy(lbox: np.ndarray, dbox: np.ndarray) -> np.ndarray:
    """[UPSTREAM box_iou(labels, detections)] in fp32, [L, D]: inter / (area_l + area_d - inter + 1e-7)."""
    a, b = np.asarray(lbox, dtype=F32).reshape(-1, 1, 4), np.asarray(dbox, dtype=F32).reshape(1, -1, 4)
    area_l = (a[..., 2] - a[..., 0]) * (a[..., 3] - a[..., 1])
    area_d = (b[..., 2] - b[..., 0]) * (b[..., 3] - b[..., 1])
    iw = np.maximum(np.minimum(a[..., 2], b[..., 2]) - np.maximum(a[..., 0], b[..., 0]), F32(0))
    ih = np.maximum(np.minimum(a[..., 3], b[..., 3]) - np.maximum(a[..., 1], b[..., 1]), F32(0))
    inter = iw * ih
    return (inter / (area_l + area_d - inter + F32(1e-7))).astype(F32)


def match_numpy(lbox: np.ndarray, lcls: np.ndarray, dbox: np.ndarray, dcls: np.ndarray, iouv: np.ndarray = IOUV) -> np.ndarray:
    """process_batch as the closed rule (aq_val_match): labels [L, 4] / [L], detections [D, 4] / [D] in descending confidence, original
    pixels -> uint16 [D], bit i = correct at iouv[i].  1. every detection's best label is the label of its class with the largest IoU, the
    higher index among equal IoUs; it is eligible at i iff that IoU >= iouv[i].  2. per (label, i) the eligible detection of lowest index
    that has the label as its best is correct; a detection that loses its best label does not fall back to another."""
    lcls, dcls = np.asarray(lcls).astype(np.int64).reshape(-1), np.asarray(dcls).astype(np.int64).reshape(-1)
    L, D = lcls.shape[0], dcls.shape[0]
    bits = np.zeros(D, np.uint16)
    if L == 0 or D == 0:
        return bits
    iou = box_iou_numpy(lbox, dbox)
    same = lcls[:, None] == dcls[None, :]
    masked = np.where(same, iou, F32(-1))
    best = L - 1 - np.argmax(masked[::-1], axis=0)                              # the largest, the highest index among equals
    d = np.arange(D)
    has = same.any(0)
    biou = iou[best, d]
    for i, t in enumerate(np.asarray(iouv, dtype=F32)):
        elig = has & (biou >= t)
        first = np.full(L, D, np.int64)
        np.minimum.at(first, best[elig], d[elig])
        bits |= ((elig & (first[best] == d)).astype(np.uint16) << np.uint16(i)).astype(np.uint16)
    return bits


def confusion_numpy(lbox: np.ndarray, lcls: np.ndarray, dbox: np.ndarray, dconf: np.ndarray, dcls: np.ndarray, nc: int,
                    conf: float = CONFUSION_CONF, iou: float = CONFUSION_IOU) -> Tuple[np.ndarray, np.ndarray]:
    """[UPSTREAM utils/metrics.py ConfusionMatrix.process_batch, called per image with labels] as the closed rule (aq_val_confusion): labels
    [L, 4] / [L], detections [D, 4] / [D] / [D] in original pixels -> (what the image adds to matrix[predicted][true], int64 [nc + 1,
    nc + 1], index nc = background; int32 [4] = labels, detections that take part, kept pairs, kept pairs of equal classes).  1. a
    detection takes part iff its confidence > conf; its best label is the label of any class with the largest IoU among those with IoU >
    iou, the higher index among equal IoUs.  2. a label keeps, of the detections whose best label it is, the one with the largest IoU, the
    higher index among equal ones: matrix[its class][label class] += 1; a label that keeps none: matrix[nc][label class] += 1; no
    fall-back.  3. with at least one kept pair, every detection that takes part and that no label keeps: matrix[its class][nc] += 1;
    without one the detections add nothing.  4. an image without labels adds nothing."""
    lcls, dcls = np.asarray(lcls).astype(np.int64).reshape(-1), np.asarray(dcls).astype(np.int64).reshape(-1)
    dconf = np.asarray(dconf, dtype=F32).reshape(-1)
    L, D, n1 = lcls.shape[0], dcls.shape[0], int(nc) + 1
    if ((lcls < 0) | (lcls >= nc)).any() or ((dcls < 0) | (dcls >= nc)).any():
        raise ValueError(f"val: a detection or label class outside [0, {nc})")
    m = np.zeros((n1, n1), np.int64)
    take = dconf > F32(conf)
    part = int(take.sum())
    if L == 0:
        return m, np.array([0, part, 0, 0], np.int32)
    keeps = np.full(L, -1, np.int64)                                            # the detection every label keeps
    if part:
        idx = np.nonzero(take)[0]
        io = box_iou_numpy(lbox, np.asarray(dbox, dtype=F32).reshape(-1, 4)[idx])
        masked = np.where(io > F32(iou), io, F32(-1))
        best = L - 1 - np.argmax(masked[::-1], axis=0)                          # the largest, the highest index among equals
        has = masked[best, np.arange(part)] > 0
        idx, best, biou = idx[has], best[has], io[best, np.arange(part)][has]
        o = np.lexsort((idx, biou))                                             # ascending (IoU, index): of repeated labels the last assignment stays
        keeps[best[o]] = idx[o]
    kept = keeps >= 0
    np.add.at(m, (dcls[keeps[kept]], lcls[kept]), 1)
    m[nc] += np.bincount(lcls[~kept], minlength=n1)
    if kept.any():
        free = take.copy()
        free[keeps[kept]] = False
        m[:, nc] += np.bincount(dcls[free], minlength=n1)
    return m, np.array([L, part, int(kept.sum()), int((dcls[keeps[kept]] == lcls[kept]).sum())], np.int32)


def confusion_tp_fp(matrix: np.ndarray) -> Tuple[np.ndarray, np.ndarray]:
    """[UPSTREAM ConfusionMatrix.tp_fp]: tp = the diagonal, fp = the row sums - tp, both without the background entry."""
    tp = matrix.diagonal()
    fp = matrix.sum(1) - tp
    return tp[:-1], fp[:-1]


def confusion_normalised(matrix: np.ndarray) -> np.ndarray:
    """[UPSTREAM ConfusionMatrix.plot, normalize=True]: every column divided by (its sum + 1e-9)."""
    return matrix / (matrix.sum(0).reshape(1, -1) + 1e-9)


def interp_numpy(x: np.ndarray, xp: np.ndarray, fp: np.ndarray, left: float) -> np.ndarray:
    """np.interp's rule, written out (interp_rule of csrc/val.hip): j = the last index with xp[j] <= x; fp[j] when j is the last index or
    xp[j] == x, else (fp[j + 1] - fp[j]) / (xp[j + 1] - xp[j]) * (x - xp[j]) + fp[j]; ``left`` below xp[0], fp[-1] above xp[-1]."""
    x, xp, fp = np.asarray(x, dtype=np.float64), np.asarray(xp, dtype=np.float64), np.asarray(fp, dtype=np.float64)
    last = xp.shape[0] - 1
    j = np.clip(np.searchsorted(xp, x, side="right") - 1, 0, last)
    j1 = np.minimum(j + 1, last)
    with np.errstate(divide="ignore", invalid="ignore"):
        line = (fp[j1] - fp[j]) / (xp[j1] - xp[j]) * (x - xp[j]) + fp[j]
    out = np.where((j == last) | (xp[j] == x), fp[j], line)
    out = np.where(x < xp[0], np.float64(left), out)
    return np.where(x > xp[last], fp[last], out)


def scores_numpy(bits: np.ndarray, conf: np.ndarray, run_range: np.ndarray, n_l: np.ndarray, x: np.ndarray = AP_X, px: np.ndarray = PX):
    """aq_val_scores_f64: bits uint16 [n] and conf float32 [n] sorted by (class, -confidence, index); run_range int64 [C, 2] and n_l [C]: the
    run and the label count of every class that has labels -> (ap [C, 10], p [C, npx], r [C, npx], pr [C, npx]) float64."""
    bits = np.asarray(bits).astype(np.uint16).reshape(-1)
    conf = np.asarray(conf, dtype=F32).reshape(-1)
    rr = np.asarray(run_range, dtype=np.int64).reshape(-1, 2)
    C_ = rr.shape[0]
    x, px = np.asarray(x, dtype=np.float64), np.asarray(px, dtype=np.float64)
    ap = np.zeros((C_, 10))
    p, r, pr = (np.zeros((C_, px.shape[0])) for _ in range(3))
    for c in range(C_):
        a, e = int(rr[c, 0]), int(rr[c, 1])
        n = e - a
        if n == 0:
            continue
        nconf = -conf[a:e].astype(np.float64)
        denom = float(n_l[c]) + EPS
        k1 = np.arange(1, n + 1, dtype=np.float64)
        for j in range(10):
            tpc = np.cumsum((bits[a:e] >> np.uint16(j)) & np.uint16(1), dtype=np.int32)
            recall = tpc / denom
            precision = tpc / k1
            mrec = np.concatenate(([0.0], recall, [1.0]))
            mpre = np.concatenate(([1.0], precision, [0.0]))
            mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
            y = interp_numpy(x, mrec, mpre, 1.0)
            s = np.float64(0.0)
            for k in range(x.shape[0] - 1):                                     # ascending x, one term at a time
                s = s + (x[k + 1] - x[k]) * (y[k + 1] + y[k]) / 2.0
            ap[c, j] = s
            if j == 0:
                r[c] = interp_numpy(-px, nconf, recall, 0.0)
                p[c] = interp_numpy(-px, nconf, precision, 1.0)
                pr[c] = interp_numpy(px, mrec, mpre, 1.0)
    return ap, p, r, pr


def smooth(y: np.ndarray, f: float = 0.05) -> np.ndarray:
    """[UPSTREAM utils/metrics.py smooth]: box filter of fraction f."""
    nf = round(len(y) * f * 2) // 2 + 1
    e = np.ones(nf // 2)
    yp = np.concatenate((e * y[0], y, e * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def summarise(ap: np.ndarray, p: np.ndarray, r: np.ndarray, n_l: np.ndarray) -> dict:
    """The small arithmetic of ap_per_class and val.py after the curves, in numpy as upstream writes it: f1, the index of the smoothed mean
    F1's maximum, P / R / F1 there, tp, fp, and the means over the classes that have labels."""
    n_l = np.asarray(n_l, dtype=np.int64)
    if ap.shape[0] == 0:
        z = np.zeros(0)
        return {"i": 0, "p": z, "r": z, "f1": z, "f1_curve": np.zeros((0, p.shape[1])), "ap50": z, "ap": z, "tp": z, "fp": z, "mp": 0.0, "mr": 0.0, "map50": 0.0, "map": 0.0}
    f1 = 2 * p * r / (p + r + EPS)
    i = int(smooth(f1.mean(0), 0.1).argmax())
    pi, ri, fi = p[:, i], r[:, i], f1[:, i]
    tp = (ri * n_l).round()
    fp = (tp / (pi + EPS) - tp).round()
    ap50, apm = ap[:, 0], ap.mean(1)
    return {"i": i, "p": pi, "r": ri, "f1": fi, "f1_curve": f1, "ap50": ap50, "ap": apm, "tp": tp, "fp": fp,
            "mp": float(pi.mean()), "mr": float(ri.mean()), "map50": float(ap50.mean()), "map": float(apm.mean())}


# ----------------------------------------------------------------- outputs ----------------------------------------------------------------
def format_table(names: Dict[int, str], seen: int, classes: np.ndarray, n_l: np.ndarray, s: dict, per_class: bool) -> str:
    """Upstream's table: the header, the ``all`` row, then one row per class that has labels."""
    lines = [TABLE_HEADER, TABLE_ROW % ("all", seen, int(np.sum(n_l)), s["mp"], s["mr"], s["map50"], s["map"])]
    if per_class:
        for k, c in enumerate(classes):
            lines.append(TABLE_ROW % (names[int(c)], seen, int(n_l[k]), s["p"][k], s["r"][k], s["ap50"][k], s["ap"][k]))
    return "\n".join(lines)


def _num(v) -> str:
    return repr(float(v))


def classes_csv(names: Dict[int, str], seen: int, classes: np.ndarray, n_l: np.ndarray, ap: np.ndarray, s: dict) -> str:
    head = ["class", "name", "images", "instances", "P", "R", "F1", "mAP50", "mAP50-95"] + [f"ap_{float(t):.2f}" for t in IOUV] + ["tp", "fp"]
    C_ = len(classes)
    mf1 = float(s["f1"].mean()) if C_ else 0.0
    mean_ap = [float(ap[:, j].mean()) if C_ else 0.0 for j in range(10)]
    rows = [",".join(head),
            ",".join(["-1", "all", str(seen), str(int(np.sum(n_l))), _num(s["mp"]), _num(s["mr"]), _num(mf1), _num(s["map50"]), _num(s["map"])] +
                     [_num(v) for v in mean_ap] + [str(int(np.sum(s["tp"]))), str(int(np.sum(s["fp"])))])]
    for k, c in enumerate(classes):
        rows.append(",".join([str(int(c)), names[int(c)], str(seen), str(int(n_l[k])), _num(s["p"][k]), _num(s["r"][k]), _num(s["f1"][k]),
                              _num(s["ap50"][k]), _num(s["ap"][k])] + [_num(v) for v in ap[k]] + [str(int(s["tp"][k])), str(int(s["fp"][k]))]))
    return "\n".join(rows) + "\n"


def curves_csv(names: Dict[int, str], classes: np.ndarray, p: np.ndarray, r: np.ndarray, f1: np.ndarray, pr: np.ndarray) -> str:
    head = ["px"]
    for c in classes:
        head += [f"{names[int(c)]}_{k}" for k in ("p", "r", "f1", "pr")]
    rows = [",".join(head)]
    for i in range(PX.shape[0]):
        row = [_num(PX[i])]
        for k in range(len(classes)):
            row += [_num(p[k, i]), _num(r[k, i]), _num(f1[k, i]), _num(pr[k, i])]
        rows.append(",".join(row))
    return "\n".join(rows) + "\n"


def confusion_csv(names: Dict[int, str], nc: int, matrix: np.ndarray, cell=str) -> str:
    """matrix[predicted][true]: the header ``predicted, <true class names>, background``, then one row per predicted class and ``background``."""
    labels = [names[c] for c in range(nc)] + ["background"]
    rows = [",".join(["predicted"] + labels)]
    for k, name in enumerate(labels):
        rows.append(",".join([name] + [cell(v) for v in matrix[k]]))
    return "\n".join(rows) + "\n"


def images_csv(files: Sequence[str], image: np.ndarray) -> str:
    """Per image in split order: labels, detections that take part, matched (kept pairs), matched_same_class, missed = labels - matched,
    false = detections - matched when matched > 0, else 0 -- the background counts the matrix holds for the image."""
    rows = ["image,labels,detections,matched,matched_same_class,missed,false"]
    for f, (n_l, n_d, n_m, n_s) in zip(files, np.asarray(image, dtype=np.int64).reshape(-1, 4).tolist()):
        rows.append(",".join([str(f), str(n_l), str(n_d), str(n_m), str(n_s), str(n_l - n_m), str(n_d - n_m if n_m > 0 else 0)]))
    return "\n".join(rows) + "\n"


def write_confusion(save_dir: str, names, nc: int, files: Sequence[str], matrix: np.ndarray, image: np.ndarray, conf: float, iou: float) -> dict:
    """--confusion-matrix: writes val_confusion.csv, val_confusion_norm.csv and val_images.csv into save_dir -> val.json's ``confusion`` object."""
    matrix = np.asarray(matrix, dtype=np.int64).reshape(nc + 1, nc + 1)
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "val_confusion.csv"), "w") as f:
        f.write(confusion_csv(names, nc, matrix, lambda v: str(int(v))))
    with open(os.path.join(save_dir, "val_confusion_norm.csv"), "w") as f:
        f.write(confusion_csv(names, nc, confusion_normalised(matrix), _num))
    with open(os.path.join(save_dir, "val_images.csv"), "w") as f:
        f.write(images_csv(files, image))
    tp, fp = confusion_tp_fp(matrix)
    return {"conf": float(conf), "iou": float(iou), "classes": [names[c] for c in range(nc)] + ["background"], "layout": "matrix[predicted][true]",
            "tp": [int(v) for v in tp], "fp": [int(v) for v in fp], "matrix": [[int(v) for v in row] for row in matrix],
            "notes": [CONFUSION_TIE_NOTE, CONFUSION_QUIRK_NOTE]}


def write_outputs(save_dir: str, names, nc: int, seen: int, classes, n_l, ap, p, r, pr, meta: dict, verbose: bool, task: str, log=print,
                  confusion: Optional[dict] = None) -> dict:
    """Prints the table and writes val_classes.csv, val_curves.csv and val.json into save_dir.  confusion = write_confusion's object (with
    --confusion-matrix): it goes into val.json and its tie rule under the departures."""
    s = summarise(ap, p, r, n_l)
    log(format_table(names, seen, classes, n_l, s, (verbose or nc < 50) and nc > 1 and len(classes) > 0))
    if int(np.sum(n_l)) == 0:
        log(NO_LABELS % task)
    os.makedirs(save_dir, exist_ok=True)
    with open(os.path.join(save_dir, "val_classes.csv"), "w") as f:
        f.write(classes_csv(names, seen, classes, n_l, ap, s))
    with open(os.path.join(save_dir, "val_curves.csv"), "w") as f:
        f.write(curves_csv(names, classes, p, r, s["f1_curve"], pr))
    meta = dict(meta)
    meta["results"] = {"P": s["mp"], "R": s["mr"], "mAP50": s["map50"], "mAP50-95": s["map"], "f1_index": s["i"]}
    meta["departures"] = list(DEPARTURES)
    if confusion is not None:
        meta["confusion"] = confusion
        meta["departures"].append(CONFUSION_TIE_NOTE)
    with open(os.path.join(save_dir, "val.json"), "w") as f:
        json.dump(meta, f, indent=1, sort_keys=True)
        f.write("\n")
    return s


# --------------------------------------------------------------- the dataset ---------------------------------------------------------------
class Split:
    """The images of one split with their labels: ``files`` (the images kept), ``labels`` (float32 [n, 5] each), ``skipped`` (corrupt label
    files: the image is left out, as upstream leaves it out), ``duplicates`` (label rows dropped)."""

    def __init__(self, files: Sequence[str], single_cls: bool = False, log=print):
        self.files, self.labels, self.skipped, self.duplicates = [], [], [], 0
        for f in files:
            lb, dup = read_label_file(img2label_path(f))
            if lb is None:
                self.skipped.append(f)
                log(f"WARNING ⚠️ {f}: ignoring corrupt image/label: a label row without five columns, a negative value or a coordinate above 1")
                continue
            if dup:
                log(f"WARNING ⚠️ {f}: {dup} duplicate labels removed")
            if single_cls:
                lb = lb.copy()
                lb[:, 0] = 0
            self.duplicates += dup
            self.files.append(f)
            self.labels.append(lb)
        self.n_labels = int(sum(lb.shape[0] for lb in self.labels))


def _check_classes(split: Split, nc: int) -> None:
    for f, lb in zip(split.files, split.labels):
        if lb.shape[0] and not (lb[:, 0] < nc).all():
            raise ValueError(f"{img2label_path(f)}: class {int(lb[:, 0].max())} in a dataset of {nc} classes")


def _runs(sorted_cls_counts: np.ndarray, label_counts: np.ndarray):
    """classes with labels, their label counts and their runs in the detections sorted by class: counts per class of both kinds -> (classes
    [C], n_l int32 [C], run_range int64 [C, 2])."""
    ends = np.cumsum(sorted_cls_counts.astype(np.int64))
    starts = ends - sorted_cls_counts
    classes = np.nonzero(label_counts)[0]
    return classes, label_counts[classes].astype(np.int32), np.stack([starts[classes], ends[classes]], 1).astype(np.int64).reshape(-1, 2)


# ------------------------------------------------------------- parse and refuse ------------------------------------------------------------
def parse_opt(argv: Optional[List[str]] = None) -> argparse.Namespace:
    """Upstream's val.py flags with its defaults, plus --precision, --jpeg-decode, --quiet, --labels, --cpu, --confusion-matrix with its
    two thresholds and --plots [N]."""
    root = Path.cwd()
    p = argparse.ArgumentParser(prog="val.py")
    p.add_argument("--data", type=str, required=True, help="dataset.yaml path")
    p.add_argument("--weights", nargs="+", type=str, default=None, help="model path")
    p.add_argument("--batch-size", type=int, default=32, help="batch size")
    p.add_argument("--imgsz", "--img", "--img-size", type=int, default=640, help="inference size (pixels)")
    p.add_argument("--conf-thres", type=float, default=0.001, help="confidence threshold")
    p.add_argument("--iou-thres", type=float, default=0.6, help="NMS IoU threshold")
    p.add_argument("--max-det", type=int, default=300, help="maximum detections per image")
    p.add_argument("--task", default="val", help="train, val or test (speed and study are refused)")
    p.add_argument("--device", default="", help="GPU ordinal (default 0)")
    p.add_argument("--workers", type=int, default=8, help="image decoders")
    p.add_argument("--single-cls", action="store_true", help="treat as single-class dataset")
    p.add_argument("--augment", action="store_true", help="(refused)")
    p.add_argument("--verbose", action="store_true", help="report mAP by class")
    p.add_argument("--save-txt", action="store_true", help="save results to *.txt")
    p.add_argument("--save-hybrid", action="store_true", help="(refused)")
    p.add_argument("--save-conf", action="store_true", help="save confidences in --save-txt labels")
    p.add_argument("--save-json", action="store_true", help="(refused)")
    p.add_argument("--project", default=str(root / "runs/val"), help="save to project/name")
    p.add_argument("--name", default="exp", help="save to project/name")
    p.add_argument("--exist-ok", action="store_true", help="existing project/name ok, do not increment")
    p.add_argument("--half", action="store_true", help="reduced precision (bf16 on MI355X; upstream: fp16)")
    p.add_argument("--dnn", action="store_true", help="(ignored)")
    p.add_argument("--precision", choices=("fp32", "bf16", "fp8w", "f16x3", "fp8"), default=None, help="default fp32 (bf16 with --half)")
    p.add_argument("--jpeg-decode", choices=("auto", "host", "split"), default="auto",
                   help="as yolov5/detect.py: split = entropy decoding in worker processes, the rest on the GPU (baseline 4:2:0 JPEGs of one size); "
                        "host = software decode; auto = split where every image qualifies")
    p.add_argument("--quiet", action="store_true", help="no per-batch log line")
    p.add_argument("--labels", default=None, metavar="DIR",
                   help="score the detections of DIR/<image stem>.txt (cls xc yc w h conf, as --save-txt --save-conf writes them) instead of running the engine")
    p.add_argument("--cpu", action="store_true", help="with --labels: the numpy restatements instead of the GPU kernels (same bytes)")
    p.add_argument("--confusion-matrix", action="store_true",
                   help="upstream's class confusion matrix in the same pass: val_confusion.csv, val_confusion_norm.csv, val_images.csv and val.json's confusion object")
    p.add_argument("--confusion-conf", type=float, default=CONFUSION_CONF, help="with --confusion-matrix: detections above this confidence take part")
    p.add_argument("--confusion-iou", type=float, default=CONFUSION_IOU, help="with --confusion-matrix: a label and a detection pair above this IoU")
    p.add_argument("--plots", nargs="?", type=int, const=3, default=0, metavar="N",
                   help="upstream's mosaics of the first N batches (bare flag: 3): val_batch{i}_labels.jpg and val_batch{i}_pred.jpg, made on the GPU")
    return p.parse_args(argv)


def check_opt(opt: argparse.Namespace) -> None:
    """The refusals: one line each."""
    if opt.task in REFUSED_TASKS:
        raise SystemExit(REFUSED_TASKS[opt.task])
    if opt.task not in TASKS:
        raise SystemExit(f"--task {opt.task}: train, val or test")
    for k, msg in REFUSED_FLAGS.items():
        if getattr(opt, k):
            raise SystemExit(msg)
    if int(os.environ.get("WORLD_SIZE", "1")) > 1:
        raise SystemExit("val.py runs on one GPU: start it without a launcher (WORLD_SIZE is %s)" % os.environ["WORLD_SIZE"])
    if opt.cpu and not opt.labels:
        raise SystemExit("--cpu scores detections read from label files: it needs --labels DIR (written by an earlier --save-txt --save-conf run)")
    if not opt.labels and not opt.weights:
        raise SystemExit("val.py needs --weights W.pt (or --labels DIR to score detections that were saved before)")
    if not (0.0 <= opt.conf_thres <= 1.0 and 0.0 <= opt.iou_thres <= 1.0 and opt.max_det >= 1 and opt.batch_size >= 1):
        raise SystemExit("--conf-thres and --iou-thres lie in [0, 1]; --max-det and --batch-size are at least 1")
    if opt.confusion_matrix and not (np.isfinite(opt.confusion_conf) and np.isfinite(opt.confusion_iou) and opt.confusion_iou > 0.0):
        raise SystemExit("--confusion-conf and --confusion-iou are finite numbers, --confusion-iou above 0")
    if getattr(opt, "plots", 0) < 0:
        raise SystemExit("--plots N: the mosaics of the first N batches, N at least 0")
    if getattr(opt, "plots", 0) and opt.labels:
        raise SystemExit("--plots draws the decoded images of an engine run: --labels DIR scores saved detections and has none")


# ------------------------------------------------------------------ runs -------------------------------------------------------------------
def _image_sizes(files: Sequence[str], workers: int) -> List[Tuple[int, int]]:
    """(width, height) of every image from its header."""
    from .dataloader import LoadImages
    return LoadImages("", raw=True, workers=workers, files=files).scan_sizes() if files else []


def read_detections(labels_dir: str, image_path: str, w0: int, h0: int, single_cls: bool):
    """The detections of one image from <labels_dir>/<stem>.txt as --save-txt --save-conf wrote them (cls xc yc w h conf, descending
    confidence) -> (boxes float32 [n, 4] in original pixels by label_boxes' arithmetic, clipped to the image; conf float32 [n]; cls int32 [n])."""
    path = os.path.join(labels_dir, Path(image_path).stem + ".txt")
    if not os.path.isfile(path):
        return np.zeros((0, 4), F32), np.zeros(0, F32), np.zeros(0, np.int32)
    with open(path) as f:
        rows = [x.split() for x in f.read().strip().splitlines() if len(x)]
    if any(len(r_) != 6 for r_ in rows):
        raise ValueError(f"{path}: a row without six columns (cls xc yc w h conf): write the files with --save-txt --save-conf")
    a = np.array(rows, dtype=F32).reshape(-1, 6)
    boxes = scale_boxes_geom(label_boxes(a[:, :5], h0, w0), np.array([0, 0, 1, w0, h0], F32))
    cls = np.zeros(a.shape[0], np.int32) if single_cls else a[:, 0].astype(np.int32)
    return boxes, a[:, 5].copy(), cls


def _sorted_order_numpy(cls: np.ndarray, conf: np.ndarray) -> np.ndarray:
    """(class ascending, confidence descending, index ascending): two stable sorts."""
    o = np.argsort(-conf, kind="stable")
    return o[np.argsort(cls[o], kind="stable")]


def score_cpu(conf: np.ndarray, cls: np.ndarray, bits: np.ndarray, label_counts: np.ndarray):
    """Sort + scores_numpy -> (classes, n_l, ap, p, r, pr)."""
    o = _sorted_order_numpy(cls, conf)
    classes, n_l, rr = _runs(np.bincount(cls, minlength=label_counts.shape[0])[:label_counts.shape[0]], label_counts)
    ap, p, r, pr = scores_numpy(bits[o], conf[o], rr, n_l)
    return classes, n_l, ap, p, r, pr


def score_gpu(conf, cls, bits, label_counts: np.ndarray, times: Optional[dict] = None):
    """The same on the device: torch's stable sorts (plumbing), then aq_val_scores_f64.  conf float32 / cls int32 / bits int16 CUDA [n]."""
    import torch
    from .engine import val_scores
    o = torch.sort(conf, descending=True, stable=True)[1]
    o = o[torch.sort(cls[o], stable=True)[1]]
    nc = label_counts.shape[0]
    per_class = torch.bincount(cls.to(torch.int64), minlength=nc)[:nc].cpu().numpy() if cls.numel() else np.zeros(nc, np.int64)
    classes, n_l, rr = _runs(per_class, label_counts)
    ap, p, r, pr = val_scores(bits[o].contiguous(), conf[o].contiguous(), rr, n_l, AP_X, PX, times=times)
    return classes, n_l, ap.cpu().numpy(), p.cpu().numpy(), r.cpu().numpy(), pr.cpu().numpy()


class _DeviceStats:
    """The run-long device arrays aq_val_match appends to."""

    def __init__(self, cap: int, dev):
        import torch
        self.conf = torch.empty(max(cap, 1), dtype=torch.float32, device=dev)
        self.cls = torch.empty(max(cap, 1), dtype=torch.int32, device=dev)
        self.bits = torch.empty(max(cap, 1), dtype=torch.int16, device=dev)
        self.total = torch.zeros(1, dtype=torch.int64, device=dev)
        self.iouv = IOUV.copy()

    def match(self, dets, counts, boxes: List[np.ndarray], classes: List[np.ndarray], geom: np.ndarray):
        """One batch: dets / counts CUDA as the NMS wrote them; the labels' pixel boxes and classes per image and the geometry table from
        the host, uploaded here.  -> the uploaded label arrays as _DeviceConfusion.add takes them."""
        import torch
        from .engine import val_match
        dev = dets.device
        start = np.zeros(len(boxes) + 1, np.int32)
        np.cumsum([b.shape[0] for b in boxes], out=start[1:])
        lbox = np.concatenate(boxes, 0).astype(F32).reshape(-1, 4) if boxes else np.zeros((0, 4), F32)
        lcls = np.concatenate(classes, 0).astype(np.int32).reshape(-1) if classes else np.zeros(0, np.int32)
        up = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a)).to(dev) if a.size else torch.empty(a.shape, dtype=dt, device=dev)
        lbox_d, lcls_d, start_d, geom_d = (up(lbox, torch.float32), up(lcls, torch.int32), torch.from_numpy(start).to(dev),
                                           up(np.ascontiguousarray(geom, dtype=F32), torch.float32))
        val_match(dets, counts, lbox_d, lcls_d, start_d, start, geom_d, self.iouv, self.conf, self.cls, self.bits, self.total)
        return lbox_d, lcls_d, lcls, start_d, start, geom_d

    def result(self):
        n = int(self.total.item())
        if n > self.conf.shape[0]:
            raise RuntimeError(f"val: {n} detections for arrays of {self.conf.shape[0]}")
        return self.conf[:n], self.cls[:n], self.bits[:n]


class _DeviceConfusion:
    """--confusion-matrix: the matrix aq_val_confusion adds every batch to, the per-image rows in split order and the class flag."""

    def __init__(self, nc: int, conf: float, iou: float, n_images: int, dev):
        import torch
        self.nc, self.conf_thres, self.iou_thres = nc, float(conf), float(iou)
        self.matrix = torch.zeros((nc + 1, nc + 1), dtype=torch.int64, device=dev)
        self.image = torch.zeros((n_images, 4), dtype=torch.int32, device=dev)
        self.flag = torch.zeros(1, dtype=torch.int32, device=dev)

    def add(self, dets, counts, uploaded, pos: Sequence[int]) -> None:
        """One batch, after _DeviceStats.match on the same dets / counts (uploaded = what it returned); pos = the images' places in the split."""
        import torch
        from .engine import val_confusion
        lbox_d, lcls_d, lcls, start_d, start, geom_d = uploaded
        rows = val_confusion(dets, counts, lbox_d, lcls_d, start_d, start, geom_d, self.nc, self.conf_thres, self.iou_thres, self.matrix,
                             label_cls_host=lcls, flag=self.flag)
        self.image[torch.as_tensor(list(pos), dtype=torch.int64, device=rows.device)] = rows

    def result(self) -> Tuple[np.ndarray, np.ndarray]:
        if int(self.flag.item()):
            raise RuntimeError(f"val: a detection class outside [0, {self.nc}) reached the confusion matrix")
        return self.matrix.cpu().numpy(), self.image.cpu().numpy()


def _label_counts(split: Split, nc: int) -> np.ndarray:
    if not split.labels or split.n_labels == 0:
        return np.zeros(nc, np.int64)
    return np.bincount(np.concatenate([lb[:, 0] for lb in split.labels]).astype(np.int64), minlength=nc)


def run_saved(opt, data: dict, split: Split, names, nc: int, save_dir: str, log=print) -> dict:
    """--labels DIR: score saved detections, on the GPU (aq_val_match, aq_val_scores_f64) or with --cpu in numpy."""
    sizes = _image_sizes(split.files, opt.workers)
    label_counts = _label_counts(split, nc)
    n_det = 0
    want_cm = bool(getattr(opt, "confusion_matrix", False))
    cm = None                                                                   # (matrix [nc + 1, nc + 1], image rows [images, 4]) with --confusion-matrix
    if opt.cpu:
        confs, clss, bitss = [], [], []
        if want_cm:
            cm = (np.zeros((nc + 1, nc + 1), np.int64), np.zeros((len(split.files), 4), np.int32))
        for k, (f, lb, (w0, h0)) in enumerate(zip(split.files, split.labels, sizes)):
            box, conf, cls = read_detections(opt.labels, f, w0, h0, opt.single_cls)
            confs.append(conf)
            clss.append(cls)
            bitss.append(match_numpy(label_boxes(lb, h0, w0), lb[:, 0], box, cls))
            if want_cm:
                delta, cm[1][k] = confusion_numpy(label_boxes(lb, h0, w0), lb[:, 0], box, conf, cls, nc, opt.confusion_conf, opt.confusion_iou)
                cm[0][...] += delta
        conf = np.concatenate(confs) if confs else np.zeros(0, F32)
        cls = np.concatenate(clss).astype(np.int32) if clss else np.zeros(0, np.int32)
        bits = np.concatenate(bitss) if bitss else np.zeros(0, np.uint16)
        n_det = int(conf.shape[0])
        classes, n_l, ap, p, r, pr = score_cpu(conf, cls, bits, label_counts)
        device = "cpu (numpy restatements)"
    else:
        import torch
        dev = torch.device("cuda", int(opt.device) if str(opt.device).strip().isdigit() else 0)
        torch.cuda.set_device(dev)
        per = [read_detections(opt.labels, f, w0, h0, opt.single_cls) for f, (w0, h0) in zip(split.files, sizes)]
        stats = _DeviceStats(sum(d[1].shape[0] for d in per), dev)
        confusion = _DeviceConfusion(nc, opt.confusion_conf, opt.confusion_iou, len(split.files), dev) if want_cm else None
        B = max(1, opt.batch_size)
        for s0 in range(0, len(per), B):
            part = per[s0:s0 + B]
            md = max(1, max(d[1].shape[0] for d in part))
            dets = np.zeros((len(part), md, 6), F32)
            for b, (box, conf, cls) in enumerate(part):
                k = conf.shape[0]
                dets[b, :k, :4], dets[b, :k, 4], dets[b, :k, 5] = box, conf, cls
            counts = np.array([d[1].shape[0] for d in part], np.int32)
            geom = np.array([[0, 0, 1, w0, h0] for (w0, h0) in sizes[s0:s0 + B]], F32)
            dets_d, counts_d = torch.from_numpy(dets).to(dev), torch.from_numpy(counts).to(dev)
            uploaded = stats.match(dets_d, counts_d, [label_boxes(lb, h0, w0) for lb, (w0, h0) in zip(split.labels[s0:s0 + B], sizes[s0:s0 + B])],
                                   [lb[:, 0] for lb in split.labels[s0:s0 + B]], geom)
            if confusion is not None:
                confusion.add(dets_d, counts_d, uploaded, range(s0, s0 + len(part)))
        conf, cls, bits = stats.result()
        if confusion is not None:
            cm = confusion.result()
        n_det = int(conf.shape[0])
        classes, n_l, ap, p, r, pr = score_gpu(conf, cls, bits, label_counts)
        device = torch.cuda.get_device_name(dev)
    meta = _meta(opt, data, split, n_det, device, precision=None)
    meta["detections_from"] = str(opt.labels)
    obj = write_confusion(save_dir, names, nc, split.files, cm[0], cm[1], opt.confusion_conf, opt.confusion_iou) if cm is not None else None
    return write_outputs(save_dir, names, nc, len(split.files), classes, n_l, ap, p, r, pr, meta, opt.verbose, opt.task, log, confusion=obj)


def _meta(opt, data: dict, split: Split, n_det: int, device: str, precision: Optional[str]) -> dict:
    return {"task": opt.task, "data": str(opt.data), "precision": precision, "imgsz": int(opt.imgsz), "conf_thres": float(opt.conf_thres),
            "iou_thres": float(opt.iou_thres), "max_det": int(opt.max_det), "single_cls": bool(opt.single_cls),
            "iouv": [float(t) for t in IOUV], "images": len(split.files), "skipped_images": len(split.skipped),
            "skipped": [str(f) for f in split.skipped], "labels": int(split.n_labels), "detections": int(n_det),
            "duplicate_label_rows_dropped": int(split.duplicates), "device": device}


def _batches(files: Sequence[str], sizes, batch_size: int, workers: int, jpeg_decode: str, imgsz, stride: int, dev, log):
    """detect.py's loading, by its own rules (dataloader.size_parts, dataloader.split_decodable): the images of the most common size first,
    the others by size, every size in batches; the decoded images go to the GPU as they are and the letterbox runs there.  One batch is
    in flight.  Yields (positions into files, tiles uint8 CUDA [b, H, W, 3], (h0, w0))."""
    import torch
    from .dataloader import LoadImages, size_parts, split_decodable
    from .engine import jpeg_slots_to_rgb, letterbox_device
    main, odd = size_parts(list(sizes))
    groups: Dict[Tuple[int, int], List[int]] = {}
    for i in main + odd:
        groups.setdefault(sizes[i], []).append(i)
    noted = False
    for (w0, h0), pos in groups.items():
        sub = LoadImages("", img_size=imgsz, stride=stride, auto=True, workers=workers, raw=True, files=[files[i] for i in pos])
        split = jpeg_decode != "host" and split_decodable(sub, jpeg_decode)
        if split and not noted:
            noted = True
            log(f"jpeg decode: split (entropy decoding in {sub.workers} worker processes, IDCT / upsampling / colour conversion on the GPU)")
        if split:
            gen = sub.pinned_batches(batch_size, 3, coef=True)
            n_ = 0
            scratch = None
            for paths, host, _, buf_i in gen:
                t = host.to(dev, non_blocking=True)
                torch.cuda.current_stream().synchronize()
                sub.release(buf_i)
                if scratch is None:
                    from .engine import load_library
                    scratch = torch.empty(load_library().aq_jpeg_scratch_bytes(batch_size, h0, w0), dtype=torch.uint8, device=dev)
                tiles0, flags = jpeg_slots_to_rgb(t, h0, w0, scratch=scratch)
                if flags is not None and bool((flags.cpu() != 0).any()):
                    bad = [paths[int(i)] for i in np.nonzero(flags.cpu().numpy())[0]]
                    raise ValueError(f"{bad[0]}: outside the split JPEG decoder's acceptance rule (use --jpeg-decode host)")
                yield pos[n_:n_ + len(paths)], letterbox_device(tiles0, tuple(imgsz), stride, True), (h0, w0)
                n_ += len(paths)
        else:
            n_ = 0
            for paths, arr, _ in sub.batches(batch_size):
                tiles0 = torch.from_numpy(arr).to(dev)
                yield pos[n_:n_ + len(paths)], letterbox_device(tiles0, tuple(imgsz), stride, True), (h0, w0)
                n_ += len(paths)


def run_sweep(opt, data: dict, split: Split, names, nc: int, save_dir: str, log=print) -> dict:
    """The engine over the split, upstream's NMS settings, aq_val_match per batch, the scores after the sweep."""
    import torch
    from .checkpoint import load_checkpoint
    from .dataloader import check_img_size
    from .engine import Engine, nms, val_expand_rows, write_label_files, VAL_NMS_ROWS
    weights = opt.weights[0] if isinstance(opt.weights, (list, tuple)) else opt.weights
    precision = opt.precision or ("bf16" if opt.half else "fp32")
    dev_i = int(opt.device) if str(opt.device).strip().isdigit() else 0
    torch.cuda.set_device(dev_i)
    dev = torch.device("cuda", dev_i)
    ck = load_checkpoint(weights)
    if not opt.single_cls and ck.nc != nc:
        raise SystemExit(f"{weights} has {ck.nc} classes, {opt.data} has {nc}: pass --single-cls or the dataset the weights were trained on")
    stride = int(max(ck.stride))
    s_ = check_img_size(int(opt.imgsz), s=stride)
    imgsz = [s_, s_]
    eng = Engine(ck, precision, dev_i, fp8_calibration="defer")
    try:
        eng.workspace_bytes(opt.batch_size, *imgsz)
    except RuntimeError as err:
        raise SystemExit(f"--batch-size {opt.batch_size}: {err}") from None
    sizes = _image_sizes(split.files, opt.workers)
    if precision == "fp8" and split.files:
        from .dataloader import read_rgb
        from .engine import letterbox_device
        picks = [read_rgb(f) for f in split.files[:: max(1, len(split.files) // 16)][:16]]
        picks = [p_ for p_ in picks if p_.shape == picks[0].shape]
        scales = eng.calibrate_fp8(letterbox_device(torch.from_numpy(np.stack(picks)).to(dev), tuple(imgsz), stride, True))
        log(f"fp8: {len(scales)} activation scales calibrated on {len(picks)} images of this split")
    labels_dir = os.path.join(save_dir, "labels")
    os.makedirs(labels_dir if opt.save_txt else save_dir, exist_ok=True)
    multi_label = ck.nc > 1 and not opt.single_cls                              # [UPSTREAM non_max_suppression] multi_label &= nc > 1
    stats = _DeviceStats(len(split.files) * opt.max_det, dev)
    confusion = (_DeviceConfusion(nc, opt.confusion_conf, opt.confusion_iou, len(split.files), dev)
                 if getattr(opt, "confusion_matrix", False) else None)
    no = ck.nc + 5
    n_files = 0
    n_plots = int(getattr(opt, "plots", 0) or 0)
    plots: List[dict] = []
    t0 = time.perf_counter()
    t_first = None
    for pos, tiles, (h0, w0) in _batches(split.files, sizes, opt.batch_size, opt.workers, opt.jpeg_decode, imgsz, stride, dev, log):
        B, H, W = int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[2])
        pred = eng.forward_raw(tiles)
        N = int(pred.shape[1])
        if multi_label:
            M = min(N * ck.nc, VAL_NMS_ROWS)
            step = max(1, ROWS_BUDGET // (M * no * 4))
            parts = []
            for a in range(0, B, step):
                rows, emitted = val_expand_rows(pred[a:a + step].contiguous(), opt.conf_thres, M)
                # an image can emit more than M rows only when M < N nc: at 640 px and 5 classes it cannot, and the counts stay on the device
                over = (emitted.cpu().numpy() > M).nonzero()[0] if M < N * ck.nc else np.zeros(0, np.int64)
                if over.size:
                    raise SystemExit(f"{split.files[pos[a + int(over[0])]]}: {int(emitted[int(over[0])])} candidate rows after the multi-label "
                                     f"expansion, the NMS takes {M} per image: raise --conf-thres")
                parts.append(nms(rows, ck.nc, opt.conf_thres, opt.iou_thres, opt.max_det))
            dets = torch.cat([p_[0] for p_ in parts], 0) if len(parts) > 1 else parts[0][0]
            counts = torch.cat([p_[1] for p_ in parts], 0) if len(parts) > 1 else parts[0][1]
        else:
            dets, counts = nms(pred, ck.nc, opt.conf_thres, opt.iou_thres, opt.max_det, agnostic=opt.single_cls)
        if opt.single_cls:
            dets[:, :, 5] = 0
        geom = np.tile(letterbox_geom((H, W), (h0, w0)), (B, 1))
        lbs = [split.labels[i] for i in pos]
        uploaded = stats.match(dets, counts, [label_boxes(lb, h0, w0) for lb in lbs], [lb[:, 0] for lb in lbs], geom)
        if confusion is not None:                                               # the same dets / counts, where the NMS left them
            confusion.add(dets, counts, uploaded, pos)
        if opt.save_txt:
            n_files += _save_txt(labels_dir, [split.files[i] for i in pos], dets.cpu().numpy(), counts.cpu().numpy(), geom[0], opt.save_conf,
                                 write_label_files)
        if len(plots) < n_plots:                                                # [UPSTREAM val.py] if plots and batch_i < 3
            from . import val_plots
            k = len(plots)
            fnames = (f"val_batch{k}_labels.jpg", f"val_batch{k}_pred.jpg")
            ltg, ptg = val_plots.batch_targets(dets[:val_plots.MAX_SUBPLOTS].cpu().numpy(), counts[:val_plots.MAX_SUBPLOTS].cpu().numpy(), lbs,
                                               (h0, w0), (H, W), stride)
            g = val_plots.plot_batch(tiles, [split.files[i] for i in pos], ltg, ptg, names, save_dir, fnames)
            plots.append({"labels": fnames[0], "pred": fnames[1], "images": g["n"], "height": g["size"][0], "width": g["size"][1]})
            if len(plots) == n_plots:
                val_plots.release_buffers()                                     # canvases and arenas: not held for the rest of the sweep
        if t_first is None:
            torch.cuda.synchronize()
            t_first = time.perf_counter()
        if not opt.quiet:
            log(f"val: {pos[-1] + 1 if len(pos) else 0}/{len(split.files)} images ({B} of {w0}x{h0} -> {W}x{H})")
    conf, cls, bits = stats.result()
    torch.cuda.synchronize()
    t1 = time.perf_counter()
    times: dict = {}
    classes, n_l, ap, p, r, pr = score_gpu(conf, cls, bits, _label_counts(split, nc), times=times)
    n_img = len(split.files)
    log(f"Speed: {n_img} images in {t1 - t0:.2f}s ({n_img / max(t1 - t0, 1e-9):.1f} images/s end to end, first batch {(t_first or t1) - t0:.2f}s), "
        f"scores of {int(conf.shape[0])} detections in {times.get('scores_ms', 0.0):.2f} ms on the GPU, {precision} at {imgsz[0]}")
    meta = _meta(opt, data, split, int(conf.shape[0]), torch.cuda.get_device_name(dev), precision)
    meta["weights"] = str(weights)
    meta["images_per_s"] = n_img / max(t1 - t0, 1e-9)
    if n_plots:
        meta["plots"] = {"batches": plots, "max_size": 1920, "jpeg_quality": 75}
    obj = None
    if confusion is not None:
        matrix, image = confusion.result()
        obj = write_confusion(save_dir, names, nc, split.files, matrix, image, opt.confusion_conf, opt.confusion_iou)
    s = write_outputs(save_dir, names, nc, n_img, classes, n_l, ap, p, r, pr, meta, opt.verbose, opt.task, log, confusion=obj)
    if opt.save_txt:
        log(f"{n_files} labels saved to {labels_dir}")
    if plots:
        from . import val_plots
        val_plots.release_buffers()                                             # (a split of fewer than N batches)
        log(f"{2 * len(plots)} mosaics saved to {save_dir}")
    log(f"Results saved to {save_dir}")
    eng.close()
    return s


def _save_txt(labels_dir: str, paths, dets: np.ndarray, counts: np.ndarray, geom: np.ndarray, save_conf: bool, writer) -> int:
    """[UPSTREAM save_one_txt]: per detection in the NMS's order ``cls, *xyxy2xywh(box) / (w0, h0, w0, h0), conf``: unrounded boxes."""
    counts = np.minimum(np.maximum(counts.astype(np.int64), 0), dets.shape[1])
    offsets = np.zeros(len(paths) + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    valid = np.arange(dets.shape[1])[None, :] < counts[:, None]
    det = dets[valid]
    b = scale_boxes_geom(det[:, :4], geom)
    rows = np.empty((det.shape[0], 6), F32)
    rows[:, 0] = det[:, 5]
    rows[:, 1] = ((b[:, 0] + b[:, 2]) / F32(2)) / geom[3]
    rows[:, 2] = ((b[:, 1] + b[:, 3]) / F32(2)) / geom[4]
    rows[:, 3] = (b[:, 2] - b[:, 0]) / geom[3]
    rows[:, 4] = (b[:, 3] - b[:, 1]) / geom[4]
    rows[:, 5] = det[:, 4]
    return writer(labels_dir, [Path(p_).stem for p_ in paths], rows, offsets, save_conf=save_conf)


def run(opt: argparse.Namespace, log=print) -> dict:
    from .detect import increment_path
    check_opt(opt)
    data = load_data_yaml(opt.data)
    if data.get(opt.task) is None:
        raise SystemExit(f"{opt.data}: no '{opt.task}' entry for --task {opt.task}")
    files = list_split_images(data[opt.task])
    nc = 1 if opt.single_cls else data["nc"]
    names = data["names"]
    split = Split(files, opt.single_cls, log)
    _check_classes(split, nc)
    if split.duplicates:
        log(f"{split.duplicates} duplicate label rows dropped (np.unique(axis=0), as upstream)")
    if split.skipped:
        log(f"{len(split.skipped)} images skipped for corrupt label files")
    save_dir = str(increment_path(Path(opt.project) / opt.name, exist_ok=opt.exist_ok))
    if opt.labels:
        return run_saved(opt, data, split, names, nc, save_dir, log)
    return run_sweep(opt, data, split, names, nc, save_dir, log)


def main(argv: Optional[List[str]] = None) -> int:
    run(parse_opt(argv))
    return 0


if __name__ == "__main__":
    sys.exit(main())
