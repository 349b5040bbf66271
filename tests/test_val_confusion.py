"""yolov5/val.py --confusion-matrix on the host: val.confusion_numpy (the closed rule aq_val_confusion implements) against upstream's
ConfusionMatrix.process_batch restated line by line (torch's box_iou, numpy's unique, argsort(kind="stable")), the fixed cases with their
matrices written out, tp_fp and the normalisation, the files of the --cpu run and the ABI surface.  The inputs are shared with
tests/test_gpu_val_confusion.py.  All results are integers: every comparison is exact."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from test_val import _grid_boxes, _png, box_iou_literal

from aquaculture_amd import val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ("aq_val_confusion_scratch_bytes", "aq_val_confusion")
CONFS = np.array([0.1, 0.25, 0.3, 0.6, 0.9], F32)                              # exactly 0.25: does not take part
VAL_JSON_KEYS = {"task", "data", "precision", "imgsz", "conf_thres", "iou_thres", "max_det", "single_cls", "iouv", "images", "skipped_images",
                 "skipped", "labels", "detections", "duplicate_label_rows_dropped", "device", "detections_from", "results", "departures"}


# ---- upstream, literally ----

def confusion_literal(lbox, lcls, dbox, dconf, dcls, nc, conf=0.25, iou_thres=0.45) -> np.ndarray:
    """[UPSTREAM utils/metrics.py ConfusionMatrix.process_batch] as [UPSTREAM val.py] calls it for one image: only when the image has
    labels, with detections=None when the NMS returned none -> what the image adds to matrix[predicted][true]."""
    matrix = np.zeros((nc + 1, nc + 1), np.int64)
    if lcls.shape[0] == 0:                                                      # val.py: `if nl:` around the call
        return matrix
    labels = torch.from_numpy(np.concatenate([np.asarray(lcls, F32)[:, None], np.asarray(lbox, F32)], 1))
    if dcls.shape[0] == 0:                                                      # detections is None
        for gc in labels[:, 0].int():
            matrix[nc, gc] += 1
        return matrix
    detections = torch.from_numpy(np.concatenate([np.asarray(dbox, F32), np.asarray(dconf, F32)[:, None], np.asarray(dcls, F32)[:, None]], 1))
    detections = detections[detections[:, 4] > conf]
    gt_classes = labels[:, 0].int()
    detection_classes = detections[:, 5].int()
    iou = box_iou_literal(labels[:, 1:], detections[:, :4])
    x = torch.where(iou > iou_thres)
    if x[0].shape[0]:
        matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
        if x[0].shape[0] > 1:
            matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
            matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
            matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
            matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
    else:
        matches = np.zeros((0, 3))
    n = matches.shape[0] > 0
    m0, m1, _ = matches.transpose().astype(int)
    for i, gc in enumerate(gt_classes):
        j = m0 == i
        if n and sum(j) == 1:
            matrix[detection_classes[m1[j]], gc] += 1
        else:
            matrix[nc, gc] += 1
    if n:
        for i, dc in enumerate(detection_classes):
            if not any(m1 == i):
                matrix[dc, nc] += 1
    return matrix


def tp_fp_literal(matrix):
    """[UPSTREAM ConfusionMatrix.tp_fp]"""
    tp = matrix.diagonal()
    fp = matrix.sum(1) - tp
    return tp[:-1], fp[:-1]


# ---- the cases (shared with the GPU test): (lbox, lcls, dbox, dconf, dcls, nc) ----

def _case(labels, dets, nc):
    lb = np.array(labels, F32).reshape(-1, 5)
    dt = np.array(dets, F32).reshape(-1, 6)
    return lb[:, 1:].copy(), lb[:, 0].astype(np.int32), dt[:, :4].copy(), dt[:, 4].copy(), dt[:, 5].astype(np.int32), nc


# name: (case, the matrix the image adds, its image row); labels as (cls, x1, y1, x2, y2), detections as (x1, y1, x2, y2, conf, cls)
FIXED = {
    "no NMS detections": (_case([(0, 0, 0, 8, 8), (1, 8, 8, 16, 16)], [], 2), [[0, 0, 0], [0, 0, 0], [1, 1, 0]], [2, 0, 0, 0]),
    "all detections below conf": (_case([(0, 0, 0, 8, 8), (1, 8, 8, 16, 16)], [(0, 0, 8, 8, 0.25, 0), (8, 8, 16, 16, 0.1, 1)], 2),
                                  [[0, 0, 0], [0, 0, 0], [1, 1, 0]], [2, 0, 0, 0]),
    # labels go to background, the detections add nothing: upstream's `if n:`
    "no pair above the iou": (_case([(0, 0, 0, 8, 8)], [(8, 8, 16, 16, 0.9, 1), (0, 0, 8, 2, 0.8, 0)], 2), [[0, 0, 0], [0, 0, 0], [1, 0, 0]], [1, 2, 0, 0]),
    "one pair": (_case([(1, 0, 0, 8, 8)], [(0, 0, 8, 8, 0.9, 1)], 2), [[0, 0, 0], [0, 1, 0], [0, 0, 0]], [1, 1, 1, 1]),
    "one pair of different classes": (_case([(1, 0, 0, 8, 8)], [(0, 0, 8, 8, 0.9, 0)], 2), [[0, 1, 0], [0, 0, 0], [0, 0, 0]], [1, 1, 1, 0]),
    # detections 0 (IoU 1) and 1 (IoU 0.8) both have label 0 as their best: the loser is background
    "two detections, one best label": (_case([(0, 0, 0, 10, 10)], [(0, 0, 10, 10, 0.9, 0), (0, 0, 10, 8, 0.8, 1)], 2),
                                       [[1, 0, 0], [0, 0, 1], [0, 0, 0]], [1, 2, 1, 1]),
    # detection 1 prefers label 0 (0.8) to label 1 (0.75) and loses it to detection 0: label 1 is missed, no fall-back
    "no fall-back": (_case([(0, 0, 0, 10, 10), (1, 0, 0, 10, 6)], [(0, 0, 10, 10, 0.9, 0), (0, 0, 10, 8, 0.8, 0)], 2),
                     [[1, 0, 1], [0, 0, 0], [0, 1, 0]], [2, 2, 1, 1]),
    "detections and no labels": (_case([], [(0, 0, 8, 8, 0.9, 0), (8, 8, 16, 16, 0.8, 1)], 2), [[0, 0, 0], [0, 0, 0], [0, 0, 0]], [0, 2, 0, 0]),
    # --single-cls: 2 x 2, every class 0: one kept pair, one missed label, one detection on background
    "single class": (_case([(0, 0, 0, 8, 8), (0, 16, 16, 24, 24)], [(0, 0, 8, 8, 0.9, 0), (32, 32, 40, 40, 0.8, 0)], 1), [[1, 1], [1, 0]], [2, 2, 1, 1]),
    # IoU exactly fp32 0.45 = 576 / 1280: does not pair (strict)
    "iou exactly 0.45": (_case([(0, 0, 0, 72, 16)], [(0, 0, 88, 8, 0.9, 0)], 1), [[0, 0], [1, 0]], [1, 1, 0, 0]),
    # one detection at equal IoU to labels 0 and 1: the higher label index takes it; two detections at equal IoU to label 2: the higher detection index stays
    "equal ious": (_case([(0, 0, 0, 8, 8), (1, 0, 0, 8, 8), (0, 32, 32, 40, 40)],
                         [(0, 0, 8, 8, 0.9, 0), (32, 32, 40, 38, 0.8, 0), (32, 34, 40, 40, 0.7, 1)], 2),
                   [[0, 1, 1], [1, 0, 0], [1, 0, 0]], [3, 3, 2, 0]),
}


@functools.lru_cache(maxsize=None)
def random_cases():
    """200 images: 0-40 labels, 0-300 detections, 1-5 classes, boxes on a coarse grid, confidences from CONFS in descending order; every
    fifth image also holds a label and a detection at IoU exactly fp32 0.45.  Shared, treat as read-only."""
    rng = np.random.default_rng(20261)
    out = []
    for k in range(200):
        nc = int(rng.integers(1, 6))
        L = 0 if k % 23 == 0 else int(rng.integers(0, 41))
        D = 0 if k % 29 == 0 else int(rng.integers(0, 301))
        if k == 7:
            L, D = 40, 300
        cells = 4 if k % 3 == 0 else 8                                          # crowded images: many equal IoUs
        lbox, dbox = _grid_boxes(rng, L, cells), _grid_boxes(rng, D, cells)
        if k % 5 == 0 and L and D:
            off = np.array([128, 128, 128, 128], F32) * F32(1 + k % 3)          # away from the grid's boxes
            lbox[int(rng.integers(0, L))] = np.array([0, 0, 72, 16], F32) + off
            dbox[int(rng.integers(0, D))] = np.array([0, 0, 88, 8], F32) + off
        dconf = np.sort(CONFS[rng.integers(0, CONFS.shape[0], D)])[::-1].copy()
        out.append((lbox, rng.integers(0, nc, L).astype(np.int32), dbox, dconf, rng.integers(0, nc, D).astype(np.int32), nc))
    return out


# ---- the rule ----

def test_closed_rule_equals_the_literal_listing():
    two_labels = two_dets = on_iou = on_conf = 0
    thr = F32(val.CONFUSION_IOU)
    for lbox, lcls, dbox, dconf, dcls, nc in random_cases():
        want = confusion_literal(lbox, lcls, dbox, dconf, dcls, nc)
        got, row = val.confusion_numpy(lbox, lcls, dbox, dconf, dcls, nc)
        assert got.dtype == np.int64 and got.shape == (nc + 1, nc + 1) and np.array_equal(got, want)
        take = dconf > F32(0.25)
        assert row.tolist()[:2] == [lcls.shape[0], int(take.sum())]
        if lcls.shape[0]:
            assert row[2] == got[:nc, :nc].sum() and row[3] == np.trace(got[:nc, :nc]) and got[nc, :nc].sum() == row[0] - row[2]
            assert got[:nc, nc].sum() == (row[1] - row[2] if row[2] else 0)
        on_conf += int((dconf == F32(0.25)).sum())
        if lcls.shape[0] and take.any():
            iou = val.box_iou_numpy(lbox, dbox[take])
            on_iou += int((iou == thr).sum())
            top = np.where(iou > thr, iou, F32(-1)).max(0)
            two_labels += int(((iou == top[None, :]).sum(0)[top > 0] > 1).sum())
            best = iou.shape[0] - 1 - np.argmax(np.where(iou > thr, iou, F32(-1))[::-1], axis=0)
            for l in np.unique(best[top > 0]):
                mine = top[(best == l) & (top > 0)]
                two_dets += int((mine == mine.max()).sum() > 1)
    assert two_labels > 0 and two_dets > 0 and on_iou > 0 and on_conf > 0, (two_labels, two_dets, on_iou, on_conf)


@pytest.mark.parametrize("name", sorted(FIXED))
def test_fixed_cases(name):
    case, matrix, row = FIXED[name]
    got, got_row = val.confusion_numpy(*case)
    assert got.tolist() == matrix and got_row.tolist() == row
    assert confusion_literal(*case).tolist() == matrix


def test_the_fixed_cases_are_what_their_names_say():
    lbox, _, dbox, _, _, _ = FIXED["iou exactly 0.45"][0]
    assert val.box_iou_numpy(lbox, dbox)[0, 0] == F32(0.45)
    lbox, _, dbox, _, _, _ = FIXED["no fall-back"][0]
    iou = val.box_iou_numpy(lbox, dbox)
    assert iou[0, 1] > iou[1, 1] > F32(0.45) and iou[0, 0] > iou[0, 1]
    lbox, _, dbox, _, _, _ = FIXED["equal ious"][0]
    iou = val.box_iou_numpy(lbox, dbox)
    assert iou[0, 0] == iou[1, 0] > F32(0.45) and iou[2, 1] == iou[2, 2] > F32(0.45)
    with pytest.raises(ValueError, match="outside"):
        val.confusion_numpy(*FIXED["one pair"][0][:5], 1)


def test_tp_fp_and_the_normalisation():
    total = np.zeros((6, 6), np.int64)
    for c in random_cases():
        if c[5] == 5:
            total += val.confusion_numpy(*c)[0]
    assert total[:5, :5].sum() > 100 and total[5, :5].sum() > 100 and total[:5, 5].sum() > 100 and total[5, 5] == 0
    tp, fp = val.confusion_tp_fp(total)
    want_tp, want_fp = tp_fp_literal(total)
    assert np.array_equal(tp, want_tp) and np.array_equal(fp, want_fp) and tp.shape == (5,)
    assert val.confusion_normalised(total).tobytes() == (total / (total.sum(0).reshape(1, -1) + 1E-9)).tobytes()     # [UPSTREAM ConfusionMatrix.plot]
    assert val.confusion_normalised(np.zeros((2, 2), np.int64)).tolist() == [[0, 0], [0, 0]]


# ---- the files ----

def _split(tmp_path):
    for k in ("a", "b", "c"):
        _png(str(tmp_path / "images" / f"{k}.png"), 100, 50)
    os.makedirs(tmp_path / "labels")
    os.makedirs(tmp_path / "dets")
    (tmp_path / "labels" / "a.txt").write_text("0 0.5 0.5 0.2 0.4\n1 0.25 0.25 0.1 0.2\n")
    (tmp_path / "labels" / "b.txt").write_text("1 0.5 0.5 0.5 0.5\n")
    # a: the circle found; a circle on the square label; a square on nothing (background, conf 0.3); one below the confidence.  b: nothing.
    (tmp_path / "dets" / "a.txt").write_text("0 0.5 0.5 0.2 0.4 0.9\n0 0.25 0.25 0.1 0.2 0.8\n1 0.8 0.8 0.1 0.1 0.3\n0 0.1 0.8 0.1 0.1 0.2\n")
    (tmp_path / "dets" / "c.txt").write_text("1 0.5 0.5 0.2 0.2 0.6\n")            # an image without labels: adds nothing
    (tmp_path / "d.yaml").write_text("val: images\nnames: [circle, square]\n")
    return ["--data", str(tmp_path / "d.yaml"), "--labels", str(tmp_path / "dets"), "--cpu", "--project", str(tmp_path / "runs")]


def test_cpu_run_writes_the_confusion_files(tmp_path, capsys):
    args = _split(tmp_path)
    assert val.main(args + ["--confusion-matrix"]) == 0
    run = tmp_path / "runs" / "exp"
    assert sorted(os.listdir(run)) == ["val.json", "val_classes.csv", "val_confusion.csv", "val_confusion_norm.csv", "val_curves.csv", "val_images.csv"]
    assert (run / "val_confusion.csv").read_text() == "predicted,circle,square,background\ncircle,1,1,0\nsquare,0,0,1\nbackground,0,1,0\n"
    one, half = repr(1 / (1 + 1e-9)), repr(1 / (2 + 1e-9))
    assert (run / "val_confusion_norm.csv").read_text() == ("predicted,circle,square,background\n"
                                                            f"circle,{one},{half},0.0\nsquare,0.0,0.0,{one}\nbackground,0.0,{half},0.0\n")
    img = lambda k: str((tmp_path / "images" / f"{k}.png").resolve())
    assert (run / "val_images.csv").read_text() == ("image,labels,detections,matched,matched_same_class,missed,false\n"
                                                    f"{img('a')},2,3,2,1,0,1\n{img('b')},1,0,0,0,1,0\n{img('c')},0,1,0,0,0,0\n")
    meta = json.loads((run / "val.json").read_text())
    assert set(meta) == VAL_JSON_KEYS | {"confusion"}
    cm = meta["confusion"]
    assert (cm["conf"], cm["iou"], cm["tp"], cm["fp"], cm["matrix"]) == (0.25, 0.45, [1, 0], [1, 1], [[1, 1, 0], [0, 0, 1], [0, 1, 0]])
    assert cm["notes"] == [val.CONFUSION_TIE_NOTE, val.CONFUSION_QUIRK_NOTE] and "higher index" in cm["notes"][0] and "without labels" in cm["notes"][1]
    assert meta["departures"] == list(val.DEPARTURES) + [val.CONFUSION_TIE_NOTE]
    # the thresholds are flags
    assert val.main(args + ["--confusion-matrix", "--confusion-conf", "0.3", "--confusion-iou", "0.999"]) == 0
    cm = json.loads((tmp_path / "runs" / "exp2" / "val.json").read_text())["confusion"]
    assert (cm["conf"], cm["iou"], cm["matrix"]) == (0.3, 0.999, [[1, 1, 0], [0, 0, 0], [0, 1, 0]])


def test_without_the_flag_nothing_changes(tmp_path, capsys):
    args = _split(tmp_path)
    assert val.main(args) == 0 and val.main(args + ["--confusion-matrix"]) == 0
    plain, flagged = tmp_path / "runs" / "exp", tmp_path / "runs" / "exp2"
    assert sorted(os.listdir(plain)) == ["val.json", "val_classes.csv", "val_curves.csv"]
    meta = json.loads((plain / "val.json").read_text())
    assert set(meta) == VAL_JSON_KEYS and meta["departures"] == list(val.DEPARTURES)
    for f in ("val_classes.csv", "val_curves.csv"):
        assert (plain / f).read_text() == (flagged / f).read_text()
    with_flag = json.loads((flagged / "val.json").read_text())
    del with_flag["confusion"]
    with_flag["departures"].pop()
    assert with_flag == meta
    opt = val.parse_opt(args)
    assert (opt.confusion_matrix, opt.confusion_conf, opt.confusion_iou) == (False, 0.25, 0.45)
    for extra in (["--confusion-iou", "0"], ["--confusion-iou", "nan"], ["--confusion-conf", "inf"]):
        with pytest.raises(SystemExit, match="--confusion-iou above 0"):
            val.check_opt(val.parse_opt(args + ["--confusion-matrix"] + extra))


# ---- the ABI surface ----

def test_exports_header_and_bindings(lib):
    from aquaculture_amd import build, engine
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aq_engine.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert ("val.hip", ["-ffp-contract=off"]) in build.SOURCES and lib.aq_version() == 8
    assert lib.aq_val_confusion_scratch_bytes(32, 300, 640) == 640 * 8 + 32 * 300 * 4
    assert lib.aq_val_confusion_scratch_bytes(3, 5, 7) == 7 * 8 + 64                       # 60 bytes of best labels, rounded up to 8
    assert lib.aq_val_confusion_scratch_bytes(1, 0, 0) == 0 and callable(engine.val_confusion)
