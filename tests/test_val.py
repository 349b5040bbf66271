"""yolov5/val.py on the host: the numpy restatements of the three kernels (val.match_numpy, val.scores_numpy, val.interp_numpy,
val.expand_rows_numpy) against upstream's procedures restated literally (process_batch with torch's box_iou and numpy's three lines,
ap_per_class on np.interp / np.trapezoid / np.maximum.accumulate / np.convolve); the label path rule, the yaml forms, corrupt and duplicate
label rows, the refusals, the table's format, the --cpu run and the ABI surface.  The inputs are shared with tests/test_gpu_val.py."""
import functools
import json
import os
import re

import numpy as np
import pytest
import torch

from aquaculture_amd import val

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NEW_SYMBOLS = ("aq_val_expand_scratch_bytes", "aq_val_expand_rows_f32", "aq_val_match", "aq_val_score_chunk", "aq_val_scores_scratch_bytes",
               "aq_val_scores_f64")


# ---- upstream, literally ----

def box_iou_literal(box1: torch.Tensor, box2: torch.Tensor, eps=1e-7) -> torch.Tensor:
    """[UPSTREAM utils/metrics.py box_iou]"""
    (a1, a2), (b1, b2) = box1.unsqueeze(1).chunk(2, 2), box2.unsqueeze(0).chunk(2, 2)
    inter = (torch.min(a2, b2) - torch.max(a1, b1)).clamp(0).prod(2)
    return inter / ((a2 - a1).prod(2) + (b2 - b1).prod(2) - inter + eps)


def process_batch_literal(lbox, lcls, dbox, dcls, iouv=val.IOUV) -> np.ndarray:
    """[UPSTREAM val.py process_batch] with argsort(kind="stable") -> bool [D, 10]."""
    D = dcls.shape[0]
    correct = np.zeros((D, 10), bool)
    if lcls.shape[0] == 0 or D == 0:
        return correct
    labels = torch.from_numpy(np.concatenate([np.asarray(lcls, F32)[:, None], np.asarray(lbox, F32)], 1))
    detections = torch.from_numpy(np.concatenate([np.asarray(dbox, F32), np.zeros((D, 1), F32), np.asarray(dcls, F32)[:, None]], 1))
    iou = box_iou_literal(labels[:, 1:], detections[:, :4])
    correct_class = labels[:, 0:1] == detections[:, 5]
    iouv = torch.from_numpy(np.asarray(iouv, F32))
    for i in range(10):
        x = torch.where((iou >= iouv[i]) & correct_class)
        if x[0].shape[0]:
            matches = torch.cat((torch.stack(x, 1), iou[x[0], x[1]][:, None]), 1).cpu().numpy()
            if x[0].shape[0] > 1:
                matches = matches[matches[:, 2].argsort(kind="stable")[::-1]]
                matches = matches[np.unique(matches[:, 1], return_index=True)[1]]
                matches = matches[np.unique(matches[:, 0], return_index=True)[1]]
            correct[matches[:, 1].astype(int), i] = True
    return correct


def compute_ap_literal(recall, precision):
    """[UPSTREAM utils/metrics.py compute_ap], method 'interp'."""
    mrec = np.concatenate(([0.0], recall, [1.0]))
    mpre = np.concatenate(([1.0], precision, [0.0]))
    mpre = np.flip(np.maximum.accumulate(np.flip(mpre)))
    x = np.linspace(0, 1, 101)
    return np.trapezoid(np.interp(x, mrec, mpre), x), mpre, mrec


def smooth_literal(y, f=0.05):
    nf = round(len(y) * f * 2) // 2 + 1
    p = np.ones(nf // 2)
    yp = np.concatenate((p * y[0], y, p * y[-1]), 0)
    return np.convolve(yp, np.ones(nf) / nf, mode="valid")


def ap_per_class_literal(tp, conf, pred_cls, target_cls, eps=1e-16):
    """[UPSTREAM utils/metrics.py ap_per_class] (the sort stable) -> (tp, fp, p, r, f1, ap, classes, p_curve, r_curve, py)."""
    i = np.argsort(-conf, kind="stable")
    tp, conf, pred_cls = tp[i], conf[i], pred_cls[i]
    unique_classes, nt = np.unique(target_cls, return_counts=True)
    nc = unique_classes.shape[0]
    px, py = np.linspace(0, 1, 1000), np.zeros((nc, 1000))
    ap, p, r = np.zeros((nc, tp.shape[1])), np.zeros((nc, 1000)), np.zeros((nc, 1000))
    for ci, c in enumerate(unique_classes):
        i = pred_cls == c
        n_l = nt[ci]
        n_p = i.sum()
        if n_p == 0 or n_l == 0:
            continue
        fpc = (1 - tp[i]).cumsum(0)
        tpc = tp[i].cumsum(0)
        recall = tpc / (n_l + eps)
        r[ci] = np.interp(-px, -conf[i], recall[:, 0], left=0)
        precision = tpc / (tpc + fpc)
        p[ci] = np.interp(-px, -conf[i], precision[:, 0], left=1)
        for j in range(tp.shape[1]):
            ap[ci, j], mpre, mrec = compute_ap_literal(recall[:, j], precision[:, j])
            if j == 0:
                py[ci] = np.interp(px, mrec, mpre)
    f1 = 2 * p * r / (p + r + eps)
    i = smooth_literal(f1.mean(0), 0.1).argmax()
    pc, rc = p, r
    p, r, f1 = p[:, i], r[:, i], f1[:, i]
    tp = (r * nt).round()
    fp = (tp / (p + eps) - tp).round()
    return tp, fp, p, r, f1, ap, unique_classes.astype(int), pc, rc, py


# ---- the matching cases (shared with the GPU test) ----

def _grid_boxes(rng, n, cells=8, step=8.0):
    x1 = rng.integers(0, cells, n)
    y1 = rng.integers(0, cells, n)
    w = rng.integers(1, 5, n)
    h = rng.integers(1, 5, n)
    return (np.stack([x1, y1, x1 + w, y1 + h], 1) * step).astype(F32)


FIXED_MATCH = {
    "no labels": (np.zeros((0, 4), F32), np.zeros(0, np.int32), np.array([[0, 0, 8, 8], [8, 8, 16, 16]], F32), np.array([0, 1], np.int32)),
    "no detections": (np.array([[0, 0, 8, 8]], F32), np.array([0], np.int32), np.zeros((0, 4), F32), np.zeros(0, np.int32)),
    "neither": (np.zeros((0, 4), F32), np.zeros(0, np.int32), np.zeros((0, 4), F32), np.zeros(0, np.int32)),
    "class mismatch only": (np.array([[0, 0, 8, 8], [8, 8, 16, 16]], F32), np.array([0, 1], np.int32),
                            np.array([[0, 0, 8, 8], [8, 8, 16, 16]], F32), np.array([1, 0], np.int32)),
    "iou exactly 0.5": (np.array([[0, 0, 2, 1]], F32), np.array([0], np.int32), np.array([[0, 0, 1, 1]], F32), np.array([0], np.int32)),
    # detections 0 and 1 both have label 0 as their best (IoU 1 and 0.8); label 1 overlaps detection 1 above 0.5 (IoU 0.6): no fall-back
    "shared best label": (np.array([[0, 0, 10, 10], [0, 0, 10, 6]], F32), np.array([0, 0], np.int32),
                          np.array([[0, 0, 10, 10], [0, 0, 10, 8]], F32), np.array([0, 0], np.int32)),
    "equal iou to two labels": (np.array([[0, 0, 8, 8], [8, 0, 16, 8], [0, 0, 8, 8]], F32), np.array([0, 0, 1], np.int32),
                                np.array([[4, 0, 12, 8]], F32), np.array([0], np.int32)),
}


@functools.lru_cache(maxsize=None)
def random_match_cases():
    """200 images: 0-40 labels, 0-300 detections, 1-5 classes, boxes on a coarse grid; shared, treat as read-only."""
    rng = np.random.default_rng(20260)
    out = []
    for k in range(200):
        nc = int(rng.integers(1, 6))
        L = 0 if k % 23 == 0 else int(rng.integers(0, 41))
        D = 0 if k % 29 == 0 else int(rng.integers(0, 301))
        if k == 7:
            L, D = 40, 300
        cells = 4 if k % 3 == 0 else 8                                          # crowded images: many equal IoUs
        out.append((_grid_boxes(rng, L, cells), rng.integers(0, nc, L).astype(np.int32), _grid_boxes(rng, D, cells), rng.integers(0, nc, D).astype(np.int32)))
    return out


def bits_of(correct: np.ndarray) -> np.ndarray:
    return (correct.astype(np.uint16) << np.arange(10, dtype=np.uint16)[None, :]).sum(1).astype(np.uint16)


# ---- the score cases (shared with the GPU test) ----

def score_case(n: int, seed: int = 0, nc: int = 5):
    """Class 0: n detections, all correct; 1: n, none correct; 2: n with repeated confidences and random bits; 3: labels but no detection;
    4: detections but no label.  -> (conf float32 [N], cls int32 [N], bits uint16 [N], label_counts int64 [nc]), in sweep order."""
    rng = np.random.default_rng(1000 + n + seed)
    conf = np.concatenate([rng.random(n), rng.random(n), rng.integers(1, 8, n) / 8.0, rng.random(max(n // 2, 1))]).astype(F32)
    cls = np.concatenate([np.full(n, 0), np.full(n, 1), np.full(n, 2), np.full(max(n // 2, 1), 4)]).astype(np.int32)
    level = rng.integers(0, 11, n)                                              # correct at the first `level` thresholds
    bits = np.concatenate([np.full(n, 0x3FF), np.zeros(n, np.int64), (1 << level) - 1, np.full(max(n // 2, 1), 0x3FF)]).astype(np.uint16)
    o = rng.permutation(conf.shape[0])
    return conf[o], cls[o], bits[o], np.array([n, 3, n + 5, 4, 0], np.int64)       # (class 0: recall reaches exactly 1, a duplicate knot)


RUNS = (1, 2, 63, 64, 65, 4097)


def literal_of(conf, cls, bits, label_counts):
    tp = ((bits[:, None] >> np.arange(10, dtype=np.uint16)[None, :]) & 1).astype(bool)
    target = np.repeat(np.arange(label_counts.shape[0]), label_counts)
    return ap_per_class_literal(tp, conf, cls, target)


# ---- matching ----

def test_matching_closed_rule_equals_upstream_procedure():
    on_threshold = ties = 0
    for lbox, lcls, dbox, dcls in list(random_match_cases()) + list(FIXED_MATCH.values()):
        want = bits_of(process_batch_literal(lbox, lcls, dbox, dcls))
        got = val.match_numpy(lbox, lcls, dbox, dcls)
        assert got.dtype == np.uint16 and np.array_equal(got, want)
        if lcls.shape[0] and dcls.shape[0]:
            iou = np.where(lcls[:, None] == dcls[None, :], val.box_iou_numpy(lbox, dbox), F32(-1))
            on_threshold += int(np.isin(iou, val.IOUV).sum())
            top = iou.max(0)
            ties += int(((iou == top[None, :]).sum(0)[top >= 0.5] > 1).sum())
    assert on_threshold > 0 and ties > 0, (on_threshold, ties)                  # the input set holds both


def test_matching_fixed_cases():
    m = lambda k: val.match_numpy(*FIXED_MATCH[k]).tolist()
    assert m("no labels") == [0, 0] and m("no detections") == [] and m("neither") == [] and m("class mismatch only") == [0, 0]
    assert F32(1) / (F32(2) + F32(1e-7)) == F32(0.5)
    assert val.box_iou_numpy(*[FIXED_MATCH["iou exactly 0.5"][i] for i in (0, 2)])[0, 0] == F32(0.5)
    assert m("iou exactly 0.5") == [1]                                          # counts at threshold 0 only
    lbox, lcls, dbox, dcls = FIXED_MATCH["shared best label"]
    iou = val.box_iou_numpy(lbox, dbox)
    assert iou[0, 1] > iou[1, 1] >= 0.55                                        # detection 1 prefers label 0, and label 1 overlaps it above threshold
    assert m("shared best label") == [0x3FF, 0]                                 # ... yet it stays unmatched: no fall-back to the second-best label
    lbox, lcls, dbox, dcls = FIXED_MATCH["equal iou to two labels"]
    iou = val.box_iou_numpy(lbox, dbox)
    assert iou[0, 0] == iou[1, 0] > 0
    # the higher index (1) takes it: a second detection that only label 0 fits better is then free to take label 0
    d2 = np.concatenate([dbox, np.array([[0, 0, 8, 8]], F32)]), np.array([0, 0], np.int32)
    assert np.array_equal(val.match_numpy(lbox, lcls, *d2), bits_of(process_batch_literal(lbox, lcls, *d2)))


# ---- interp ----

def test_interp_rule_equals_np_interp_bit_for_bit():
    rng = np.random.default_rng(5)
    for trial in range(50):
        n = int(rng.integers(1, 40))
        xp = np.sort(rng.integers(0, 12, n) / 8.0)                              # duplicate knots
        fp = rng.random(n)
        between = rng.random(64) * 2 - 0.25                                     # inside, between and outside the knots
        x = np.concatenate([xp, between, [xp[0], xp[-1], xp[0] - 1, xp[-1] + 1]])
        for left in (0.0, 1.0):
            want, got = np.interp(x, xp, fp, left=left), val.interp_numpy(x, xp, fp, left)
            assert got.tobytes() == want.tobytes(), trial


# ---- scores ----

@pytest.mark.parametrize("n", RUNS)
def test_scores_equal_literal_ap_per_class(n):
    conf, cls, bits, label_counts = score_case(n)
    classes, n_l, ap, p, r, pr = val.score_cpu(conf, cls, bits, label_counts)
    tp_, fp_, p_, r_, f1_, ap_, classes_, pc_, rc_, py_ = literal_of(conf, cls, bits, label_counts)
    assert classes.tolist() == classes_.tolist() == [0, 1, 2, 3]                # class 4 has no labels: no part; class 3 counts with AP 0
    assert np.array_equal(p, pc_) and np.array_equal(r, rc_) and np.array_equal(pr, py_)        # curves: equal
    s = val.summarise(ap, p, r, n_l)
    assert np.array_equal(s["tp"], tp_) and np.array_equal(s["fp"], fp_)        # integer counts: equal
    assert np.array_equal(s["p"], p_) and np.array_equal(s["r"], r_) and np.array_equal(s["f1"], f1_)
    # AP: the order of 100 additions of terms that sum to at most 1 (about 1e-14 in fp64); 100 x for numpy's pairwise blocks
    assert np.abs(ap - ap_).max() <= 1e-12
    assert (ap[3] == 0).all() and (ap[0] > 0.9).all() and (ap[1] == 0).all()
    assert s["map50"] == ap[:, 0].mean() and s["map"] == ap.mean(1).mean()


# ---- expand ----

def expand_case(B, N, nc, seed=0):
    """pred [B, N, 5 + nc]: obj and obj * cls at, just under and just over the threshold; image 1 has no passing row, image 2 only passing ones."""
    rng = np.random.default_rng(seed + 31 * N + nc)
    t = F32(0.001)
    pred = rng.random((B, N, 5 + nc)).astype(F32)
    pred[..., :4] *= 640
    edge = np.array([t, np.nextafter(t, F32(0)), np.nextafter(t, F32(1)), 0.5, 1.0, 0.03], F32)
    pred[..., 4] = edge[rng.integers(0, edge.shape[0], (B, N))]
    pick = rng.random((B, N, nc)) < 0.5
    with np.errstate(divide="ignore"):
        at = (t / pred[..., 4:5]).astype(F32)                                   # obj * cls lands on or next to the threshold
    pred[..., 5:] = np.where(pick, np.minimum(at * edge[rng.integers(0, 3, (B, N, nc))] / t, F32(1)), pred[..., 5:])
    if B > 1:
        pred[1, :, 4] = np.nextafter(t, F32(0))
    if B > 2:
        pred[2, :, 4:] = 1.0
    return pred


def test_expand_restatement_against_plain_loops():
    for N, nc in ((1, 1), (65, 2), (200, 5)):
        pred = expand_case(3, N, nc)
        rows, counts = val.expand_rows_numpy(pred, 0.001, N * nc)
        for b in range(3):
            want = []
            for r in range(N):
                for j in range(nc):
                    if pred[b, r, 4] > F32(0.001) and F32(pred[b, r, 4] * pred[b, r, 5 + j]) > F32(0.001):
                        row = np.zeros(5 + nc, F32)
                        row[:5], row[5 + j] = pred[b, r, :5], pred[b, r, 5 + j]
                        want.append(row)
            assert counts[b] == len(want)
            assert np.array_equal(rows[b, :len(want)], np.array(want, F32).reshape(-1, 5 + nc)) and (rows[b, len(want):] == 0).all()
        assert counts[1] == 0 and counts[2] == N * nc and 0 < counts[0] < N * nc or N == 1
    poisoned = np.full((3, 4, 7), 9.0, F32)
    rows, counts = val.expand_rows_numpy(expand_case(3, 65, 2), 0.001, 4, rows=poisoned.copy())
    assert counts[2] == 130 and np.array_equal(rows, poisoned)                  # overflow: the true count, the buffer untouched


# ---- data ----

def test_label_path_rule_replaces_the_last_images():
    s = os.sep
    assert val.img2label_path(f"{s}d{s}images{s}set{s}images{s}a.b.jpg") == f"{s}d{s}images{s}set{s}labels{s}a.b.txt"
    assert val.img2label_path(f"{s}d{s}images{s}x.jpeg") == f"{s}d{s}labels{s}x.txt"
    assert val.img2label_path(f"{s}d{s}pics{s}x.png") == f"{s}d{s}pics{s}x.txt"


def _png(path, w=8, h=6):
    from PIL import Image
    os.makedirs(os.path.dirname(path), exist_ok=True)
    Image.fromarray(np.zeros((h, w, 3), np.uint8)).save(path)


def test_yaml_forms(tmp_path):
    for k in ("a", "b"):
        _png(str(tmp_path / "set" / "images" / "val" / f"{k}.png"))
    _png(str(tmp_path / "set" / "images" / "extra" / "c.png"))
    (tmp_path / "set" / "list.txt").write_text("./images/extra/c.png\n")
    y = tmp_path / "d.yaml"
    y.write_text("path: set\nval: images/val\ntest: [images/val, list.txt]\nnames: [circle, square]\n")
    d = val.load_data_yaml(str(y))
    assert d["nc"] == 2 and d["names"] == {0: "circle", 1: "square"} and d["train"] is None
    assert [os.path.basename(f) for f in val.list_split_images(d["val"])] == ["a.png", "b.png"]
    assert sorted(os.path.basename(f) for f in val.list_split_images(d["test"])) == ["a.png", "b.png", "c.png"]
    y.write_text(f"path: {tmp_path / 'set'}\nval: list.txt\nnc: 2\nnames:\n  0: circle\n  1: square\n")
    d = val.load_data_yaml(str(y))
    assert d["names"] == {0: "circle", 1: "square"} and [os.path.basename(f) for f in val.list_split_images(d["val"])] == ["c.png"]
    y.write_text("val: set/images/val\nnc: 3\nnames: [circle, square]\n")
    with pytest.raises(ValueError, match="names"):
        val.load_data_yaml(str(y))


def test_corrupt_and_duplicate_label_rows(tmp_path):
    w = lambda name, text: (tmp_path / name).write_text(text) and str(tmp_path / name)
    lb, dup = val.read_label_file(w("ok.txt", "1 0.5 0.5 0.2 0.2\n0 0.25 0.25 0.1 0.1\n\n"))
    assert dup == 0 and lb.tolist() == np.array([[1, .5, .5, .2, .2], [0, .25, .25, .1, .1]], F32).tolist()      # order kept
    lb, dup = val.read_label_file(w("dup.txt", "1 0.5 0.5 0.2 0.2\n0 0.25 0.25 0.1 0.1\n1 0.5 0.5 0.2 0.2\n"))
    assert dup == 1 and lb.tolist() == np.array([[0, .25, .25, .1, .1], [1, .5, .5, .2, .2]], F32).tolist()      # np.unique's order
    assert val.read_label_file(w("six.txt", "1 0.5 0.5 0.2 0.2 0.9\n"))[0] is None
    assert val.read_label_file(w("four.txt", "1 0.5 0.5 0.2\n"))[0] is None
    assert val.read_label_file(w("neg.txt", "1 0.5 -0.5 0.2 0.2\n"))[0] is None
    assert val.read_label_file(w("big.txt", "1 0.5 0.5 1.2 0.2\n"))[0] is None
    assert val.read_label_file(str(tmp_path / "missing.txt"))[0].shape == (0, 5)
    assert val.read_label_file(w("empty.txt", ""))[0].shape == (0, 5)
    box = val.label_boxes(np.array([[0, 0.5, 0.25, 0.2, 0.1]], F32), 100, 200)
    assert box.dtype == F32 and box.tolist() == [[(F32(0.5) - F32(0.2) / F32(2)) * F32(200), (F32(0.25) - F32(0.1) / F32(2)) * F32(100),
                                                  (F32(0.5) + F32(0.2) / F32(2)) * F32(200), (F32(0.25) + F32(0.1) / F32(2)) * F32(100)]]


def test_refusals(monkeypatch):
    base = ["--data", "d.yaml", "--weights", "w.pt"]
    for extra, word in ((["--task", "speed"], "speed"), (["--task", "study"], "study"), (["--task", "other"], "train, val or test"),
                        (["--augment"], "--augment"), (["--save-hybrid"], "--save-hybrid"), (["--save-json"], "--save-json"),
                        (["--cpu"], "--labels")):
        with pytest.raises(SystemExit) as e:
            val.check_opt(val.parse_opt(base + extra))
        assert word in str(e.value) and "\n" not in str(e.value)
    val.check_opt(val.parse_opt(base + ["--dnn"]))                              # ignored
    with pytest.raises(SystemExit, match="--weights"):
        val.check_opt(val.parse_opt(["--data", "d.yaml"]))
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU"):
        val.check_opt(val.parse_opt(base))
    opt = val.parse_opt(["--data", "d.yaml"])
    assert (opt.batch_size, opt.imgsz, opt.conf_thres, opt.iou_thres, opt.max_det, opt.task, opt.name) == (32, 640, 0.001, 0.6, 300, "val", "exp")
    assert opt.project.endswith(os.path.join("runs", "val")) and not opt.half and opt.precision is None


def test_table_format():
    s = {"mp": 0.5, "mr": 0.25, "map50": 0.123456, "map": 1.0, "p": np.array([1.0, 0.0]), "r": np.array([0.5, 0.0]),
         "ap50": np.array([0.246912, 0.0]), "ap": np.array([1e-5, 0.0])}
    got = val.format_table({0: "circle_farm", 1: "square_farm"}, 10, np.array([0, 1]), np.array([7, 5]), s, True)
    want = ("                 Class     Images  Instances          P          R      mAP50   mAP50-95\n"
            "                   all         10         12        0.5       0.25      0.123          1\n"
            "           circle_farm         10          7          1        0.5      0.247      1e-05\n"
            "           square_farm         10          5          0          0          0          0")
    assert got == want
    assert val.format_table({0: "a"}, 1, np.array([0]), np.array([1]), {**s, "p": s["p"][:1]}, False).count("\n") == 1


# ---- the --cpu run ----

def test_cpu_run_writes_the_three_files(tmp_path, capsys):
    for k in ("a", "b", "c", "d"):
        _png(str(tmp_path / "images" / f"{k}.png"), 100, 50)
    os.makedirs(tmp_path / "labels")
    os.makedirs(tmp_path / "dets")
    (tmp_path / "labels" / "a.txt").write_text("0 0.5 0.5 0.2 0.4\n1 0.25 0.25 0.1 0.2\n0 0.5 0.5 0.2 0.4\n")     # one duplicate
    (tmp_path / "labels" / "b.txt").write_text("1 0.5 0.5 0.5 0.5\n")
    (tmp_path / "labels" / "d.txt").write_text("1 0.5 0.5 0.5\n")                                                   # corrupt: skipped
    (tmp_path / "dets" / "a.txt").write_text("0 0.5 0.5 0.2 0.4 0.9\n1 0.25 0.25 0.1 0.18 0.8\n0 0.1 0.1 0.1 0.1 0.3\n")
    (tmp_path / "dets" / "c.txt").write_text("1 0.5 0.5 0.2 0.2 0.6\n")                                             # an image without labels: a false positive
    (tmp_path / "d.yaml").write_text("val: images\nnames: [circle, square]\n")
    args = ["--data", str(tmp_path / "d.yaml"), "--labels", str(tmp_path / "dets"), "--cpu", "--project", str(tmp_path / "runs")]
    assert val.main(args) == 0
    out = capsys.readouterr().out
    assert "duplicate" in out and val.TABLE_HEADER in out
    run = tmp_path / "runs" / "exp"
    rows = (run / "val_classes.csv").read_text().splitlines()
    assert rows[0].startswith("class,name,images,instances,P,R,F1,mAP50,mAP50-95,ap_0.50,ap_0.55,") and rows[0].endswith("ap_0.95,tp,fp")
    assert rows[1].split(",")[:4] == ["-1", "all", "3", "3"] and [r.split(",")[1] for r in rows[2:]] == ["circle", "square"]
    assert float(rows[2].split(",")[7]) > 0.99                                                      # circle: its one label found first
    assert float(rows[3].split(",")[9]) > 0 and float(rows[3].split(",")[-3]) == 0                   # square: IoU 0.9: found at 0.5, lost at 0.95
    meta = json.loads((run / "val.json").read_text())
    assert (meta["images"], meta["skipped_images"], meta["labels"], meta["detections"], meta["duplicate_label_rows_dropped"]) == (3, 1, 3, 4, 1)
    assert meta["departures"] and meta["conf_thres"] == 0.001 and meta["device"].startswith("cpu")
    curves = (run / "val_curves.csv").read_text().splitlines()
    assert curves[0] == "px,circle_p,circle_r,circle_f1,circle_pr,square_p,square_r,square_f1,square_pr" and len(curves) == 1001
    assert val.main(args) == 0 and (tmp_path / "runs" / "exp2" / "val_classes.csv").read_text() == (run / "val_classes.csv").read_text()
    # no labels at all: upstream's warning
    (tmp_path / "e.yaml").write_text("val: [images/c.png]\nnames: [circle, square]\n")
    assert val.main(["--data", str(tmp_path / "e.yaml"), "--labels", str(tmp_path / "dets"), "--cpu", "--project", str(tmp_path / "runs")]) == 0
    assert "no labels found in val set" in capsys.readouterr().out


# ---- the ABI surface ----

def test_exports_header_and_build(lib):
    from aquaculture_amd import build, engine
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "aq_engine.h")).read(), flags=re.S)
    for name in NEW_SYMBOLS:
        assert name + "(" in header and name in engine.EXPORTS and hasattr(lib, name) and getattr(lib, name).argtypes is not None
    assert ("val.hip", ["-ffp-contract=off"]) in build.SOURCES and lib.aq_version() == 8
    assert lib.aq_val_score_chunk() == 2048
    assert lib.aq_val_scores_scratch_bytes(10 ** 7, 4883) == 10 ** 7 * 120 + 4883 * 240 + 8
    assert lib.aq_val_expand_scratch_bytes(32, 25200, 5) == (32 * 124 + 1) * 4
    shim = open(os.path.join(ROOT, "yolov5", "val.py")).read()
    assert "from aquaculture_amd.val import main" in shim
