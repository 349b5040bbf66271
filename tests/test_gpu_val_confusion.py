"""yolov5/val.py --confusion-matrix on the GPU: aq_val_confusion against val.confusion_numpy, matrix and image rows equal, on the inputs of
tests/test_val_confusion.py and on both sides of every size at which the kernel takes another path; accumulation; the refusals; yolov5/val.py
end to end in fp32 against confusion_numpy on the run's own detections."""
import json
import os

import numpy as np
import pytest
import torch

from poison import poisoned
from test_val_confusion import CONFS, FIXED, _split, random_cases

from aquaculture_amd import engine, val

pytestmark = pytest.mark.gpu
F32 = np.float32
DEV = "cuda:0"
TILES = [0, 1, 2, 3, 19, 20, 21, 22, 23, 24]                                   # the split of tests/test_gpu_val.py
IDENT = np.array([0, 0, 1, 4096, 4096], F32)


def _inside(a: np.ndarray) -> torch.Tensor:
    """The array inside a torch.empty allocation (poisoned and guarded inside a `poisoned` block)."""
    a = np.ascontiguousarray(a)
    t = torch.empty(a.shape, dtype=torch.from_numpy(a).dtype, device=DEV)
    if a.size:
        t.copy_(torch.from_numpy(a))
    return t


def _pack(cases, nets=None, max_det=300):
    """dets [B, max_det, 6] (NaN past each count), counts, the concatenated labels and their starts."""
    B = len(cases)
    dets = np.full((B, max_det, 6), np.nan, F32)
    counts = np.array([c[4].shape[0] for c in cases], np.int32)
    for b, c in enumerate(cases):
        k = counts[b]
        dets[b, :k, :4], dets[b, :k, 4], dets[b, :k, 5] = (nets[b] if nets is not None else c[2]), c[3], c[4]
    start = np.zeros(B + 1, np.int32)
    np.cumsum([c[1].shape[0] for c in cases], out=start[1:])
    lbox = np.concatenate([c[0] for c in cases]).astype(F32).reshape(-1, 4)
    lcls = np.concatenate([c[1] for c in cases]).astype(np.int32)
    return dets, counts, lbox, lcls, start


def _confusion_batch(cases, nc, monkeypatch, geoms=None, nets=None, matrix0=None, thresholds=(0.25, 0.45), host_classes=True):
    """One aq_val_confusion call with every buffer inside a poisoned allocation -> (matrix, image rows, flag)."""
    dets, counts, lbox, lcls, start = _pack(cases, nets)
    geom = np.stack(geoms) if geoms is not None else np.tile(IDENT, (len(cases), 1))
    with poisoned(monkeypatch, 0xFF) as p:
        matrix = _inside(np.zeros((nc + 1, nc + 1), np.int64) if matrix0 is None else matrix0)
        flag = _inside(np.zeros(1, np.int32))
        image = engine.val_confusion(_inside(dets), _inside(counts), _inside(lbox), _inside(lcls), _inside(start), start, _inside(geom), nc,
                                     thresholds[0], thresholds[1], matrix, label_cls_host=lcls if host_classes else None, flag=flag)
        torch.cuda.synchronize()
        p.check_guards()
        assert not p.passed_through
        return matrix.cpu().numpy(), image.cpu().numpy(), int(flag.item())


def _numpy_batch(cases, nc, thresholds=(0.25, 0.45)):
    out = [val.confusion_numpy(*c[:5], nc, *thresholds) for c in cases]
    return sum((o[0] for o in out), np.zeros((nc + 1, nc + 1), np.int64)), np.stack([o[1] for o in out])


# ---- the kernel against the restatement ----

def test_confusion_equals_the_restatement_on_the_cpu_cases(lib, monkeypatch):
    cases = list(random_cases()) + [c for c, _, _ in FIXED.values()]
    kept = 0
    for nc in sorted({c[5] for c in cases}):
        part = [c for c in cases if c[5] == nc]
        for s in range(0, len(part), 64):
            matrix, image, flag = _confusion_batch(part[s:s + 64], nc, monkeypatch)
            want, want_image = _numpy_batch(part[s:s + 64], nc)
            assert flag == 0 and np.array_equal(matrix, want) and np.array_equal(image, want_image), nc
            kept += int(image[:, 2].sum())
    assert kept > 1000
    for name, (case, matrix, row) in FIXED.items():                             # each fixed case alone, against its written-out matrix
        got, image, _ = _confusion_batch([case], case[5], monkeypatch)
        assert got.tolist() == matrix and image.tolist() == [row], name


def _image_case(rng, L, D, nc, h0, w0):
    """L labels and D detections scattered around them (exact copies: IoU 1 and equal IoUs), in network pixels of a 640 letterbox."""
    geom = val.letterbox_geom((640, 640), (h0, w0))
    lb = np.concatenate([rng.integers(0, nc, (L, 1)), rng.random((L, 2)) * 0.8 + 0.1, rng.random((L, 2)) * 0.15 + 0.02], 1).astype(F32)
    lbox = val.label_boxes(lb, h0, w0)
    pick = rng.integers(0, max(L, 1), D)
    src = lbox[pick] if L else np.tile(np.array([[10, 10, 50, 50]], F32), (D, 1))
    orig = (src + rng.normal(0, 2, (D, 4))).astype(F32)
    orig[::7] = src[::7]
    net = (orig * geom[2] + np.array([geom[0], geom[1], geom[0], geom[1]], F32)).astype(F32)
    net[::13] += 700                                                            # outside the image: clipped
    dcls = np.where(rng.random(D) < 0.8, lb[pick, 0] if L else 0, rng.integers(0, nc, D)).astype(np.int32)
    dconf = np.sort(CONFS[rng.integers(0, CONFS.shape[0], D)])[::-1].copy()
    return (lbox, lb[:, 0].astype(np.int32), val.scale_boxes_geom(net, geom), dconf, dcls, nc), geom, net


@pytest.mark.parametrize("nc", (1, 2, 5, 80))
def test_confusion_label_and_detection_counts_mixed_sizes(lib, monkeypatch, nc):
    """Labels per image 0, 1, 64, 65, 512, 513 and 700 (both sides of the 512 labels whose keys fit LDS) x detections 0, 1, 63, 64, 65 and
    300 (both sides of the wavefront), images of different original sizes and pads in one batch."""
    rng = np.random.default_rng(100 + nc)
    sizes = [(1024, 1024), (480, 640), (640, 480), (333, 500), (1000, 700)]     # (h0, w0)
    cases, geoms, nets = [], [], []
    for L in (0, 1, 64, 65, 512, 513, 700):
        for D in (0, 1, 63, 64, 65, 300):
            case, geom, net = _image_case(rng, L, D, nc, *sizes[len(cases) % len(sizes)])
            cases.append(case)
            geoms.append(geom)
            nets.append(net)
    assert len({tuple(g[:3]) for g in geoms}) >= 4
    matrix, image, flag = _confusion_batch(cases, nc, monkeypatch, geoms, nets)
    want, want_image = _numpy_batch(cases, nc)
    assert flag == 0 and np.array_equal(image, want_image) and np.array_equal(matrix, want)
    assert want[:nc, :nc].sum() > 300 and want[nc, :nc].sum() > 300 and want[:nc, nc].sum() > 100
    assert nc == 1 or want[:nc, :nc].sum() > np.trace(want[:nc, :nc]) > 0       # pairs on and off the diagonal


def test_confusion_accumulates(lib, monkeypatch):
    cases = [c for c in random_cases() if c[5] == 3]
    assert len(cases) >= 8
    half = len(cases) // 2
    start = np.arange(16, dtype=np.int64).reshape(4, 4) * 1_000_000_007        # a matrix that is not zero, past 32 bits
    first, image_a, _ = _confusion_batch(cases[:half], 3, monkeypatch, matrix0=start)
    both, image_b, _ = _confusion_batch(cases[half:], 3, monkeypatch, matrix0=first)
    once, image, _ = _confusion_batch(cases, 3, monkeypatch)
    assert np.array_equal(both, start + once) and np.array_equal(np.concatenate([image_a, image_b]), image) and once.sum() > 100
    assert np.array_equal(once, _numpy_batch(cases, 3)[0])
    other, _, _ = _confusion_batch(cases, 3, monkeypatch, thresholds=(0.3, 0.7))
    assert np.array_equal(other, _numpy_batch(cases, 3, (0.3, 0.7))[0]) and not np.array_equal(other, once)


# ---- refusals ----

def test_confusion_refusals_leave_the_outputs_untouched(lib):
    case = FIXED["no fall-back"][0]
    dets, counts, lbox, lcls, start = _pack([case, case], max_det=4)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    t = {"dets": dev(dets), "counts": dev(counts), "lbox": dev(lbox), "lcls": dev(lcls), "start": dev(start), "geom": dev(np.tile(IDENT, (2, 1))),
         "scratch": torch.zeros(lib.aq_val_confusion_scratch_bytes(2, 4, 4) + 8, dtype=torch.uint8, device=DEV)}
    matrix = torch.full((3, 3), 7, dtype=torch.int64, device=DEV)
    image = torch.full((2, 4), -3, dtype=torch.int32, device=DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    need = lib.aq_val_confusion_scratch_bytes(2, 4, 4)
    assert need == 4 * 8 + 2 * 4 * 4

    def call(**o):
        a = {"dets": t["dets"].data_ptr(), "counts": t["counts"].data_ptr(), "B": 2, "max_det": 4, "lbox": t["lbox"].data_ptr(),
             "lcls": t["lcls"].data_ptr(), "lcls_host": lcls.ctypes.data, "start": t["start"].data_ptr(), "start_host": start, "L": 4,
             "geom": t["geom"].data_ptr(), "nc": 2, "conf": 0.25, "iou": 0.45, "scratch": t["scratch"].data_ptr(), "scratch_bytes": need,
             "matrix": matrix.data_ptr(), "image": image.data_ptr(), "flag": flag.data_ptr()}
        a.update(o)
        sh = np.ascontiguousarray(a["start_host"], dtype=np.int32)
        engine._check(lib.aq_val_confusion(a["dets"], a["counts"], a["B"], a["max_det"], a["lbox"], a["lcls"], a["lcls_host"], a["start"],
                                           sh.ctypes.data, a["L"], a["geom"], a["nc"], a["conf"], a["iou"], a["scratch"], a["scratch_bytes"],
                                           a["matrix"], a["image"], a["flag"], None))

    bad_classes = np.array([0, 1, 2, 0], np.int32)
    refused = (("classes", {"nc": 0}), ("classes", {"nc": -1}), ("max_det", {"max_det": 0}), ("images", {"B": -1}),
               ("null pointer", {"dets": None}), ("null pointer", {"matrix": None}), ("null pointer", {"image": None}), ("null pointer", {"flag": None}),
               ("null pointer", {"lcls": None}), ("null pointer", {"scratch": None}),
               ("unaligned", {"matrix": matrix.data_ptr() + 4}), ("unaligned", {"lbox": t["lbox"].data_ptr() + 4}),
               ("unaligned", {"image": image.data_ptr() + 2}), ("unaligned", {"scratch": t["scratch"].data_ptr() + 4}),
               ("label start", {"start_host": [0, 3, 2]}), ("label start", {"start_host": [0, 2, 5]}), ("label start", {"start_host": [-1, 2, 4]}),
               ("scratch of", {"scratch_bytes": need - 1}),
               ("threshold", {"conf": float("nan")}), ("threshold", {"conf": float("inf")}), ("threshold", {"iou": float("nan")}),
               ("threshold", {"iou": float("inf")}), ("threshold", {"iou": 0.0}), ("threshold", {"iou": -0.5}),
               ("has class 2", {"lcls_host": bad_classes.ctypes.data}))
    for word, o in refused:
        with pytest.raises(RuntimeError, match=word):
            call(**o)
    torch.cuda.synchronize()
    assert bool((matrix == 7).all()) and bool((image == -3).all()) and int(flag.item()) == 0
    call(B=0)                                                                   # does nothing
    torch.cuda.synchronize()
    assert bool((matrix == 7).all()) and bool((image == -3).all())
    call()                                                                      # and the same arguments, accepted
    want = val.confusion_numpy(*case)
    assert np.array_equal(matrix.cpu().numpy(), 7 + 2 * want[0]) and image.cpu().tolist() == [want[1].tolist()] * 2 and int(flag.item()) == 0


def test_confusion_class_outside_the_range_raises_and_adds_nothing(lib, monkeypatch):
    good = FIXED["no fall-back"][0]
    lbox, lcls, dbox, dconf, dcls, nc = good
    bad_det = (lbox, lcls, dbox, dconf, np.array([0, 2], np.int32), nc)         # a detection of class nc
    want = val.confusion_numpy(*good)
    matrix, image, flag = _confusion_batch([bad_det, good], nc, monkeypatch)
    assert flag == 1 and np.array_equal(matrix, want[0]) and image.tolist() == [[2, 0, 0, 0], want[1].tolist()]     # the image adds nothing, the other one does
    for cls in (-1.0, float("nan"), 2.5):
        dets, counts, lb, lc, start = _pack([good], max_det=4)
        dets[0, 1, 5] = cls
        dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
        m = torch.zeros((3, 3), dtype=torch.int64, device=DEV)
        with pytest.raises(RuntimeError, match="outside"):                      # without a flag of the caller's the wrapper raises
            engine.val_confusion(dev(dets), dev(counts), dev(lb), dev(lc), dev(start), start, dev(IDENT[None]), nc, 0.25, 0.45, m)
        assert int(m.abs().sum()) == 0
    bad_label = (lbox, np.array([0, 2], np.int32), dbox, dconf, dcls, nc)       # a label class the host was not shown
    matrix, image, flag = _confusion_batch([bad_label], nc, monkeypatch, host_classes=False)
    assert flag == 1 and int(np.abs(matrix).sum()) == 0 and image.tolist() == [[2, 0, 0, 0]]
    with pytest.raises(RuntimeError, match="has class 2"):
        _confusion_batch([bad_label], nc, monkeypatch)


# ---- saved detections ----

def test_saved_detections_give_the_same_confusion_files_on_both_paths(lib, tmp_path, capsys):
    """--labels DIR --confusion-matrix on the GPU (aq_val_confusion, two batches) and with --cpu (confusion_numpy): the same three files."""
    args = [a for a in _split(tmp_path) if a != "--cpu"] + ["--confusion-matrix", "--batch-size", "2"]
    assert val.main(args + ["--name", "gpu"]) == 0 and val.main(args + ["--name", "cpu", "--cpu"]) == 0
    for f in ("val_confusion.csv", "val_confusion_norm.csv", "val_images.csv", "val_classes.csv"):
        assert (tmp_path / "runs" / "gpu" / f).read_bytes() == (tmp_path / "runs" / "cpu" / f).read_bytes(), f
    assert (tmp_path / "runs" / "gpu" / "val_confusion.csv").read_text() == "predicted,circle,square,background\ncircle,1,1,0\nsquare,0,0,1\nbackground,0,1,0\n"
    got, want = (json.loads((tmp_path / "runs" / k / "val.json").read_text())["confusion"] for k in ("gpu", "cpu"))
    assert got == want


# ---- end to end ----

def test_val_end_to_end_confusion_matrix(lib, tmp_path, monkeypatch):
    """yolov5/val.py --confusion-matrix in fp32 on the synthetic checkpoint and jpegs: the matrix in val.json is confusion_numpy of the run's
    own detections, copied from the device where the kernel read them (not of the %g label files: DESIGN.md section 28); the score files
    are those of the run without the flag."""
    from aquaculture_amd import checkpoint, tiles
    d = tmp_path
    tiles.write_synthetic_jpegs(str(d / "set" / "images"), TILES, size=640)
    weights = str(d / "multilabel_farms_synth.pt")
    checkpoint.write_synthetic_checkpoint(weights, "yolov5m", 5)
    names = checkpoint.load_checkpoint(weights).names
    (d / "data.yaml").write_text(f"path: {d / 'set'}\nval: images\nnames:\n" + "".join(f"  {i}: {names[i]}\n" for i in range(5)))
    base = ["--data", str(d / "data.yaml"), "--weights", weights, "--project", str(d / "runs"), "--batch-size", "4", "--quiet"]
    quiet = lambda *_: None
    # labels: the fp32 detections at detect.py's thresholds, confidence column stripped
    val.run(val.parse_opt(base + ["--name", "labels", "--save-txt", "--conf-thres", "0.25", "--iou-thres", "0.45"]), log=quiet)
    os.makedirs(d / "set" / "labels")
    n_lines = 0
    for f in sorted(os.listdir(d / "runs" / "labels" / "labels")):
        lines = list(dict.fromkeys(open(d / "runs" / "labels" / "labels" / f).read().splitlines()))
        (d / "set" / "labels" / f).write_text("\n".join(lines) + "\n")
        n_lines += len(lines)
    assert n_lines > 100
    seen = []
    real = engine.val_confusion

    def spy(dets, counts, label_box, label_cls, label_start, label_start_host, geom, nc, conf, iou, matrix, **kw):
        seen.append((dets.cpu().numpy(), counts.cpu().numpy(), label_box.cpu().numpy(), label_cls.cpu().numpy(), np.array(label_start_host), geom.cpu().numpy()))
        return real(dets, counts, label_box, label_cls, label_start, label_start_host, geom, nc, conf, iou, matrix, **kw)
    monkeypatch.setattr(engine, "val_confusion", spy)
    val.run(val.parse_opt(base + ["--name", "flag", "--confusion-matrix"]), log=quiet)
    assert len(seen) == 3                                                       # ten images in batches of four
    monkeypatch.setattr(engine, "val_confusion", real)
    val.run(val.parse_opt(base + ["--name", "plain"]), log=quiet)
    want, rows = np.zeros((6, 6), np.int64), []
    for dets, counts, lbox, lcls, start, geom in seen:
        for b in range(counts.shape[0]):
            k, (a, e) = int(counts[b]), start[b:b + 2]
            delta, row = val.confusion_numpy(lbox[a:e], lcls[a:e], val.scale_boxes_geom(dets[b, :k, :4], geom[b]), dets[b, :k, 4], dets[b, :k, 5], 5)
            want += delta
            rows.append(row.tolist())
    run = d / "runs" / "flag"
    cm = json.loads((run / "val.json").read_text())["confusion"]
    assert cm["matrix"] == want.tolist() and want[:5, :5].sum() > 50 and sum(r[0] for r in rows) == n_lines
    assert cm["tp"] == np.diag(want)[:5].tolist() and cm["fp"] == (want.sum(1) - np.diag(want))[:5].tolist()
    images = [l.split(",") for l in (run / "val_images.csv").read_text().splitlines()[1:]]
    assert [[int(v) for v in l[1:5]] for l in images] == rows and [os.path.basename(l[0]) for l in images] == sorted(os.listdir(d / "set" / "images"))
    assert (run / "val_confusion.csv").read_text().splitlines()[0] == "predicted," + ",".join(names[i] for i in range(5)) + ",background"
    for f in ("val_classes.csv", "val_curves.csv"):
        assert (run / f).read_bytes() == (d / "runs" / "plain" / f).read_bytes()
    assert sorted(os.listdir(d / "runs" / "plain")) == ["val.json", "val_classes.csv", "val_curves.csv"]
