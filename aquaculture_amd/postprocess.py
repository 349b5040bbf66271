"""Box rescale + YOLO label text: the output contract of the hot path.

Restates, in numpy fp32 with the same operation order, what ``yolov5/detect.py`` does after NMS
[UPSTREAM detect.py run(): ``det[:, :4] = scale_boxes(im.shape[2:], det[:, :4], im0.shape).round()``,
then per detection ``xywh = (xyxy2xywh(xyxy.view(1,4)) / gn).view(-1).tolist()`` and
``('%g ' * len(line)).rstrip() % line`` with ``line = (cls, *xywh, conf)`` under ``--save-conf``;
utils/general.py scale_boxes / clip_boxes / xyxy2xywh].

The consumer is reference src/process_yolo/geocode_results.py:140-172 (``np.loadtxt`` rows
``cls xc yc w h conf``; one file per image stem, *no file when there are no detections*,
reference src/process_yolo/geocode_results.py:46-55).  Because the consumer truncates
``int(IM_WIDTH * (xc - w / 2))`` on the printed 6-significant-digit values
(reference src/process_yolo/geocode_results.py:160-163), label lines must be byte-identical to
upstream's whenever the rounded pixel boxes agree; this module therefore works on the exact fp32
values and prints with ``%g``.
"""
from __future__ import annotations

import os
from typing import Iterable, List, Sequence, Tuple

import numpy as np

F32 = np.float32


def scale_boxes(img1_shape: Sequence[int], boxes: np.ndarray, img0_shape: Sequence[int]) -> np.ndarray:
    """Letterbox inverse (fp32) + clip.  img1 = network input (h, w), img0 = original image (h, w)."""
    gain = min(img1_shape[0] / img0_shape[0], img1_shape[1] / img0_shape[1])
    pad = ((img1_shape[1] - img0_shape[1] * gain) / 2, (img1_shape[0] - img0_shape[0] * gain) / 2)
    b = np.array(boxes, dtype=F32, copy=True)
    b[..., [0, 2]] -= F32(pad[0])
    b[..., [1, 3]] -= F32(pad[1])
    b[..., :4] /= F32(gain)
    np.clip(b[..., 0], 0, img0_shape[1], out=b[..., 0])
    np.clip(b[..., 1], 0, img0_shape[0], out=b[..., 1])
    np.clip(b[..., 2], 0, img0_shape[1], out=b[..., 2])
    np.clip(b[..., 3], 0, img0_shape[0], out=b[..., 3])
    return b


def detections_to_rows(det: np.ndarray, img1_shape, img0_shape) -> np.ndarray:
    """(n,6) [x1,y1,x2,y2,conf,cls] in network pixels (descending conf) -> (n,6) float32 rows
    [cls, xc, yc, w, h, conf] normalised by the ORIGINAL size, in file order (ascending conf)."""
    det = np.asarray(det, dtype=F32)
    if det.shape[0] == 0:
        return np.zeros((0, 6), F32)
    xyxy = np.rint(scale_boxes(img1_shape, det[:, :4], img0_shape)).astype(F32)   # torch.round = half-to-even
    h0, w0 = F32(img0_shape[0]), F32(img0_shape[1])
    rows = np.empty((det.shape[0], 6), F32)
    rows[:, 0] = det[:, 5]
    rows[:, 1] = ((xyxy[:, 0] + xyxy[:, 2]) / F32(2)) / w0
    rows[:, 2] = ((xyxy[:, 1] + xyxy[:, 3]) / F32(2)) / h0
    rows[:, 3] = (xyxy[:, 2] - xyxy[:, 0]) / w0
    rows[:, 4] = (xyxy[:, 3] - xyxy[:, 1]) / h0
    rows[:, 5] = det[:, 4]
    return rows[::-1].copy()   # `for *xyxy, conf, cls in reversed(det)`


def batch_rows(det_all: np.ndarray, counts: np.ndarray, img1_shape, img0_shape):
    """detections_to_rows for a whole batch of tiles of ONE original size in a single pass: det_all [B, max_det, 6], counts [B] ->
    (rows float32 [N, 6] with every tile's rows in file order, tile after tile; offsets int64 [B + 1]).  The arithmetic is elementwise,
    so the values equal the per-tile function's bit for bit; what it saves is ~20 numpy calls per tile on threads that share one GIL."""
    counts = np.asarray(counts, dtype=np.int64)
    B = counts.shape[0]
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    n = int(offsets[-1])
    if n == 0:
        return np.zeros((0, 6), F32), offsets
    valid = np.arange(det_all.shape[1])[None, :] < counts[:, None]
    det = np.asarray(det_all[:B], dtype=F32)[valid]                     # [N, 6], tile-major, descending confidence inside a tile
    xyxy = np.rint(scale_boxes(img1_shape, det[:, :4], img0_shape)).astype(F32)
    h0, w0 = F32(img0_shape[0]), F32(img0_shape[1])
    rows = np.empty((n, 6), F32)
    rows[:, 0] = det[:, 5]
    rows[:, 1] = ((xyxy[:, 0] + xyxy[:, 2]) / F32(2)) / w0
    rows[:, 2] = ((xyxy[:, 1] + xyxy[:, 3]) / F32(2)) / h0
    rows[:, 3] = (xyxy[:, 2] - xyxy[:, 0]) / w0
    rows[:, 4] = (xyxy[:, 3] - xyxy[:, 1]) / h0
    rows[:, 5] = det[:, 4]
    tile = np.repeat(np.arange(B), counts)
    pos = np.arange(n)
    rev = offsets[tile] + (counts[tile] - 1) - (pos - offsets[tile])     # `for *xyxy, conf, cls in reversed(det)`, per tile
    return rows[rev], offsets


def crop_rects(xyxy: np.ndarray, h0, w0) -> np.ndarray:
    """--save-crop geometry [UPSTREAM utils/plots.py save_one_box(xyxy, im, gain=1.02, pad=10)] in fp32, one operation at a time as PyTorch's
    CPU kernels run it: xyxy2xywh, ``b[:, 2:] * 1.02 + 10``, xywh2xyxy, ``.long()`` (truncation toward zero), clip_boxes to the image
    (x in [0, w0], y in [0, h0]).  xyxy float32 [n, 4] = the rounded boxes in original pixels; h0 / w0 scalars or [n].  -> int64 [n, 4]
    (x1, y1, x2, y2): the crop is ``im[y1:y2, x1:x2]``."""
    b = np.asarray(xyxy, dtype=F32).reshape(-1, 4)
    xc = (b[:, 0] + b[:, 2]) / F32(2)
    yc = (b[:, 1] + b[:, 3]) / F32(2)
    w = (b[:, 2] - b[:, 0]) * F32(1.02) + F32(10)
    h = (b[:, 3] - b[:, 1]) * F32(1.02) + F32(10)
    r = np.stack([xc - w / F32(2), yc - h / F32(2), xc + w / F32(2), yc + h / F32(2)], 1).astype(np.int64)
    w0 = np.asarray(w0, dtype=np.int64)
    h0 = np.asarray(h0, dtype=np.int64)
    r[:, 0] = np.clip(r[:, 0], 0, w0)
    r[:, 2] = np.clip(r[:, 2], 0, w0)
    r[:, 1] = np.clip(r[:, 1], 0, h0)
    r[:, 3] = np.clip(r[:, 3], 0, h0)
    return r


def batch_crops(det_all: np.ndarray, counts: np.ndarray, img1_shape, img0_shape):
    """--save-crop for a whole batch of tiles of ONE original size in one pass: det_all [B, max_det, 6], counts [B] -> (tile int64 [N],
    cls int64 [N], rects int64 [N, 4], ordinal int64 [N]), every tile's crops in upstream's order (``for *xyxy, conf, cls in reversed(det)``,
    ascending confidence), tile after tile.  ordinal k counts the crops of one class in one tile from 1: upstream's increment_path names
    them <stem>.jpg, <stem>2.jpg, ... in a fresh directory (crop_file_name)."""
    counts = np.asarray(counts, dtype=np.int64)
    B = counts.shape[0]
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    n = int(offsets[-1])
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), np.zeros((0, 4), np.int64), z.copy()
    valid = np.arange(det_all.shape[1])[None, :] < counts[:, None]
    det = np.asarray(det_all[:B], dtype=F32)[valid]                     # [N, 6], tile-major, descending confidence inside a tile
    tile = np.repeat(np.arange(B), counts)
    pos = np.arange(n)
    rev = offsets[tile] + (counts[tile] - 1) - (pos - offsets[tile])     # reversed(det), per tile
    det = det[rev]
    xyxy = np.rint(scale_boxes(img1_shape, det[:, :4], img0_shape)).astype(F32)   # det[:, :4] = scale_boxes(...).round()
    rects = crop_rects(xyxy, img0_shape[0], img0_shape[1])
    cls = det[:, 5].astype(np.int64)
    order = np.lexsort((pos, cls, tile))                                # stable: (tile, class), then upstream's order
    key = tile[order] * (int(cls.max()) + 1) + cls[order]
    first = np.r_[True, key[1:] != key[:-1]]
    start = np.maximum.accumulate(np.where(first, np.arange(n), 0))
    ordinal = np.empty(n, np.int64)
    ordinal[order] = np.arange(n) - start + 1
    return tile, cls, rects, ordinal


def crop_file_name(stem: str, ordinal: int) -> str:
    """<stem>.jpg for the first crop of a class in an image, <stem>2.jpg, <stem>3.jpg, ... for the next ([UPSTREAM increment_path] with
    sep='' in a directory that holds no crops of this image yet)."""
    return f"{stem}{ordinal if ordinal > 1 else ''}.jpg"


# ---- annotated images: upstream's Annotator.box_label (Pillow branch) as primitives for aq_annotate_u8 ----

# [UPSTREAM utils/plots.py Colors]: the 20-entry palette, indexed cls % 20, as RGB
PALETTE = np.array([[int(h_[i:i + 2], 16) for i in (0, 2, 4)] for h_ in (
    "FF3838", "FF9D97", "FF701F", "FFB21D", "CFD231", "48F90A", "92CC17", "3DDB86", "1A9334", "00D4BB",
    "2C99A8", "00C2FF", "344593", "6473FF", "0018EC", "8438FF", "520085", "CB38FF", "FF95C8", "FF37C7")], dtype=np.int64)
PRIM_FIELDS = ("x0", "y0", "x1", "y1", "rgb", "mask_w", "mask")


def batch_boxes(det_all: np.ndarray, counts: np.ndarray, img1_shape, img0_shape):
    """The boxes upstream draws for a whole batch of tiles of ONE original size: det_all [B, max_det, 6], counts [B] -> (tile int64 [N],
    cls int64 [N], conf float32 [N], xyxy int64 [N, 4]), every tile's detections in upstream's order (``reversed(det)``: ascending confidence,
    the best box drawn last), tile after tile; xyxy = the rounded scale_boxes corners (a corner may equal the width or height)."""
    counts = np.asarray(counts, dtype=np.int64)
    B = counts.shape[0]
    offsets = np.zeros(B + 1, np.int64)
    np.cumsum(counts, out=offsets[1:])
    n = int(offsets[-1])
    if n == 0:
        z = np.zeros(0, np.int64)
        return z, z.copy(), np.zeros(0, F32), np.zeros((0, 4), np.int64)
    valid = np.arange(det_all.shape[1])[None, :] < counts[:, None]
    det = np.asarray(det_all[:B], dtype=F32)[valid]
    tile = np.repeat(np.arange(B), counts)
    pos = np.arange(n)
    det = det[offsets[tile] + (counts[tile] - 1) - (pos - offsets[tile])]     # reversed(det), per tile
    xyxy = np.rint(scale_boxes(img1_shape, det[:, :4], img0_shape)).astype(np.int64)
    return tile, det[:, 5].astype(np.int64), det[:, 4].copy(), xyxy


def label_strings(names, cls: np.ndarray, conf: np.ndarray, hide_conf: bool = False):
    """[UPSTREAM detect.py] ``names[c] if hide_conf else f'{names[c]} {conf:.2f}'`` per detection."""
    if hide_conf:
        return [names[int(c)] for c in cls]
    return [f"{names[int(c)]} {float(v):.2f}" for c, v in zip(cls, conf)]


def annotation_prims(image: np.ndarray, cls: np.ndarray, xyxy: np.ndarray, sizes, line_width: int, labels=None):
    """[UPSTREAM utils/plots.py Annotator.box_label, Pillow branch] for N detections as aq_prim rows (engine.PRIM_DTYPE fields as a dict of
    arrays) and the image index of each row, in drawing order.  image int [N] (index into sizes), cls int [N], xyxy int [N, 4], sizes int
    [n_images, 2] (h, w), line_width = upstream's lw.  labels = None (--hide-labels) or int64 [N, 7]: (w, h) of ``font.getbbox(label)[2:]``,
    the (width, height) of the label's 8-bit mask, its (x, y) offset, the mask's first byte in the atlas (annotate.LabelAtlas.lookup).

    Per detection, in this order: the outline ``ImageDraw.rectangle(box, width=lw, outline=colour)`` -- ImagingDrawRectangle draws, for
    i < lw, the rows y0 + i and y1 - i from x0 to x1 and the columns x0 + i and x1 - i from y0 + lw towards y1 - lw + 1, that
    last row left out (upwards when the box is thinner than 2 lw - 1: such a box is painted beyond its corners), four rectangles --, the label's filled rectangle
    ``(x0, y0 - h if outside else y0, x0 + w + 1, y0 + 1 if outside else y0 + h + 1)`` with ``outside = y0 - h >= 0``, and the text mask in
    white at ``(x0, y0 - h if outside else y0)`` + the mask's offset.  Everything is clipped to the image; what is left empty is dropped."""
    image = np.asarray(image, dtype=np.int64)
    n = image.shape[0]
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    X0, Y0, X1, Y1 = (np.asarray(xyxy, dtype=np.int64).reshape(-1, 4)[:, i] for i in range(4))
    lw = int(line_width)
    colour = PALETTE[np.asarray(cls, dtype=np.int64) % 20]
    rgb = colour[:, 0] | (colour[:, 1] << 8) | (colour[:, 2] << 16)
    k = 4 if labels is None else 6
    P = {f: np.zeros((n, k), np.int64) for f in PRIM_FIELDS}
    a, b = Y0 + lw, Y1 - lw + 1                               # ImagingDrawLine, vertical: |b - a| points from a towards b, b itself left out
    ya, yb = np.where(a < b, a, b + 1), np.where(a < b, b - 1, a)
    for j, (a_, b_, c_, d_) in enumerate(((X0, Y0, X1, Y0 + lw - 1), (X0, Y1 - lw + 1, X1, Y1), (X1 - lw + 1, ya, X1, yb), (X0, ya, X0 + lw - 1, yb))):
        P["x0"][:, j], P["y0"][:, j], P["x1"][:, j], P["y1"][:, j] = a_, b_, c_, d_
    if lw <= 0:                                                # ImageDraw.rectangle draws no outline at width 0
        P["x1"][:, :4] = P["x0"][:, :4] - 1
    P["rgb"][:, :4] = rgb[:, None]
    if labels is not None:
        L = np.asarray(labels, dtype=np.int64).reshape(-1, 7)
        w, h, mw, mh, ox, oy, off = (L[:, i] for i in range(7))
        ty = np.where(Y0 - h >= 0, Y0 - h, Y0)
        P["x0"][:, 4], P["y0"][:, 4], P["x1"][:, 4], P["y1"][:, 4], P["rgb"][:, 4] = X0, ty, X0 + w + 1, ty + h + 1, rgb
        P["x0"][:, 5], P["y0"][:, 5], P["x1"][:, 5], P["y1"][:, 5], P["rgb"][:, 5] = X0 + ox, ty + oy, X0 + ox + mw - 1, ty + oy + mh - 1, 0xFFFFFF
        P["mask_w"][:, 5], P["mask"][:, 5] = mw, off
        P["x1"][:, 5] = np.where(mw > 0, P["x1"][:, 5], P["x0"][:, 5] - 1)   # (a label without ink, e.g. a blank: nothing to composite)
    img = np.repeat(image, k)
    P = {f: v.reshape(-1) for f, v in P.items()}
    H, W = sizes[img, 0], sizes[img, 1]
    cx0, cy0 = np.maximum(P["x0"], 0), np.maximum(P["y0"], 0)
    P["mask"] = P["mask"] + (cy0 - P["y0"]) * P["mask_w"] + (cx0 - P["x0"])    # the mask byte of the first pixel kept
    P["x0"], P["y0"], P["x1"], P["y1"] = cx0, cy0, np.minimum(P["x1"], W - 1), np.minimum(P["y1"], H - 1)
    keep = (P["x1"] >= P["x0"]) & (P["y1"] >= P["y0"])
    return {f: v[keep] for f, v in P.items()}, img[keep]


def prims_array(P: dict, dtype) -> np.ndarray:
    """annotation_prims' columns as one structured array (engine.PRIM_DTYPE)."""
    out = np.zeros(P["x0"].shape[0], dtype)
    for f in PRIM_FIELDS:
        out[f] = P[f]
    return out


def bin_prims(P: dict, image: np.ndarray, sizes):
    """The primitives of annotation_prims binned per 16 x 16-pixel cell: image i has ceil(w / 16) ceil(h / 16) cells in raster order, the
    images' cells follow each other.  -> (cell_start int32 [cells + 1], cell_prims int32 [entries]): cell c applies the primitives
    cell_prims[cell_start[c]:cell_start[c + 1]], ascending.  The work is that of the cells the primitives touch, not cells x primitives."""
    sizes = np.asarray(sizes, dtype=np.int64).reshape(-1, 2)
    cw, ch = (sizes[:, 1] + 15) // 16, (sizes[:, 0] + 15) // 16
    first = np.zeros(sizes.shape[0] + 1, np.int64)
    np.cumsum(cw * ch, out=first[1:])
    n_cells = int(first[-1])
    if n_cells >= 1 << 31:
        raise ValueError("bin_prims: more than 2^31 cells")
    cx0, cy0, cx1, cy1 = P["x0"] >> 4, P["y0"] >> 4, P["x1"] >> 4, P["y1"] >> 4
    nx = cx1 - cx0 + 1
    cnt = nx * (cy1 - cy0 + 1)
    total = int(cnt.sum())
    if total >= 1 << 31:
        raise ValueError("bin_prims: more than 2^31 cell entries")
    idx = np.repeat(np.arange(cnt.shape[0]), cnt)
    start = np.cumsum(cnt) - cnt
    local = np.arange(total) - start[idx]
    nxi = nx[idx]
    cell = first[image[idx]] + (cy0[idx] + local // nxi) * cw[image[idx]] + cx0[idx] + local % nxi
    # by cell, ascending primitive index inside a cell: one sort of (cell, entry number) keys -- the entries are generated in primitive order
    key = np.sort(cell * max(total, 1) + np.arange(total))
    cell_start = np.zeros(n_cells + 1, np.int64)
    np.cumsum(np.bincount(cell, minlength=n_cells), out=cell_start[1:])
    return cell_start.astype(np.int32), idx[key % max(total, 1)].astype(np.int32)


def format_rows(rows: np.ndarray, save_conf: bool = True) -> str:
    """Text of one label file.  Each value through ``%g`` of the double that equals the fp32 value
    (one C-level format call for the whole file: the same conversions as upstream's per-line ``%``)."""
    n = 6 if save_conf else 5
    k = rows.shape[0]
    if k == 0:
        return ""
    line = ("%g " * n).rstrip() + "\n"
    return (line * k) % tuple(np.asarray(rows[:, :n], dtype=np.float64).ravel().tolist())


def write_label_file(labels_dir: str, stem: str, rows: np.ndarray, save_conf: bool = True) -> bool:
    """Appends like upstream (``open(f'{txt_path}.txt', 'a')``); writes nothing for zero detections."""
    if rows.shape[0] == 0:
        return False
    with open(os.path.join(labels_dir, stem + ".txt"), "a") as f:
        f.write(format_rows(rows, save_conf))
    return True


def class_summary(det_cls: np.ndarray, names) -> str:
    """The per-image log fragment upstream prints: "3 circle_farms, 1 square_farm, "."""
    s = ""
    for c in np.unique(det_cls):
        n = int((det_cls == c).sum())
        s += f"{n} {names[int(c)]}{'s' * (n > 1)}, "
    return s
