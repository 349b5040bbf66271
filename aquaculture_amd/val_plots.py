"""val.py --plots: val_batch{i}_labels.jpg and val_batch{i}_pred.jpg, the mosaics of upstream's plot_images, made on the GPU.

The definition [UPSTREAM utils/plots.py plot_images, output_to_target; val.py's two calls], as include/aq_engine.h states it:

Grid.  The images are the first ``n = min(B, 16)`` letterboxed network inputs of a batch (uint8 RGB, H x W).  ``ns = ceil(sqrt(n))``; image i
has its origin at ``(W (i // ns), H (i % ns))`` -- column-major -- of a white (255) ``ns H x ns W`` source mosaic.  ``scale = max_size / ns /
max(H, W)`` with max_size = 1920.  When scale < 1: ``h = ceil(scale H)``, ``w = ceil(scale W)`` and the mosaic is ``cv2.resize``d
(INTER_LINEAR) to ``(w ns, h ns)``, the x and y ratios being ``ns W / (ns w)`` and ``ns H / (ns h)``; otherwise h = H, w = W and the mosaic
is the paste itself.

Pixels.  The uint8 letterboxed pixels themselves (upstream pastes ``(im / 255) * 255`` truncated to uint8, which loses a count on some
values: a deliberate departure).  The resize is dataloader's restatement of OpenCV's fixed-point INTER_LINEAR, from the same tables.

Annotation.  Upstream's ``Annotator(mosaic, line_width=round(fs / 10), font_size=fs, pil=True)`` with ``fs = int((h + w) ns 0.01)``, a value
of 0 falling back to the Annotator's own rule from the mosaic's size (annotate.line_width, annotate.font_size); the font is
annotate.load_font's.  Per image i in order: a white outline of width 2 on ``[x, y, x + w, y + h]`` with ``(x, y) = (w (i // ns), h (i % ns))``;
the file name ``Path(path).name[:40]`` in (220, 220, 220) at ``(x + 5, y + 5)`` (ImageDraw.text: a mask blit at the mask's offset); then the
image's boxes in their order through ``box_label`` in ``colors(cls)``.  Boxes are float lists there: Pillow truncates rectangle
coordinates towards zero and renders text at the position's fractional part, and so do the primitives here.

Label mosaic.  The image's labels carried into network pixels by upstream's chain in float32 (label_targets), then ``xywh2xyxy``, ``* (w, h, w, h)``
if ``boxes.max() <= 1.01`` else ``* scale`` when scale < 1, ``+ (x, y)``; text ``names[cls]``.

Prediction mosaic.  The image's NMS output in network pixels, the first 300 rows, ``xyxy2xywh`` (pred_targets), the same chain; only
``conf > 0.25`` is drawn, text ``f'{name} {conf:.1f}'``.  Boxes are not clipped to their cell; primitives apply in index order.

File.  ``Image.save(fname)``: quality 75, 4:2:0, standard Huffman tables (aq_image_jpeg_coefs_q / aq_write_image_files_q at 75).
"""
from __future__ import annotations

import math
import os
from pathlib import Path
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

from . import annotate, postprocess
from .dataloader import _axis_coeffs, letterbox_geometry

F32 = np.float32
MAX_SIZE = 1920
MAX_SUBPLOTS = 16
MAX_DET = 300                     # output_to_target(max_det=300)
PLOT_CONF = 0.25                  # plot_images: predictions above it are drawn
JPEG_QUALITY = 75                 # Pillow's Image.save() default
NAME_RGB = (220, 220, 220)


# ----------------------------------------------------------------- the grid -----------------------------------------------------------------
def mosaic_geometry(n: int, H: int, W: int, max_size: int = MAX_SIZE) -> dict:
    """-> n (capped to 16), ns, h, w (cell size in the output), scale, resized, origins (int [n, 2]: (x, y) of every cell in the output),
    src_origins (the same in the source mosaic), size (output (height, width)) and src_size."""
    n = min(int(n), MAX_SUBPLOTS)
    if n < 1 or H < 1 or W < 1:
        raise ValueError(f"mosaic_geometry: {n} images of {H} x {W}")
    ns = int(np.ceil(n ** 0.5))
    scale = max_size / ns / max(H, W)
    h, w = H, W
    if scale < 1:
        h, w = math.ceil(scale * H), math.ceil(scale * W)
    return _grid(n, ns, H, W, h, w, scale, scale < 1)


def cell_geometry(n: int, H: int, W: int, h: int, w: int) -> dict:
    """Test support, not for the command line (no --plots run has such cells): mosaic_geometry's record for cells of any size h x w, as
    aq_val_mosaic_u8 and mosaic_numpy take them.  Upstream's own geometry only
    shrinks, by exactly W / w and H / h on a grid whose cell edges map onto each other, and then no tap pair straddles a cell edge (a
    straddling column x of edge k would need |x + 0.5 - k w| W / w < 0.5); cells larger than the images do put taps across the edges."""
    n = min(int(n), MAX_SUBPLOTS)
    return _grid(n, int(np.ceil(n ** 0.5)), H, W, h, w, min(h / H, w / W), (h, w) != (H, W))


def _grid(n, ns, H, W, h, w, scale, resized) -> dict:
    i = np.arange(n)
    return {"n": n, "ns": ns, "h": int(h), "w": int(w), "H": int(H), "W": int(W), "scale": scale, "resized": bool(resized),
            "origins": np.stack([w * (i // ns), h * (i % ns)], 1).astype(np.int64),
            "src_origins": np.stack([W * (i // ns), H * (i % ns)], 1).astype(np.int64),
            "size": (ns * int(h), ns * int(w)), "src_size": (ns * H, ns * W)}


def mosaic_tables(geo: dict) -> Tuple[np.ndarray, np.ndarray]:
    """The resize tables of the whole mosaic, (i0, i1, w0, w1) per output column (ns W -> ns w) and row (ns H -> ns h): dataloader's, which
    are the identity (w0 = 2048, w1 = 0) where nothing is resized.  int32 [ns w, 4], [ns h, 4]."""
    (sh, sw), (oh, ow) = geo["src_size"], geo["size"]
    return (np.ascontiguousarray(np.stack(_axis_coeffs(sw, ow), 1).astype(np.int32)),
            np.ascontiguousarray(np.stack(_axis_coeffs(sh, oh), 1).astype(np.int32)))


def mosaic_numpy(images: np.ndarray, geo: dict, xtab: Optional[np.ndarray] = None, ytab: Optional[np.ndarray] = None) -> np.ndarray:
    """aq_val_mosaic_u8 in numpy, byte for byte: every output pixel from its four taps, each tap resolved to its image or to white; the
    source mosaic is not built.  images uint8 [>= n, H, W, 3] -> uint8 [ns h, ns w, 3]."""
    n, ns, H, W = geo["n"], geo["ns"], geo["H"], geo["W"]
    images = np.asarray(images)[:n]
    assert images.dtype == np.uint8 and images.shape == (n, H, W, 3)
    if xtab is None or ytab is None:
        xtab, ytab = mosaic_tables(geo)
    xtab, ytab = np.asarray(xtab, np.int64), np.asarray(ytab, np.int64)
    flat = np.concatenate([images.reshape(n * H * W, 3), np.full((1, 3), 255, np.uint8)]).astype(np.int32)   # the last row: white

    def taps(sx, sy):                                         # [out_w], [out_h] source coordinates -> int32 [out_h, out_w, 3]
        cx, cy = sx // W, sy // H
        img = cx[None, :] * ns + cy[:, None]
        idx = (img * H + (sy - cy * H)[:, None]) * W + (sx - cx * W)[None, :]
        return flat[np.where(img < n, idx, n * H * W)]

    a0, a1 = xtab[None, :, 2, None].astype(np.int32), xtab[None, :, 3, None].astype(np.int32)
    b0, b1 = ytab[:, None, 2, None].astype(np.int32), ytab[:, None, 3, None].astype(np.int32)
    r0 = taps(xtab[:, 0], ytab[:, 0]) * a0 + taps(xtab[:, 1], ytab[:, 0]) * a1
    r1 = taps(xtab[:, 0], ytab[:, 1]) * a0 + taps(xtab[:, 1], ytab[:, 1]) * a1
    out = (((b0 * (r0 >> 4)) >> 16) + ((b1 * (r1 >> 4)) >> 16) + 2) >> 2
    return np.clip(out, 0, 255).astype(np.uint8)


# ---------------------------------------------------------------- the boxes -----------------------------------------------------------------
def label_targets(lb: np.ndarray, img0_shape: Tuple[int, int], img1_shape: Tuple[int, int], stride: int = 32) -> np.ndarray:
    """One image's label rows (cls xc yc w h, normalised to the original h0 x w0 image) -> float32 [n, 5] (cls, xc, yc, w, h) in network
    pixels, by upstream's chain: the dataloader's ``xywhn2xyxy(labels, ratio_w w0, ratio_h h0, padw, padh)`` (ratio and the unrounded
    half-paddings of the letterbox that made the H x W input), ``xyxy2xywhn(w=W, h=H, clip=True, eps=1e-3)``, val.py's ``*= (W, H, W, H)``."""
    lb = np.asarray(lb, dtype=F32).reshape(-1, 5)
    (h0, w0), (H, W) = img0_shape, img1_shape
    r = min(H / h0, W / w0)
    (nw, nh), _ = letterbox_geometry((h0, w0), (H, W), True, True, stride)
    padw, padh = (W - nw) / 2, (H - nh) / 2
    sw, sh = F32(r * w0), F32(r * h0)
    x = lb[:, 1:]
    y = np.empty_like(x)
    y[:, 0] = sw * (x[:, 0] - x[:, 2] / F32(2)) + F32(padw)   # xywhn2xyxy
    y[:, 1] = sh * (x[:, 1] - x[:, 3] / F32(2)) + F32(padh)
    y[:, 2] = sw * (x[:, 0] + x[:, 2] / F32(2)) + F32(padw)
    y[:, 3] = sh * (x[:, 1] + x[:, 3] / F32(2)) + F32(padh)
    y[:, [0, 2]] = y[:, [0, 2]].clip(F32(0), F32(W - 1e-3))   # xyxy2xywhn: clip_boxes(x, (h - eps, w - eps))
    y[:, [1, 3]] = y[:, [1, 3]].clip(F32(0), F32(H - 1e-3))
    out = np.empty((lb.shape[0], 5), F32)
    out[:, 0] = lb[:, 0]
    out[:, 1] = ((y[:, 0] + y[:, 2]) / F32(2)) / F32(W)
    out[:, 2] = ((y[:, 1] + y[:, 3]) / F32(2)) / F32(H)
    out[:, 3] = (y[:, 2] - y[:, 0]) / F32(W)
    out[:, 4] = (y[:, 3] - y[:, 1]) / F32(H)
    out[:, 1:] *= np.array([W, H, W, H], F32)                 # val.py: targets[:, 2:] *= (width, height, width, height)
    return out


def pred_targets(det: np.ndarray, count: int) -> np.ndarray:
    """One image's NMS output (x1 y1 x2 y2 conf cls, network pixels) -> float32 [min(count, 300), 6] (cls, xc, yc, w, h, conf):
    output_to_target's rows of this image."""
    d = np.asarray(det, dtype=F32).reshape(-1, 6)[:max(0, min(int(count), MAX_DET))]
    out = np.empty((d.shape[0], 6), F32)
    out[:, 0] = d[:, 5]
    out[:, 1] = (d[:, 0] + d[:, 2]) / F32(2)                  # xyxy2xywh
    out[:, 2] = (d[:, 1] + d[:, 3]) / F32(2)
    out[:, 3] = d[:, 2] - d[:, 0]
    out[:, 4] = d[:, 3] - d[:, 1]
    out[:, 5] = d[:, 4]
    return out


def cell_boxes(t: np.ndarray, geo: dict, i: int) -> np.ndarray:
    """plot_images on the rows of image i (cls, xc, yc, w, h[, conf]): ``xywh2xyxy``, ``* (w, h, w, h)`` if ``boxes.max() <= 1.01`` else
    ``* scale`` when scale < 1, ``+ (x, y)``.  float32 [n, 4] in mosaic pixels."""
    t = np.asarray(t, dtype=F32)
    b = np.empty((t.shape[0], 4), F32)
    b[:, 0] = t[:, 1] - t[:, 3] / F32(2)
    b[:, 1] = t[:, 2] - t[:, 4] / F32(2)
    b[:, 2] = t[:, 1] + t[:, 3] / F32(2)
    b[:, 3] = t[:, 2] + t[:, 4] / F32(2)
    if b.shape[0]:
        if b.max() <= 1.01:
            b[:, [0, 2]] *= F32(geo["w"])
            b[:, [1, 3]] *= F32(geo["h"])
        elif geo["scale"] < 1:
            b *= F32(geo["scale"])
    x, y = geo["origins"][i]
    b[:, [0, 2]] += F32(x)
    b[:, [1, 3]] += F32(y)
    return b


# -------------------------------------------------------------- the primitives --------------------------------------------------------------
class MaskAtlas:
    """The text masks of one mosaic, back to back: every distinct (string, size, fractional start) rasterised once as ImageDraw.text does
    (``font.getmask2(text, "L", start=start)``: an 8-bit mask and its offset)."""

    def __init__(self):
        self.parts: List[np.ndarray] = []
        self.used = 0
        self.entries: Dict[tuple, tuple] = {}
        self.sizes: Dict[tuple, tuple] = {}                   # (text, size) -> getbbox's (w, h): the same at every fractional start

    def lookup(self, text: str, size: int, start=(0.0, 0.0)) -> tuple:
        """-> (w, h of ``font.getbbox(text)[2:]``, mask width, mask height, offset x, offset y, first atlas byte)."""
        key = (text, size, float(start[0]), float(start[1]))
        e = self.entries.get(key)
        if e is None:
            from PIL import Image
            font = annotate.load_font(size)
            if key[:2] not in self.sizes:
                self.sizes[key[:2]] = tuple(int(v) for v in font.getbbox(text)[2:])
            w, h = self.sizes[key[:2]]
            try:
                core, (ox, oy) = font.getmask2(text, "L", start=key[2:])
            except AttributeError:                            # the bitmap font: getmask only, no offset, no fractional start
                core, (ox, oy) = font.getmask(text, "L"), (0, 0)
            mw, mh = core.size
            if mw == 0 or mh == 0:
                mask = np.zeros((0, 0), np.uint8)
            else:
                im = Image.Image()._new(core)
                mask = np.asarray(im.convert("L") if im.mode != "L" else im, dtype=np.uint8).reshape(mh, mw)
            e = (w, h, mask.shape[1] if mask.size else 0, mask.shape[0] if mask.size else 0, int(ox), int(oy), self.used)
            self.parts.append(mask.reshape(-1))
            self.used += mask.size
            self.entries[key] = e
        return e

    def bytes(self) -> np.ndarray:
        return np.concatenate(self.parts) if self.parts else np.zeros(0, np.uint8)


def annotator_sizes(geo: dict) -> Tuple[int, int]:
    """(line width, font size) of upstream's ``Annotator(mosaic, line_width=round(fs / 10), font_size=fs, pil=True)``, with its fallbacks
    from the mosaic's size where a value is 0."""
    fs = int((geo["h"] + geo["w"]) * geo["ns"] * 0.01)
    mh, mw = geo["size"]
    return annotate.line_width(mh, mw, round(fs / 10)), fs or annotate.font_size(mh, mw)


def _trunc(v) -> np.ndarray:
    """Pillow's (int) cast of a drawing coordinate: towards zero."""
    return np.trunc(np.asarray(v, dtype=np.float64)).astype(np.int64)


def mosaic_prims(geo: dict, paths: Sequence[str], targets: Sequence[np.ndarray], names, line_width: Optional[int] = None,
                 font_size: Optional[int] = None, atlas: Optional[MaskAtlas] = None):
    """The primitives of one mosaic in drawing order -> (P: dict of PRIM_FIELDS columns, clipped to the mosaic; cell_start, cell_prims: P
    binned per 16-pixel cell for aq_annotate_u8; atlas).  targets[i]: image i's rows, float32 [k, 5] (labels: cls xc yc w h) or [k, 6]
    (predictions: + conf, drawn above 0.25 with the confidence in the text).  line_width / font_size: None = annotator_sizes(geo)."""
    n, h, w = geo["n"], geo["h"], geo["w"]
    mh, mw = geo["size"]
    lw_, fs_ = annotator_sizes(geo)
    lw = lw_ if line_width is None else int(line_width)
    fs = fs_ if font_size is None else int(font_size)
    atlas = atlas or MaskAtlas()
    # drawing items in order: (kind 0 outline only | 1 text only | 2 box with label, colour, float box, text, text position)
    boxes, colour, lws, item = [], [], [], []
    extra = {f: [] for f in postprocess.PRIM_FIELDS}
    extra_item: List[int] = []

    def add_extra(k, x0, y0, x1, y1, rgb, mask_w=0, mask=0):
        for f, v in zip(postprocess.PRIM_FIELDS, (x0, y0, x1, y1, rgb, mask_w, mask)):
            extra[f].append(int(v))
        extra_item.append(k)

    def add_text(k, x, y, text, rgb):                         # ImageDraw.text((x, y), text): int() of the position, its fraction to the rasteriser
        fx, fy = math.modf(x)[0], math.modf(y)[0]
        e = atlas.lookup(text, fs, (fx, fy))
        if e[2] > 0:
            tx, ty = int(x) + e[4], int(y) + e[5]
            add_extra(k, tx, ty, tx + e[2] - 1, ty + e[3] - 1, rgb, e[2], e[6])
        return e

    k = 0
    white = 0xFFFFFF
    for i in range(n):
        x, y = (int(v) for v in geo["origins"][i])
        boxes.append((x, y, x + w, y + h)); colour.append(white); lws.append(2); item.append(k)      # annotator.rectangle(..., width=2)
        k += 1
        if paths:
            add_text(k, x + 5, y + 5, Path(paths[i]).name[:40], NAME_RGB[0] | (NAME_RGB[1] << 8) | (NAME_RGB[2] << 16))
            k += 1
        t = np.asarray(targets[i], dtype=F32) if i < len(targets) else np.zeros((0, 5), F32)
        t = t.reshape(-1, t.shape[-1] if t.ndim == 2 else 5)
        is_labels = t.shape[1] == 5
        for j, box in enumerate(cell_boxes(t, geo, i).tolist()):
            c = int(t[j, 0])
            if not (is_labels or t[j, 5] > PLOT_CONF):
                continue
            name = names[c] if names else c
            text = f"{name}" if is_labels else f"{name} {t[j, 5]:.1f}"
            pal = postprocess.PALETTE[c % 20]
            rgb = int(pal[0]) | (int(pal[1]) << 8) | (int(pal[2]) << 16)
            boxes.append(tuple(box)); colour.append(rgb); lws.append(lw); item.append(k)
            # box_label: the filled rectangle and the text, on Pillow's float arithmetic
            tw, th = atlas.lookup(text, fs)[:2]
            outside = box[1] - th >= 0
            ty = box[1] - th if outside else box[1]
            r = _trunc([box[0], ty, box[0] + tw + 1, box[1] + 1 if outside else box[1] + th + 1])
            add_extra(k, r[0], r[1], r[2], r[3], rgb)
            add_text(k, box[0], ty, text, white)
            k += 1
    # outlines through annotation_prims (ImagingDrawRectangle's four rectangles), one call per line width; `image` carries the item number
    size1 = np.array([[mh, mw]], np.int64)
    cols = {f: [np.asarray(extra[f], np.int64)] for f in postprocess.PRIM_FIELDS}
    items = [np.asarray(extra_item, np.int64)]
    sub = [np.ones(len(extra_item), np.int64)]                # inside an item: the outline first, then rectangle and text as appended
    bx, co, lv, it = _trunc(np.asarray(boxes, np.float64).reshape(-1, 4)), np.asarray(colour, np.int64), np.asarray(lws), np.asarray(item, np.int64)
    for width in sorted(set(lws)):
        m = lv == width
        P, img = postprocess.annotation_prims(np.arange(int(m.sum())), np.zeros(int(m.sum()), np.int64), bx[m], np.tile(size1, (int(m.sum()), 1)), width)
        P["rgb"] = co[m][img]
        for f in postprocess.PRIM_FIELDS:
            cols[f].append(P[f])
        items.append(it[m][img])
        sub.append(np.zeros(img.shape[0], np.int64))
    P = {f: np.concatenate(v) for f, v in cols.items()}
    items, sub = np.concatenate(items), np.concatenate(sub)
    # clip rectangle and text primitives to the mosaic (annotation_prims has clipped its own)
    cx0, cy0 = np.maximum(P["x0"], 0), np.maximum(P["y0"], 0)
    P["mask"] = P["mask"] + (cy0 - P["y0"]) * P["mask_w"] + (cx0 - P["x0"])
    P["x0"], P["y0"], P["x1"], P["y1"] = cx0, cy0, np.minimum(P["x1"], mw - 1), np.minimum(P["y1"], mh - 1)
    keep = (P["x1"] >= P["x0"]) & (P["y1"] >= P["y0"])
    order = np.lexsort((np.arange(items.shape[0]), sub, items))
    order = order[keep[order]]
    P = {f: v[order] for f, v in P.items()}
    cell_start, cell_prims = postprocess.bin_prims(P, np.zeros(order.shape[0], np.int64), size1)
    return P, cell_start, cell_prims, atlas


def draw_numpy(mosaic: np.ndarray, P: dict, atlas_bytes: np.ndarray) -> np.ndarray:
    """aq_annotate_u8 in numpy: the primitives applied in order on a copy of the mosaic (fills; BLEND8 through the masks)."""
    out = mosaic.copy()
    for i in range(P["x0"].shape[0]):
        x0, y0, x1, y1 = (int(P[f][i]) for f in ("x0", "y0", "x1", "y1"))
        rgb = int(P["rgb"][i])
        ink = np.array([rgb & 255, (rgb >> 8) & 255, (rgb >> 16) & 255], np.uint32)
        if P["mask_w"][i] <= 0:
            out[y0:y1 + 1, x0:x1 + 1] = ink.astype(np.uint8)
        else:
            mw_, off = int(P["mask_w"][i]), int(P["mask"][i])
            rows = off + np.arange(y1 - y0 + 1)[:, None] * mw_ + np.arange(x1 - x0 + 1)[None, :]
            m = atlas_bytes[rows].astype(np.uint32)[:, :, None]
            t = out[y0:y1 + 1, x0:x1 + 1].astype(np.uint32) * (255 - m) + ink[None, None, :] * m + 128
            out[y0:y1 + 1, x0:x1 + 1] = (((t >> 8) + t) >> 8).astype(np.uint8)
    return out


# ---------------------------------------------------------------- on the device ----------------------------------------------------------------
_buffers: dict = {}


def plot_batch(tiles, paths: Sequence[str], label_tgts: Sequence[np.ndarray], pred_tgts: Sequence[np.ndarray], names, save_dir: str,
               file_names: Tuple[str, str], max_size: int = MAX_SIZE, threads: int = 2, times: Optional[dict] = None) -> dict:
    """The two mosaics of one batch: tiles uint8 CUDA [B, H, W, 3] (the network inputs), paths [B], label_tgts / pred_tgts: per image the
    rows of label_targets / pred_targets.  One aq_val_mosaic_u8 launch, two aq_annotate_u8 launches from that mosaic into two canvases, one
    aq_image_jpeg_coefs_q(75) over both, aq_write_image_files_q on host threads -> save_dir/file_names.  Returns the geometry."""
    import torch
    from . import engine
    B, H, W = int(tiles.shape[0]), int(tiles.shape[1]), int(tiles.shape[2])
    geo = mosaic_geometry(B, H, W, max_size)
    mh, mw = geo["size"]
    xtab, ytab = mosaic_tables(geo)
    drawn = []                                                # host work first: the launches then follow each other
    for tg in (label_tgts, pred_tgts):
        P, cell_start, cell_prims, atlas = mosaic_prims(geo, paths, tg, names)
        ab = atlas.bytes()
        drawn.append((postprocess.prims_array(P, engine.PRIM_DTYPE), cell_start, cell_prims, torch.from_numpy(ab).to(tiles.device) if ab.size else None))
    canvas, nbytes = engine.canvas_table([0], 3 * mw, [(mh, mw)])
    key = (tiles.device.index, 2 * nbytes)
    if key not in _buffers:
        _buffers.clear()
        _buffers[key] = (torch.empty(2 * nbytes, dtype=torch.uint8, device=tiles.device),
                         torch.empty(engine.FRAME_ARENA_MCUS * 384, dtype=torch.int16, device=tiles.device),
                         torch.empty(engine.FRAME_ARENA_MCUS * 384, dtype=torch.int16, pin_memory=True))
    out, arena, arena_host = _buffers[key]
    ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if times is not None else None
    if ev:
        ev[0].record()
    mosaic = engine.val_mosaic(tiles, geo["n"], geo["ns"], geo["h"], geo["w"], xtab, ytab)
    if ev:
        ev[1].record()
    src = mosaic.reshape(-1)
    for k, (prims, cell_start, cell_prims, atlas_dev) in enumerate(drawn):
        c = canvas.copy()
        c["dst"] = k * nbytes
        engine.annotate_images(src, c, prims, cell_start, cell_prims, atlas_dev, 2 * nbytes, out=out)
        if atlas_dev is not None:
            atlas_dev.record_stream(torch.cuda.current_stream())
    if ev:
        ev[2].record()
    table = engine.frame_table([0, nbytes], 3 * mw, [(mh, mw), (mh, mw)])
    coef, table = engine.encode_frames(out, table, arena=arena, arena_host=arena_host, quality=JPEG_QUALITY)
    if ev:
        ev[3].record()
        ev[3].synchronize()
        times["mosaic_ms"] = ev[0].elapsed_time(ev[1])
        times["annotate_ms"] = ev[1].elapsed_time(ev[2])      # both launches with their table uploads
        times["coefs_ms"] = ev[2].elapsed_time(ev[3])         # the launch(es), the read-back of the coefficients and its synchronisation
    os.makedirs(save_dir, exist_ok=True)
    engine.write_image_files(save_dir, list(file_names), coef, table, threads=threads, quality=JPEG_QUALITY)
    return geo


def release_buffers() -> None:
    """Drops plot_batch's canvases, coefficient arena and pinned arena (val.run_sweep: after the last mosaic of a sweep)."""
    _buffers.clear()


def batch_targets(dets: np.ndarray, counts: np.ndarray, labels: Sequence[np.ndarray], img0_shape, img1_shape, stride: int = 32):
    """val.py's two target lists for the first 16 images of a batch: dets [B, max_det, 6] / counts [B] as the NMS left them (after
    --single-cls has zeroed the class), labels: the images' label rows."""
    n = min(len(labels), MAX_SUBPLOTS)
    return ([label_targets(labels[i], img0_shape, img1_shape, stride) for i in range(n)],
            [pred_targets(dets[i], counts[i]) for i in range(n)])
