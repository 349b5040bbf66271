"""Test-time augmentation (``detect.py --augment``) [UPSTREAM models/yolo.py DetectionModel._forward_augment].

Upstream runs three passes over the letterboxed float image ``x`` (B, 3, H, W) and concatenates their clipped, de-scaled Detect outputs::

    s = [1, 0.83, 0.67]; f = [None, 3, None]                       # scales, flips (3 = left-right)
    xi = scale_img(x.flip(f) if f else x, s, gs=32)               # [UPSTREAM utils/torch_utils.py scale_img]
    yi = forward_once(xi)[0]; yi = _descale_pred(yi, f, s, img_size)
    y = _clip_augmented(y); return torch.cat(y, 1)

The engine does all of it on the device (``Engine.infer(..., augment=True)``); the pass geometry comes from the C library
(``aq_augment_geometry``), the one place it is derived.  This module restates upstream's formulas -- the reference the tests hold the
library's geometry and the kernels' tap tables to -- and wraps the C geometry for the Python side.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import List, NamedTuple

import numpy as np

SCALES = (1, 0.83, 0.67)     # [UPSTREAM _forward_augment: s]
FLIPS = (None, 3, None)      # [UPSTREAM _forward_augment: f]; 3 = flip the width axis
GS = 32                      # [UPSTREAM scale_img(gs=32)]
PAD_VALUE = 0.447            # [UPSTREAM scale_img: F.pad(img, ..., value=0.447)  # value = imagenet mean]
NMS_ROW_LIMIT = 1 << 17      # aq_nms: fewer rows per image than this (include/aq_engine.h)


class Pass(NamedTuple):
    scale: float
    flip: bool
    h: int; w: int               # interpolated size
    hp: int; wp: int             # padded network input
    rows: int                    # rows of the pass's Detect output
    keep_first: int; keep_count: int
    out_first: int               # first row of the concatenation the kept rows fill
    level_mask: int


class _CPass(C.Structure):
    _fields_ = [("scale", C.c_float), ("flip", C.c_int32), ("h", C.c_int32), ("w", C.c_int32), ("hp", C.c_int32), ("wp", C.c_int32),
                ("rows", C.c_int32), ("keep_first", C.c_int32), ("keep_count", C.c_int32), ("out_first", C.c_int32), ("level_mask", C.c_int32)]


class _CTap(C.Structure):
    _fields_ = [("i0", C.c_int32), ("i1", C.c_int32), ("l0", C.c_float), ("l1", C.c_float)]


# --------------------------------------------------------------------------------------
# upstream's formulas, restated
# --------------------------------------------------------------------------------------
def scale_img_sizes(h: int, w: int, ratio: float, gs: int = GS):
    """[UPSTREAM scale_img]: ((interpolated h, w), (padded h, w)); ratio 1.0 returns the image as it is."""
    if ratio == 1.0:
        return (h, w), (h, w)
    s = (int(h * ratio), int(w * ratio))
    return s, tuple(math.ceil(x * ratio / gs) * gs for x in (h, w))


def clip_augmented(rows: List[int], nl: int = 3):
    """[UPSTREAM _clip_augmented] on the passes' row counts: (rows dropped from the end of pass 0, rows dropped from the start of the last)."""
    g = sum(4 ** x for x in range(nl))
    e = 1
    i0 = (rows[0] // g) * sum(4 ** x for x in range(e))
    i2 = (rows[-1] // g) * sum(4 ** (nl - 1 - x) for x in range(e))
    return i0, i2


def bilinear_taps(n_in: int, n_out: int, flip: bool = False) -> np.ndarray:
    """Taps of F.interpolate(mode='bilinear', align_corners=False) along one axis, in PyTorch's CPU fp32 arithmetic
    [UPSTREAM aten/src/ATen/native/UpSample.h area_pixel_compute_source_index, cpu/UpSampleKernel.cpp compute_indices_weights_linear]:
    src = max(fma(float(in) / out, d + 0.5, -0.5), 0); i0 = int(src); i1 = i0 + (i0 < in - 1); l1 = src - i0; l0 = 1 - l1.
    ``flip``: the source indices mirrored (in - 1 - i), i.e. the taps of the flipped image.  Returns the aq_tap records (i0, i1, l0, l1)
    as a structured array whose bytes are what aq_stem_conv_scaled reads."""
    f32 = np.float32
    scale = f32(n_in) / f32(n_out)
    d = np.arange(n_out, dtype=np.float32)
    # one rounding for scale * (d + 0.5) - 0.5: PyTorch's CPU build contracts it into a fused multiply-add (the float64 product of two
    # float32 values is exact, and so is the subtraction of 0.5 from it)
    src = np.maximum((np.float64(scale) * (d + f32(0.5)).astype(np.float64) - 0.5).astype(np.float32), f32(0))
    i0 = src.astype(np.int32)
    i1 = i0 + (i0 < n_in - 1).astype(np.int32)
    l1 = np.clip(src - i0.astype(np.float32), f32(0), f32(1))
    l0 = f32(1) - l1
    if flip:
        i0, i1 = n_in - 1 - i0, n_in - 1 - i1
    out = np.empty(n_out, dtype=[("i0", "<i4"), ("i1", "<i4"), ("l0", "<f4"), ("l1", "<f4")])
    out["i0"], out["i1"], out["l0"], out["l1"] = i0, i1, l0, l1
    return out


def apply_taps(img: np.ndarray, ytab: np.ndarray, xtab: np.ndarray) -> np.ndarray:
    """float32 (..., H, W) -> (..., h, w): h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11), every step rounded to fp32 (what the kernels compute)."""
    r0, r1 = img[..., ytab["i0"], :], img[..., ytab["i1"], :]
    w0, w1 = xtab["l0"], xtab["l1"]
    t0 = w0 * r0[..., xtab["i0"]] + w1 * r0[..., xtab["i1"]]
    t1 = w0 * r1[..., xtab["i0"]] + w1 * r1[..., xtab["i1"]]
    return (ytab["l0"][:, None] * t0 + ytab["l1"][:, None] * t1).astype(np.float32)


# --------------------------------------------------------------------------------------
# the library's geometry (the one used to run)
# --------------------------------------------------------------------------------------
def geometry(H: int, W: int, na: int = 3):
    """The three passes of an H x W tile and N_aug, the rows per image of the augmented prediction (aq_augment_geometry)."""
    from .engine import load_library, _check
    lib = load_library()
    passes = (_CPass * 3)()
    n = C.c_int()
    _check(lib.aq_augment_geometry(H, W, na, passes, C.byref(n)))
    return [Pass(float(p.scale), bool(p.flip), p.h, p.w, p.hp, p.wp, p.rows, p.keep_first, p.keep_count, p.out_first, p.level_mask)
            for p in passes], int(n.value)


def library_taps(n_in: int, n_out: int, flip: bool = False) -> np.ndarray:
    """aq_augment_taps: the taps the engine's augmented call builds (on the device, with the same arithmetic)."""
    from .engine import load_library, _check
    lib = load_library()
    buf = (_CTap * n_out)()
    _check(lib.aq_augment_taps(n_in, n_out, int(bool(flip)), buf))
    out = np.empty(n_out, dtype=[("i0", "<i4"), ("i1", "<i4"), ("l0", "<f4"), ("l1", "<f4")])
    C.memmove(out.ctypes.data, buf, out.nbytes)
    return out
