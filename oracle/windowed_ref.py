"""Windowed fp64 references for convolutions too large to check whole (yolov5x at 1280 px): a conv's output is checked on small windows
of output pixels, each computed from just the input region it reads.  CPU only; used by tests/test_gpu_bench_layers.py, checked against
F.conv2d on whole images by tests/test_layer_windows.py.

A window is (image, y0, y1, x0, x1, tag) in output pixels, half-open.  Its input region is what a k x k / stride s / pad p conv reads for
those outputs, clipped to the image: the part that falls outside the image is zero padding (true image borders); nothing is padded at
the window's own cut.
"""
from typing import List, NamedTuple, Optional, Sequence

import numpy as np
import torch
import torch.nn.functional as F


class Window(NamedTuple):
    image: int
    y0: int
    y1: int
    x0: int
    x1: int
    tag: str


class Region(NamedTuple):
    """Input rows [y0, y1) and columns [x0, x1) inside the image, and the zero padding (top, bottom, left, right) beyond its borders."""
    y0: int
    y1: int
    x0: int
    x1: int
    pad: tuple


def pick_windows(B: int, Ho: int, Wo: int, images: Sequence[int], bn: Optional[int] = None, size: int = 8, seam: Sequence[int] = (),
                 n_interior: int = 2, seed: int = 0, max_frac: float = 0.25) -> List[Window]:
    """Windows of about size x size output pixels on each of `images` (of a batch of B images of Ho x Wo outputs): the four corners, the
    middle of each edge, at least one window holding a boundary between two pixel tiles of `bn` pixels (tile n0 = k * bn of the flattened
    [B, Ho, Wo] pixel range, as the implicit-GEMM and halo kernels walk it) on every image that has one, and `n_interior` seeded interior
    windows.  `seam` = (a, a + 1): image a's last rows and image a + 1's first rows.  Where the windows would cover more than `max_frac`
    of the plane, one window is the whole plane."""
    hs, ws = min(size, Ho), min(size, Wo)
    out: List[Window] = []
    for img in images:
        per = []

        def add(y, x, tag):
            y0 = min(max(y, 0), Ho - hs)
            x0 = min(max(x, 0), Wo - ws)
            per.append(Window(img, y0, y0 + hs, x0, x0 + ws, tag))
        add(0, 0, "corner top-left"); add(0, Wo, "corner top-right"); add(Ho, 0, "corner bottom-left"); add(Ho, Wo, "corner bottom-right")
        add(0, (Wo - ws) // 2, "edge top"); add(Ho, (Wo - ws) // 2, "edge bottom")
        add((Ho - hs) // 2, 0, "edge left"); add((Ho - hs) // 2, Wo, "edge right")
        if len(seam) == 2 and img == seam[0]:
            add(Ho, Wo // 3, f"seam: last rows of image {img}")
        if len(seam) == 2 and img == seam[1]:
            add(0, Wo // 3, f"seam: first rows of image {img}")
        if bn:
            plane = Ho * Wo
            lo, hi = img * plane, (img + 1) * plane
            ks = list(range(-(-lo // bn), -(-hi // bn)))               # tiles starting inside this image
            ks = [k for k in ks if k * bn != lo] or ks                  # (the image's first pixel is a corner already)
            if ks:
                for k in sorted({ks[len(ks) // 2], ks[-1]}):            # one mid-image boundary and the image's last one
                    y, x = divmod(k * bn - lo, Wo)
                    # the pixels (y, x - 1) and (y, x) on either side of the boundary; at a row start, (y - 1, Wo - 1) and (y, 0)
                    add(y - hs // 2, x - ws // 2, f"tile boundary n0 = {k} x {bn}")
                    if x == 0:
                        add(y - 1 - hs // 2, Wo, f"tile boundary n0 = {k} x {bn} (previous row's end)")
        rng = np.random.default_rng(seed * 7919 + img)
        for q in range(n_interior):
            add(int(rng.integers(1, max(Ho - hs, 1) + 1)), int(rng.integers(1, max(Wo - ws, 1) + 1)), f"interior {q}")
        covered = np.zeros((Ho, Wo), bool)
        for w in per:
            covered[w.y0:w.y1, w.x0:w.x1] = True
        if covered.sum() > max_frac * Ho * Wo:
            per = [Window(img, 0, Ho, 0, Wo, "whole plane")]
        out += per
    return out


def input_region(w: Window, k: int, stride: int, pad: int, H: int, W: int) -> Region:
    """The input a k x k / stride / pad conv reads for output window w, clipped to the H x W image, and the zero padding past it."""
    ry0, ry1 = w.y0 * stride - pad, (w.y1 - 1) * stride - pad + k
    rx0, rx1 = w.x0 * stride - pad, (w.x1 - 1) * stride - pad + k
    cy0, cy1, cx0, cx1 = max(ry0, 0), min(ry1, H), max(rx0, 0), min(rx1, W)
    return Region(cy0, cy1, cx0, cx1, (cy0 - ry0, ry1 - cy1, cx0 - rx0, rx1 - cx1))


def conv_window(x_region: torch.Tensor, region: Region, w_krsc: torch.Tensor, bias, stride: int, act: bool,
                res: Optional[torch.Tensor] = None, scale: Optional[torch.Tensor] = None, dtype=torch.float64) -> torch.Tensor:
    """fp64 conv of one window: x_region [rh, rw, cin] the input region's values (as the kernel reads them), w_krsc [cout, k, k, cin]
    the values the kernel multiplies; res [wh, ww, cout] the residual on the window; scale a per-Cout factor (fp8 consumers).
    Returns [wh, ww, cout] float64 = res + SiLU(scale * conv + bias) (dtype float32: the same computed in fp32)."""
    x = x_region.to(dtype).permute(2, 0, 1)[None]
    t, b_, l, r = region.pad
    x = F.pad(x, (l, r, t, b_))
    w = torch.as_tensor(w_krsc).to(dtype).permute(0, 3, 1, 2)
    y = F.conv2d(x, w, None, stride=stride)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1)
    y = y + torch.as_tensor(bias).to(dtype).view(1, -1, 1, 1)
    if act:
        y = F.silu(y)
    y = y[0].permute(1, 2, 0)
    if res is not None:
        y = y + res.to(dtype)
    return y


def compare(got: torch.Tensor, ref: torch.Tensor, rel: float, abs_: float):
    """(ok, max err, mean err, index of the worst element, its ratio to the bound) of |got - ref| against rel |ref| + abs_."""
    err = (got.double() - ref).abs()
    ratio = err / (rel * ref.abs() + abs_)
    ratio = torch.where(torch.isnan(ratio), torch.full_like(ratio, float("inf")), ratio)
    k = np.unravel_index(int(torch.argmax(ratio)), tuple(ratio.shape))
    return bool((ratio <= 1).all()), float(err.max()), float(err.mean()), tuple(int(i) for i in k), float(ratio.max())
