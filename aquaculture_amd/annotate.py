"""Label text for the annotated images: upstream's font fallback, rasterised once per string, kept in an atlas.

[UPSTREAM utils/plots.py Annotator.__init__, check_pil_font]: the font is Arial.ttf at ``max(round(sum(im.size) / 2 * 0.035), 12)``, fetched
from the network when it is missing; when that fails upstream falls back to ``ImageFont.load_default()``.  This project never fetches, so
the fallback is the font: Pillow's built-in one, at upstream's size where load_default takes a size (Pillow >= 10.1 with FreeType: Aileron),
at its only size otherwise.  Each distinct (label, size) is rasterised once, exactly as ``ImageDraw.text`` does on an RGB image
(``font.getmask2(label, "L")``: an 8-bit mask and its offset); the masks lie back to back in one byte array that aq_annotate_u8 reads.
"""
from __future__ import annotations

import threading
from typing import Dict, List, Optional, Tuple

import numpy as np


def font_size(h0: int, w0: int) -> int:
    """[UPSTREAM Annotator.__init__] ``font_size or max(round(sum(im.size) / 2 * 0.035), 12)``."""
    return max(round((w0 + h0) / 2 * 0.035), 12)


def line_width(h0: int, w0: int, line_thickness: Optional[int] = None) -> int:
    """[UPSTREAM Annotator.__init__] ``line_width or max(round(sum(im.shape) / 2 * 0.003), 2)`` (im.shape includes the 3 channels)."""
    return int(line_thickness) if line_thickness else max(round((h0 + w0 + 3) / 2 * 0.003), 2)


_fonts: Dict[int, object] = {}


def load_font(size: int):
    from PIL import ImageFont
    if size not in _fonts:
        try:
            _fonts[size] = ImageFont.load_default(size)
        except (TypeError, OSError):                      # Pillow < 10.1, or built without FreeType: the bitmap font, one size
            _fonts[size] = ImageFont.load_default()
    return _fonts[size]


def rasterise(label: str, size: int) -> Tuple[int, int, np.ndarray, int, int]:
    """(w, h) = ``font.getbbox(label)[2:]`` as box_label uses them, the 8-bit mask ImageDraw.text composites, and its (x, y) offset."""
    from PIL import Image
    font = load_font(size)
    w, h = (int(v) for v in font.getbbox(label)[2:])
    try:
        core, (ox, oy) = font.getmask2(label, "L")
    except AttributeError:                                # the bitmap font: getmask only, no offset
        core, (ox, oy) = font.getmask(label, "L"), (0, 0)
    mw, mh = core.size
    if mw == 0 or mh == 0:
        return w, h, np.zeros((0, 0), np.uint8), int(ox), int(oy)
    im = Image.Image()._new(core)
    a = np.asarray(im.convert("L") if im.mode != "L" else im, dtype=np.uint8).reshape(mh, mw)
    return w, h, a, int(ox), int(oy)


class LabelAtlas:
    """Every label string seen so far as an 8-bit mask, back to back in `self.host` (and, with a device, in `self.dev`).  lookup() is safe to
    call from several threads.  The device atlas grows by replacement: earlier buffers stay alive, a kernel in flight keeps reading its own."""

    def __init__(self, device=None, capacity: int = 1 << 20):
        self.device = device
        self.host = np.zeros(capacity, np.uint8)
        self.used = 0
        self.entries: Dict[Tuple[str, int], Tuple[int, ...]] = {}
        self.lock = threading.Lock()
        self.dev = None
        self._retired: List[object] = []
        self._synced = 0

    def lookup(self, labels: List[str], size: int) -> np.ndarray:
        """int64 [n, 7]: (w, h, mask width, mask height, offset x, offset y, first atlas byte) per label -- postprocess.annotation_prims'
        `labels`."""
        with self.lock:
            rows = []
            for lab in labels:
                e = self.entries.get((lab, size))
                if e is None:
                    w, h, mask, ox, oy = rasterise(lab, size)
                    need = self.used + mask.size
                    if need > self.host.shape[0]:
                        grown = np.zeros(max(2 * self.host.shape[0], need), np.uint8)
                        grown[:self.used] = self.host[:self.used]
                        self.host = grown
                    self.host[self.used:need] = mask.reshape(-1)
                    e = (w, h, mask.shape[1] if mask.size else 0, mask.shape[0] if mask.size else 0, ox, oy, self.used)
                    self.used = need
                    self.entries[(lab, size)] = e
                rows.append(e)
            return np.asarray(rows, dtype=np.int64).reshape(-1, 7)

    def device_atlas(self):
        """The atlas in device memory, holding every mask lookup() has returned so far (uploaded before this returns)."""
        import torch
        with self.lock:
            if self.used == 0:
                return None
            if self.dev is None or self.dev.numel() < self.host.shape[0]:
                if self.dev is not None:
                    self._retired.append(self.dev)
                self.dev = torch.zeros(self.host.shape[0], dtype=torch.uint8, device=self.device)
                self._synced = 0
            if self._synced < self.used:
                self.dev[self._synced:self.used].copy_(torch.from_numpy(self.host[self._synced:self.used]))
                torch.cuda.current_stream().synchronize()  # (rare: only when a new string appeared) other streams may read it next
                self._synced = self.used
            return self.dev
