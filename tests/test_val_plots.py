"""val.py --plots on the host: the mosaic grid against a transcription of upstream's lines, mosaic_numpy against "paste, then resize" (the
host resize and the oracle's C resize), and the primitives against a literal Pillow restatement of plot_images, pixel for pixel."""
import ctypes as C
import math
import os
import subprocess
from pathlib import Path

import numpy as np
import pytest
from PIL import Image, ImageDraw

from aquaculture_amd import annotate, dataloader, postprocess, val, val_plots

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F32 = np.float32
NAMES = {0: "circle_farm", 1: "square_farm", 2: "barge", 3: "raft", 4: "net"}


# ---- upstream, transcribed ----

def geometry_literal(bs, h, w, max_size=1920, max_subplots=16):
    """[UPSTREAM plot_images] the lines between ``bs, _, h, w = images.shape`` and the Annotator."""
    bs = min(bs, max_subplots)
    ns = np.ceil(bs ** 0.5)
    mosaic_shape = (int(ns * h), int(ns * w))
    origins = []
    for i in range(bs):
        x, y = int(w * (i // ns)), int(h * (i % ns))
        origins.append((x, y))
    scale = max_size / ns / max(h, w)
    H, W = h, w
    if scale < 1:
        h = math.ceil(scale * h)
        w = math.ceil(scale * w)
        out_shape = (int(ns * h), int(ns * w))                                  # cv2.resize(mosaic, tuple(int(x * ns) for x in (w, h)))
    else:
        out_shape = mosaic_shape
    fs = int((h + w) * ns * 0.01)
    return int(ns), h, w, scale, origins, mosaic_shape, out_shape, fs


class LiteralAnnotator:
    """[UPSTREAM utils/plots.py Annotator, pil=True], the font being annotate.load_font's."""

    def __init__(self, im, line_width=None, font_size=None):
        self.im = Image.fromarray(im)
        self.draw = ImageDraw.Draw(self.im)
        self.font = annotate.load_font(font_size or max(round(sum(self.im.size) / 2 * 0.035), 12))
        self.lw = line_width or max(round(sum(im.shape) / 2 * 0.003), 2)

    def box_label(self, box, label="", color=(128, 128, 128), txt_color=(255, 255, 255)):
        self.draw.rectangle(box, width=self.lw, outline=color)
        if label:
            w, h = self.font.getbbox(label)[2:]
            outside = box[1] - h >= 0
            self.draw.rectangle((box[0], box[1] - h if outside else box[1], box[0] + w + 1, box[1] + 1 if outside else box[1] + h + 1), fill=color)
            self.draw.text((box[0], box[1] - h if outside else box[1]), label, fill=txt_color, font=self.font)

    def rectangle(self, xy, fill=None, outline=None, width=1):
        self.draw.rectangle(xy, fill, outline, width)

    def text(self, xy, text, txt_color=(255, 255, 255)):
        self.draw.text(xy, text, fill=txt_color, font=self.font)


def colors(c):
    return tuple(int(v) for v in postprocess.PALETTE[int(c) % 20])


def xywh2xyxy(x):
    y = np.copy(x)
    y[..., 0] = x[..., 0] - x[..., 2] / 2
    y[..., 1] = x[..., 1] - x[..., 3] / 2
    y[..., 2] = x[..., 0] + x[..., 2] / 2
    y[..., 3] = x[..., 1] + x[..., 3] / 2
    return y


def xyxy2xywh(x):
    y = np.copy(x)
    y[..., 0] = (x[..., 0] + x[..., 2]) / 2
    y[..., 1] = (x[..., 1] + x[..., 3]) / 2
    y[..., 2] = x[..., 2] - x[..., 0]
    y[..., 3] = x[..., 3] - x[..., 1]
    return y


def xywhn2xyxy(x, w=640, h=640, padw=0, padh=0):
    y = np.copy(x)
    y[..., 0] = w * (x[..., 0] - x[..., 2] / 2) + padw
    y[..., 1] = h * (x[..., 1] - x[..., 3] / 2) + padh
    y[..., 2] = w * (x[..., 0] + x[..., 2] / 2) + padw
    y[..., 3] = h * (x[..., 1] + x[..., 3] / 2) + padh
    return y


def xyxy2xywhn(x, w=640, h=640, clip=False, eps=0.0):
    if clip:
        x[..., [0, 2]] = x[..., [0, 2]].clip(0, w - eps)                        # clip_boxes(x, (h - eps, w - eps))
        x[..., [1, 3]] = x[..., [1, 3]].clip(0, h - eps)
    y = np.copy(x)
    y[..., 0] = ((x[..., 0] + x[..., 2]) / 2) / w
    y[..., 1] = ((x[..., 1] + x[..., 3]) / 2) / h
    y[..., 2] = (x[..., 2] - x[..., 0]) / w
    y[..., 3] = (x[..., 3] - x[..., 1]) / h
    return y


def label_chain_literal(lb, h0, w0, H, W, stride=32):
    """The dataloader's and val.py's lines for one image's labels -> rows (cls, x, y, w, h) in network pixels."""
    r = min(H / h0, W / w0)
    ratio = (r, r)
    (nw, nh), _ = dataloader.letterbox_geometry((h0, w0), (H, W), True, True, stride)
    pad = ((W - nw) / 2, (H - nh) / 2)
    labels = np.array(lb, dtype=np.float32).reshape(-1, 5)
    if labels.size:
        labels[:, 1:] = xywhn2xyxy(labels[:, 1:], ratio[0] * w0, ratio[1] * h0, padw=pad[0], padh=pad[1])
    if len(labels):
        labels[:, 1:5] = xyxy2xywhn(labels[:, 1:5], w=W, h=H, clip=True, eps=1e-3)
    labels[:, 1:] *= np.array((W, H, W, H), np.float32)
    return labels


def output_to_target_literal(output, max_det=300):
    targets = []
    for i, o in enumerate(output):
        o = np.asarray(o, np.float32).reshape(-1, 6)[:max_det]
        box, conf, cls = o[:, :4], o[:, 4:5], o[:, 5:6]
        j = np.full((conf.shape[0], 1), i, np.float32)
        targets.append(np.concatenate((j, cls, xyxy2xywh(box), conf), 1))
    return np.concatenate(targets, 0)


def plot_images_literal(mosaic, bs, H, W, targets, paths, fname, names, max_size=1920):
    """[UPSTREAM plot_images] from the Annotator on, `mosaic` being the pasted (and resized) uint8 mosaic."""
    ns, h, w, scale, _, _, _, fs = geometry_literal(bs, H, W, max_size)
    bs = min(bs, 16)
    annotator = LiteralAnnotator(mosaic, line_width=round(fs / 10), font_size=fs)
    for i in range(bs):
        x, y = int(w * (i // ns)), int(h * (i % ns))
        annotator.rectangle([x, y, x + w, y + h], None, (255, 255, 255), width=2)
        if paths:
            annotator.text([x + 5, y + 5], text=Path(paths[i]).name[:40], txt_color=(220, 220, 220))
        if len(targets) > 0:
            ti = targets[targets[:, 0] == i]
            boxes = xywh2xyxy(ti[:, 2:6]).T
            classes = ti[:, 1].astype("int")
            labels = ti.shape[1] == 6
            conf = None if labels else ti[:, 6]
            if boxes.shape[1]:
                if boxes.max() <= 1.01:
                    boxes[[0, 2]] *= w
                    boxes[[1, 3]] *= h
                elif scale < 1:
                    boxes *= scale
            boxes[[0, 2]] += x
            boxes[[1, 3]] += y
            for j, box in enumerate(boxes.T.tolist()):
                cls = classes[j]
                color = colors(cls)
                cls = names[cls] if names else cls
                if labels or conf[j] > 0.25:
                    label = f"{cls}" if labels else f"{cls} {conf[j]:.1f}"
                    annotator.box_label(box, label, color=color)
    if fname:
        annotator.im.save(fname)
    return np.asarray(annotator.im)


def stack_targets(per_image):
    """Per-image rows (cls, x, y, w, h[, conf]) -> upstream's target array with the image index in front."""
    k = per_image[0].shape[1] if per_image else 5
    return np.concatenate([np.concatenate([np.full((t.shape[0], 1), i, F32), t.astype(F32)], 1) for i, t in enumerate(per_image)]
                          + [np.zeros((0, k + 1), F32)], 0)


# ---- the grid ----

SHAPES = ((640, 640), (384, 640), (640, 384), (24, 40), (17, 23))


@pytest.mark.parametrize("n", (1, 2, 3, 4, 5, 9, 10, 16, 17))
@pytest.mark.parametrize("hw", SHAPES)
def test_geometry_is_upstreams(n, hw):
    H, W = hw
    ns = math.ceil(math.sqrt(min(n, 16)))
    at_one = ns * max(H, W)                                                     # scale == 1 exactly
    for max_size in (1920, at_one - 1, at_one, at_one + 1, max(at_one // 2, 1), 3 * at_one):
        g = val_plots.mosaic_geometry(n, H, W, max_size)
        ns_, h, w, scale, origins, mosaic_shape, out_shape, fs = geometry_literal(n, H, W, max_size)
        assert (g["n"], g["ns"], g["h"], g["w"], g["scale"]) == (min(n, 16), ns_, h, w, scale)
        assert g["resized"] == (scale < 1) and g["src_size"] == mosaic_shape and g["size"] == out_shape
        assert [tuple(o) for o in g["src_origins"].tolist()] == origins
        assert [tuple(o) for o in g["origins"].tolist()] == [(int(w * (i // ns_)), int(h * (i % ns_))) for i in range(min(n, 16))]
        lw, size = val_plots.annotator_sizes(g)
        assert lw == (round(fs / 10) or max(round((out_shape[0] + out_shape[1] + 3) / 2 * 0.003), 2))
        assert size == (fs or max(round((out_shape[0] + out_shape[1]) / 2 * 0.035), 12))
    assert val_plots.mosaic_geometry(n, H, W, at_one - 1)["resized"] and not val_plots.mosaic_geometry(n, H, W, at_one)["resized"]


# ---- mosaic_numpy against paste, then resize ----

def paste(images, geo):
    H, W, ns = geo["H"], geo["W"], geo["ns"]
    m = np.full((ns * H, ns * W, 3), 255, np.uint8)
    for i in range(geo["n"]):
        x, y = geo["src_origins"][i]
        m[y:y + H, x:x + W] = images[i]
    return m


def oracle_lib():
    subprocess.run(["make", "-s", "-C", os.path.join(ROOT, "oracle")], check=True)
    return C.CDLL(os.path.join(ROOT, "oracle", "_build", "libref_kernels.so"))


def oracle_resize(lib, im, nh, nw):
    im = np.ascontiguousarray(im)
    out = np.empty((nh, nw, 3), np.uint8)
    lib.ref_resize_linear_u8(im.ctypes.data_as(C.c_void_p), im.shape[0], im.shape[1], 3, out.ctypes.data_as(C.c_void_p), nh, nw)
    return out


def boundary_blends(geo):
    """Per inner cell boundary of the source mosaic, the output columns (rows) whose two taps lie on both sides with both weights non-zero."""
    xtab, ytab = val_plots.mosaic_tables(geo)
    out = {}
    for axis, tab, size in (("x", xtab, geo["W"]), ("y", ytab, geo["H"])):
        for k in range(1, geo["ns"]):
            out[(axis, k)] = np.nonzero((tab[:, 0] == k * size - 1) & (tab[:, 1] == k * size) & (tab[:, 2] > 0) & (tab[:, 3] > 0))[0]
    return out


# (n, H, W, max_size) -- upstream's geometry -- or (n, H, W, (h, w)) -- cells of a given size --: odd widths, four white cells (n = 5 on
# 3 x 3), one white column (n = 2), a paste.  Upstream's geometry shrinks by exactly W / w on a grid whose cell edges map onto each other,
# and then no tap pair straddles a cell edge (val_plots.cell_geometry); the cases with cells LARGER than the images have ratios that put
# a tap pair across every cell boundary in both directions (asserted below), the blend the kernel has to get right.
MOSAIC_CASES = ((5, 17, 23, 62), (5, 24, 40, 100), (2, 17, 23, 37), (2, 24, 40, 71), (3, 24, 40, 71), (9, 17, 23, 62), (16, 17, 23, 83),
                (10, 24, 40, 141), (5, 24, 40, 1920), (1, 17, 23, 20), (4, 17, 23, 46),
                (5, 17, 23, (18, 25)), (5, 24, 40, (29, 47)), (2, 17, 23, (18, 24)), (2, 24, 40, (29, 50)), (9, 17, 23, (21, 33)),
                (16, 17, 23, (18, 26)), (10, 24, 40, (25, 41)), (3, 24, 40, (31, 43)))
BLEND_CASES = tuple(c for c in MOSAIC_CASES if isinstance(c[3], tuple))


def case_id(c):
    return "n%d_%dx%d_" % c[:3] + ("m%d" % c[3] if isinstance(c[3], int) else "cells%dx%d" % c[3])


def case_geometry(c):
    return val_plots.mosaic_geometry(*c) if isinstance(c[3], int) else val_plots.cell_geometry(*c[:3], *c[3])


def case_images(n, H, W, seed=0):
    rng = np.random.default_rng(1000 * n + H + seed)
    im = rng.integers(0, 256, (n, H, W, 3), dtype=np.uint8)
    im[:, :, -1] = rng.integers(0, 60, (n, H, 3), dtype=np.uint8)               # dark last columns and rows: a blend with white or the neighbour shows
    im[:, -1] = rng.integers(0, 60, (n, W, 3), dtype=np.uint8)
    return im


@pytest.fixture(scope="module")
def oracle():
    return oracle_lib()


@pytest.mark.parametrize("case", MOSAIC_CASES, ids=case_id)
def test_mosaic_numpy_is_paste_then_resize(case, oracle):
    n, H, W = case[:3]
    geo = case_geometry(case)
    images = case_images(n, H, W)
    got = val_plots.mosaic_numpy(images, geo)
    src = paste(images, geo)
    oh, ow = geo["size"]
    assert got.shape == (oh, ow, 3)
    if geo["resized"]:
        assert got.tobytes() == dataloader.resize_linear_u8(src, ow, oh).tobytes()
        assert got.tobytes() == oracle_resize(oracle, src, oh, ow).tobytes()
    else:
        assert got.tobytes() == src.tobytes()
        assert got.tobytes() == dataloader.resize_linear_u8(src, ow, oh).tobytes()      # (the identity tables)


@pytest.mark.parametrize("case", BLEND_CASES, ids=case_id)
def test_the_cases_blend_across_every_cell_boundary(case):
    """A condition on the inputs: per cell boundary, in both directions, one output pixel blends two images and (where a white cell lies
    there) one blends an image with white."""
    n, H, W = case[:3]
    geo = case_geometry(case)
    assert geo["resized"]
    ns = geo["ns"]
    xtab, ytab = val_plots.mosaic_tables(geo)
    cell = lambda cx, cy: cx * ns + cy
    two_images = image_white = 0
    for (axis, k), hits in boundary_blends(geo).items():
        assert hits.size, (axis, k)
        for other in range(ns):                                                 # the cells on both sides of boundary k, along the other axis
            a, b = (cell(k - 1, other), cell(k, other)) if axis == "x" else (cell(other, k - 1), cell(other, k))
            two_images += a < n and b < n
            image_white += (a < n) != (b < n)
    assert two_images >= 1 and (image_white >= 1 or n == ns * ns)
    # and the pixels show it: a mosaic of constant images takes values between two images', and between an image's and white
    flat = np.stack([np.full((H, W, 3), 10 + 12 * i, np.uint8) for i in range(n)])
    m = val_plots.mosaic_numpy(flat, geo)
    values = set(np.unique(m).tolist()) - ({255} | {10 + 12 * i for i in range(n)})
    assert any(v < 10 + 12 * (n - 1) for v in values) and (n == ns * ns or any(v > 10 + 12 * (n - 1) for v in values))


def test_upstreams_geometry_never_straddles_a_cell_edge():
    """Why the blend cases are not upstream's own sizes: with ratios W / w >= 1 on aligned cell edges the two taps of a pixel share a cell."""
    for n, H, W in ((5, 17, 23), (16, 24, 40), (16, 640, 640), (9, 384, 640)):
        ns = math.ceil(math.sqrt(n))
        for max_size in (ns * max(H, W) - 1, ns * max(H, W) * 3 // 4, ns * max(H, W) // 2, ns * max(H, W) // 3):
            geo = val_plots.mosaic_geometry(n, H, W, max_size)
            assert geo["resized"] and all(v.size == 0 for v in boundary_blends(geo).values())


def test_mosaic_numpy_takes_only_the_first_sixteen():
    geo = val_plots.mosaic_geometry(17, 17, 23, 83)
    images = case_images(17, 17, 23)
    assert geo["n"] == 16
    assert val_plots.mosaic_numpy(images, geo).tobytes() == val_plots.mosaic_numpy(images[:16], geo).tobytes()


# ---- boxes and primitives against Pillow ----

def plot_case(n, H, W, h0, w0, seed):
    """Labels (normalised to the original h0 x w0) and NMS outputs (network pixels) of n images with the edge cases of the issue."""
    rng = np.random.default_rng(seed)
    labels, dets, counts = [], [], []
    for i in range(n):
        k = int(rng.integers(1, 5))
        c = rng.uniform(0.15, 0.85, (k, 2))
        wh = rng.uniform(0.05, 0.4, (k, 2))
        lb = np.concatenate([rng.integers(0, 5, (k, 1)), c, wh], 1).astype(F32)
        lb = np.concatenate([lb, np.array([[1, 0.01, 0.01, 0.02, 0.02],         # at the cell's corner (clipped at 0)
                                           [2, 0.99, 0.99, 0.02, 0.02],         # at the opposite corner (clipped at W - eps, H - eps)
                                           [3, 0.5, 0.04, 0.3, 0.08]], F32)])   # at the top: the label text goes inside in the first row of cells
        labels.append(lb)
        m = int(rng.integers(2, 7))
        xy = rng.uniform(0, [W, H], (m, 2))
        sz = rng.uniform(2, [W / 2, H / 2], (m, 2))
        d = np.concatenate([xy - sz / 2, xy + sz / 2, rng.uniform(0.05, 0.95, (m, 1)), rng.integers(0, 5, (m, 1))], 1).astype(F32)
        d = np.concatenate([d, np.array([[-6.5, -3.25, 8.75, 6.5, 0.9, 1],               # leaves the cell to the left and the top (negative fractions)
                                         [W - 7.5, H - 5.5, W + 9.25, H + 7.75, 0.8, 2],  # into the neighbours (or the white, or off the mosaic)
                                         [0.0, 0.0, W, H, 0.7, 3],                        # the whole cell, corner to corner
                                         [3.5, 1.5, W / 2, H / 2, 0.25, 4],               # conf 0.25 exactly: not drawn
                                         [3.5, 1.5, W / 2, H / 2, 0.2500001, 0]], F32)])  # just above: drawn
        dets.append(d)
        counts.append(d.shape[0])
    labels[1 % n] = np.zeros((0, 5), F32)                                       # an image without labels
    many = np.concatenate([np.tile(np.array([[2.0, 2.0, 6.0, 6.0, 0.1, 0]], F32), (300, 1)),
                           np.array([[1.0, 1.0, W - 1.0, H - 1.0, 0.99, 1]], F32)])              # the 301st row would be drawn
    dets[n - 1], counts[n - 1] = many, 301
    paths = [f"/data/set/images/tile_{i:03d}.jpg" for i in range(n)]
    paths[0] = "/data/set/images/" + "a_long_name_of_forty_five_characters_0123456.jpg"[:41] + ".jpg"
    assert len(Path(paths[0]).name) == 45
    return labels, dets, counts, paths


# (n, H, W, original size, max_size): real sizes with and without the resize (fs = 20), and tiny ones where fs is 0 and both Annotator
# fallbacks apply, or fs is 1 and the line width falls back alone
PRIM_CASES = ((4, 384, 640, (768, 1280), 1920), (5, 640, 640, (1024, 1024), 1000), (5, 24, 40, (48, 80), 60), (5, 24, 40, (24, 40), 1920),
              (3, 17, 23, (34, 46), 40), (2, 640, 384, (1000, 600), 1920))


@pytest.mark.parametrize("case", PRIM_CASES, ids=lambda c: "n%d_%dx%d_m%d" % (c[0], c[1], c[2], c[4]))
def test_prims_draw_what_pillow_draws(case, tmp_path):
    n, H, W, (h0, w0), max_size = case
    geo = val_plots.mosaic_geometry(n, H, W, max_size)
    rng = np.random.default_rng(5)
    mosaic = rng.integers(0, 256, (*geo["size"], 3), dtype=np.uint8)
    labels, dets, counts, paths = plot_case(n, H, W, h0, w0, seed=n + H)
    ltg =[val_plots.label_targets(lb, (h0, w0), (H, W)) for lb in labels]
    ptg = [val_plots.pred_targets(d, c) for d, c in zip(dets, counts)]
    # the two chains against upstream's lines
    for lb, t in zip(labels, ltg):
        assert t.tobytes() == label_chain_literal(lb, h0, w0, H, W).astype(F32).tobytes()
    want_p = output_to_target_literal(dets)
    assert np.concatenate(ptg).tobytes() == want_p[:, 1:].astype(F32).tobytes() and ptg[-1].shape[0] == 300
    fs = geometry_literal(n, H, W, max_size)[7]
    if H <= 24:
        assert round(fs / 10) == 0                                              # the line-width fallback (and the font's where fs == 0)
    for name, tg, want_t in (("labels", ltg, stack_targets(ltg)), ("pred", ptg, want_p)):
        P, cell_start, cell_prims, atlas = val_plots.mosaic_prims(geo, paths, tg, NAMES)
        got = val_plots.draw_numpy(mosaic, P, atlas.bytes())
        want = plot_images_literal(mosaic.copy(), n, H, W, want_t, paths, str(tmp_path / f"{name}.jpg"), NAMES, max_size)
        assert got.shape == want.shape
        bad = np.argwhere((got != want).any(2))
        assert bad.size == 0, (name, bad[:5].tolist())
        assert (got != mosaic).any()
        # the cell table holds every primitive in every cell it touches, ascending
        cw = (geo["size"][1] + 15) // 16
        for c in range(cell_start.shape[0] - 1):
            ids = cell_prims[cell_start[c]:cell_start[c + 1]]
            assert np.all(np.diff(ids) > 0)
            x0, y0 = 16 * (c % cw), 16 * (c // cw)
            touch = (P["x0"] <= x0 + 15) & (P["x1"] >= x0) & (P["y0"] <= y0 + 15) & (P["y1"] >= y0)
            assert np.array_equal(np.nonzero(touch)[0], ids)


def test_undrawn_predictions_leave_no_primitive():
    geo = val_plots.mosaic_geometry(1, 384, 640, 1920)
    low = np.array([[10, 10, 100, 100, 0.25, 1], [20, 20, 90, 90, 0.1, 2]], F32)
    P0 = val_plots.mosaic_prims(geo, [], [val_plots.pred_targets(low, 2)], NAMES)[0]
    P1 = val_plots.mosaic_prims(geo, [], [np.zeros((0, 6), F32)], NAMES)[0]
    assert P0["x0"].shape[0] == P1["x0"].shape[0] == 4                          # the cell's border alone


# ---- the flag ----

def test_plots_flag_parses():
    base = ["--data", "d.yaml", "--weights", "w.pt"]
    assert val.parse_opt(base).plots == 0
    assert val.parse_opt(base + ["--plots"]).plots == 3
    assert val.parse_opt(base + ["--plots", "1"]).plots == 1
    val.check_opt(val.parse_opt(base + ["--plots", "--single-cls", "--confusion-matrix", "--save-txt", "--precision", "fp8"]))


def test_plots_is_refused_on_saved_detections():
    with pytest.raises(SystemExit, match="--plots"):
        val.check_opt(val.parse_opt(["--data", "d.yaml", "--labels", "runs/labels", "--cpu", "--plots"]))
    with pytest.raises(SystemExit, match="--plots"):
        val.check_opt(val.parse_opt(["--data", "d.yaml", "--weights", "w.pt", "--plots", "-1"]))
