"""Annotated images, host side: the whole-frame 4:2:0 JPEG writer against Pillow's bytes, the primitive builder against upstream's
Pillow-branch ``Annotator.box_label`` run through ImageDraw, and the new entry points' presence.

Two restatements live here.  reference_coefs_420: libjpeg(-turbo)'s pixel path at quality 95 with 2x2 chroma subsampling in numpy (what
aq_image_jpeg_coefs computes on the device; tests/test_gpu_save_img.py holds the kernel to it) -- fed to aq_image_jpeg_bytes it must give
the file ``Image.fromarray(rgb).save(f, "JPEG", quality=95, subsampling=2)`` writes, which is what ``cv2.imwrite`` of a .jpg encodes with the
same library.  pillow_box_label: upstream's drawing code, literally, on a Pillow image with the font upstream falls back to."""
import io
import os

import numpy as np
import pytest

from test_save_crop import KINDS, STD_CHROMA, STD_LUMA, ZIGZAG, _content, _fdct_1d, pillow_bytes, quality_table, reference_coefs


def reference_coefs_420(rgb: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> int16 [MCUs, 6, 64]: 16 x 16 MCUs in raster order, Y00 Y01 Y10 Y11 Cb Cr, zigzag order.  Pixels replicated to whole
    MCUs to the right and down (jcprepct.c, jcsample.c expand_right_edge), rgb_ycc_convert, h2v2_downsample (sum of four + bias 1, 2, 1, 2 ...
    along the output row, >> 2) -- the downsampled rows below the last real one repeat it (expand_bottom_edge works on the downsampled
    plane) --, level shift, islow FDCT, quantisation; Y blocks outside the component's ceil(w/8) x ceil(h/8) blocks are libjpeg's dummy
    blocks (jccoefct.c compress_data: zero, with the DC of the block before them in the MCU)."""
    h, w, _ = rgb.shape
    H, W = (h + 15) // 16 * 16, (w + 15) // 16 * 16
    p = np.pad(rgb, ((0, H - h), (0, W - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    bias = np.tile([1, 2], W // 4)[None, :]
    rows = (h + 1) // 2                                            # real downsampled rows

    def down(c):
        d = (c[0::2, 0::2] + c[0::2, 1::2] + c[1::2, 0::2] + c[1::2, 1::2] + bias) >> 2
        d[rows:] = d[rows - 1]
        return d

    def blocks(plane, q):                                          # [Hp, Wp] -> [Hp/8, Wp/8, 64] quantised, zigzag
        Hp, Wp = plane.shape
        blk = (plane - 128).reshape(Hp // 8, 8, Wp // 8, 8).transpose(0, 2, 1, 3)
        blk = _fdct_1d(blk, False)
        blk = _fdct_1d(blk.swapaxes(-1, -2), True).swapaxes(-1, -2).reshape(Hp // 8, Wp // 8, 64)
        a = (np.abs(blk) + (q * 8 >> 1)) // (q * 8)
        return np.where(blk < 0, -a, a)[..., ZIGZAG]

    ql, qc = quality_table(STD_LUMA), quality_table(STD_CHROMA)
    Y, Cb, Cr = blocks(y, ql), blocks(down(cb), qc), blocks(down(cr), qc)
    wib, hib = (w + 7) // 8, (h + 7) // 8
    out = np.zeros((H // 16, W // 16, 6, 64), np.int64)
    for my in range(H // 16):
        for mx in range(W // 16):
            m = out[my, mx]
            for i in range(2):
                for j in range(2):
                    k = 2 * i + j
                    if 2 * my + i < hib and 2 * mx + j < wib:
                        m[k] = Y[2 * my + i, 2 * mx + j]
                    elif 2 * my + i < hib:                       # dummy block at the right edge: the DC of the block to its left
                        m[k, 0] = m[k - 1, 0]
                    else:                                        # a dummy row at the bottom: the DC of the last block of the row above
                        m[k, 0] = m[1, 0]
            m[4], m[5] = Cb[my, mx], Cr[my, mx]
    return out.reshape(-1, 6, 64).astype(np.int16)


def pillow_bytes_420(rgb: np.ndarray) -> bytes:
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(f, format="JPEG", quality=95, subsampling=2)
    return f.getvalue()


SIZES = [(1, 1), (1, 9), (9, 1), (15, 17), (16, 16), (17, 33), (37, 53), (300, 211), (640, 480)]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_frame_writer_bytes_equal_pillow(lib, hw, kind):
    from aquaculture_amd import engine
    h, w = hw
    rgb = _content(kind, h, w, np.random.default_rng(h * 1000 + w + KINDS.index(kind)))
    assert engine.image_jpeg_bytes(reference_coefs_420(rgb).reshape(-1, 384), w, h) == pillow_bytes_420(rgb)


def test_restatement_decodes_back_as_pillows_file(lib):
    """Checked before it is relied on: Pillow reads our file as 4:2:0 with the quality-95 tables, and to the pixels of its own file."""
    from PIL import Image
    from aquaculture_amd import engine
    rgb = _content("random", 37, 53, np.random.default_rng(5))
    ours = engine.image_jpeg_bytes(reference_coefs_420(rgb).reshape(-1, 384), 53, 37)
    im = Image.open(io.BytesIO(ours))
    assert im.mode == "RGB" and im.size == (53, 37) and im.layer == [(1, 2, 2, 0), (2, 1, 1, 1), (3, 1, 1, 1)]
    assert list(im.quantization[0]) == quality_table(STD_LUMA).tolist() and list(im.quantization[1]) == quality_table(STD_CHROMA).tolist()
    assert np.array_equal(np.asarray(im), np.asarray(Image.open(io.BytesIO(pillow_bytes_420(rgb)))))


def test_crop_writer_bytes_unchanged(lib):
    """The 4:4:4 entry points share the coder with the frames now; their bytes are what they were."""
    from aquaculture_amd import engine
    rgb = _content("random", 37, 53, np.random.default_rng(37 * 1000 + 53))
    assert engine.crop_jpeg_bytes(reference_coefs(rgb).reshape(-1, 192), 53, 37) == pillow_bytes(rgb)


def test_write_image_files_threads_and_truncation(lib, tmp_path):
    from aquaculture_amd import engine
    rng = np.random.default_rng(9)
    ims = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(40, 56), (16, 16), (1, 1), (33, 17)] * 3]
    table = engine.frame_table(np.zeros(len(ims), np.int64), [3 * im.shape[1] for im in ims], [im.shape[:2] for im in ims])
    coef = np.concatenate([reference_coefs_420(im).reshape(-1, 384) for im in ims])
    assert coef.shape[0] == int(engine.frame_mcus(table).sum())
    rel = [f"t{i}.jpg" for i in range(len(ims))]
    for _ in range(2):
        assert engine.write_image_files(str(tmp_path), rel, coef, table, threads=4) == len(ims)
    for i, im in enumerate(ims):
        assert (tmp_path / rel[i]).read_bytes() == pillow_bytes_420(im), i
    with pytest.raises(OSError):
        (tmp_path / "blocked").write_text("a file where a directory should be")
        engine.write_image_files(str(tmp_path), ["blocked/x.jpg"], coef, table[:1])


# ---- drawing ----

UPSTREAM_HEX = ("FF3838", "FF9D97", "FF701F", "FFB21D", "CFD231", "48F90A", "92CC17", "3DDB86", "1A9334", "00D4BB",
                "2C99A8", "00C2FF", "344593", "6473FF", "0018EC", "8438FF", "520085", "CB38FF", "FF95C8", "FF37C7")


def upstream_color(i):
    """[UPSTREAM utils/plots.py Colors.__call__ / hex2rgb], bgr=False: the image here is RGB."""
    h = "#" + UPSTREAM_HEX[int(i) % len(UPSTREAM_HEX)]
    return tuple(int(h[1 + k:1 + k + 2], 16) for k in (0, 2, 4))


def pillow_box_label(rgb, boxes, classes, labels, lw):
    """[UPSTREAM utils/plots.py Annotator, pil=True] literally: __init__'s font size with the ImageFont.load_default fallback of
    check_pil_font, then box_label per detection, in the order given.  labels[i] = '' or None: no label (--hide-labels)."""
    from PIL import Image, ImageDraw, ImageFont
    im = Image.fromarray(np.ascontiguousarray(rgb))
    draw = ImageDraw.Draw(im)
    size = max(round(sum(im.size) / 2 * 0.035), 12)
    try:
        font = ImageFont.load_default(size)
    except TypeError:
        font = ImageFont.load_default()
    for box, c, label in zip(boxes, classes, labels):
        box = [int(v) for v in box]
        color, txt_color = upstream_color(c), (255, 255, 255)
        draw.rectangle(box, width=lw, outline=color)  # box
        if label:
            _, _, w, h = font.getbbox(label)  # text width, height
            outside = box[1] - h >= 0  # label fits outside box
            draw.rectangle((box[0], box[1] - h if outside else box[1], box[0] + w + 1, box[1] + 1 if outside else box[1] + h + 1), fill=color)
            draw.text((box[0], box[1] - h if outside else box[1]), label, fill=txt_color, font=font)
    return np.asarray(im)


def numpy_painter(rgb, prims, cell_start, cell_prims, atlas, cell0=0):
    """What aq_annotate_u8 does, cell by cell: every pixel applies the primitives of its cell in order."""
    out = rgb.astype(np.int64)
    h, w, _ = rgb.shape
    cw = (w + 15) // 16
    for cy in range((h + 15) // 16):
        for cx in range(cw):
            c = cell0 + cy * cw + cx
            for pi in cell_prims[cell_start[c]:cell_start[c + 1]]:
                p = prims[pi]
                x0, x1 = max(int(p["x0"]), 16 * cx), min(int(p["x1"]), 16 * cx + 15, w - 1)
                y0, y1 = max(int(p["y0"]), 16 * cy), min(int(p["y1"]), 16 * cy + 15, h - 1)
                if x1 < x0 or y1 < y0:
                    continue
                ink = np.array([int(p["rgb"]) & 255, (int(p["rgb"]) >> 8) & 255, (int(p["rgb"]) >> 16) & 255])
                if p["mask_w"] == 0:
                    out[y0:y1 + 1, x0:x1 + 1] = ink
                else:
                    yy, xx = np.mgrid[y0:y1 + 1, x0:x1 + 1]
                    m = atlas[int(p["mask"]) + (yy - int(p["y0"])) * int(p["mask_w"]) + (xx - int(p["x0"]))].astype(np.int64)[..., None]
                    t = out[y0:y1 + 1, x0:x1 + 1] * (255 - m) + ink * m + 128
                    out[y0:y1 + 1, x0:x1 + 1] = ((t >> 8) + t) >> 8
    return out.astype(np.uint8)


NAMES = ["circle_farms", "square_farms", "é-ponton", "net pens", "raft"]


def build(rgb, boxes, classes, confs, lw, hide_labels=False, hide_conf=False, atlas=None):
    """The project's path for one image: label strings, atlas lookup, primitives, bins."""
    from aquaculture_amd import annotate, engine, postprocess
    h, w, _ = rgb.shape
    atlas = atlas or annotate.LabelAtlas()
    labels = None
    if not hide_labels:
        labels = atlas.lookup(postprocess.label_strings([NAMES[i % len(NAMES)] for i in range(100)], classes, confs, hide_conf), annotate.font_size(h, w))
    P, img = postprocess.annotation_prims(np.zeros(len(boxes), np.int64), classes, boxes, [(h, w)], lw, labels)
    cs, cp = postprocess.bin_prims(P, img, [(h, w)])
    return postprocess.prims_array(P, engine.PRIM_DTYPE), cs, cp, atlas


def want_labels(classes, confs, hide_labels, hide_conf):
    """[UPSTREAM detect.py] label = None if hide_labels else (names[c] if hide_conf else f'{names[c]} {conf:.2f}')."""
    return [None if hide_labels else (NAMES[int(c) % len(NAMES)] if hide_conf else f"{NAMES[int(c) % len(NAMES)]} {float(v):.2f}")
            for c, v in zip(classes, confs)]


def edge_cases(S):
    """(boxes, classes, confs) the issue lists: each edge, a corner at W / H, one-pixel and thinner-than-lw boxes, nested and overlapping boxes
    of different classes, labels that do not fit above their box, class indices above 20."""
    boxes = [(0, 100, 80, 180), (100, 0, 200, 60), (S - 90, 200, S, 300), (200, S - 70, 330, S),        # touching each edge; corners at W / H
             (S - 40, S - 40, S, S), (0, 0, S, S),
             (300, 300, 300, 300), (310, 300, 311, 301), (320, 300, 322, 340), (330, 300, 400, 303), (350, 320, 351, 320),   # one pixel; thinner than lw
             (120, 120, 420, 420), (150, 150, 390, 390), (200, 200, 300, 300), (250, 130, 500, 260), (260, 10, 380, 200),   # nested, overlapping
             (S - 60, 5, S - 2, 50), (400, 3, 470, 90), (S - 3, S - 3, S - 1, S - 1), (5, 40, 60, 41)]         # label does not fit above / runs off the right edge
    classes = np.array([0, 1, 2, 3, 4, 21, 22, 23, 44, 79, 20, 0, 1, 2, 3, 4, 25, 39, 61, 19])
    confs = np.linspace(0.25, 0.995, len(boxes)).astype(np.float32)
    return np.array(boxes, np.int64), classes, confs


@pytest.mark.parametrize("S", [640, 1024])
@pytest.mark.parametrize("lw,hide_labels,hide_conf", [(3, False, False), (1, False, False), (3, True, False), (3, False, True), (1, True, True)])
def test_primitives_equal_upstream_box_label(S, lw, hide_labels, hide_conf):
    rgb = _content("random", S, S, np.random.default_rng(S + lw))
    boxes, classes, confs = edge_cases(S)
    prims, cs, cp, atlas = build(rgb, boxes, classes, confs, lw, hide_labels, hide_conf)
    got = numpy_painter(rgb, prims, cs, cp, atlas.host)
    want = pillow_box_label(rgb, boxes, classes, want_labels(classes, confs, hide_labels, hide_conf), lw)
    assert np.array_equal(got, want), np.argwhere((got != want).any(2))[:5]
    assert (got != rgb).any()


def test_two_font_sizes_and_non_square_image():
    from aquaculture_amd import annotate
    assert annotate.font_size(640, 640) == 22 and annotate.font_size(1024, 1024) == 36 and annotate.font_size(100, 120) == 12
    rgb = _content("gradient", 333, 517, np.random.default_rng(1))
    boxes = np.array([(10, 30, 200, 120), (480, 300, 517, 333), (0, 0, 30, 10)], np.int64)
    classes, confs = np.array([3, 7, 30]), np.array([0.5, 0.875, 0.999], np.float32)
    prims, cs, cp, atlas = build(rgb, boxes, classes, confs, 2)
    got = numpy_painter(rgb, prims, cs, cp, atlas.host)
    assert np.array_equal(got, pillow_box_label(rgb, boxes, classes, want_labels(classes, confs, False, False), 2))


def test_batch_boxes_order_and_rounding():
    """`for *xyxy, conf, cls in reversed(det)` on `scale_boxes(...).round()`, per tile."""
    from aquaculture_amd import postprocess
    rng = np.random.default_rng(3)
    B, M = 4, 30
    counts = np.array([0, 5, 30, 1])
    det = np.zeros((B, M, 6), np.float32)
    for b in range(B):
        n = counts[b]
        xy = np.sort(rng.uniform(0, 640, (n, 2, 2)), 1)
        det[b, :n, :4] = np.stack([xy[:, 0, 0], xy[:, 0, 1], xy[:, 1, 0], xy[:, 1, 1]], 1)
        det[b, :n, 4] = np.sort(rng.uniform(0.25, 1, n))[::-1]
        det[b, :n, 5] = rng.integers(0, 4, n)
    tile, cls, conf, xyxy = postprocess.batch_boxes(det, counts, (640, 640), (1024, 1024))
    i = 0
    for b in range(B):
        for row in det[b, :counts[b]][::-1]:
            want = np.rint(postprocess.scale_boxes((640, 640), row[None, :4], (1024, 1024))).astype(np.int64)[0]
            assert tile[i] == b and cls[i] == int(row[5]) and conf[i] == row[4] and np.array_equal(xyxy[i], want)
            i += 1
    assert i == tile.shape[0]
    assert all(a.shape[0] == 0 for a in postprocess.batch_boxes(det, np.zeros(B, np.int64), (640, 640), (1024, 1024)))


def test_bins_hold_each_primitive_once_per_cell_in_order():
    from aquaculture_amd import postprocess
    rng = np.random.default_rng(4)
    sizes = [(100, 70), (33, 200)]
    n = 200
    image = np.sort(rng.integers(0, 2, n))
    xy = np.stack([rng.integers(-20, 220, n), rng.integers(-20, 120, n), rng.integers(-20, 220, n), rng.integers(-20, 120, n)], 1)
    xy = np.stack([xy[:, [0, 2]].min(1), xy[:, [1, 3]].min(1), xy[:, [0, 2]].max(1), xy[:, [1, 3]].max(1)], 1)
    P, img = postprocess.annotation_prims(image, rng.integers(0, 50, n), xy, sizes, 2)
    cs, cp = postprocess.bin_prims(P, img, sizes)
    cells = sum(((h + 15) // 16) * ((w + 15) // 16) for h, w in sizes)
    assert cs.shape[0] == cells + 1 and cs[-1] == cp.shape[0]
    first = 0
    for i, (h, w) in enumerate(sizes):
        cw = (w + 15) // 16
        for c in range(((h + 15) // 16) * cw):
            cy, cx = divmod(c, cw)
            touching = [k for k in range(img.shape[0]) if img[k] == i and P["x0"][k] <= 16 * cx + 15 and P["x1"][k] >= 16 * cx
                        and P["y0"][k] <= 16 * cy + 15 and P["y1"][k] >= 16 * cy]
            assert cp[cs[first + c]:cs[first + c + 1]].tolist() == touching
        first += ((h + 15) // 16) * cw
    assert (P["x0"] >= 0).all() and (P["y0"] >= 0).all() and (P["x1"] < np.asarray(sizes)[img, 1]).all() and (P["y1"] < np.asarray(sizes)[img, 0]).all()


def test_run_params_record_image_saving_only_when_set():
    from aquaculture_amd import detect
    base = detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)
    assert detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True, save_img=None) == base
    got = detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True, save_img=(3, False, True))
    assert got == dict(base, save_img=True, line_thickness=3, hide_labels=False, hide_conf=True)


def test_new_symbols_are_exported_and_bound(lib):
    """Fails without the feature: the library exports the drawing and whole-frame entry points, and engine.py binds them."""
    import ctypes
    from aquaculture_amd import engine
    for name in ("aq_annotate_u8", "aq_image_jpeg_coefs", "aq_image_jpeg_bytes", "aq_write_image_files"):
        assert name in engine.EXPORTS and hasattr(lib, name), name
        assert getattr(lib, name).argtypes is not None, name
    assert lib.aq_image_jpeg_bytes.restype is ctypes.c_long and lib.aq_write_image_files.restype is ctypes.c_long
    header = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aq_engine.h")).read()
    assert all(s in header for s in ("aq_annotate_u8(", "aq_image_jpeg_coefs(", "typedef struct aq_prim", "typedef struct aq_frame"))
    assert engine.PRIM_DTYPE.itemsize == 32 and engine.CANVAS_DTYPE.itemsize == 40 and engine.FRAME_DTYPE.itemsize == 24
