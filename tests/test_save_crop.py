"""--save-crop, host side: the crop JPEG writer against Pillow's bytes, the crop geometry against upstream's literal torch code, the names.

The device half of the encoder (colour conversion, islow FDCT, quantisation) is restated here in numpy, as libjpeg(-turbo) does it; fed
with those coefficients, aq_crop_jpeg_bytes / aq_write_crop_files must produce exactly the file that
``Image.fromarray(rgb).save(f, quality=95, subsampling=0)`` writes [UPSTREAM utils/plots.py save_one_box].  tests/test_gpu_save_crop.py holds
the kernel to the same restatement."""
import io
import os

import numpy as np
import pytest

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63])
STD_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
                     18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99])
STD_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99, 99]
                      + [99] * 32)


def quality_table(base, quality=95):
    """jcparam.c jpeg_quality_scaling + jpeg_add_quant_table(force_baseline)."""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return np.clip((base * scale + 50) // 100, 1, 255).astype(np.int64)


def _fdct_1d(d, pass2):
    """jfdctint.c jpeg_fdct_islow, one dimension along the last axis (int64 holds every value the library's int32 arithmetic does)."""
    CB, P1 = 13, 2
    tmp0, tmp7 = d[..., 0] + d[..., 7], d[..., 0] - d[..., 7]
    tmp1, tmp6 = d[..., 1] + d[..., 6], d[..., 1] - d[..., 6]
    tmp2, tmp5 = d[..., 2] + d[..., 5], d[..., 2] - d[..., 5]
    tmp3, tmp4 = d[..., 3] + d[..., 4], d[..., 3] - d[..., 4]
    tmp10, tmp13, tmp11, tmp12 = tmp0 + tmp3, tmp0 - tmp3, tmp1 + tmp2, tmp1 - tmp2
    sh = CB + P1 if pass2 else CB - P1
    ds = lambda x: (x + (1 << (sh - 1))) >> sh
    o = np.empty_like(d)
    if pass2:
        o[..., 0] = (tmp10 + tmp11 + (1 << (P1 - 1))) >> P1
        o[..., 4] = (tmp10 - tmp11 + (1 << (P1 - 1))) >> P1
    else:
        o[..., 0] = (tmp10 + tmp11) << P1
        o[..., 4] = (tmp10 - tmp11) << P1
    z1 = (tmp12 + tmp13) * 4433
    o[..., 2] = ds(z1 + tmp13 * 6270)
    o[..., 6] = ds(z1 - tmp12 * 15137)
    z1, z2, z3, z4 = tmp4 + tmp7, tmp5 + tmp6, tmp4 + tmp6, tmp5 + tmp7
    z5 = (z3 + z4) * 9633
    tmp4, tmp5, tmp6, tmp7 = tmp4 * 2446, tmp5 * 16819, tmp6 * 25172, tmp7 * 12299
    z1, z2, z3, z4 = z1 * -7373, z2 * -20995, z3 * -16069 + z5, z4 * -3196 + z5
    o[..., 7] = ds(tmp4 + z1 + z3)
    o[..., 5] = ds(tmp5 + z2 + z4)
    o[..., 3] = ds(tmp6 + z2 + z3)
    o[..., 1] = ds(tmp7 + z1 + z4)
    return o


def reference_coefs(rgb: np.ndarray) -> np.ndarray:
    """uint8 [h, w, 3] -> int16 [ceil(h/8) ceil(w/8), 3, 64]: what libjpeg(-turbo) quantises at quality 95, 4:4:4 (block positions in raster
    order, Y / Cb / Cr, zigzag order).  Edge replication (jcprepct.c), rgb_ycc_convert (jccolor.c), level shift, islow FDCT, jcdctmgr.c
    quantisation (divisor q << 3, rounding half away from zero)."""
    h, w, _ = rgb.shape
    H, W = (h + 7) // 8 * 8, (w + 7) // 8 * 8
    p = np.pad(rgb, ((0, H - h), (0, W - w), (0, 0)), mode="edge").astype(np.int64)
    r, g, b = p[..., 0], p[..., 1], p[..., 2]
    y = (19595 * r + 38470 * g + 7471 * b + 32768) >> 16
    cb = (-11059 * r - 21709 * g + 32768 * b + (128 << 16) + 32767) >> 16
    cr = (32768 * r - 27439 * g - 5329 * b + (128 << 16) + 32767) >> 16
    planes = np.stack([y, cb, cr]) - 128                                         # [3, H, W]
    blk = planes.reshape(3, H // 8, 8, W // 8, 8).transpose(1, 3, 0, 2, 4)       # [by, bx, comp, row, col]
    blk = _fdct_1d(blk, False)                                                   # rows
    blk = _fdct_1d(blk.swapaxes(-1, -2), True).swapaxes(-1, -2)                  # columns
    blk = blk.reshape(-1, 3, 64)
    q = np.stack([quality_table(STD_LUMA), quality_table(STD_CHROMA), quality_table(STD_CHROMA)]) * 8
    a = (np.abs(blk) + (q >> 1)) // q
    out = np.where(blk < 0, -a, a)
    return out[:, :, ZIGZAG].astype(np.int16)


def pillow_bytes(rgb: np.ndarray) -> bytes:
    from PIL import Image
    f = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(rgb)).save(f, format="JPEG", quality=95, subsampling=0)
    return f.getvalue()


def _content(kind, h, w, rng):
    if kind == "random":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "flat":
        return np.broadcast_to(rng.integers(0, 256, 3, dtype=np.uint8), (h, w, 3)).copy()
    if kind == "gradient":
        yy, xx = np.mgrid[0:h, 0:w]
        return np.stack([(xx * 255 // max(w - 1, 1)), (yy * 255 // max(h - 1, 1)), ((xx + yy) * 7) % 256], -1).astype(np.uint8)
    return (rng.integers(0, 2, (h, w, 3)) * 255).astype(np.uint8)        # saturated 0 / 255


SIZES = [(1, 1), (1, 9), (9, 1), (7, 7), (8, 8), (9, 17), (37, 53), (300, 211)]
KINDS = ["random", "flat", "gradient", "saturated"]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("hw", SIZES, ids=[f"{h}x{w}" for h, w in SIZES])
def test_writer_bytes_equal_pillow(lib, hw, kind):
    from aquaculture_amd import engine
    h, w = hw
    rgb = _content(kind, h, w, np.random.default_rng(h * 1000 + w + KINDS.index(kind)))
    coef = reference_coefs(rgb)
    assert engine.crop_jpeg_bytes(coef.reshape(-1, 192), w, h) == pillow_bytes(rgb)


def test_reference_coefs_decode_back_like_pillow(lib):
    """The restatement's coefficients are Pillow's own: libjpeg reading the file Pillow wrote sees the same quantised blocks."""
    from PIL import Image
    rgb = _content("random", 21, 30, np.random.default_rng(5))
    im = Image.open(io.BytesIO(pillow_bytes(rgb)))
    assert im.mode == "RGB" and im.size == (30, 21) and im.layer == [(1, 1, 1, 0), (2, 1, 1, 1), (3, 1, 1, 1)]   # 4:4:4, tables 0 / 1 / 1
    q = im.quantization                                              # (Pillow reports the tables in natural order)
    assert list(q[0]) == quality_table(STD_LUMA).tolist() and list(q[1]) == quality_table(STD_CHROMA).tolist()


def test_write_crop_files_threads_dirs_and_truncation(lib, tmp_path):
    """aq_write_crop_files: one file per crop under directories it creates, the bytes of aq_crop_jpeg_bytes, over several threads; a second
    write of the same names truncates (a tile processed again leaves the same bytes)."""
    from aquaculture_amd import engine
    rng = np.random.default_rng(7)
    img = rng.integers(0, 256, (64, 80, 3), dtype=np.uint8)
    rects = np.array([[0, 0, 80, 64], [3, 5, 4, 6], [70, 50, 80, 64], [10, 20, 47, 33]] * 5)
    table = engine.crop_table(np.zeros(len(rects), np.int64), 80 * 3, rects)
    coef = np.concatenate([reference_coefs(img[y1:y2, x1:x2]).reshape(-1, 192) for x1, y1, x2, y2 in rects])
    assert coef.shape[0] == int(engine.crop_blocks(table).sum())
    rel = [f"crops/c{i % 3}/t{i}.jpg" for i in range(len(rects))]
    for _ in range(2):
        assert engine.write_crop_files(str(tmp_path), rel, coef, table, threads=4) == len(rects)
    for i, (x1, y1, x2, y2) in enumerate(rects):
        assert (tmp_path / rel[i]).read_bytes() == pillow_bytes(img[y1:y2, x1:x2]), i
    assert sorted(os.listdir(tmp_path / "crops")) == ["c0", "c1", "c2"]
    with pytest.raises(OSError):
        (tmp_path / "blocked").write_text("a file where a directory should be")
        engine.write_crop_files(str(tmp_path), ["blocked/x.jpg"], coef, table[:1])


def torch_save_one_box_rect(xyxy, shape):
    """The literal v7.0 code [UPSTREAM utils/plots.py save_one_box; utils/general.py xyxy2xywh, xywh2xyxy, clip_boxes], vectorised over boxes
    exactly as it runs on one: float32 tensors, one op at a time."""
    import torch
    xyxy = torch.tensor(xyxy, dtype=torch.float32).view(-1, 4)
    x = xyxy
    b = x.clone()
    b[..., 0] = (x[..., 0] + x[..., 2]) / 2
    b[..., 1] = (x[..., 1] + x[..., 3]) / 2
    b[..., 2] = x[..., 2] - x[..., 0]
    b[..., 3] = x[..., 3] - x[..., 1]
    b[:, 2:] = b[:, 2:] * 1.02 + 10
    y = b.clone()
    y[..., 0] = b[..., 0] - b[..., 2] / 2
    y[..., 1] = b[..., 1] - b[..., 3] / 2
    y[..., 2] = b[..., 0] + b[..., 2] / 2
    y[..., 3] = b[..., 1] + b[..., 3] / 2
    xyxy = y.long()
    xyxy[..., 0].clamp_(0, shape[1])
    xyxy[..., 1].clamp_(0, shape[0])
    xyxy[..., 2].clamp_(0, shape[1])
    xyxy[..., 3].clamp_(0, shape[0])
    return xyxy.numpy()


def test_crop_rects_equal_upstream_torch_code():
    from aquaculture_amd import postprocess
    rng = np.random.default_rng(11)
    n = 100_000
    H0, W0 = 1024, 768
    x = np.sort(rng.integers(0, W0 + 1, (n, 2)), 1).astype(np.float32)
    y = np.sort(rng.integers(0, H0 + 1, (n, 2)), 1).astype(np.float32)
    xyxy = np.stack([x[:, 0], y[:, 0], x[:, 1], y[:, 1]], 1)
    xyxy[: n // 10, 2] = xyxy[: n // 10, 0]                       # zero-size boxes
    xyxy[n // 10: n // 5, 3] = xyxy[n // 10: n // 5, 1]
    k = n // 5
    xyxy[k:k + 1000, 0] = 0                                         # boxes touching each edge
    xyxy[k + 1000:k + 2000, 1] = 0
    xyxy[k + 2000:k + 3000, 2] = W0
    xyxy[k + 3000:k + 4000, 3] = H0
    # .5 ties: odd widths make xc end in .5, and w * 1.02 + 10 halves that land on .5 / 0.25 fractions
    xyxy[k + 4000:k + 6000, 2] = np.minimum(xyxy[k + 4000:k + 6000, 0] + 2 * rng.integers(0, 30, 2000) + 1, W0)
    xyxy[k + 6000:k + 6100] = [[100, 100, 150, 150]]                 # w = 50: 1.02 w + 10 = 61, xc - 30.5 = 94.5
    got = postprocess.crop_rects(xyxy, H0, W0)
    want = torch_save_one_box_rect(xyxy, (H0, W0))
    assert np.array_equal(got, want), np.nonzero((got != want).any(1))[0][:5]
    assert (got[:, 2] > got[:, 0]).all() and (got[:, 3] > got[:, 1]).all()
    frac = (xyxy[:, 0] + xyxy[:, 2]) / 2 - np.floor((xyxy[:, 0] + xyxy[:, 2]) / 2)
    assert (frac == 0.5).sum() > 1000


def test_batch_crops_order_names_and_geometry():
    """Upstream's loop `for *xyxy, conf, cls in reversed(det)`: ascending confidence; per class and tile the k-th crop is <stem>k.jpg
    (no number for the first), the geometry that of the rounded, rescaled box."""
    from aquaculture_amd import postprocess
    rng = np.random.default_rng(3)
    B, M = 5, 40
    counts = np.array([0, 7, 40, 1, 23])
    det = np.zeros((B, M, 6), np.float32)
    for b in range(B):
        n = counts[b]
        xy = np.sort(rng.uniform(0, 640, (n, 2, 2)), 1)
        det[b, :n, :4] = np.stack([xy[:, 0, 0], xy[:, 0, 1], xy[:, 1, 0], xy[:, 1, 1]], 1)
        det[b, :n, 4] = np.sort(rng.uniform(0.25, 1, n))[::-1]
        det[b, :n, 5] = rng.integers(0, 4, n)
    tile, cls, rects, ordinal = postprocess.batch_crops(det, counts, (640, 640), (1024, 1024))
    assert tile.shape[0] == counts.sum()
    i = 0
    for b in range(B):
        d = det[b, :counts[b]]
        seen = {}
        for row in d[::-1]:                                         # reversed(det)
            c = int(row[5])
            seen[c] = seen.get(c, 0) + 1
            xyxy = np.rint(postprocess.scale_boxes((640, 640), row[None, :4], (1024, 1024))).astype(np.float32)
            assert tile[i] == b and cls[i] == c and ordinal[i] == seen[c]
            assert np.array_equal(rects[i], torch_save_one_box_rect(xyxy, (1024, 1024))[0])
            i += 1
    names = [postprocess.crop_file_name("t", k) for k in ordinal[tile == 2][cls[tile == 2] == cls[tile == 2][0]]]
    assert names[:3] == ["t.jpg", "t2.jpg", "t3.jpg"]
    z = postprocess.batch_crops(det, np.zeros(B, np.int64), (640, 640), (1024, 1024))
    assert all(a.shape[0] == 0 for a in z)


def test_run_params_record_save_crop_only_when_set():
    from aquaculture_amd import detect
    base = detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True)
    assert "save_crop" not in base and detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True, save_crop=False) == base
    assert detect.run_params("w", 0.25, 0.45, 1000, [640, 640], "fp32", True, save_crop=True) == dict(base, save_crop=True)
    assert "save_crop" not in detect.UNSUPPORTED
