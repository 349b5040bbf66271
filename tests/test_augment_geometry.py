"""--augment without a GPU: the pass geometry the library derives against upstream's formulas, the bilinear tap tables against
F.interpolate, the run-parameter record, and the CLI's refusal of --augment with fp8 activations
[UPSTREAM models/yolo.py DetectionModel._forward_augment, _clip_augmented; utils/torch_utils.py scale_img]."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F


def _upstream_passes(H, W, na=3):
    """The passes as upstream computes them: scale_img's sizes, the Detect rows at the padded size, then _clip_augmented."""
    from aquaculture_amd import augment
    sizes, rows = [], []
    for s in augment.SCALES:
        (h, w), (hp, wp) = augment.scale_img_sizes(H, W, s)
        if s != 1:      # restated here once more from upstream's source text
            assert (h, w) == (int(H * s), int(W * s)) and (hp, wp) == (math.ceil(H * s / 32) * 32, math.ceil(W * s / 32) * 32)
        sizes.append((h, w, hp, wp))
        rows.append(sum(na * (hp // st) * (wp // st) for st in (8, 16, 32)))
    drop0, drop2 = augment.clip_augmented(rows)
    keep = [(0, rows[0] - drop0), (0, rows[1]), (drop2, rows[2] - drop2)]
    return sizes, rows, keep


@pytest.mark.parametrize("hw", [(640, 640), (320, 320), (1280, 1280), (384, 640)])
def test_geometry_matches_upstream(lib, hw):
    from aquaculture_amd import augment
    H, W = hw
    passes, n = augment.geometry(H, W, 3)
    sizes, rows, keep = _upstream_passes(H, W)
    out = 0
    for ps, sz, r, (k0, kn), s, f in zip(passes, sizes, rows, keep, augment.SCALES, augment.FLIPS):
        assert (ps.h, ps.w, ps.hp, ps.wp) == sz
        assert ps.rows == r and (ps.keep_first, ps.keep_count) == (k0, kn) and ps.out_first == out
        assert ps.flip == (f == 3) and ps.scale == np.float32(s)
        out += kn
    assert n == out
    # with H, W multiples of 32 the clip removes exactly pass 0's P5 level and pass 2's P3 level
    p5 = lambda ps: 3 * (ps.hp // 32) * (ps.wp // 32)
    assert rows[0] - keep[0][1] == p5(passes[0]) and keep[2][0] == 16 * p5(passes[2])
    assert [ps.level_mask for ps in passes] == [3, 7, 6]


def test_geometry_640_and_the_nms_limit(lib):
    from aquaculture_amd import augment
    passes, n = augment.geometry(640, 640, 3)
    assert [(p.h, p.hp) for p in passes] == [(640, 640), (531, 544), (428, 448)]
    assert [p.keep_count for p in passes] == [24000, 18207, 2940] and n == 45147 < augment.NMS_ROW_LIMIT
    assert augment.geometry(1280, 1280, 3)[1] == 179763 >= augment.NMS_ROW_LIMIT      # yolov5x at 1280 px: refused by the engine


@pytest.mark.parametrize("size", [(531, 531), (428, 428), (200, 300)])
@pytest.mark.parametrize("flip", [False, True])
def test_taps_match_f_interpolate(lib, size, flip):
    """The tap tables, applied in numpy with the kernels' op order, reproduce F.interpolate(bilinear, align_corners=False) on random fp32
    images (flip first, then scale, as upstream) within 2 ulp of 1.0; the library builds the same tables bit for bit."""
    from aquaculture_amd import augment
    h, w = size
    g = torch.Generator().manual_seed(h * 7 + w + flip)
    x = torch.rand(2, 3, 640, 640, generator=g)
    xi = x.flip(3) if flip else x
    ref = F.interpolate(xi, size=(h, w), mode="bilinear", align_corners=False).numpy()
    ytab, xtab = augment.bilinear_taps(640, h), augment.bilinear_taps(640, w, flip)
    got = augment.apply_taps(x.numpy(), ytab, xtab)
    assert got.shape == ref.shape
    assert np.abs(got - ref).max() <= 2 * np.finfo(np.float32).eps
    for n_out, fl, tab in ((h, False, ytab), (w, flip, xtab)):
        lt = augment.library_taps(640, n_out, fl)
        assert lt.tobytes() == tab.tobytes()
        assert tab["i0"].min() >= 0 and tab["i1"].max() <= 639


def test_run_params_record_augment_only_when_set():
    from aquaculture_amd import detect
    args = ("sha", 0.25, 0.45, 1000, [640, 640], "bf16", True)
    plain = detect.run_params(*args)
    assert plain == {"weights_sha256": "sha", "conf_thres": 0.25, "iou_thres": 0.45, "max_det": 1000, "imgsz": [640, 640],
                     "precision": "bf16", "save_conf": True}           # the record of a plain run is what it always was
    aug = detect.run_params(*args, augment=True)
    assert aug == {**plain, "augment": True}


def test_resume_refuses_to_mix_augmented_and_plain(tmp_path):
    from aquaculture_amd import detect, manifest
    args = ("sha", 0.25, 0.45, 1000, [640, 640], "bf16", True)
    manifest.check_run_params(str(tmp_path), detect.run_params(*args, augment=True), resume=False)
    with pytest.raises(manifest.RunParamsMismatch):
        manifest.check_run_params(str(tmp_path), detect.run_params(*args), resume=True)


def test_augment_with_fp8_refused_before_the_gpu(tmp_path):
    from aquaculture_amd import detect
    with pytest.raises(ValueError, match="--augment does not run with --precision fp8"):
        detect.run(weights=str(tmp_path / "none.pt"), source=str(tmp_path), precision="fp8", augment=True, project=str(tmp_path), log=lambda *a: None)
    opt = detect.parse_opt(["--weights", "w.pt", "--source", "s", "--augment"])
    assert opt.augment is True
