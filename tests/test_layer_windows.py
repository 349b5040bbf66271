"""The harness of tests/test_gpu_bench_layers.py, checked without a GPU: the windowed fp64 conv reference (oracle/windowed_ref.py) equals
F.conv2d on the whole image, the window picker covers what it promises, the comparator names a single corrupted element, and every
shipped tuned table has an entry in the layer-by-layer test."""
import json
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import windowed_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("k,stride", [(1, 1), (3, 1), (3, 2), (1, 2)])
@pytest.mark.parametrize("H,Wd", [(21, 17), (16, 16)])
def test_windowed_conv_equals_full_conv(k, stride, H, Wd):
    g = torch.Generator().manual_seed(k * 10 + stride + H)
    B, cin, cout, pad = 3, 5, 7, k // 2
    x = torch.randn(B, H, Wd, cin, generator=g, dtype=torch.float64)
    w = torch.randn(cout, k, k, cin, generator=g, dtype=torch.float64)
    b = torch.randn(cout, generator=g, dtype=torch.float64)
    full = F.silu(F.conv2d(x.permute(0, 3, 1, 2), w.permute(0, 3, 1, 2), b, stride=stride, padding=pad)).permute(0, 2, 3, 1)
    res = torch.randn_like(full)
    Ho, Wo = full.shape[1:3]
    wins = W.pick_windows(B, Ho, Wo, [0, 1, 2], bn=13, size=4, seam=(1, 2), max_frac=1.0)
    tags = {w_.tag.split(":")[0].split(" n0")[0] for w_ in wins}
    assert {"corner top-left", "corner bottom-right", "edge top", "edge right", "seam", "tile boundary", "interior 0"} <= tags, tags
    for w_ in wins:
        r = W.input_region(w_, k, stride, pad, H, Wd)
        assert 0 <= r.y0 < r.y1 <= H and 0 <= r.x0 < r.x1 <= Wd and min(r.pad) >= 0
        # a window's cut is never padded: only a window on the image border has padding on that side
        assert (r.pad[0] > 0) <= (w_.y0 == 0) and (r.pad[2] > 0) <= (w_.x0 == 0)
        got = W.conv_window(x[w_.image, r.y0:r.y1, r.x0:r.x1], r, w, b, stride, True, res=res[w_.image, w_.y0:w_.y1, w_.x0:w_.x1])
        want = full[w_.image, w_.y0:w_.y1, w_.x0:w_.x1] + res[w_.image, w_.y0:w_.y1, w_.x0:w_.x1]
        torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-12, msg=str(w_))


@pytest.mark.parametrize("bn", [64, 128, 256, 512, 1000])
def test_window_picker_covers_corners_edges_seams_and_tile_boundaries(bn):
    B, Ho, Wo, size = 16, 80, 80, 8
    images = [0, 7, 8, 15]
    wins = W.pick_windows(B, Ho, Wo, images, bn=bn, size=size, seam=(7, 8))
    for img in images:
        mine = [w for w in wins if w.image == img]
        assert all(w.y1 - w.y0 == size and w.x1 - w.x0 == size and 0 <= w.y0 and w.y1 <= Ho and 0 <= w.x0 and w.x1 <= Wo for w in mine)

        def covered(y, x):
            return any(w.y0 <= y < w.y1 and w.x0 <= x < w.x1 for w in mine)
        for y, x in [(0, 0), (0, Wo - 1), (Ho - 1, 0), (Ho - 1, Wo - 1), (0, Wo // 2), (Ho - 1, Wo // 2), (Ho // 2, 0), (Ho // 2, Wo - 1)]:
            assert covered(y, x), (img, y, x)
        # both pixels on either side of every picked tile boundary, and one boundary inside each image that has one
        lo = img * Ho * Wo
        starts = [n0 for n0 in range(0, B * Ho * Wo, bn) if lo < n0 < lo + Ho * Wo]
        tiles = [w for w in mine if w.tag.startswith("tile boundary")]
        assert bool(tiles) == bool(starts)
        for w in tiles:
            n0 = int(w.tag.split("=")[1].split("x")[0]) * bn
            assert n0 in starts
            a, b = divmod(n0 - 1 - lo, Wo), divmod(n0 - lo, Wo)
            assert covered(*a) and covered(*b), (img, n0, w)
        if starts:
            assert any(int(w.tag.split("=")[1].split("x")[0]) * bn == starts[-1] for w in tiles)   # the image's last tile boundary
        assert sum(w.tag.startswith("interior") for w in mine) == 2
    assert any(w.image == 7 and w.tag.startswith("seam") and w.y1 == Ho for w in wins)
    assert any(w.image == 8 and w.tag.startswith("seam") and w.y0 == 0 for w in wins)
    # a small plane (yolov5x's 40 x 40 level at 1280 px): the windows would cover most of it, so the whole plane is checked
    small = W.pick_windows(B, 20, 20, [3], bn=bn, size=size)
    assert small == [W.Window(3, 0, 20, 0, 20, "whole plane")]
    # deterministic
    assert W.pick_windows(B, Ho, Wo, images, bn=bn, size=size, seam=(7, 8)) == wins


def test_comparator_flags_one_corrupted_element():
    g = torch.Generator().manual_seed(3)
    ref = torch.randn(16, 8, 8, 32, generator=g, dtype=torch.float64)
    got = ref.float().double()
    ok, *_ = W.compare(got, ref, 2e-5, 2e-5)
    assert ok
    bn = 128
    for where in [(0, 0, 0, 5), (15, 7, 7, 31), np.unravel_index(3 * bn, (16, 8, 8)) + (0,)]:   # corners of the first / last image, a tile start
        bad = got.clone()
        bad[tuple(where)] += 1e-3
        ok, mx, _, k, ratio = W.compare(bad, ref, 2e-5, 2e-5)
        assert not ok and tuple(k) == tuple(int(i) for i in where) and ratio > 1 and mx == pytest.approx(1e-3, rel=1e-3)
        bad[tuple(where)] = float("nan")
        ok, _, _, k, _ = W.compare(bad, ref, 2e-5, 2e-5)
        assert not ok and tuple(k) == tuple(int(i) for i in where)


def test_every_shipped_tuned_table_has_a_layer_check():
    """Each key of aquaculture_amd/data/tuned_tables.json maps to exactly one CONFIGS entry of test_gpu_bench_layers.py that installs
    the shipped table, and that entry's plan has the key's op count: a table added later without a layer check fails here."""
    import test_gpu_bench_layers as L
    from aquaculture_amd import spec
    with open(os.path.join(ROOT, "aquaculture_amd", "data", "tuned_tables.json")) as f:
        keys = list(json.load(f))
    covered = {}
    for key in keys:
        m = re.match(r"(\w+):nc(\d+):p(\w+):(\d+)x(\d+)x(\d+):n\d+:v\d+:ops(\d+)$", key)
        assert m, key
        variant, _, prec, B, H, Wd, nops = m.groups()
        ids = [cid for cid, c in L.CONFIGS.items() if c.tuning == "shipped table" and
               (c.variant, c.precision, c.batch, c.size, c.size) == (variant, prec, int(B), int(H), int(Wd))]
        assert len(ids) == 1, f"tuned table {key}: layer-check entries {ids}"
        c = L.CONFIGS[ids[0]]
        plan = spec.build_plan(c.variant, 5, 3, fused_stem=True, fused_bottleneck=c.precision in ("bf16", "fp8w", "fp8"))
        assert len(plan.ops) == int(nops), (key, ids[0], len(plan.ops))
        covered[key] = ids[0]
    print(covered)
    assert sorted(c for c, e in L.CONFIGS.items() if e.tuning == "shipped table") == sorted(covered.values())
    assert [c for c, e in L.CONFIGS.items() if e.tuning != "shipped table"] == ["parity_fp32", "fp32_b128", "bf16_b448"]
    assert L.CONFIGS["parity_fp32"].tuning is None and L.CONFIGS["fp32_b128"].tuning is None and L.CONFIGS["bf16_b448"].tuning is None
    assert set(L.FAMILIES) == set(L.CONFIGS)                   # every entry pins the kernel families its ops launch
    for cid, e in L.CONFIGS.items():
        assert 0 < e.ragged < e.batch and e.ragged % 2 == 1, cid
        assert e.sample[0] == 0 and e.sample[-1] == e.batch - 1, cid

