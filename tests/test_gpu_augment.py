"""--augment on the GPU engine against upstream's augmented forward restated on the CPU oracle
[UPSTREAM models/yolo.py DetectionModel._forward_augment]: F.interpolate / flip / F.pad, OracleModel.forward, _descale_pred,
_clip_augmented and torch.cat, then non_max_suppression unchanged."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _match(dets, counts, ref_list, box_tol, conf_tol):
    """tests/test_gpu_engine.py::_match, restated: same number of boxes per tile and a one-to-one pairing (same class) within tolerance."""
    for b, ref in enumerate(ref_list):
        n = int(counts[b])
        assert n == ref.shape[0], f"tile {b}: {n} boxes vs oracle {ref.shape[0]}"
        got = dets[b, :n]
        assert np.all(np.diff(got[:, 4]) <= 0), f"tile {b}: confidences not descending"
        used = np.zeros(n, bool)
        for r in ref:
            d = np.abs(got[:, :4] - r[:4]).max(1) / box_tol + np.abs(got[:, 4] - r[4]) / conf_tol
            d[used | (got[:, 5] != r[5])] = np.inf
            j = int(np.argmin(d))
            assert np.abs(got[j, :4] - r[:4]).max() <= box_tol and abs(got[j, 4] - r[4]) <= conf_tol, \
                f"tile {b}: oracle box {r} has no engine match (closest {got[j]})"
            used[j] = True


def scaled_input(x, ps, W):
    """[UPSTREAM scale_img(x.flip(3) if flip else x, s, gs=32)] on float (B, 3, H, W)."""
    from aquaculture_amd import augment
    xi = x.flip(3) if ps.flip else x
    if ps.scale == 1.0:
        return xi
    xi = F.interpolate(xi, size=(ps.h, ps.w), mode="bilinear", align_corners=False)
    return F.pad(xi, [0, ps.wp - ps.w, 0, ps.hp - ps.h], value=augment.PAD_VALUE)


def oracle_augmented_pred(m, tiles_u8, na=3):
    """model(im, augment=True) on the oracle: the three passes de-scaled, clipped, concatenated."""
    from aquaculture_amd import augment
    from oracle import yolov5_oracle as O
    x = O.preprocess(tiles_u8)
    H, W = x.shape[2:]
    passes, n = augment.geometry(H, W, na)
    ys = []
    for ps, s in zip(passes, augment.SCALES):
        y = m.forward(scaled_input(x, ps, W))
        y[..., :4] /= s                                             # [UPSTREAM _descale_pred]
        if ps.flip:
            y[..., 0] = W - y[..., 0]
        ys.append(y)
    drop0, drop2 = augment.clip_augmented([y.shape[1] for y in ys])  # [UPSTREAM _clip_augmented]
    ys[0] = ys[0][:, :-drop0]
    ys[-1] = ys[-1][:, drop2:]
    out = torch.cat(ys, 1)
    assert out.shape[1] == n
    return out


@pytest.fixture(scope="module")
def tiles_640():
    from aquaculture_amd import tiles
    return tiles.synthetic_batch([0, 1, 2], 640)


@pytest.fixture(scope="module")
def ref_fp32(synth_ck, tiles_640):
    from oracle import yolov5_oracle as O
    return oracle_augmented_pred(O.model_from_checkpoint(synth_ck), tiles_640)


# ---- kernels -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pass_i", [1, 2])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stem_scaled_matches_reference(lib, pass_i, flip, precision):
    """aq_stem_conv_scaled against F.conv2d on the reference scaled image (both scales, both flips; the 531 / 544 and 428 / 448 borders
    fall inside the compared output)."""
    from aquaculture_amd import augment, engine
    ps = augment.geometry(640, 640)[0][pass_i]._replace(flip=flip)
    g = torch.Generator().manual_seed(pass_i * 2 + flip)
    x = torch.randint(0, 256, (2, 640, 640, 3), generator=g, dtype=torch.uint8)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    b = torch.randn(48, generator=g) * 0.1
    xin = scaled_input(x.permute(0, 3, 1, 2).float() / 255, ps, 640)
    wq = w
    if precision == "bf16":
        xin, wq = xin.bfloat16().float(), w.bfloat16().float()
    ref = F.silu(F.conv2d(xin, wq, b, stride=2, padding=2)).permute(0, 2, 3, 1).contiguous()
    out = engine.stem_conv_scaled_nhwc(x.cuda(), w, b, ps.h, ps.w, ps.hp, ps.wp, flip, precision=precision).cpu().float()
    assert out.shape == ref.shape == (2, ps.hp // 2, ps.wp // 2, 48)
    if precision == "fp32":
        assert (out - ref).abs().max().item() <= 1e-5
    else:
        torch.testing.assert_close(out, ref.bfloat16().float(), rtol=2 ** -7, atol=1e-3)


@pytest.mark.parametrize("pass_i", [1, 2])
@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_preprocess_s2d_scaled_matches_reference(lib, pass_i, flip, precision):
    """aq_preprocess_s2d_scaled (yolov5x's path) against the reference scaled image in space-to-depth order; bf16: the fp32 sample rounded
    once to nearest even, so against the bf16-rounded reference within one bf16 step (a sample within 2 fp32 ulp of a rounding tie may
    round the other way), nearly all of them equal."""
    from aquaculture_amd import augment, engine
    ps = augment.geometry(640, 640)[0][pass_i]._replace(flip=flip)
    g = torch.Generator().manual_seed(7 + 2 * pass_i + flip)
    x = torch.randint(0, 256, (2, 640, 640, 3), generator=g, dtype=torch.uint8)
    xin = scaled_input(x.permute(0, 3, 1, 2).float() / 255, ps, 640)                       # (B, 3, hp, wp)
    ref = F.pixel_unshuffle(xin, 2)                                                        # (B, 3*4, hp/2, wp/2): c*4 + dy*2 + dx
    ref = ref.view(2, 3, 2, 2, ps.hp // 2, ps.wp // 2).permute(0, 4, 5, 2, 3, 1).reshape(2, ps.hp // 2, ps.wp // 2, 12)
    out = engine.preprocess_s2d_scaled(x.cuda(), ps.h, ps.w, ps.hp, ps.wp, flip, precision).cpu()
    assert out.shape == (2, ps.hp // 2, ps.wp // 2, 16)
    assert (out[..., 12:] == 0).all()
    if precision == "fp32":
        assert out.dtype == torch.float32
        assert (out[..., :12] - ref).abs().max().item() <= 2 * np.finfo(np.float32).eps
    else:
        assert out.dtype == torch.bfloat16
        got, want = out[..., :12].float(), ref.bfloat16().float()
        assert ((got - want).abs() <= 2 ** -7 * want.abs()).all()        # one bf16 step: 2^-7 of the value's binade
        assert (got == want).float().mean().item() >= 0.999


def test_detect_decode_aug_matches_descaled_oracle(lib, synth_ck):
    """aq_detect_decode_aug on oracle head maps against the oracle's Detect + _descale_pred (pass 2: 0.67, P3 dropped; pass 1 flipped)."""
    from aquaculture_amd import augment, engine
    from oracle import yolov5_oracle as O
    m = O.model_from_checkpoint(synth_ck)
    m.taps = {}
    passes, n = augment.geometry(640, 640)
    for pi in (1, 2):
        ps = passes[pi]
        g = torch.Generator().manual_seed(pi)
        x = torch.rand(1, 3, ps.hp, ps.wp, generator=g)
        feats = m.features(x)
        y = m.detect(feats)
        y[..., :4] /= augment.SCALES[pi]
        if ps.flip:
            y[..., 0] = 640 - y[..., 0]
        heads = [m.taps[f"model.24.m.{l}"].permute(0, 2, 3, 1).contiguous().cuda() for l in range(3)]
        ag = synth_ck.anchor_grid_px().numpy().tolist()
        pred = engine.detect_decode_aug(heads, ps.hp, ps.wp, synth_ck.nc, ag, synth_ck.stride, ps.level_mask,
                                        ps.out_first - ps.keep_first, n, ps.scale, 640.0 if ps.flip else 0.0).cpu()
        got = pred[:, ps.out_first:ps.out_first + ps.keep_count]
        want = y[:, ps.keep_first:ps.keep_first + ps.keep_count]
        assert (got - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
        outside = torch.ones(n, dtype=torch.bool)
        outside[ps.out_first:ps.out_first + ps.keep_count] = False
        assert (pred[:, outside] == 0).all()


def _head_decode_aug_descales(shape, scale, flip_w, nc=5):
    from aquaculture_amd import engine
    anchors = [(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)]
    B, ny, nx, cin = shape
    g = torch.Generator().manual_seed(3)
    x = (torch.randn(B, ny, nx, cin, generator=g) * 0.7).bfloat16().cuda()
    w = torch.randn(3 * (nc + 5), cin, generator=g) * (1.5 / cin ** 0.5)
    b = torch.randn(3 * (nc + 5), generator=g) * 0.5
    cap = 3 * ny * nx
    c0, i0, r0 = (t.cpu() for t in engine.head_decode_level(x, w, b, 100, 16.0, anchors, nc, 0.25, cap))
    c1, i1, r1 = (t.cpu() for t in engine.head_decode_level_aug(x, w, b, 100, 16.0, anchors, nc, 0.25, cap, scale, flip_w))
    assert torch.equal(c0, c1) and int(c0.sum()) > 0
    for bi in range(B):
        n = int(c0[bi])
        o0, o1 = torch.argsort(i0[bi, :n]), torch.argsort(i1[bi, :n])
        assert torch.equal(i0[bi, :n][o0], i1[bi, :n][o1])
        want = r0[bi, :n][o0].clone()
        want[:, :4] /= scale                          # (on the CPU: an IEEE division, as _descale_pred's)
        if flip_w != 0.0:
            want[:, 0] = flip_w - want[:, 0]
        assert torch.equal(r1[bi, :n][o1], want)


def test_head_decode_aug_descales(lib):
    """aq_head_decode_aug = aq_head_decode's candidates with xywh / scale and x mirrored."""
    _head_decode_aug_descales((2, 28, 28, 384), 0.67, 640.0)


@pytest.mark.parametrize("cin,scale,flip_w,nc", [(c, 0.67, 640.0, 5) for c in (128, 192, 256, 320, 384, 512, 640, 768, 1024, 1280)] +
                         [(192, 0.67, 0.0, 5), (768, 0.83, 0.0, 5), (384, 0.83, 640.0, 4), (1280, 0.67, 0.0, 4)])
def test_head_decode_aug_descales_at_every_width(lib, cin, scale, flip_w, nc):
    """The same for the AUG twin of every entry of the fused head's kernel table (cin / 32 = 4 .. 40 k-steps), 35 pixels per image: an
    iteration of 64, 32 or 16 pixels covers one image or straddles two; with flip_w = 0 (pass 2 of an augmented call: scaled, not
    mirrored) x is divided only; at four classes rows are 9 floats."""
    assert lib.aq_head_decode_supported(cin, 3, nc) == 1
    _head_decode_aug_descales((2, 5, 7, cin), scale, flip_w, nc)


# ---- engine --------------------------------------------------------------------------------------------------------------------------
def test_forward_raw_augment_fp32(lib, synth_ck, tiles_640, ref_fp32):
    from aquaculture_amd import engine
    eng = engine.Engine(synth_ck, "fp32")
    pred = eng.forward_raw(torch.from_numpy(tiles_640).cuda(), augment=True).cpu()
    assert pred.shape == ref_fp32.shape == (3, 45147, 10)
    assert (pred[..., 4:] - ref_fp32[..., 4:]).abs().max().item() <= 1e-4
    assert (pred[..., :4] - ref_fp32[..., :4]).abs().max().item() <= 640 * 1e-4


@pytest.mark.parametrize("precision", ["fp32", "f16x3"])
def test_infer_augment_matches_oracle_nms(lib, synth_ck, tiles_640, ref_fp32, precision):
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    ref = O.non_max_suppression(ref_fp32.numpy())
    eng = engine.Engine(synth_ck, precision)
    dets, counts = eng.infer(torch.from_numpy(tiles_640).cuda(), augment=True)
    _match(dets.cpu().numpy(), counts.cpu().numpy(), ref, box_tol=640 * 1e-4, conf_tol=1e-4)
    assert sum(r.shape[0] for r in ref) > 100


def test_infer_augment_bf16_close_to_emulated_oracle(lib, synth_ck, tiles_640):
    """The bar of tests/test_gpu_engine.py::test_infer_bf16_close_to_emulated_oracle, on the augmented prediction."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    eng = engine.Engine(synth_ck, "bf16")
    ref = oracle_augmented_pred(O.model_from_checkpoint(synth_ck, O.q_bf16), tiles_640)
    t = torch.from_numpy(tiles_640).cuda()
    pred = eng.forward_raw(t, augment=True).cpu()
    d_conf = (pred[..., 4:] - ref[..., 4:]).abs().flatten()
    assert d_conf.mean().item() <= 1.04e-2
    assert d_conf.kthvalue(int(0.999 * d_conf.numel()))[0].item() <= 7.3e-2
    assert (pred[..., :4] - ref[..., :4]).abs().mean().item() <= 1.02
    ref_counts = [r.shape[0] for r in O.non_max_suppression(ref.numpy())]
    _, counts = eng.infer(t, augment=True)
    for got, want in zip(counts.cpu().tolist(), ref_counts):
        assert abs(got - want) <= 8


def test_infer_augment_deterministic_batch_invariant_and_plain_unchanged(lib, synth_ck):
    """Two augmented calls are bit-identical; B = 1 equals the same tile inside B = 64; plain calls on the same engine, before and after
    augmented ones, equal a fresh engine's bit for bit."""
    from aquaculture_amd import engine, tiles
    x64 = torch.from_numpy(tiles.synthetic_batch(list(range(64)), 640)).cuda()
    fresh = engine.Engine(synth_ck, "bf16")
    d_ref, c_ref = (t.clone() for t in fresh.infer(x64[:8]))
    fresh.close()
    eng = engine.Engine(synth_ck, "bf16")
    d_p0, c_p0 = (t.clone() for t in eng.infer(x64[:8]))
    d0, c0 = (t.clone() for t in eng.infer(x64, augment=True))
    d1, c1 = (t.clone() for t in eng.infer(x64, augment=True))
    assert torch.equal(c0, c1) and all(torch.equal(d0[b, :c0[b]], d1[b, :c1[b]]) for b in range(64))
    for b in (0, 37, 63):
        d, c = eng.infer(x64[b:b + 1].contiguous(), augment=True)
        assert int(c[0]) == int(c0[b]) and torch.equal(d[0, :c[0]], d0[b, :c0[b]]), b
    d_p1, c_p1 = eng.infer(x64[:8])
    for c, d in ((c_p0, d_p0), (c_p1, d_p1)):
        assert torch.equal(c, c_ref) and all(torch.equal(d[b, :c[b]], d_ref[b, :c_ref[b]]) for b in range(8))
    assert [f for f, _ in eng.last_launches(augment_pass=1)][0] == "stem"


def test_infer_augment_classes_and_agnostic(lib, synth_ck, tiles_640, ref_fp32):
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    eng = engine.Engine(synth_ck, "fp32")
    t = torch.from_numpy(tiles_640).cuda()
    for classes, agnostic in (([0, 2], False), (None, True)):
        eng.set_nms_options(agnostic=agnostic, classes=classes)
        ref = O.non_max_suppression(ref_fp32.numpy(), agnostic=agnostic, classes=classes)
        dets, counts = eng.infer(t, augment=True)
        _match(dets.cpu().numpy(), counts.cpu().numpy(), ref, box_tol=640 * 1e-4, conf_tol=1e-4)


def test_refused_geometry_leaves_the_augmented_layout_intact(lib, synth_ck, tiles_640):
    """An augmented call refused for its tile size (1280 px: over the NMS kernel's rows) between two 640-px augmented calls on one engine:
    the second 640-px call must still run the 640 passes in the 640 layout -- bit-identical detections and counts to the first."""
    from aquaculture_amd import engine
    eng = engine.Engine(synth_ck, "bf16")
    t = torch.from_numpy(tiles_640).cuda()
    d0, c0 = (v.clone() for v in eng.infer(t, augment=True))
    big = torch.zeros((1, 1280, 1280, 3), dtype=torch.uint8, device=t.device)
    with pytest.raises(RuntimeError, match=r"error -1: .*NMS"):
        eng.infer(big, augment=True)
    with pytest.raises(RuntimeError, match=r"error -1: .*NMS"):
        eng.workspace(1, 1280, 1280, augment=True)
    ws = eng.workspace(3, 640, 640, augment=True)
    dets = torch.empty((3, 1000, 6), dtype=torch.float32, device=t.device)
    counts = torch.empty((3,), dtype=torch.int32, device=t.device)
    rc = eng.lib.aq_engine_infer_augment(eng.handle, big.data_ptr(), 1, 1280, 1280, ws.data_ptr(), ws.numel(), dets.data_ptr(),
                                         counts.data_ptr(), 0.25, 0.45, 1000, engine._stream_ptr())
    assert rc == -1                                     # the C entry point itself refuses, before anything is launched
    d1, c1 = eng.infer(t, augment=True)
    torch.cuda.synchronize()
    assert torch.equal(c0, c1) and all(torch.equal(d0[b, :c0[b]], d1[b, :c1[b]]) for b in range(3))


def test_fp8_engine_refuses_augmented_calls(lib, synth_ck, tiles_640):
    """fp8 activation scales are calibrated at one geometry; the augmented passes run at three: the engine refuses (AQ_ERR_INVALID)."""
    from aquaculture_amd import engine
    eng = engine.Engine(synth_ck, "fp8")
    assert eng.fp8_scales
    t = torch.from_numpy(tiles_640).cuda()
    with pytest.raises(RuntimeError, match=r"error -1: augment: .*fp8"):
        eng.infer(t, augment=True)
    with pytest.raises(RuntimeError, match=r"error -1: augment: .*fp8"):
        eng.forward_raw(t, augment=True)
    _, counts = eng.infer(t)                           # the plain path of the same engine is untouched
    assert int(counts.sum()) > 0


def test_yolov5x_augment_and_the_row_limit(lib):
    """yolov5x (no fused stem: the scaled space-to-depth preprocess) fp32 at 128 px against the oracle; at 1280 px the augmented
    prediction would exceed the NMS kernel's rows, and the call is refused with AQ_ERR_INVALID."""
    from aquaculture_amd import checkpoint, engine, tiles
    from oracle import yolov5_oracle as O
    ck = checkpoint.synthetic_checkpoint("yolov5x", 5)
    eng = engine.Engine(ck, "fp32")
    assert eng.plan.ops[0].kind == 0                   # AQ_OP_PREPROCESS
    x = tiles.synthetic_batch([0, 19], 128)
    ref = oracle_augmented_pred(O.model_from_checkpoint(ck), x)
    pred = eng.forward_raw(torch.from_numpy(x).cuda(), augment=True).cpu()
    assert pred.shape == ref.shape
    assert (pred[..., 4:] - ref[..., 4:]).abs().max().item() <= 1e-4
    assert (pred[..., :4] - ref[..., :4]).abs().max().item() <= 128 * 1e-4
    with pytest.raises(RuntimeError, match=r"error -1: .*NMS"):
        eng.workspace(1, 1280, 1280, augment=True)


def test_cli_augment_labels_and_resume(lib, tmp_path):
    """detect.py --augment --save-txt --save-conf on a few synthetic jpegs: per tile the label lines of the fp32 augmented oracle -- as many
    lines, paired one to one with the same class, boxes within one pixel (the writer rounds to whole pixels: a 1e-5 px difference can cross a
    .5) and confidences within 1e-4, the fp32 parity bar --; --resume of that directory without --augment is refused."""
    from aquaculture_amd import checkpoint, dataloader, tiles
    from oracle import yolov5_oracle as O
    src = tmp_path / "jpegs"
    idx = [0, 1, 2]
    tiles.write_synthetic_jpegs(str(src), idx, size=640)
    w = tmp_path / "multilabel_farms_synth.pt"
    checkpoint.write_synthetic_checkpoint(str(w), "yolov5m", 5)
    base = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(w), "--source", str(src), "--nosave", "--save-txt",
            "--save-conf", "--project", str(tmp_path / "runs"), "--name", "aug", "--batch-size", "4"]
    r = subprocess.run(base + ["--augment"], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
    m = O.model_from_checkpoint(checkpoint.load_checkpoint(str(w)))
    n_lines = 0
    for i in idx:
        stem = tiles.tile_name(i)[:-5]
        im = dataloader.read_rgb(str(src / (stem + ".jpeg")))
        det = O.non_max_suppression(oracle_augmented_pred(m, im[None]).numpy())[0]
        want = O.label_lines(det, im.shape[:2], im.shape[:2])
        path = tmp_path / "runs" / "aug" / "labels" / (stem + ".txt")
        got = path.read_text().splitlines() if path.exists() else []
        assert len(got) == len(want), (stem, len(got), len(want))
        g = np.array([[float(v) for v in l.split()] for l in got]).reshape(-1, 6)
        used = np.zeros(len(g), bool)
        for l in want:
            r = np.array([float(v) for v in l.split()])
            d = np.abs(g[:, 1:5] - r[1:5]).max(1) * 640 + np.abs(g[:, 5] - r[5]) * 1e4
            d[used | (g[:, 0] != r[0])] = np.inf
            j = int(np.argmin(d))
            assert np.abs(g[j, 1:5] - r[1:5]).max() <= 1.0001 / 640 and abs(g[j, 5] - r[5]) <= 1e-4, (stem, l, got[j])
            used[j] = True
        n_lines += len(want)
    assert n_lines > 0
    assert '"augment": true' in (tmp_path / "runs" / "aug" / "run_params.json").read_text()
    r = subprocess.run(base + ["--resume"], capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "augment" in (r.stdout + r.stderr)
