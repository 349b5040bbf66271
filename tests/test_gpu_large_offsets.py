"""Kernels on tensors that extend past 2^31 bytes, and the size guards at the engine's batch limits.

Every other test runs tensors of at most about 1 GB; a 32-bit product or buffer-descriptor size in a kernel's addressing would go
unnoticed there.  Here each family runs one case whose input or output tensor crosses 2^31 bytes, reached with a large batch of
moderate images at the layer shapes, channel pitches and channel slices of yolov5m's plan, inputs filled on the device from a seeded
generator.  Checks:
  * far images equal the same images run alone: the first image, the one holding byte 2^31 (and 2^32 where the tensor reaches it) and the
    last one, bit for bit against a small batch of just those images (the kernels' parity tests vouch for the small batch).  A wrapped
    address corrupts a far image or overwrites a near one, and this catches both;
  * where the large batch selects another form of the kernel (assembly -> HIP-source Bottleneck) or where the form sizes its tile from
    the batch (planar 3x3, implicit GEMM), those images against fp64 with the kernel's own parity-test bounds instead;
  * canaries: output channels outside the written slice and a guard region behind the output allocation keep their sentinel values;
  * guard edges, where the limit is within memory: the largest batch a guard accepts runs and passes the checks, the next one is refused
    before anything is launched (buffers are allocated for the refused size too, so a guard that failed to refuse would still write
    inside them) -- the assembly 1x1, planar 3x3 (bf16, w8, f8), planar 3x3/s2, upsample rows, the implicit-GEMM pixel count, the
    Bottleneck builds' switch and the C3 tail.  The fp8 planar kernel cannot reach 2^31 bytes at all (its guard stops just short), so it
    is tested at that edge.  Guards on 2^31 pixels or elements (stem, down-block, HIP Bottleneck, direct 1x1, SPPF, preprocess, upsample
    elements, fused head 2^30 pixels) would need 30-400 GB tensors at the plan's channel counts: their edges are not run here; the
    engine's sizing check applies them (test_engine_refuses_*).
Nothing is copied to the host but the checked images.  Sizes are derived from the guard formulas, not hand-copied.
"""
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

from oracle import guards

pytestmark = pytest.mark.gpu

B31, B32 = 1 << 31, 1 << 32
GUARD = 1 << 16                       # elements of the untouched region behind each output allocation
SENT = -7.25                          # sentinel (exact in bf16 and fp32)
BF16_TOL = (2.0 ** -7, 4e-3)          # tests/test_gpu_bench_layers.py CONV_TOL["bf16"]
FP32_TOL = (2e-5, 2e-5)               # tests/test_gpu_conv.py fp32


def _gen(seed):
    return torch.Generator(device="cuda").manual_seed(seed)


def _randn(shape, dtype, seed, scale=1.0):
    t = torch.randn(shape, generator=_gen(seed), device="cuda", dtype=torch.float32 if dtype == torch.float32 else torch.bfloat16)
    return t.mul_(scale) if scale != 1.0 else t


def _guarded(shape, dtype):
    """(tensor of `shape` filled with SENT, the whole allocation) -- GUARD sentinel elements follow the tensor."""
    n = 1
    for s in shape:
        n *= s
    flat = torch.full((n + GUARD,), SENT, dtype=dtype, device="cuda")
    return flat[:n].view(shape), flat


def _guard_ok(flat):
    return bool((flat[-GUARD:] == SENT).all())


def _batch_past(bytes_per_image, mark=B31):
    """Smallest batch whose tensor ends past byte `mark`, plus one image."""
    return mark // bytes_per_image + 2


def _far(B, bytes_per_image):
    """Images to check: the first, the ones holding bytes 2^31 and 2^32 of the tensor (where it reaches them), the last."""
    return sorted({0, *(m // bytes_per_image for m in (B31, B32) if m // bytes_per_image < B), B - 1})


def _pack_direct1x1(lib, w):
    """Weight image of aq_conv1x1_direct / aq_conv1x1_direct_f8out for w [cout, cin, 1, 1]."""
    import ctypes as C
    import numpy as np
    cout, cin = w.shape[:2]
    wh = np.ascontiguousarray(w.reshape(cout, cin).float().numpy())
    n = C.c_size_t()
    wp = wh.ctypes.data_as(C.POINTER(C.c_float))
    assert lib.aq_pack_conv1x1_direct(wp, cin, cout, None, C.byref(n), None) == 0
    buf = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    assert lib.aq_pack_conv1x1_direct(wp, cin, cout, buf.data_ptr(), C.byref(n), torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    return buf


def _weights(cout, cin, k, seed):
    g = torch.Generator().manual_seed(seed)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    return w, torch.randn(cout, generator=g) * 0.1


def _ref_conv(x, w, b, stride, pad, act=True, res=None, rnd=torch.bfloat16):
    """fp64 conv of NHWC x with the weights rounded as the kernel stores them."""
    wq = w.to(rnd).double()
    y = F.conv2d(x.double().permute(0, 3, 1, 2), wq, b.double(), stride=stride, padding=pad)
    if act:
        y = F.silu(y)
    y = y.permute(0, 2, 3, 1)
    return y if res is None else y + res.double()


def _assert_close(got, ref, tol, what):
    rel, abs_ = tol
    err = (got.double() - ref).abs()
    ratio = float((err / (rel * ref.abs() + abs_)).max())
    assert ratio <= 1.0, f"{what}: max err {float(err.max()):.3g}, {ratio:.2f} x the bound {rel:g} |ref| + {abs_:g}"


def _same(big, small, idx, what):
    """big: the large batch's images `idx` (gathered), small: the same images run as a batch of their own."""
    for j, i in enumerate(idx):
        a, b = big[j], small[j]
        if not torch.equal(a, b):
            bad = int((a != b).sum())
            raise AssertionError(f"{what}: image {i} of the large batch differs from the same image run alone ({bad} elements)")


# ---------------------------------------------------------------------------------------------------------------------------------
def test_stem_fp32_and_bf16_past_2_31(lib):
    """model.0 (6x6/s2, 3 -> 48) at 640 px: the fp32 stem output is 19.7 MB per image (byte 2^31 in image 109), the bf16 one 9.8 MB."""
    from aquaculture_amd import engine
    w, b = _weights(48, 3, 6, 1)
    for prec, eb in (("fp32", 4), ("bf16", 2)):
        per = 320 * 320 * 48 * eb
        B = _batch_past(per)
        x = torch.randint(0, 256, (B, 640, 640, 3), generator=_gen(2), device="cuda", dtype=torch.uint8)
        out = engine.stem_conv_nhwc(x, w, b, precision=prec)
        assert B * per > B31
        idx = _far(B, per)
        small = engine.stem_conv_nhwc(x[idx].contiguous(), w, b, precision=prec)
        _same(out[idx], small, idx, f"stem {prec}, batch {B}")
        del out, x
        torch.cuda.empty_cache()


def test_stemdown_past_2_31(lib):
    """model.0 + model.1 + model.2.cv1|cv2 as one launch: output [B, 160, 160, 96] bf16 (4.9 MB per image)."""
    from aquaculture_amd import engine
    ws, bs = _weights(48, 3, 6, 3)
    wa, ba = _weights(96, 48, 3, 4)
    wb, bb = _weights(96, 96, 1, 5)
    per = 160 * 160 * 96 * 2
    B = _batch_past(per)
    x = torch.randint(0, 256, (B, 640, 640, 3), generator=_gen(6), device="cuda", dtype=torch.uint8)
    out = engine.stemdown_nhwc(x, ws, bs, wa, ba, wb, bb)
    idx = _far(B, per)
    small = engine.stemdown_nhwc(x[idx].contiguous(), ws, bs, wa, ba, wb, bb)
    _same(out[idx], small, idx, f"stem-down, batch {B}")


def test_downblock_input_past_2_31(lib):
    """model.1 + model.2.cv1|cv2: input [B, 320, 320, 48] bf16 (9.8 MB per image) into the 96-channel m2.cat tensor."""
    from aquaculture_amd import engine
    wa, ba = _weights(96, 48, 3, 7)
    wb, bb = _weights(96, 96, 1, 8)
    per = 320 * 320 * 48 * 2
    B = _batch_past(per)
    x = _randn((B, 320, 320, 48), torch.bfloat16, 9)
    out, flat = _guarded((B, 160, 160, 96), torch.bfloat16)
    engine.downblock_nhwc(x, wa, ba, wb, bb, out=out)
    assert _guard_ok(flat)
    idx = _far(B, per)
    small = engine.downblock_nhwc(x[idx].contiguous(), wa, ba, wb, bb)
    _same(out[idx], small, idx, f"down-block, batch {B}")


def test_conv3x3s2_direct_input_past_2_31(lib):
    """model.3 (96 -> 192, 3x3/s2) on [B, 160, 160, 96] bf16 (4.9 MB per image)."""
    from aquaculture_amd import engine
    w, b = _weights(192, 96, 3, 10)
    per = 160 * 160 * 96 * 2
    B = _batch_past(per)
    x = _randn((B, 160, 160, 96), torch.bfloat16, 11)
    out, flat = _guarded((B, 80, 80, 192), torch.bfloat16)
    engine.conv3x3s2_direct_nhwc(x, w, b, out=out)
    assert _guard_ok(flat)
    idx = _far(B, per)
    small = engine.conv3x3s2_direct_nhwc(x[idx].contiguous(), w, b)
    _same(out[idx], small, idx, f"direct 3x3/s2, batch {B}")


# ---- Bottleneck: the assembly builds' 32-bit offsets (input < 2^30 B, output < 2^31 B) and the HIP-source form beyond them ----
def _largest(pred, hi=1 << 20):
    lo = 1
    assert pred(lo)
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


@pytest.mark.parametrize("C,H,in_ld,out_ld,name", [(48, 160, 96, 48, "model.2.m.0"), (48, 160, 48, 96, "model.2.m.1"),
                                                   (96, 80, 192, 96, "model.4.m.0"), (96, 80, 96, 192, "model.4.m.1")])
def test_bottleneck_form_switch_points(lib, C, H, in_ld, out_ld, name):
    """The batch at which each of yolov5m's Bottleneck launches leaves the assembly build: the library's own answer
    (aq_bottleneck_asm_form) equals the guard formula on both sides of the edge -- 219 for model.2.m.0, 437 for model.2.m.1 and
    model.4.m.0 (the 192-channel m4.cat input), 874 for model.4.m.1."""
    Bmax = _largest(lambda B: guards.btl_asm_fits(C, B, H, H, in_ld, out_ld))
    assert Bmax == {"model.2.m.0": 218, "model.4.m.1": 873}.get(name, 436), (name, Bmax)
    for B in (1, Bmax - 1, Bmax, Bmax + 1, 2 * Bmax):
        assert lib.aq_bottleneck_asm_form(C, B, H, H, in_ld, out_ld) == int(B <= Bmax), (name, B)


def _btl_ref(x, w1, b1, w2, b2, shortcut):
    t = _ref_conv(x, w1, b1, 1, 0).to(torch.bfloat16)
    return _ref_conv(t, w2, b2, 1, 1, res=x if shortcut else None)


@pytest.mark.parametrize("C,H", [(48, 160), (96, 80)])
def test_bottleneck_asm_at_its_largest_batch_and_hip_past_2_31(lib, C, H, tmp_path):
    """Assembly build at the largest batch its guard takes (output slice just under 2^31 bytes, ld 2C, canary channels beside it): far
    images bit-identical to a small batch.  HIP-source build on an input slice of the 2C-channel concat that passes 2^31 bytes: far images
    against fp64 (the Bottleneck bounds of the layer check: 2^-7 |ref| + 2e-2), and bit-identical to the same images run in a process with
    AQ_BTL_ASM=0 -- the HIP-source kernel by switch, so the guard really launched that kernel and not the assembly build."""
    from aquaculture_amd import engine
    w1, b1 = _weights(C, C, 1, 20 + C)
    w2, b2 = _weights(C, C, 3, 21 + C)
    Bmax = _largest(lambda B: guards.btl_asm_fits(C, B, H, H, C, 2 * C))
    x = _randn((Bmax, H, H, C), torch.bfloat16, 22)
    out, flat = _guarded((Bmax, H, H, 2 * C), torch.bfloat16)
    assert lib.aq_bottleneck_asm_form(C, Bmax, H, H, C, 2 * C) == 1
    engine.bottleneck_nhwc(x, w1, b1, w2, b2, shortcut=True, out=out[..., C:])
    assert _guard_ok(flat) and bool((out[..., :C] == SENT).all()), "canaries overwritten"
    per = H * H * 2 * C * 2
    idx = _far(Bmax, per)
    small = engine.bottleneck_nhwc(x[idx].contiguous(), w1, b1, w2, b2, shortcut=True)
    _same(out[idx, ..., C:].contiguous(), small, idx, f"assembly Bottleneck C = {C}, batch {Bmax}")
    del x, out, flat
    torch.cuda.empty_cache()

    per = H * H * 2 * C * 2                       # input: a C-channel slice of the 2C-channel concat
    B = _batch_past(per)
    assert lib.aq_bottleneck_asm_form(C, B, H, H, 2 * C, C) == 0
    cat = _randn((B, H, H, 2 * C), torch.bfloat16, 23)
    out, flat = _guarded((B, H, H, C), torch.bfloat16)
    engine.bottleneck_nhwc(cat[..., C:], w1, b1, w2, b2, shortcut=True, out=out)
    assert _guard_ok(flat)
    for i in _far(B, per):
        xi = cat[i:i + 1, ..., C:].cpu()
        _assert_close(out[i:i + 1].cpu(), _btl_ref(xi, w1, b1, w2, b2, True), (2.0 ** -7, 2e-2), f"HIP Bottleneck C = {C}, image {i} of {B}")
    idx = _far(B, per)
    got = out[idx].cpu()
    d = str(tmp_path / "btl_hip.pt")
    torch.save({"x": cat[idx].cpu(), "w1": w1, "b1": b1, "w2": w2, "b2": b2, "C": C}, d)
    del cat, out, flat
    torch.cuda.empty_cache()
    child = ("import sys, torch; sys.path.insert(0, sys.argv[2]); from aquaculture_amd import engine; d = torch.load(sys.argv[1]); C = d['C']; "
             "x = d['x'].cuda(); n, H = x.shape[0], x.shape[1]; "
             "assert engine.load_library().aq_bottleneck_asm_form(C, n, H, H, 2 * C, C) == 0; "
             "y = engine.bottleneck_nhwc(x[..., C:], d['w1'], d['b1'], d['w2'], d['b2'], shortcut=True); torch.save(y.cpu(), sys.argv[1] + '.y')")
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    subprocess.run([sys.executable, "-c", child, d, root], env=dict(os.environ, AQ_BTL_ASM="0"), check=True, timeout=300)
    ref = torch.load(d + ".y")
    _same(got, ref, idx, f"HIP Bottleneck C = {C} by guard vs AQ_BTL_ASM=0")


def test_c3tail_at_its_largest_batch(lib):
    """model.2's last Bottleneck + cv3 in one launch at the largest batch aq_bottleneck_c3tail_supported takes (96-channel output just
    under 2^31 bytes): far images bit-identical to a small batch; one more image is refused by the query."""
    from aquaculture_amd import engine
    Bmax = _largest(lambda B: engine.bottleneck_c3tail_supported(B, 160, 160), hi=4096)
    assert Bmax == _largest(lambda B: guards.btl_asm_fits(48, B, 160, 160, 48, 96) and B * 160 * 160 * 96 * 2 < B31)
    assert not engine.bottleneck_c3tail_supported(Bmax + 1, 160, 160)
    w1, b1 = _weights(48, 48, 1, 30)
    w2, b2 = _weights(48, 48, 3, 31)
    w3, b3 = _weights(96, 96, 1, 32)
    packed = engine.pack_bottleneck_c3tail(w1, b1, w2, b2, w3, b3, torch.device("cuda"))
    x = _randn((Bmax, 160, 160, 48), torch.bfloat16, 33)
    cat = _randn((Bmax, 160, 160, 96), torch.bfloat16, 34)
    out, flat = _guarded((Bmax, 160, 160, 96), torch.bfloat16)
    engine.bottleneck_c3tail_nhwc(x, cat[..., 48:], packed, out=out)
    assert _guard_ok(flat)
    idx = _far(Bmax, 160 * 160 * 96 * 2)
    small = engine.bottleneck_c3tail_nhwc(x[idx].contiguous(), cat[idx].contiguous()[..., 48:], packed)
    _same(out[idx], small, idx, f"C3 tail, batch {Bmax}")


# ---- implicit GEMM ----
def test_igemm_fp32_model1_past_2_31_and_its_pixel_limit(lib):
    """fp32 model.1 (48 -> 96, 3x3/s2) on [B, 320, 320, 48] fp32 (19.7 MB per image) with the heuristic tile shape: far images against
    fp64 within the fp32 bounds.  The pixel-index guard (npix < 2^24) refuses one image past its largest batch, from the C ABI."""
    from aquaculture_amd import engine
    w, b = _weights(96, 48, 3, 40)
    per = 320 * 320 * 48 * 4
    B = _batch_past(per)
    x = _randn((B, 320, 320, 48), torch.float32, 41)
    out = engine.conv2d_nhwc(x, w, b, stride=2, precision="fp32")
    for i in _far(B, per):
        _assert_close(out[i:i + 1].cpu(), _ref_conv(x[i:i + 1].cpu(), w, b, 2, 1, rnd=torch.float32), FP32_TOL, f"igemm fp32, image {i} of {B}")
    del x, out
    torch.cuda.empty_cache()
    # the guard edge at a small image (the limit is in pixels): 2^24 output pixels of 16 x 16 -> 65536 images
    Bmax = (1 << 24) // (16 * 16) - 1
    x = _randn((Bmax + 1, 32, 32, 8), torch.float32, 42)
    w8, b8 = _weights(16, 8, 3, 43)
    out = engine.conv2d_nhwc(x[:Bmax], w8, b8, stride=2, precision="fp32")
    _assert_close(out[-1:].cpu(), _ref_conv(x[Bmax - 1:Bmax].cpu(), w8, b8, 2, 1, rnd=torch.float32), FP32_TOL, f"igemm at {Bmax} images")
    with pytest.raises(RuntimeError, match="fast-index range"):
        engine.conv2d_nhwc(x, w8, b8, stride=2, precision="fp32")


# ---- 1x1 ----
def test_conv1x1_direct_slices_past_2_31(lib):
    """model.2.cv3-like 96 -> 96 direct 1x1 reading channels 96..191 of a 192-channel tensor and writing channels 0..95 of another
    (9.8 MB per image each, both past 2^31 bytes); channels 96..191 of the output stay sentinels."""
    from aquaculture_amd import engine
    w, b = _weights(96, 96, 1, 50)
    per = 160 * 160 * 192 * 2
    B = _batch_past(per)
    x = _randn((B, 160, 160, 192), torch.bfloat16, 51)
    out, flat = _guarded((B, 160, 160, 192), torch.bfloat16)
    engine.conv1x1_direct_nhwc(x[..., 96:], w, b, out=out[..., :96])
    assert _guard_ok(flat) and bool((out[..., 96:] == SENT).all()), "canaries overwritten"
    idx = _far(B, per)
    small = engine.conv1x1_direct_nhwc(x[idx].contiguous()[..., 96:], w, b)
    _same(out[idx, ..., :96].contiguous(), small, idx, f"direct 1x1, batch {B}")


def test_conv1x1_direct_f8out_past_2_31(lib):
    """The fp8 pair's producer (192 -> 192 1x1 writing e4m3 codes into the first bytes of each pixel's bf16 slot, pitch 384 bytes) on
    [B, 40, 40, 192] bf16 (input and code tensor 614 KB per image, both past 2^31): far images bit-identical to a small batch; the other
    half of every slot and the guard region keep their sentinel bytes."""
    w, b = _weights(192, 192, 1, 55)
    wbuf = _pack_direct1x1(lib, w)
    bias = b.float().cuda()
    per = 40 * 40 * 384
    B = _batch_past(per)
    x = _randn((B, 40, 40, 192), torch.bfloat16, 56)
    n = B * 40 * 40 * 384
    flat = torch.full((n + GUARD,), 0xA5, dtype=torch.uint8, device="cuda")
    out = flat[:n].view(B, 40, 40, 384)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.aq_conv1x1_direct_f8out(x.data_ptr(), 192, 0, out.data_ptr(), 384, 0, 192, 192, wbuf.data_ptr(), bias.data_ptr(), B * 1600, 1,
                                       0.05, s) == 0
    idx = _far(B, per)
    small = torch.full((len(idx), 40, 40, 384), 0xA5, dtype=torch.uint8, device="cuda")
    xs = x[idx].contiguous()
    assert lib.aq_conv1x1_direct_f8out(xs.data_ptr(), 192, 0, small.data_ptr(), 384, 0, 192, 192, wbuf.data_ptr(), bias.data_ptr(),
                                       len(idx) * 1600, 1, 0.05, s) == 0
    torch.cuda.synchronize()
    assert bool((flat[-GUARD:] == 0xA5).all()) and bool((out[..., 192:] == 0xA5).all()), "canaries overwritten"
    _same(out[idx], small, idx, f"direct 1x1 f8out, batch {B}")


def test_igemm_and_halo_bf16_past_2_31(lib):
    """bf16 192 -> 192 3x3 (model.6 cv2 shape) on [B, 40, 40, 192] (input and output past 2^31 bytes) through aq_conv2d: the heuristic tile
    shape against fp64; a halo tile configuration (the last id) bit-identical to a small batch on the far images, and its one-workgroup-
    per-tile form bit-identical to the persistent grid."""
    from aquaculture_amd import engine
    per = 40 * 40 * 192 * 2
    B = _batch_past(per)
    x = _randn((B, 40, 40, 192), torch.bfloat16, 57)
    w, b = _weights(192, 192, 3, 58)
    idx = _far(B, per)
    out = engine.conv2d_nhwc(x, w, b, precision="bf16")
    for i in idx:
        _assert_close(out[i:i + 1].cpu(), _ref_conv(x[i:i + 1].cpu(), w, b, 1, 1), BF16_TOL, f"igemm bf16, image {i} of {B}")
    del out
    halo = lib.aq_conv_num_configs() - 1
    xs = x[idx].contiguous()
    small = engine.conv2d_nhwc(xs, w, b, precision="bf16", cfg=halo)
    out = engine.conv2d_nhwc(x, w, b, precision="bf16", cfg=halo)
    far = out[idx]
    del out
    _same(far, small, idx, f"halo cfg {halo}, batch {B}")
    out = engine.conv2d_nhwc(x, w, b, precision="bf16", cfg=halo | engine.CONV_CFG_ONE_TILE_PER_WG)
    _same(out[idx], far, idx, f"halo cfg {halo} one tile per workgroup vs persistent, batch {B}")


def test_head_decode_input_past_2_31(lib):
    """The P3 head conv + decode (192 channels at 80 x 80, 2.46 MB per image; 19200 candidate slots of 10 floats per image): the far images'
    candidate sets and rows bit-identical to a small batch (order within an image is free).  Its guard (B x ny x nx < 2^30 pixels) would
    need a 400 GB input at this width."""
    from aquaculture_amd import engine
    nc, anchors = 5, [(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)]
    no = nc + 5
    per = 80 * 80 * 192 * 2
    B = _batch_past(per)
    x = _randn((B, 80, 80, 192), torch.bfloat16, 120)
    g = torch.Generator().manual_seed(121)
    w = torch.randn(3 * no, 192, generator=g) * 0.08
    b = torch.randn(3 * no, generator=g) * 0.5 - 1.5
    cap = 3 * 80 * 80
    counts, cand, rows = engine.head_decode_level(x, w, b, 0, 8.0, anchors, nc, 0.25, cap)
    idx = _far(B, per)
    c2, k2, r2 = engine.head_decode_level(x[idx].contiguous(), w, b, 0, 8.0, anchors, nc, 0.25, cap)
    assert int(c2.min()) > 0
    for j, i in enumerate(idx):
        n = int(counts[i])
        assert n == int(c2[j]), (i, n, int(c2[j]))
        oa, ob = torch.argsort(cand[i, :n]), torch.argsort(k2[j, :n])
        assert torch.equal(cand[i, :n][oa], k2[j, :n][ob]) and torch.equal(rows[i, :n][oa], r2[j, :n][ob]), f"head decode: image {i} of {B}"


def test_detect_decode_and_nms_past_2_31(lib):
    """The unfused decode (three fp32 head maps, ld 32) writing the full prediction [B, 25200, 10] fp32 (1 MB per image) with the P3 map and
    the prediction past 2^31 bytes, then NMS over all 2623 images of it: the far images' predictions, detections and counts bit-identical to
    a small batch; the guard region behind the prediction untouched.  (Batch guard: B <= 65535 grid rows, 64 GB of head maps.)"""
    import ctypes as C
    from aquaculture_amd import engine
    nc, na, ld, no = 5, 3, 32, 10
    sizes, strides = (80, 40, 20), (8.0, 16.0, 32.0)
    N = na * sum(n * n for n in sizes)
    B = _batch_past(80 * 80 * ld * 4)
    heads = [_randn((B, n, n, ld), torch.float32, 130 + l).sub_(2.0) for l, n in enumerate(sizes)]
    anchors = (C.c_float * 18)(10, 13, 16, 30, 33, 23, 30, 61, 62, 45, 59, 119, 116, 90, 156, 198, 373, 326)
    st = (C.c_float * 3)(*strides)
    s = torch.cuda.current_stream().cuda_stream

    def decode(hs, n_img, pred):
        ptrs = (C.c_void_p * 3)(*[h.data_ptr() for h in hs])
        assert lib.aq_detect_decode(ptrs, ld, n_img, 640, 640, nc, na, anchors, st, pred.data_ptr(), 0.25, None, None, None, 0, s) == 0
    pred, flat = _guarded((B, N, no), torch.float32)
    assert B * N * no * 4 > B31
    decode(heads, B, pred)
    idx = _far(B, N * no * 4) + [B31 // (80 * 80 * ld * 4)]
    idx = sorted(set(idx))
    small = torch.empty((len(idx), N, no), dtype=torch.float32, device="cuda")
    decode([h[idx].contiguous() for h in heads], len(idx), small)
    torch.cuda.synchronize()
    assert _guard_ok(flat)
    _same(pred[idx], small, idx, f"detect decode, batch {B}")
    del heads
    torch.cuda.empty_cache()
    dets, counts = engine.nms(pred, nc)
    d2, c2 = engine.nms(small, nc)
    torch.cuda.synchronize()
    assert int(c2.min()) > 0
    for j, i in enumerate(idx):
        n = int(counts[i])
        assert n == int(c2[j]) and torch.equal(dets[i, :n], d2[j, :n]), f"NMS: image {i} of {B}"


def test_conv1x1_asm_output_near_2_32(lib):
    """Assembly 1x1 (96 -> 384, 40 x 40 images) at the largest batch its guard takes: output npix x 768 B < 2^32 - 2^22, so the output
    ends less than one image (1.2 MB) short of that limit, about 5 MiB below 2^32.  Far images (byte 2^31, the last images) bit-identical
    to a small batch; one image more is refused, nothing written."""
    from aquaculture_amd import engine
    cin, cout, hw = 96, 384, 40 * 40

    def fits(B):
        return B * hw * cin * 2 < B31 - (1 << 22) and B * hw * cout * 2 < B32 - (1 << 22)
    Bmax = _largest(fits)
    w, b = _weights(cout, cin, 1, 60)
    x = _randn((Bmax + 1, 40, 40, cin), torch.bfloat16, 61)
    out, flat = _guarded((Bmax + 1, 40, 40, cout), torch.bfloat16)
    engine.conv1x1_asm_nhwc(x[:Bmax], w, b, out=out[:Bmax])
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all())
    per = hw * cout * 2
    assert B32 - (1 << 22) - per <= Bmax * per < B32 - (1 << 22)
    idx = sorted(set(_far(Bmax, per)) | {Bmax - 2})
    small = engine.conv1x1_asm_nhwc(x[idx].contiguous(), w, b)
    _same(out[idx], small, idx, f"assembly 1x1, batch {Bmax}")
    with pytest.raises(RuntimeError):
        engine.conv1x1_asm_nhwc(x, w, b, out=out)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all()), "a refused launch wrote"


# ---- planar 3x3 ----
def test_planar3x3_bf16_and_w8_input_past_2_31_at_their_largest_batch(lib):
    """model.6-like 192 -> 192 planar 3x3 on 40 x 40 images reading channels 192..383 of a 384-channel tensor (input 4.29 GB, just under
    2^32) at the largest batch the output guard takes (B x 1600 x 192 x 2 < 2^31), with the bf16 weight stream and the e4m3 one (w8,
    weights on an fp8 grid): far images against fp64; one image more is refused by both."""
    from aquaculture_amd import quant
    from aquaculture_amd import engine
    hw = 40 * 40

    def fits(B):
        return B * 41 * 41 + 42 < (1 << 23) and B * hw * 192 * 2 < B31
    Bmax = _largest(fits)
    w, b = _weights(192, 192, 3, 70)
    x = _randn((Bmax + 1, 40, 40, 384), torch.bfloat16, 71)
    out, flat = _guarded((Bmax + 1, 40, 40, 192), torch.bfloat16)
    engine.conv3x3_pl_nhwc(x[:Bmax, ..., 192:], w, b, out=out[:Bmax])
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all())
    per_in = hw * 384 * 2
    for i in sorted(set(_far(Bmax, per_in)) | {B31 // (hw * 192 * 2)} - {Bmax}):
        _assert_close(out[i:i + 1].cpu(), _ref_conv(x[i:i + 1, ..., 192:].cpu(), w, b, 1, 1), BF16_TOL, f"planar 3x3, image {i} of {Bmax}")
    with pytest.raises(RuntimeError):
        engine.conv3x3_pl_nhwc(x[..., 192:], w, b, out=out)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all()), "a refused launch wrote"
    w8 = torch.from_numpy(quant.quantize_rows(w.numpy())[0])
    out[:Bmax].fill_(SENT)
    engine.conv3x3_pl_nhwc(x[:Bmax, ..., 192:], w8, b, out=out[:Bmax], w8=True)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all())
    for i in sorted(set(_far(Bmax, per_in)) | {B31 // (hw * 192 * 2)} - {Bmax}):
        _assert_close(out[i:i + 1].cpu(), _ref_conv(x[i:i + 1, ..., 192:].cpu(), w8, b, 1, 1), BF16_TOL, f"planar 3x3 w8, image {i} of {Bmax}")
    with pytest.raises(RuntimeError):
        engine.conv3x3_pl_nhwc(x[..., 192:], w8, b, out=out, w8=True)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all()), "a refused launch wrote"


def test_planar3x3_f8_at_its_largest_batch(lib):
    """fp8 x fp8 planar 3x3 (model.6 cv2 of an fp8 engine): e4m3 codes in the first bytes of each pixel's bf16 slot (pitch 384 bytes, as the
    engine's fp8 pairs lay them out).  Its guard keeps input and output under 2^31 bytes, so this family cannot pass 2^31: it runs at the
    largest batch the guard takes (both tensors within one image of 2^31) against fp64, and one image more is refused, nothing written."""
    from aquaculture_amd import engine
    hw = 40 * 40
    Bmax = _largest(lambda B: B * 41 * 41 + 42 < (1 << 23) and B * hw * 192 * 2 < B31 and B * hw * 384 < B31)
    assert lib.aq_conv3x3_pl_f8_supported(192, 192, Bmax, 40, 40) == 1
    g = _gen(75)
    slots = torch.randint(0, 127, (Bmax + 1, 40, 40, 384), generator=g, device="cuda", dtype=torch.uint8)
    slots |= torch.randint(0, 2, (Bmax + 1, 40, 40, 384), generator=g, device="cuda", dtype=torch.uint8) << 7   # no NaN codes
    xq = slots[..., :192]
    act_scale = 4.0 / 448.0
    w, b = _weights(192, 192, 3, 76)
    out, flat = _guarded((Bmax + 1, 40, 40, 192), torch.bfloat16)
    engine.conv3x3_pl_f8_nhwc(xq[:Bmax], act_scale, w, b, out=out[:Bmax])
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all())
    ws = w.abs().amax(dim=(1, 2, 3)) / 448.0
    wq = (w / ws.view(-1, 1, 1, 1)).to(torch.float8_e4m3fn).double() * ws.double().view(-1, 1, 1, 1)
    for i in (0, Bmax // 2, Bmax - 1):
        xi = xq[i:i + 1].cpu().view(torch.float8_e4m3fn).double() * act_scale
        _assert_close(out[i:i + 1].cpu(), _ref_conv(xi, wq, b, 1, 1, rnd=torch.float64), BF16_TOL, f"planar 3x3 f8, image {i} of {Bmax}")
    with pytest.raises(RuntimeError):
        engine.conv3x3_pl_f8_nhwc(xq, act_scale, w, b, out=out)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all()), "a refused launch wrote"


def test_planar3x3s2_guard_edge(lib):
    """model.5 (192 -> 384, 3x3/s2) planar on channels 192..383 of the 384-channel m4 tensor: the launcher's 31-bit input guard
    (B x 80 x 80 x 384 x 2 < 2^31) takes 436 images and refuses 437 from the C ABI (aq_conv3x3_pl_s2_supported checks channel counts and the
    index range only); at 436 the far images match fp64."""
    from aquaculture_amd import engine
    per_in = 80 * 80 * 384 * 2
    Bmax = (B31 - 1) // per_in
    assert lib.aq_conv3x3_pl_s2_supported(192, 384, Bmax + 1, 80, 80) == 1
    w, b = _weights(384, 192, 3, 80)
    x = _randn((Bmax + 1, 80, 80, 384), torch.bfloat16, 81)
    out, flat = _guarded((Bmax + 1, 40, 40, 384), torch.bfloat16)
    engine.conv3x3_pl_s2_nhwc(x[:Bmax, ..., 192:], w, b, out=out[:Bmax])
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all())
    for i in _far(Bmax, per_in):
        _assert_close(out[i:i + 1].cpu(), _ref_conv(x[i:i + 1, ..., 192:].cpu(), w, b, 2, 1), BF16_TOL, f"planar 3x3/s2, image {i} of {Bmax}")
    with pytest.raises(RuntimeError, match="31-bit"):
        engine.conv3x3_pl_s2_nhwc(x[..., 192:], w, b, out=out)
    assert _guard_ok(flat) and bool((out[Bmax] == SENT).all()), "a refused launch wrote"


# ---- pointwise ----
def test_upsample2x_past_2_31_and_row_limit(lib):
    """model.11-like upsample (384 ch, 20 -> 40) into channels 0..383 of the 768-channel concat (2.46 MB per image): exact on the far
    images, the other half of the concat untouched.  The grid's row guard (B x H < 65536) takes 1638 40-row images and refuses 1639."""
    from aquaculture_amd import engine
    per = 40 * 40 * 768 * 2
    B = _batch_past(per)
    x = _randn((B, 20, 20, 384), torch.bfloat16, 90)
    out, flat = _guarded((B, 40, 40, 768), torch.bfloat16)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.aq_upsample2x(x.data_ptr(), 384, 0, out.data_ptr(), 768, 0, 384, B, 20, 20, 0, s) == 0
    torch.cuda.synchronize()
    assert _guard_ok(flat) and bool((out[..., 384:] == SENT).all())
    for i in _far(B, per):
        assert torch.equal(out[i, ..., :384], x[i].repeat_interleave(2, 0).repeat_interleave(2, 1)), i
    del x, out, flat
    torch.cuda.empty_cache()
    rows = guards.largest(lambda B: guards.upsample2x_rows_fit(B, 40))
    x = _randn((rows + 1, 40, 8, 8), torch.bfloat16, 91)
    out, flat = _guarded((rows + 1, 80, 16, 8), torch.bfloat16)
    assert lib.aq_upsample2x(x.data_ptr(), 8, 0, out.data_ptr(), 8, 0, 8, rows, 40, 8, 0, s) == 0
    assert lib.aq_upsample2x(x.data_ptr(), 8, 0, out.data_ptr(), 8, 0, 8, rows + 1, 40, 8, 0, s) != 0
    torch.cuda.synchronize()
    assert torch.equal(out[rows - 1], x[rows - 1].repeat_interleave(2, 0).repeat_interleave(2, 1))
    assert bool((out[rows] == SENT).all()) and _guard_ok(flat), "a refused launch wrote"


def test_sppf_pool_past_2_31(lib):
    """SPPF's three chained 5x5 max pools on [B, 20, 20, 1536] bf16 (x | y1 | y2 | y3, 1.2 MB per image): exact on the far images."""
    per = 20 * 20 * 1536 * 2
    B = _batch_past(per)
    buf = _randn((B, 20, 20, 1536), torch.bfloat16, 100)
    x_far = {i: buf[i, ..., :384].clone() for i in _far(B, per)}
    assert lib.aq_sppf_pool(buf.data_ptr(), 1536, 0, 384, B, 20, 20, 0, torch.cuda.current_stream().cuda_stream) == 0
    torch.cuda.synchronize()
    for i, x in x_far.items():
        y, ys = x.permute(2, 0, 1)[None].float(), []
        for _ in range(3):
            y = F.max_pool2d(y, 5, 1, 2)
            ys.append(y)
        ref = torch.cat([x.permute(2, 0, 1)[None].float()] + ys, 1)[0].permute(1, 2, 0).to(torch.bfloat16)
        assert torch.equal(buf[i], ref), i


def test_preprocess_s2d_fp32_past_2_31(lib):
    """Space-to-depth of x / 255 into [B, 320, 320, 16] fp32 (6.5 MB per image): far images bit-identical to a small batch, within one
    fp32 ulp of x / 255, channels 12..15 zero."""
    per = 320 * 320 * 16 * 4
    B = _batch_past(per)
    x = torch.randint(0, 256, (B, 640, 640, 3), generator=_gen(110), device="cuda", dtype=torch.uint8)
    out, flat = _guarded((B, 320, 320, 16), torch.float32)
    s = torch.cuda.current_stream().cuda_stream
    assert lib.aq_preprocess_s2d(x.data_ptr(), out.data_ptr(), B, 640, 640, 1, s) == 0
    idx = _far(B, per)
    small = torch.empty((len(idx), 320, 320, 16), dtype=torch.float32, device="cuda")
    assert lib.aq_preprocess_s2d(x[idx].contiguous().data_ptr(), small.data_ptr(), len(idx), 640, 640, 1, s) == 0
    torch.cuda.synchronize()
    assert _guard_ok(flat)
    _same(out[idx], small, idx, f"preprocess fp32, batch {B}")
    for i in idx:
        v = (x[i].double() / 255.0).view(320, 2, 320, 2, 3).permute(0, 2, 1, 3, 4).reshape(320, 320, 12)
        assert float((out[i, ..., :12].double() - v).abs().max()) <= 2.0 ** -24 and bool((out[i, ..., 12:] == 0).all()), i


# ---- the engine refuses a batch it cannot run, before allocating anything (workspace sizing only) ----
def test_engine_refuses_fp32_batch_past_model1_pixel_limit(synth_ck):
    """fp32 at 640 px: model.1's implicit GEMM takes npix = B x 160 x 160 < 2^24, i.e. 655 images; 656 is refused by the sizing call,
    naming the op and the largest batch that fits."""
    from aquaculture_amd.engine import Engine
    eng = Engine(synth_ck, "fp32", 0)
    try:
        limit, op = guards.plan_batch_limit(eng.plan, 640, 640, 4)
        assert (limit, op) == (655, "model.1")
        assert eng.workspace_bytes(limit, 640, 640) > 0
        with pytest.raises(RuntimeError, match=rf"model\.1\).*largest batch that fits is {limit}\b"):
            eng.workspace_bytes(limit + 1, 640, 640)
        assert eng._ws is None and not eng._slots, "sizing allocated a workspace"
    finally:
        eng.close()


def test_engine_refuses_bf16_batch_past_upsample_rows(synth_ck):
    """bf16 on bench.py's shipped table: the upsample of the 40-row level takes B x 40 < 65536, i.e. 1638 images; 1639 is refused.
    The same engine without a table (implicit GEMM on the 160 x 160 1x1 layers) stops at 655."""
    import json
    import os
    from aquaculture_amd import spec
    from aquaculture_amd.engine import Engine
    eng = Engine(synth_ck, "bf16", 0, fused_stem=True, fused_bottleneck=True)
    try:
        with pytest.raises(RuntimeError, match=r"largest batch that fits is 655\b"):
            eng.workspace_bytes(656, 640, 640)
        import aquaculture_amd
        with open(os.path.join(os.path.dirname(aquaculture_amd.__file__), "data", "tuned_tables.json")) as f:
            ship = json.load(f)
        eng.set_tuned_table(64, 640, 640, ship[eng.tune_key(64, 640, 640)])
        limit = guards.largest(lambda B: guards.upsample2x_rows_fit(B, 40))
        assert limit == 1638
        assert eng.workspace_bytes(limit, 640, 640) > 0
        up = [o.name for o in eng.plan.ops if o.kind == spec.OP_UPSAMPLE2X]
        with pytest.raises(RuntimeError, match=rf"\((?:{'|'.join(n.replace('.', '[.]') for n in up)})\).*largest batch that fits is {limit}\b"):
            eng.workspace_bytes(limit + 1, 640, 640)
    finally:
        eng.close()


@pytest.mark.parametrize("precision,eb", [("bf16", 2), ("fp32", 4)])
def test_engine_sizing_limit_at_32_px_tiles(synth_ck, precision, eb):
    """Sizing only, nothing launched: at 32 x 32 tiles the sizing call takes the largest batch the restated predicates give for the engine's
    plan -- 32767, set by the row guard of the second upsample (model.15: B x 2 input rows < 65536), below the 65535 grid cap -- and
    refuses one more, naming that op and that batch."""
    from aquaculture_amd.engine import Engine
    eng = Engine(synth_ck, precision, 0)
    try:
        limit, op = guards.plan_batch_limit(eng.plan, 32, 32, eb)
        assert 0 < limit < guards.BATCH_CAP and op is not None, (limit, op)
        assert eng.workspace_bytes(limit, 32, 32) > 0
        with pytest.raises(RuntimeError, match=rf"\({op.replace('.', '[.]')}\).*largest batch that fits is {limit}\b"):
            eng.workspace_bytes(limit + 1, 32, 32)
        assert eng._ws is None and not eng._slots, "sizing allocated a workspace"
    finally:
        eng.close()
