"""Every copy of the fused bias + SiLU (+ residual) + bf16-pack epilogue over a trained model's activation range.

The families' parity tests keep the pre-activation z inside +-6 and compare with an absolute floor; here tests/silu_range.py's Z_GRID
(0 .. +-104, the exp2 / rcp overflow block round -88, +1000) is laid over the output channels as the bias, rotated until every value has
sat in every position of an 8-channel store group, and every element is held to silu_tol: an fp64 reference of the same operation on the
kernel's own operands under a derived bound that stays relative on the negative tail.  Set-ups (channel slices, guard channels, variant
switches, seeds) are those of the families' own tests at their smallest shapes; only the bias (and for the stage-1 sweeps of the two-stage
kernels the second convolution's weights) and the comparator differ.

Each case asserts: every output finite; every element inside the bound; guard channels untouched; and that the launches really spanned
the range (z <= -88.73 and >= 88 seen, every Z_GRID value within 3 of some pre-activation) -- RangeCheck.finish fails otherwise.

  * aq_conv2d (conv_device.h: implicit-GEMM and halo kernels; conv_igemm.hip), every configuration, bf16 / fp32 / f16x3.  f16x3 keeps its
    own rule (within max(4 x the exact-fp32 kernel's error, 2e-6) of fp64 against the per-channel scale) beside the fp32-mode bound.
  * aq_stem_conv: the LDS-DMA kernel, the plain bf16 kernel (W % 4 != 0), fp32; aq_stem_conv_scaled, both flips.
  * aq_conv1x1_direct (with and without the activation), aq_conv1x1_asm (both tile heights), aq_conv3x3s2_direct, aq_conv3x3_pl_s2,
    aq_conv3x3_pl (every build of test_planar_conv3x3_matches_reference), aq_conv3x3_pl_f8, aq_conv1x1_direct_f8out (codes).
  * aq_downblock and aq_bottleneck (C = 16 .. 96, HIP and assembly builds), (a) stage 1 over the range through a second convolution that is
    one permuted centre tap of 2^-4, (b) stage 2 over the range, both in silu_range's two-stage form.
  * aq_stemdown and aq_bottleneck_c3tail: bit-identical to the composed kernels (range-checked above) with every bias on the grid.
  * aq_head_decode and aq_detect_decode: sigmoid on logits of the grid.

Largest err / tol per family, measured on an MI355X in the one run this file was written from (recorded by RangeCheck into
silu_range.WORST and printed, not asserted; every family passed, so no kernel needed a fix).  A bf16 family sits just below 1 by
construction: half an ulp is 2^-8 of a value at the bottom of its binade, which is the bound's leading term; the room above it is what the
other terms leave.

    family                                        err / tol
    conv2d bf16, 3x3 / 1x1 (all configurations)   0.976 / 0.984
    conv2d fp32, 3x3 / 1x1                        0.107 / 0.347
    conv2d f16x3, 3x3 / 1x1                       0.063 / 0.347
    stem bf16 LDS-DMA / bf16 plain / fp32         0.975 / 0.973 / 0.347
    stem_scaled bf16 / fp32                       0.800 / 0.347
    conv1x1_direct 96->96 / 384->192              0.987 / 0.988
    conv1x1_asm nb13 / nb7                        0.979 / 0.979
    conv3x3s2_direct                              0.961
    conv3x3_pl_s2                                 0.975
    conv3x3_pl 13asm, 13slot-asm, 13pm-asm,
               13, 10, 7 (each)                   0.990        (7asm, 8asm: not built, skipped)
    conv3x3_pl_f8                                 0.973
    downblock stage 1 / stage 2                   0.915 / 0.814
    bottleneck HIP, stage 1, C = 16 32 48 64 96   0.986 0.986 0.967 0.984 0.990
    bottleneck HIP, stage 2, C = 16 32 48 64 96   0.961 0.958 0.821 0.957 0.917
    bottleneck asm, stage 1 / 2, C = 48           0.984 / 0.952
    bottleneck asm, stage 1 / 2, C = 96           0.988 / 0.949
    conv1x1_direct_f8out                          every code equal to the reference's (no neighbouring code)
    head_decode cin 192 / 384                     0.001 / 0.002 of the family's row bound
    detect_decode                                 0.141 of the family's bound
    stemdown, c3tail                              bit-identical to the composed kernels
"""
import ctypes as C
import functools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from cu_cases import btl_is_asm, stem_uses_dma
from silu_range import WORST, Z_GRID, RangeCheck, grid_bias, grid_rotations, silu64, silu_tol
from test_gpu_c3tail import _assert_same, _fused, _inputs, _two_launches, _weights
from test_gpu_conv import CASES
from test_gpu_fp8 import F8_CASES
from test_gpu_head_decode import ANCHORS, check_level, make_level, reference as head_reference
from test_gpu_nms import _assert_decode_bounds, _decode, _oracle_decode
from test_gpu_poison_kernels import C3TAIL_SHAPES

pytestmark = pytest.mark.gpu


def nchw(t):
    return t.permute(0, 3, 1, 2)


def terms(x_nhwc, w, stride=1, pad=0):
    """(conv(x, w), conv(|x|, |w|)) in float64, NHWC: the bias-free pre-activation and its absolute sum, from the kernel's own operands."""
    xd, wd = nchw(x_nhwc.double().cpu()), w.double()
    lin = F.conv2d(xd, wd, None, stride=stride, padding=pad)
    mag = F.conv2d(xd.abs(), wd.abs(), None, stride=stride, padding=pad)
    return lin.permute(0, 2, 3, 1).contiguous(), mag.permute(0, 2, 3, 1).contiguous()


def sweep(chk, cout, lin, mag, launch, mode="bf16", act=True, res=None, extra_dz=None):
    """launch(bias) -> [(label, output)], once per rotation of the grid; every output against the one reference of that rotation."""
    for rot in grid_rotations(cout):
        b = grid_bias(cout, rot)
        z = lin + b.double()
        ref, tol = silu_tol(z, mag + b.double().abs(), res, mode, act, extra_dz)
        if act:
            chk.span(z)
        for label, got in launch(b):
            chk.add(got, z, ref, tol, f"rotation {rot} {label}")


# ---- aq_conv2d -------------------------------------------------------------------------------------------------------------------------
CONV_RANGE_CASES = [(1, 9, 7, 32, 64, 3, 1, True, True), (2, 20, 20, 64, 64, 1, 1, True, False)]
assert all(c in CASES for c in CONV_RANGE_CASES)


@pytest.mark.parametrize("case", CONV_RANGE_CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_conv2d_every_configuration(lib, case, precision):
    from aquaculture_amd import engine
    B, H, W, cin, cout, k, stride, act, use_res = case
    g = torch.Generator().manual_seed(1234 + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    torch.randn(cout, generator=g)                                               # (the family's bias draw: the residual keeps its values)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(B, Ho, Wo, cout, generator=g) if use_res else None
    dt = torch.float32 if precision == "fp32" else torch.bfloat16
    xd = x.to(dt).cuda()
    rd = res.to(dt).cuda() if res is not None else None
    lin, mag = terms(xd, w.bfloat16() if precision == "bf16" else w, stride, pad)
    ran = set()

    def launch(b):
        for cfg in range(lib.aq_conv_num_configs()):
            try:
                out = engine.conv2d_nhwc(xd, w, b, stride=stride, act=act, residual=rd, precision=precision, cfg=cfg)
            except RuntimeError as err:          # tile shape not applicable to this layer (e.g. halo kernel on a 1x1 conv)
                assert "halo conv" in str(err), err
                continue
            ran.add(cfg)
            yield f"cfg {cfg}", out

    chk = RangeCheck(f"conv2d {precision} {k}x{k}")
    sweep(chk, cout, lin, mag, launch, mode=precision, res=rd.cpu() if rd is not None else None)
    assert len(ran) >= 10
    chk.finish()


@pytest.mark.parametrize("case", CONV_RANGE_CASES)
def test_conv2d_split_mode(lib, case):
    """f16x3: the family's own rule against the per-channel scale, and fp32 mode's bound."""
    from aquaculture_amd import engine
    B, H, W, cin, cout, k, stride, act, use_res = case
    g = torch.Generator().manual_seed(4321 + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g) * 2.0
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    w = w * (10.0 ** torch.linspace(-3, 1, cout)).view(-1, 1, 1, 1)            # rows from 1e-3 to 10 times the usual scale
    torch.randn(cout, generator=g)
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    res = torch.randn(B, Ho, Wo, cout, generator=g) if use_res else None
    xd = x.cuda()
    rd = res.cuda() if res is not None else None
    lin, mag = terms(x, w, stride, pad)
    chk = RangeCheck(f"conv2d f16x3 {k}x{k}")
    ran = set()
    for rot in grid_rotations(cout):
        b = grid_bias(cout, rot)
        z = lin + b.double()
        ref, tol = silu_tol(z, mag + b.double().abs(), res, "fp32")
        chk.span(z)
        scale = ref.abs().amax(dim=(0, 1, 2), keepdim=True).clamp_min(1e-30)       # per output channel
        e32 = None
        for cfg in range(lib.aq_conv_num_configs()):
            try:
                out = engine.conv2d_nhwc(xd, w, b, stride=stride, act=act, residual=rd, precision="f16x3", cfg=cfg).cpu().double()
            except RuntimeError as err:
                assert "halo conv" in str(err), err
                continue
            ran.add(cfg)
            e3 = ((out - ref).abs() / scale).max().item()
            if e32 is None:
                o32 = engine.conv2d_nhwc(xd, w, b, stride=stride, act=act, residual=rd, precision="fp32", cfg=cfg).cpu().double()
                e32 = ((o32 - ref).abs() / scale).max().item()
            assert e3 <= max(4.0 * e32, 2e-6), (rot, cfg, e3, e32)
            chk.add(out, z, ref, tol, f"rotation {rot} cfg {cfg}")
    assert len(ran) >= 10
    chk.finish()


# ---- stem ------------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,precision", [((1, 16, 24), "bf16"), ((1, 16, 24), "fp32"), ((1, 16, 26), "bf16")])
def test_stem(lib, shape, precision):
    from aquaculture_amd import engine
    B, H, W = shape
    assert stem_uses_dma(precision, W) == (shape == (1, 16, 24) and precision == "bf16")
    g = torch.Generator().manual_seed(H * 31 + W)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    xin = x.float() / 255
    if precision == "bf16":
        xin, wq = xin.bfloat16(), w.bfloat16()
    else:
        wq = w
    lin, mag = terms(xin, wq, 2, 2)
    xd = x.cuda()
    kind = "LDS-DMA" if stem_uses_dma(precision, W) else "plain"
    chk = RangeCheck(f"stem {precision} {kind}")
    sweep(chk, 48, lin, mag, lambda b: [("", engine.stem_conv_nhwc(xd, w, b, precision=precision))], mode=precision)
    chk.finish()


@pytest.mark.parametrize("flip", [False, True])
@pytest.mark.parametrize("precision", ["bf16", "fp32"])
def test_stem_scaled(lib, precision, flip):
    """The kernel interpolates the pixels in fp32 and, in bf16 mode, rounds them to bf16 itself: the reference keeps torch's interpolated
    input unrounded and the bound takes silu_range's input term 2^-8 sum |w| |x| (the two-stage F)."""
    from aquaculture_amd import engine
    from cu_cases import scaled_pass
    from test_gpu_augment import scaled_input
    B, H, W = 1, 64, 64
    ps = scaled_pass(H, W, flip)
    g = torch.Generator().manual_seed(H + 2 * flip)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    x = torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(H + W + flip), dtype=torch.uint8)
    xin = scaled_input(x.permute(0, 3, 1, 2).float() / 255, ps, W).permute(0, 2, 3, 1)
    lin, mag = terms(xin, w.bfloat16() if precision == "bf16" else w, 2, 2)
    xd = x.cuda()
    chk = RangeCheck(f"stem_scaled {precision}")
    sweep(chk, 48, lin, mag, lambda b: [("", engine.stem_conv_scaled_nhwc(xd, w, b, ps.h, ps.w, ps.hp, ps.wp, flip, precision=precision))],
          mode=precision, extra_dz=2.0 ** -8 * mag if precision == "bf16" else None)
    chk.finish()


# ---- 1x1 kernels -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(96, 96), (384, 192)])
def test_direct_conv1x1(lib, cin, cout):
    from aquaculture_amd import engine
    B, H, W = 1, 16, 16
    g = torch.Generator().manual_seed(cin + H)
    xw = (torch.randn(B, H, W, cin + 16, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:8 + cin]
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    lin, mag = terms(x, w.bfloat16())
    outw = torch.full((B, H, W, cout + 8), 7.0, dtype=torch.bfloat16, device="cuda")

    def launch(act, b):
        engine.conv1x1_direct_nhwc(x, w, b, act, out=outw[..., 8:])
        assert (outw[..., :8] == 7.0).all()
        return [("", outw[..., 8:])]

    chk = RangeCheck(f"conv1x1_direct {cin}->{cout}")
    for act in (True, False):
        sweep(chk, cout, lin, mag, functools.partial(launch, act), act=act)
    chk.finish()


@pytest.mark.parametrize("cin,cout", [(96, 384), (768, 384)])
@pytest.mark.parametrize("npix_shape", [(1, 5, 7), (1, 13, 16)])
@pytest.mark.parametrize("family", [13, 7])
def test_asm_conv1x1(lib, monkeypatch, cin, cout, npix_shape, family):
    from aquaculture_amd import engine
    monkeypatch.setenv("AQ_C1_ASM_NB", str(family))
    B, H, W = npix_shape
    g = torch.Generator().manual_seed(cin + H)
    xw = (torch.randn(B, H, W, cin + 16, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:8 + cin]
    w = torch.randn(cout, cin, 1, 1, generator=g) * (2.0 / cin) ** 0.5
    lin, mag = terms(x, w.bfloat16())
    outw = torch.full((B, H, W, cout + 8), 7.0, dtype=torch.bfloat16, device="cuda")

    def launch(b):
        engine.conv1x1_asm_nhwc(x, w, b, out=outw[..., 4:4 + cout])
        assert (outw[..., :4] == 7.0).all() and (outw[..., 4 + cout:] == 7.0).all()
        return [("", outw[..., 4:4 + cout])]

    chk = RangeCheck(f"conv1x1_asm nb{family}")
    sweep(chk, cout, lin, mag, launch)
    chk.finish()


# ---- 3x3 kernels -----------------------------------------------------------------------------------------------------------------------
def test_direct_conv3x3s2(lib):
    from aquaculture_amd import engine
    B, H, W = 1, 6, 10
    g = torch.Generator().manual_seed(H * 5 + W)
    xw = (torch.randn(B, H, W, 112, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:104]
    w = torch.randn(192, 96, 3, 3, generator=g) * (2.0 / (9 * 96)) ** 0.5
    lin, mag = terms(x, w.bfloat16(), 2, 1)
    outw = torch.full((B, H // 2, W // 2, 200), 7.0, dtype=torch.bfloat16, device="cuda")

    def launch(act, b):
        engine.conv3x3s2_direct_nhwc(x, w, b, act, out=outw[..., 8:])
        assert (outw[..., :8] == 7.0).all()
        return [("", outw[..., 8:])]

    chk = RangeCheck("conv3x3s2_direct")
    for act in (True, False):
        sweep(chk, 192, lin, mag, functools.partial(launch, act), act=act)
    chk.finish()


def test_planar_conv3x3_s2(lib):
    from aquaculture_amd import engine
    B, H, W, cin, c, act = 1, 18, 14, 64, 192, True
    assert engine.load_library().aq_conv3x3_pl_s2_supported(cin, c, B, H, W)
    g = torch.Generator().manual_seed(c * 5 + H * 3 + cin)
    xw = (torch.randn(B, H, W, cin + 16, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:8 + cin]
    w = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    lin, mag = terms(x, w.bfloat16(), 2, 1)
    outw = torch.full((B, H // 2, W // 2, c + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    out = outw[..., 16:16 + c]

    def launch(b):
        engine.conv3x3_pl_s2_nhwc(x, w, b, act, out=out)
        assert (outw[..., :16] == 7.0).all() and (outw[..., 16 + c:] == 7.0).all(), "wrote outside its channel slice"
        return [("", out)]

    chk = RangeCheck("conv3x3_pl_s2")
    sweep(chk, c, lin, mag, launch)
    chk.finish()


PL_RANGE_CASES = [(1, 9, 7, 192, 192, "sep"), (2, 13, 24, 128, 192, None), (2, 20, 20, 384, 384, "sep")]


@functools.lru_cache(maxsize=None)
def planar_case(case):
    """Inputs and the fp64 terms of one planar case, shared by every build (the family's set-up at its nb = 13 seed)."""
    B, H, W, cin, c, resmode = case
    g = torch.Generator().manual_seed(c * 7 + H * 3 + 13)
    xw = (torch.randn(B, H, W, cin + 16, generator=g) * 0.8).bfloat16()
    w = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    torch.randn(c, generator=g)
    resw = torch.randn(B, H, W, c + 8, generator=g).bfloat16() if resmode == "sep" else None
    lin, mag = terms(xw[..., 8:8 + cin], w.bfloat16(), 1, 1)
    return xw, w, resw, lin, mag


@pytest.mark.parametrize("case", PL_RANGE_CASES)
@pytest.mark.parametrize("nb", ["13asm", "13slot-asm", "13pm-asm", "7asm", "8asm", 13, 10, 7])
def test_planar_conv3x3(lib, case, nb, monkeypatch):
    from aquaculture_amd import engine
    B, H, W, cin, c, resmode = case
    build = nb
    monkeypatch.setenv("AQ_PL_ASM", "1" if isinstance(nb, str) else "0")
    if nb in ("13slot-asm", "13pm-asm"):
        monkeypatch.setenv("AQ_PL_PM", "0" if nb == "13slot-asm" else "2")
        nb = "13asm"
    if isinstance(nb, str) and not lib.aq_conv3x3_pl_asm_family(int(nb[:-3])):
        pytest.skip("experimental assembly family: built only with AQ_GEN_EXPERIMENTAL=1")
    nb = int(nb[:-3]) if isinstance(nb, str) else nb
    monkeypatch.setenv("AQ_PL_NB", str(nb))
    xw, w, resw, lin, mag = planar_case(case)
    x = xw.cuda()[..., 8:8 + cin]
    outw = torch.full((B, H, W, c + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    out = outw[..., 16:16 + c]
    res = resw.cuda()[..., 8:] if resw is not None else None

    def launch(b):
        engine.conv3x3_pl_nhwc(x, w, b, True, residual=res, out=out)
        assert (outw[..., :16] == 7.0).all() and (outw[..., 16 + c:] == 7.0).all(), "wrote outside its channel slice"
        return [("", out)]

    chk = RangeCheck(f"conv3x3_pl {build}")
    sweep(chk, c, lin, mag, launch, res=resw[..., 8:] if resw is not None else None)
    chk.finish()


# ---- two-stage kernels -----------------------------------------------------------------------------------------------------------------
K2 = 4                                          # stage-1 sweeps: z2 = 2^-4 t <= 1006 / 16, inside +-104


def tap_weights(c_out, c_in, k):
    """[c_out, c_in, k, k], zero but for the centre tap: output channel c reads channel perm[c] = (5 c + 3) % c_in, times 2^-K2 -- each
    output depends on exactly one stage-1 value, which sat in another lane and another store position."""
    perm = [(5 * c + 3) % c_in for c in range(c_out)]
    assert sorted(perm) == list(range(c_in))
    w = torch.zeros(c_out, c_in, k, k)
    w[torch.arange(c_out), torch.tensor(perm), k // 2, k // 2] = 2.0 ** -K2
    return w, perm


def two_stage(chk, c1, c2, lin1, mag1, run, b1_fixed, w2, pad2, res, which):
    """which == 1: b1 on the grid, b2 = 0 (w2: tap_weights); which == 2: b1 as the family draws it, b2 on the grid.  run(b1, b2) -> output."""
    if which == 2:
        t = silu64(lin1 + b1_fixed.double())
        lin2, mag2 = terms(t, w2, 1, pad2)
    for rot in grid_rotations(c1 if which == 1 else c2):
        if which == 1:
            b1, b2 = grid_bias(c1, rot), torch.zeros(c2)
            z1 = lin1 + b1.double()
            chk.span(z1)
            lin2, mag2 = terms(silu64(z1), w2, 1, pad2)
        else:
            b1, b2 = b1_fixed, grid_bias(c2, rot)
        z2 = lin2 + b2.double()
        if which == 2:
            chk.span(z2)
        ref, tol = silu_tol(z2, mag2 + b2.double().abs(), res, extra_dz=2.0 ** -8 * mag2)
        chk.add(run(b1, b2), z2, ref, tol, f"stage {which} rotation {rot}")


@pytest.mark.parametrize("which", [1, 2])
def test_downblock(lib, which):
    from aquaculture_amd import engine
    B, H, W = 1, 6, 10
    g = torch.Generator().manual_seed(H * 7 + W)
    xw = (torch.randn(B, H, W, 64, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:56]
    wa = torch.randn(96, 48, 3, 3, generator=g) * (2.0 / (9 * 48)) ** 0.5
    wb = torch.randn(96, 96, 1, 1, generator=g) * (2.0 / 96) ** 0.5
    ba = torch.randn(96, generator=g) * 0.2
    if which == 1:
        wb = tap_weights(96, 96, 1)[0]
    outw = torch.full((B, H // 2, W // 2, 112), 7.0, dtype=torch.bfloat16, device="cuda")
    lin1, mag1 = terms(x, wa.bfloat16(), 2, 1)

    def run(b1, b2):
        engine.downblock_nhwc(x, wa, b1, wb, b2, out=outw[..., 16:])
        assert (outw[..., :16] == 7.0).all(), "wrote outside its channel slice"
        return outw[..., 16:]

    chk = RangeCheck(f"downblock stage {which}")
    two_stage(chk, 96, 96, lin1, mag1, run, ba, wb.bfloat16(), 0, None, which)
    chk.finish()


BTL_SHAPES = [(1, 7, 5), (2, 16, 32)]


def test_bottleneck_shapes_reach_both_builds():
    for c in (48, 96):
        assert {btl_is_asm(c, *s) for s in BTL_SHAPES} == {True, False}, c
    assert not any(btl_is_asm(c, *s) for c in (16, 32, 64) for s in BTL_SHAPES)


@pytest.mark.parametrize("which", [1, 2])
@pytest.mark.parametrize("c", [16, 32, 48, 64, 96])
@pytest.mark.parametrize("shape", BTL_SHAPES)
def test_bottleneck(lib, c, shape, which):
    from aquaculture_amd import engine
    B, H, W = shape
    g = torch.Generator().manual_seed(c * 1000 + H)
    xw = (torch.randn(B, H, W, 2 * c, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:8 + c]
    w1 = torch.randn(c, c, 1, 1, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5
    b1 = torch.randn(c, generator=g) * 0.2
    if which == 1:
        w2 = tap_weights(c, c, 3)[0]
    outw = torch.full((B, H, W, c + 16), 7.0, dtype=torch.bfloat16, device="cuda")
    lin1, mag1 = terms(x, w1.bfloat16())
    build = "asm" if btl_is_asm(c, B, H, W) else "HIP"
    chk = RangeCheck(f"bottleneck c{c} {build} stage {which}")
    for shortcut in (True, False):
        def run(bb1, bb2):
            engine.bottleneck_nhwc(x, w1, bb1, w2, bb2, shortcut, out=outw[..., 16:])
            assert (outw[..., :16] == 7.0).all(), "wrote outside its channel slice"
            return outw[..., 16:]

        two_stage(chk, c, c, lin1, mag1, run, b1, w2.bfloat16(), 1, x.cpu() if shortcut else None, which)
    chk.finish()


# ---- fused composites: bit-identical to the composed kernels -----------------------------------------------------------------------------
COMPOSITE_ROTATIONS = (0, 11, 22)


def test_stemdown_on_the_grid(lib):
    from aquaculture_amd import engine
    B, Hi, Wi = 1, 16, 24
    g = torch.Generator().manual_seed(Hi + Wi)
    tiles = torch.randint(0, 256, (B, Hi, Wi, 3), generator=g, dtype=torch.uint8).cuda()
    ws = torch.randn(48, 3, 6, 6, generator=g) * 0.25
    wa = torch.randn(96, 48, 3, 3, generator=g) * (2.0 / (9 * 48)) ** 0.5
    wb = torch.randn(96, 96, 1, 1, generator=g) * (2.0 / 96) ** 0.5
    for rot in COMPOSITE_ROTATIONS:
        bs, ba, bb = grid_bias(48, rot), grid_bias(96, rot + 5), grid_bias(96, rot + 17)
        x = engine.stem_conv_nhwc(tiles, ws, bs, act=True, precision="bf16")
        ref = engine.downblock_nhwc(x, wa, ba, wb, bb)
        outw = torch.full((B, Hi // 4, Wi // 4, 96 + 16), 5.0, dtype=torch.bfloat16, device="cuda")
        got = engine.stemdown_nhwc(tiles, ws, bs, wa, ba, wb, bb, out=outw[..., 8:104])
        assert bool(torch.isfinite(ref.float()).all())
        assert torch.equal(got.cpu().view(torch.int16), ref.cpu().view(torch.int16)), rot
        assert (outw[..., :8] == 5.0).all() and (outw[..., 104:] == 5.0).all(), "wrote outside its channel slice"
        assert float(ref.float().abs().mean()) > 0.05


@pytest.mark.parametrize("shortcut", [True, False])
def test_c3tail_on_the_grid(lib, shortcut):
    from aquaculture_amd import engine
    B, H, W = min(C3TAIL_SHAPES, key=lambda s: s[0] * s[1] * s[2])
    assert engine.bottleneck_c3tail_supported(B, H, W)
    x, cat = _inputs(B, H, W, seed=W)
    for rot in COMPOSITE_ROTATIONS:
        p = _weights(B + H)
        p.update(b1=grid_bias(48, rot), b2=grid_bias(48, rot + 5), b3=grid_bias(96, rot + 17))
        ref = _two_launches(x, cat, p, shortcut)
        assert bool(torch.isfinite(ref.float()).all())
        _assert_same(_fused(x, cat, p, shortcut), ref, f"rotation {rot}")
        assert float(ref.float().abs().mean()) > 0.01


# ---- fp8 -------------------------------------------------------------------------------------------------------------------------------
def test_direct_conv1x1_f8out_codes(lib):
    """The producer of an fp8 pair with its bias on the grid and a scale at which |z| >= 60 saturates: never the NaN code, the largest code
    448, every code the code of the fp64 reference or its neighbour."""
    from aquaculture_amd import engine
    c, B, H, W = 192, 1, 7, 9
    g = torch.Generator().manual_seed(c + H)
    xw = (torch.randn(B, H, W, c + 16, generator=g) * 0.8).bfloat16().cuda()
    x = xw[..., 8:8 + c]
    w = torch.randn(c, c, 1, 1, generator=g) * (2.0 / c) ** 0.5
    lin, mag = terms(x, w.bfloat16())
    scale = 60.0 / 448.0
    wk = np.ascontiguousarray(w.permute(0, 2, 3, 1).float().numpy())
    n = C.c_size_t()
    wp = wk.ctypes.data_as(C.POINTER(C.c_float))
    engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, wbuf.data_ptr(), C.byref(n), engine._stream_ptr()))
    pitch = 2 * c + 32
    chk = RangeCheck("conv1x1_direct_f8out")
    same = []
    for rot in grid_rotations(c):
        b = grid_bias(c, rot)
        z = lin + b.double()
        chk.span(z)
        want = (silu64(z) / scale).clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
        bbuf = b.cuda()
        out = torch.full((B, H, W, pitch), 0xAA, dtype=torch.uint8, device="cuda")
        engine._check(lib.aq_conv1x1_direct_f8out(x.data_ptr(), c + 16, 0, out.data_ptr(), pitch, 16, c, c, wbuf.data_ptr(), bbuf.data_ptr(),
                                                  B * H * W, 1, scale, engine._stream_ptr()))
        torch.cuda.synchronize()
        got = out[..., 16:16 + c].cpu()
        assert (out[..., :16] == 0xAA).all() and (out[..., 16 + c:] == 0xAA).all()
        gv = got.view(torch.float8_e4m3fn).float()
        assert not torch.isnan(gv).any() and float(gv.max()) == 448.0
        order = lambda codes: (codes & 0x7f).int() * (1 - 2 * (codes >> 7).int())       # signed position on the code line; +-0 -> 0
        apart = (order(got) - order(want)).abs()
        assert int(apart.max()) <= 1, (rot, z[apart > 1][:4].tolist(), gv[apart > 1][:4].tolist())
        same.append(float((apart == 0).float().mean()))
    chk.finish()
    WORST["conv1x1_direct_f8out"] = 1.0 - min(same)                                         # the share of neighbouring codes
    print(f"activation range, conv1x1_direct_f8out: share of neighbouring codes {1.0 - min(same):.4f}")


def test_planar_conv3x3_f8(lib):
    from aquaculture_amd import engine
    B, H, W, cin, c, resmode, act = min(F8_CASES, key=lambda s: s[0] * s[1] * s[2] * s[3] * s[4])
    assert resmode is None and act and lib.aq_conv3x3_pl_f8_supported(cin, c, B, H, W)
    g = torch.Generator().manual_seed(c * 3 + H * 5 + cin)
    x = torch.randn(B, H, W, cin + 32, generator=g).abs() * 0.9 - 0.25
    act_scale = float(x.abs().max()) / 448.0
    xq = (x / act_scale).to(torch.float8_e4m3fn)
    xs = xq.cuda()[..., 16:16 + cin]
    w = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    w = w * (10.0 ** torch.linspace(-1, 1, c)).view(-1, 1, 1, 1)
    ws = w.abs().amax(dim=(1, 2, 3), keepdim=True) / 448.0
    wq = (w / ws).to(torch.float8_e4m3fn)
    lin, mag = terms(xq[..., 16:16 + cin].float(), wq.float(), 1, 1)
    deq = act_scale * ws.view(1, 1, 1, -1).double()
    lin, mag = lin * deq, mag * deq
    outw = torch.full((B, H, W, c + 24), 7.0, dtype=torch.bfloat16, device="cuda")
    out = outw[..., 16:16 + c]

    def launch(b):
        engine.conv3x3_pl_f8_nhwc(xs, act_scale, w, b, act, out=out)
        assert (outw[..., :16] == 7.0).all() and (outw[..., 16 + c:] == 7.0).all(), "wrote outside its channel slice"
        return [("", out)]

    chk = RangeCheck("conv3x3_pl_f8")
    sweep(chk, c, lin, mag, launch)
    chk.finish()


# ---- detection tail --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin", [192, 384])
def test_head_decode(lib, cin):
    """1 / (1 + expf(-x)) on logits of the grid, through the family's reference and comparator.  cap holds every candidate, so the count
    never passes the slot count.  A logit of +100 gives a confidence of exactly 1.0 and finite boxes, an objectness logit of -100 no row."""
    from aquaculture_amd import engine
    B, ny, nx, nc, off, stride, thr = 3, 5, 7, 5, 1000, 16.0, 0.25
    na, no, hw = 3, nc + 5, ny * nx
    xw, x, w, _ = make_level(B, ny, nx, cin, na, nc, cin + ny)
    lin = x.reshape(-1, cin).double() @ w.bfloat16().double().t()
    cap = na * hw
    chk = RangeCheck(f"head_decode {cin}")
    sure_rows = no_rows = 0
    for rot in range(len(Z_GRID)):
        b = grid_bias(na * no, rot)
        raw = (lin + b.double()).reshape(B, hw, na, no).permute(0, 2, 1, 3).reshape(B, cap, no)         # candidate order (a, y, x)
        chk.span(raw)
        counts, cand, rows = engine.head_decode_level(xw.cuda()[..., 8:8 + cin], w, b, off, stride, ANCHORS, nc, thr, cap)
        ref = head_reference(x, w, b, ANCHORS, nc, stride)
        rel, _, _, _ = check_level(counts, cand, rows, ref, off, thr, cap)
        chk.worst = max(chk.worst, rel)
        counts, cand, rows = counts.cpu(), cand.cpu(), rows.cpu()
        for bi in range(B):
            n = int(counts[bi])
            assert n <= cap and (cand[bi, n:] == -1).all()
            got, r = (cand[bi, :n] - off).long(), rows[bi, :n]
            assert bool(torch.isfinite(r).all())
            lg = raw[bi, got]
            assert bool((r[:, 4:][lg[:, 4:] >= 20.0] == 1.0).all())
            present = torch.zeros(cap, dtype=torch.bool)
            present[got] = True
            assert bool(present[raw[bi, :, 4] >= 20.0].all()) and not bool(present[raw[bi, :, 4] <= -80.0].any())
            sure_rows += int((raw[bi, :, 4] >= 95.0).sum())
            no_rows += int((raw[bi, :, 4] <= -95.0).sum())
    assert sure_rows > 0 and no_rows > 0
    chk.finish()


def test_detect_decode(lib):
    """The unfused decode on fp32 head maps whose channels carry the grid, against the oracle's decode under the family's bounds."""
    from aquaculture_amd import checkpoint
    from oracle import yolov5_oracle as O
    ck = checkpoint.synthetic_checkpoint("yolov5m", 5)
    B, H, W, na, nc, conf, head_ld = 3, 64, 96, 3, 5, 0.25, 32
    no = nc + 5
    g = torch.Generator().manual_seed(45)
    noise = [torch.randn(B, H // s, W // s, head_ld, generator=g) * 1.5 for s in (8, 16, 32)]
    m = O.OracleModel({}, nc, ck.anchors, ck.stride, ck.bn_eps)
    chk = RangeCheck("detect_decode")
    sure_rows = no_rows = 0
    for rot in range(len(Z_GRID)):
        heads = [h + grid_bias(head_ld, rot + 9 * i) for i, h in enumerate(noise)]
        chk.span(torch.cat([h[..., :na * no].reshape(-1) for h in heads]))
        want = _oracle_decode(m, [h[..., :na * no] for h in heads])
        N = want.shape[1]
        pred, counts, cand, rows = _decode(lib, [h.cuda().contiguous() for h in heads], H, W, nc, na, ck.anchor_grid_px().numpy().tolist(), ck.stride,
                                           conf, N, head_ld)
        assert bool(torch.isfinite(pred).all())
        d, bound = _assert_decode_bounds(pred, want, f"detect_decode rotation {rot}")
        chk.worst = max(chk.worst, d / bound)
        assert counts.tolist() == (pred[..., 4] > conf).sum(1).tolist()
        obj = torch.cat([h[..., :na * no].reshape(B, -1, na, no).permute(0, 2, 1, 3).reshape(B, -1, no) for h in heads], 1)[..., 4]
        for bi in range(B):
            n = int(counts[bi])
            present = torch.zeros(N, dtype=torch.bool)
            present[cand[bi, :n].long()] = True
            assert bool(present[obj[bi] >= 20.0].all()) and not bool(present[obj[bi] <= -80.0].any())
            assert bool((pred[bi, :, 4][obj[bi] >= 20.0] == 1.0).all())
            assert torch.equal(rows[bi, :n], pred[bi, cand[bi, :n].long()])
        sure_rows += int((obj >= 95.0).sum())
        no_rows += int((obj <= -95.0).sum())
    assert sure_rows > 0 and no_rows > 0
    chk.finish()
