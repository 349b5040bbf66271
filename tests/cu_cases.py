"""Every launcher that sizes a persistent grid from the CU count, on shapes of a few tiles -- test infrastructure (a plain module with a
``main``: imported by tests/test_cu_cases.py, run as a child process by tests/test_gpu_cu_counts.py; not a conftest, not collected).

    python tests/cu_cases.py --out FILE.json

runs CASES in this process, under whatever AQ_NUM_CUS the environment holds (the library reads it once per process; this module never sets
it), and writes one record per case: id, n_tiles (the work-item count of the launch, computed here from the tile constants), what the
family's comparator measured, its verdict `ok`, and the sha256 of the owned output bytes.  The parent compares the digests of children
run at different CU counts: which workgroup computes a tile must not change a byte.

References and tolerances are the families' own: each case calls the reference and asserts the bounds of the family's parity test
(imported from it, as tests/test_gpu_poison_kernels.py does).  After every case the device is synchronised; on a HIP error the records so
far are written and the process exits non-zero without launching anything more.

The ladders: per convolution family, one image and one tile row (or one tile column where the kernel wants it) whose tile count runs through
LADDER, once in whole tiles and once with a partial last tile.  With 1 .. 8 resident workgroups per CU that gives every family workgroups
of 1, 2, 3 and >= 4 trips and uneven last trips at AQ_NUM_CUS = 1, 2, 3.  The families tiled in image rows have a third ladder with a partial
tile in the middle of the walk (MID_LADDER).

A case that launches nothing -- a halo configuration the launcher refuses for the layer, an assembly family this build does not hold --
is recorded with `skipped` and the reason; the parent lists them.
"""
import argparse
import ctypes as C
import functools
import hashlib
import json
import os
import re
import sys
from typing import Callable, NamedTuple, Optional, Tuple

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
for _p in (ROOT, HERE):
    if _p not in sys.path:
        sys.path.insert(0, _p)

from test_gpu_conv import _bottleneck_reference, _ref                                                   # noqa: E402
from test_gpu_head_decode import ANCHORS, WIDTHS, check_level, ksplit, make_level, reference as head_reference   # noqa: E402
from test_gpu_poison_kernels import C3TAIL_SHAPES, CONV_CASES, PL_SHAPES, RESMODES, conv_inputs, downblock_weights   # noqa: E402
from test_gpu_save_crop import SIZES as CROP_SIZES                                                      # noqa: E402
from test_gpu_save_img import MIXED                                                                     # noqa: E402

LADDER = (1, 2, 3, 4, 5, 6, 7, 8, 9, 16, 17, 25)

# ---- tile constants of the launchers (csrc/size_guards.h where it has them, else the launcher named) ---------------------------------
STEM_TW, STEM_TH = 64, 8                                     # kStemTW, kStemTH
DOWN_TW, DOWNBLOCK_TH, CONV3X3S2_TH = 16, 8, 4               # kDownTW, kDownblockTH, kConv3x3s2TH
C1_DIRECT_TP = {(96, 96): 256, (192, 192): 128, (384, 192): 64, (384, 384): 64}      # conv1x1_direct.hip C1Geom::TP per instantiation
C1_ASM_TPX, C1_ASM_NT = {13: 208, 7: 112}, 384               # conv1x1_asm.hip kTPX, kNT
PL_BM, PL_F8_BN, PL_S2_NB = 192, 208, 13                     # conv3x3_pl.hip
# conv_igemm.hip kConfigs, then conv_halo.hip kHalo: (bm, bn) by config id (the child checks them against aq_conv_config_tiles)
IGEMM_TILES = [(256, 256), (192, 256), (128, 256), (96, 512), (64, 512), (32, 512), (192, 128), (128, 128), (64, 256), (96, 256), (64, 128),
               (192, 128), (128, 256), (128, 128), (64, 256), (96, 256), (64, 128), (256, 128), (192, 192), (192, 256), (128, 256)]
HALO_TILES = [(192, 256), (96, 256), (64, 256), (192, 128), (384, 128), (128, 256), (96, 128), (64, 128), (256, 128), (192, 256), (384, 128),
              (256, 256), (128, 256)]
CONV_TILES = IGEMM_TILES + HALO_TILES


def cdiv(a, b):
    return (a + b - 1) // b


def btl_tile(c):
    return (32 if c == 16 else 16), (8 if c == 96 else 16)   # btl_tile_w, btl_tile_h


def btl_is_asm(c, B, H, W):
    """sg::btl_asm_tiles_fit at these small sizes: the assembly builds want two tiles per row (and so per image)."""
    return c in (48, 96) and cdiv(W, 16) >= 2


def tiles_of(g):
    """The work items of the launch described by g (kind, then the dimensions the launcher counts tiles from)."""
    k = g[0]
    if k == "stem":                                          # B, H, W of the uint8 input (the scaled form: of the padded pass)
        return g[1] * cdiv(g[3] // 2, STEM_TW) * cdiv(g[2] // 2, STEM_TH)
    if k == "stemdown":                                      # B, Hi, Wi of the uint8 input; the tiles are the down-block's, of its output
        return g[1] * cdiv(g[3] // 4, DOWN_TW) * cdiv(g[2] // 4, DOWNBLOCK_TH)
    if k in ("downblock", "conv3x3s2"):                      # B, H, W of the input
        return g[1] * cdiv(g[3] // 2, DOWN_TW) * cdiv(g[2] // 2, DOWNBLOCK_TH if k == "downblock" else CONV3X3S2_TH)
    if k == "bottleneck":                                    # C, B, H, W
        tw, th = btl_tile(g[1])
        return g[2] * cdiv(g[4], tw) * cdiv(g[3], th)
    if k == "c3tail":                                        # B, H, W: 16 x 16 tiles
        return g[1] * cdiv(g[3], 16) * cdiv(g[2], 16)
    if k == "c1direct":                                      # cin, cout, npix
        return cdiv(g[3], C1_DIRECT_TP[(g[1], g[2])])
    if k == "c1asm":                                         # family, cout, npix
        return cdiv(g[3], C1_ASM_TPX[g[1]]) * (g[2] // C1_ASM_NT)
    if k == "pl":                                            # pixel blocks per tile, cout, npix (of the output)
        return cdiv(g[3], 16 * g[1]) * (g[2] // PL_BM)
    if k == "conv2d":                                        # config id, cout, npix
        bm, bn = CONV_TILES[g[1]]
        return cdiv(g[2], bm) * cdiv(g[3], bn)
    if k == "head":                                          # cin, npix: workgroup iterations of 64 / split pixels
        return cdiv(g[2], 64 // ksplit(g[1]))
    if k == "count":                                         # counted by the case itself (image-side launchers, the engine)
        return int(g[1])
    raise ValueError(k)


class Case(NamedTuple):
    id: str
    family: str                       # the ladder family, or the launcher family of a stand-alone case
    launchers: Tuple[str, ...]        # exported entry points the case goes through
    geom: tuple                       # tiles_of's argument
    run: Callable                     # () -> (metrics dict, [owned outputs]); raises AssertionError where the comparator fails
    ladder: Optional[str] = None      # "full" / "partial": a ladder case whose last tile is whole / partial
    asm: bool = False                 # a generated-assembly build takes the launch

    @property
    def n_tiles(self):
        return tiles_of(self.geom)


CASES = []
# Order is undefined by design for these: their digest is taken over rows sorted as check_level sorts them (by candidate index)
EXEMPT = {}


def add(id_, family, launchers, geom, run, ladder=None, asm=False):
    CASES.append(Case(id_, family, tuple(launchers), tuple(geom), run, ladder, asm))


def close(got, ref, rtol, atol):
    err = float((got - ref).abs().max())
    torch.testing.assert_close(got, ref, rtol=rtol, atol=atol)
    return {"max_err": err}


def bf16_close(got, ref, atol):
    return close(got.float().cpu(), ref.bfloat16().float(), 2 ** -7, atol)


def env(**kw):
    """The per-call switches of the launchers (read with getenv at every launch)."""
    for k, v in kw.items():
        if v is None:
            os.environ.pop(k, None)
        else:
            os.environ[k] = str(v)


def u8_tiles(B, H, W, seed):
    return torch.randint(0, 256, (B, H, W, 3), generator=torch.Generator().manual_seed(seed), dtype=torch.uint8)


# ---- aq_conv2d ------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=4)
def conv2d_inputs(case, precision):
    B, H, W, cin, cout, k, stride, act, use_res = case
    g = torch.Generator().manual_seed(1234 + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.1
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    xv = x.to(dt)
    rv = torch.randn(B, Ho, Wo, cout, generator=g).to(dt) if use_res else None
    return xv, w, b, rv, _ref(xv, w, b, stride, pad, act, rv, precision == "bf16")


def run_conv2d(case, precision, cfg):
    from aquaculture_amd import engine
    lib = engine.load_library()
    bm, bn = C.c_int(), C.c_int()
    assert lib.aq_conv_num_configs() == len(CONV_TILES) and lib.aq_conv_config_tiles(cfg, C.byref(bm), C.byref(bn)) == 0
    assert (bm.value, bn.value) == CONV_TILES[cfg], (cfg, bm.value, bn.value)
    xv, w, b, rv, ref = conv2d_inputs(case, precision)
    try:
        out = engine.conv2d_nhwc(xv.cuda(), w, b, stride=case[6], act=case[7], residual=rv.cuda() if rv is not None else None, precision=precision, cfg=cfg)
    except RuntimeError as err:                              # a configuration the layer cannot run is refused before any launch,
        assert "halo conv" in str(err), err                  # as the family's parity test expects
        return {"skipped": "refused: " + str(err).split("halo conv: ")[-1][:80]}, []
    m = close(out.cpu(), ref, 2e-5, 2e-5) if precision == "fp32" else close(out.float().cpu(), ref.bfloat16().float(), 2 ** -7, 1e-3)
    return m, [out]


@functools.lru_cache(maxsize=2)
def conv2d_f16x3_inputs(case):
    """Inputs, fp64 reference and the exact-fp32 kernel's error on the same layer, as test_conv_split_mode_is_fp32_grade sets them up."""
    from aquaculture_amd import engine
    B, H, W, cin, cout, k, stride, act, use_res = case
    g = torch.Generator().manual_seed(1234 + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g) * 2.0
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    w = w * (10.0 ** torch.linspace(-3, 1, cout)).view(-1, 1, 1, 1)
    b = torch.randn(cout, generator=g) * 0.1
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    rv = torch.randn(B, Ho, Wo, cout, generator=g) if use_res else None
    y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=stride, padding=pad)
    y = F.silu(y) if act else y
    ref = (y + rv.double().permute(0, 3, 1, 2) if use_res else y).permute(0, 2, 3, 1)
    scale = ref.abs().amax(dim=(0, 1, 2), keepdim=True).clamp_min(1e-30)
    o32 = engine.conv2d_nhwc(x.cuda(), w, b, stride=stride, act=act, residual=rv.cuda() if use_res else None, precision="fp32", cfg=0)
    e32 = ((o32.cpu().double() - ref).abs() / scale).max().item()
    return x, w, b, rv, ref, scale, e32


def run_conv2d_f16x3(case, cfg):
    """The split mode (fp32 activations, three fp16 MFMAs): within 4x the exact-fp32 kernel's error against an fp64 reference."""
    from aquaculture_amd import engine
    x, w, b, rv, ref, scale, e32 = conv2d_f16x3_inputs(case)
    out = engine.conv2d_nhwc(x.cuda(), w, b, stride=case[6], act=case[7], residual=rv.cuda() if rv is not None else None, precision="f16x3", cfg=cfg)
    e3 = ((out.cpu().double() - ref).abs() / scale).max().item()
    assert e3 <= max(4.0 * e32, 2e-6), (cfg, e3, e32)
    torch.testing.assert_close(out.cpu(), ref.float(), rtol=2e-5, atol=2e-5 * float(scale.max()))
    return {"max_rel_err": e3, "fp32_max_rel_err": e32}, [out]


def conv2d_geom(case, cfg):
    B, H, W, cin, cout, k, stride, _, _ = case
    pad = k // 2
    return ("conv2d", cfg, cout, B * ((H + 2 * pad - k) // stride + 1) * ((W + 2 * pad - k) // stride + 1))


for _ci, _case in enumerate(CONV_CASES):
    for _prec in ("fp32", "bf16"):
        for _cfg in range(len(CONV_TILES)):
            if _cfg >= len(IGEMM_TILES) and (_case[5], _case[6]) != (3, 1):
                continue                                     # the halo kernel is 3x3 / stride 1 only
            add(f"conv2d-{_ci}-{_prec}-cfg{_cfg}", "conv2d", ["aq_conv2d"], conv2d_geom(_case, _cfg),
                functools.partial(run_conv2d, _case, _prec, _cfg))
    for _cfg in range(len(IGEMM_TILES)):                     # (the halo kernel has no split-mode build)
        add(f"conv2d-{_ci}-f16x3-cfg{_cfg}", "conv2d", ["aq_conv2d"], conv2d_geom(_case, _cfg), functools.partial(run_conv2d_f16x3, _case, _cfg))


def conv2d_ladder(Hh):
    """3x3 / stride 1, 32 -> 64 channels, bf16, on a 1 x Hh x 16 image: tiles of 128 pixels are 8 rows."""
    return (1, Hh, 16, 32, 64, 3, 1, True, True)


for _name, _cfg in (("igemm", 10), ("halo", len(IGEMM_TILES) + 7)):      # both (64, 128) tiles
    for _n in LADDER:
        for _lad, _Hh in (("full", 8 * _n), ("partial", 8 * _n - 3)):
            _case = conv2d_ladder(_Hh)
            add(f"ladder-conv2d-{_name}-{_lad}-{_n}", f"conv2d-{_name}", ["aq_conv2d"], conv2d_geom(_case, _cfg),
                functools.partial(run_conv2d, _case, "bf16", _cfg), _lad)


# ---- stem, scaled stem, stem + down-block ----------------------------------------------------------------------------------------------
def run_stem(B, H, W, precision):
    from aquaculture_amd import engine
    g = torch.Generator().manual_seed(H * 31 + W)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    b = torch.randn(48, generator=g) * 0.1
    x = u8_tiles(B, H, W, H + W)
    xin, wq = x.permute(0, 3, 1, 2).float() / 255, w
    if precision == "bf16":
        xin, wq = xin.bfloat16().float(), w.bfloat16().float()
    ref = F.silu(F.conv2d(xin, wq, b, stride=2, padding=2)).permute(0, 2, 3, 1).contiguous()
    out = engine.stem_conv_nhwc(x.cuda(), w, b, precision=precision)
    m = close(out.cpu(), ref, 2e-5, 2e-5) if precision == "fp32" else bf16_close(out, ref, 1e-3)
    return m, [out]


for _shape in ((1, 16, 24), (3, 32, 160)):
    for _prec in ("fp32", "bf16"):
        add("stem-%dx%dx%d-%s" % (*_shape, _prec), "stem", ["aq_stem_conv"], ("stem", *_shape), functools.partial(run_stem, *_shape, _prec))
# aq_stem_conv runs bf16 tiles whose width is a multiple of 4 (rows of whole dwords) through its LDS-DMA kernel, the one with the two-deep
# pipeline and the counted waits, and every other launch through the plain kernel.  The bf16 ladders keep to the DMA kernel: their partial
# tile is 128 n - 48 pixels wide (40 of 64 outputs).  "stem-bf16-plain" is the plain bf16 kernel at 128 n - 50; it has no whole-tile ladder
# (a whole number of tiles is a multiple of 4 wide).  fp32 always runs the plain kernel.
STEM_CUT = {"fp32": 50, "bf16": 48, "bf16-plain": 50}


def stem_uses_dma(precision, W):
    return precision == "bf16" and W % 4 == 0


for _fam in STEM_CUT:
    _prec = _fam.split("-")[0]
    for _n in LADDER:                                        # a tile is 64 x 8 outputs = 128 x 16 input pixels
        for _lad, _W in (("full", 128 * _n), ("partial", 128 * _n - STEM_CUT[_fam])):
            if _fam == "bf16-plain" and _lad == "full":
                continue
            add(f"ladder-stem-{_fam}-{_lad}-{_n}", f"stem-{_fam}", ["aq_stem_conv"], ("stem", 1, 16, _W), functools.partial(run_stem, 1, 16, _W, _prec), _lad)


def scaled_pass(H, W, flip):
    from aquaculture_amd import augment
    return augment.geometry(H, W)[0][2]._replace(flip=flip)


def run_stem_scaled(B, H, W, precision, flip):
    """aq_stem_conv_scaled (and the pointwise scaled preprocess beside it) at the bounds of test_gpu_augment.py."""
    from aquaculture_amd import engine
    from test_gpu_augment import scaled_input
    ps = scaled_pass(H, W, flip)
    g = torch.Generator().manual_seed(H + 2 * flip)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    b = torch.randn(48, generator=g) * 0.1
    x = u8_tiles(B, H, W, H + W + flip)
    xin = scaled_input(x.permute(0, 3, 1, 2).float() / 255, ps, W)
    stem = engine.stem_conv_scaled_nhwc(x.cuda(), w, b, ps.h, ps.w, ps.hp, ps.wp, flip, precision=precision)
    xq, wq = (xin.bfloat16().float(), w.bfloat16().float()) if precision == "bf16" else (xin, w)
    sref = F.silu(F.conv2d(xq, wq, b, stride=2, padding=2)).permute(0, 2, 3, 1).contiguous()
    if precision == "fp32":
        err = (stem.cpu() - sref).abs().max().item()
        assert err <= 1e-5, err
        return {"max_err": err}, [stem]
    return bf16_close(stem, sref, 1e-3), [stem]


def stem_scaled_geom(B, H, W):
    ps = scaled_pass(H, W, False)
    return ("stem", B, ps.hp, ps.wp)


for _shape in ((1, 64, 64), (3, 96, 160)):
    for _prec in ("fp32", "bf16"):
        for _flip in (False, True):
            add("stem_scaled-%dx%dx%d-%s-flip%d" % (*_shape, _prec, _flip), "stem_scaled", ["aq_stem_conv_scaled"], stem_scaled_geom(*_shape),
                functools.partial(run_stem_scaled, *_shape, _prec, _flip))


def run_stemdown(B, Hi, Wi):
    """aq_stemdown: bit-identical to aq_stem_conv followed by aq_downblock (its own test's reference); the two against torch below."""
    from aquaculture_amd import engine
    g = torch.Generator().manual_seed(Hi + Wi)
    ws = torch.randn(48, 3, 6, 6, generator=g) * 0.25
    bs = torch.randn(48, generator=g) * 0.3
    wa, ba, wb, bb = downblock_weights(g)
    x = u8_tiles(B, Hi, Wi, Hi * 3 + Wi).cuda()
    ref = engine.downblock_nhwc(engine.stem_conv_nhwc(x, ws, bs, act=True, precision="bf16"), wa, ba, wb, bb)
    out = engine.stemdown_nhwc(x, ws, bs, wa, ba, wb, bb)
    differing = int((out.view(torch.int16) != ref.view(torch.int16)).sum())
    assert differing == 0 and float(ref.float().abs().mean()) > 0.05, differing
    return {"differing": differing}, [out]


for _shape in ((1, 16, 24), (3, 148, 92)):
    add("stemdown-%dx%dx%d" % _shape, "stemdown", ["aq_stemdown", "aq_stem_conv", "aq_downblock"], ("stemdown", *_shape), functools.partial(run_stemdown, *_shape))
for _n in LADDER:                                            # a tile is 16 x 8 outputs = 64 x 32 input pixels
    for _lad, _W in (("full", 64 * _n), ("partial", 64 * _n - 24)):
        add(f"ladder-stemdown-{_lad}-{_n}", "stemdown", ["aq_stemdown"], ("stemdown", 1, 32, _W), functools.partial(run_stemdown, 1, 32, _W), _lad)


# ---- down-block, direct 3x3/s2 ---------------------------------------------------------------------------------------------------------
def run_downblock(B, H, W):
    from aquaculture_amd import engine
    g = torch.Generator().manual_seed(H * 7 + W)
    x = (torch.randn(B, H, W, 48, generator=g) * 0.8).bfloat16()
    wa, ba, wb, bb = downblock_weights(g)
    out = engine.downblock_nhwc(x.cuda(), wa, ba, wb, bb)
    t = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), wa.bfloat16().float(), ba, stride=2, padding=1)).bfloat16().float()
    ref = F.silu(F.conv2d(t, wb.bfloat16().float(), bb)).permute(0, 2, 3, 1).contiguous()
    err = (out.float().cpu() - ref).abs()
    assert (err <= 2 ** -7 * ref.abs() + 2e-2).all(), float(err.max())
    assert float(err.mean()) < 3e-3
    return {"max_err": float(err.max()), "mean_err": float(err.mean())}, [out]


def run_conv3x3s2(B, H, W):
    from aquaculture_amd import engine
    g, x, w, b = conv_inputs(B, H, W, 96, 192, 3, H * 5 + W)
    x = x.bfloat16()
    outs, worst = [], 0.0
    for act in (True, False):
        out = engine.conv3x3s2_direct_nhwc(x.cuda(), w, b, act)
        ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, stride=2, padding=1)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
        worst = max(worst, bf16_close(out, ref, 4e-3)["max_err"])
        outs.append(out)
    return {"max_err": worst}, outs


for _shape in ((1, 6, 10), (1, 36, 44)):
    add("downblock-%dx%dx%d" % _shape, "downblock", ["aq_downblock"], ("downblock", *_shape), functools.partial(run_downblock, *_shape))
    add("conv3x3s2_direct-%dx%dx%d" % _shape, "conv3x3s2_direct", ["aq_conv3x3s2_direct"], ("conv3x3s2", *_shape), functools.partial(run_conv3x3s2, *_shape))
for _n in LADDER:                                            # tiles of 16 x 8 (down-block) and 16 x 4 (direct 3x3/s2) outputs
    for _lad, _W in (("full", 32 * _n), ("partial", 32 * _n - 10)):
        add(f"ladder-downblock-{_lad}-{_n}", "downblock", ["aq_downblock"], ("downblock", 1, 16, _W), functools.partial(run_downblock, 1, 16, _W), _lad)
        add(f"ladder-conv3x3s2_direct-{_lad}-{_n}", "conv3x3s2_direct", ["aq_conv3x3s2_direct"], ("conv3x3s2", 1, 8, _W),
            functools.partial(run_conv3x3s2, 1, 8, _W), _lad)


# ---- fused Bottleneck and C3 tail ------------------------------------------------------------------------------------------------------
def run_bottleneck(c, B, H, W):
    from aquaculture_amd import engine
    g = torch.Generator().manual_seed(c * 1000 + H)
    x = (torch.randn(B, H, W, c, generator=g) * 0.8).bfloat16()
    w1 = torch.randn(c, c, 1, 1, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5
    b1, b2 = torch.randn(c, generator=g) * 0.2, torch.randn(c, generator=g) * 0.2
    outs, worst, mean = [], 0.0, 0.0
    for shortcut in (True, False):
        out = engine.bottleneck_nhwc(x.cuda(), w1, b1, w2, b2, shortcut)
        ref = _bottleneck_reference(x, w1, b1, w2, b2, shortcut)
        err = (out.float().cpu() - ref).abs()
        assert (err <= 2 ** -7 * ref.abs() + 2e-2).all(), float(err.max())
        assert float(err.mean()) < 3e-3
        worst, mean = max(worst, float(err.max())), max(mean, float(err.mean()))
        outs.append(out)
    return {"max_err": worst, "mean_err": mean}, outs


def add_bottleneck(id_, family, c, B, H, W, ladder=None):
    add(id_, family, ["aq_bottleneck"], ("bottleneck", c, B, H, W), functools.partial(run_bottleneck, c, B, H, W), ladder, btl_is_asm(c, B, H, W))


for _c in (16, 32, 48, 64, 96):
    for _shape in ((1, 7, 5), (2, 16, 32), (1, 40, 56)):
        add_bottleneck("bottleneck-c%d-%dx%dx%d" % (_c, *_shape), "bottleneck", _c, *_shape)
    _tw, _th = btl_tile(_c)
    for _n in LADDER:                                        # the HIP-source kernel: C = 48 and 96 run it on images one tile wide, so
        if _c in (48, 96):                                   # their ladder is one tile column
            _full, _part = (1, _th * _n, 16), (1, _th * _n - 3, 16)
        else:
            _full, _part = (1, _th, _tw * _n), (1, _th, _tw * _n - 5)
        add_bottleneck(f"ladder-bottleneck-hip-c{_c}-full-{_n}", f"bottleneck-hip-c{_c}", _c, *_full, "full")
        add_bottleneck(f"ladder-bottleneck-hip-c{_c}-partial-{_n}", f"bottleneck-hip-c{_c}", _c, *_part, "partial")
# The assembly builds (C = 48, C = 96, the C3 tail) need two tiles per row and per image: their ladders start at 2 tiles, count 1 is
# replaced by 2 (ASM_LADDER); every other count of LADDER is one row of that many tiles.
ASM_LADDER = tuple(n for n in LADDER if n >= 2)
for _c in (48, 96):
    _tw, _th = btl_tile(_c)
    for _n in ASM_LADDER:
        add_bottleneck(f"ladder-bottleneck-asm-c{_c}-full-{_n}", f"bottleneck-asm-c{_c}", _c, 1, _th, 16 * _n, "full")
        add_bottleneck(f"ladder-bottleneck-asm-c{_c}-partial-{_n}", f"bottleneck-asm-c{_c}", _c, 1, _th, 16 * _n - 5, "partial")


def run_c3tail(B, H, W, shortcut):
    """aq_bottleneck_c3tail against its own test's reference: aq_bottleneck into the concat buffer, then aq_conv1x1_direct, bit for bit."""
    from aquaculture_amd import engine
    from test_gpu_c3tail import _weights
    assert engine.bottleneck_c3tail_supported(B, H, W)
    p = _weights(B + H)
    g = torch.Generator().manual_seed(W)
    x = torch.randn(B, H, W, 48, generator=g).bfloat16().cuda()
    cv2 = torch.randn(B, H, W, 48, generator=g).bfloat16().cuda()
    cat = torch.zeros(B, H, W, 96, dtype=torch.bfloat16, device="cuda")
    cat[..., 48:] = cv2
    engine.bottleneck_nhwc(x, p["w1"], p["b1"], p["w2"], p["b2"], shortcut, out=cat[..., :48])
    ref = engine.conv1x1_direct_nhwc(cat, p["w3"], p["b3"])
    packed = engine.pack_bottleneck_c3tail(p["w1"], p["b1"], p["w2"], p["b2"], p["w3"], p["b3"], "cuda")
    out = engine.bottleneck_c3tail_nhwc(x, cv2, packed, shortcut)
    differing = int((out.view(torch.int16) != ref.view(torch.int16)).sum())
    assert differing == 0 and float(ref.float().abs().mean()) > 0.01, differing
    return {"differing": differing}, [out]


for _shape in C3TAIL_SHAPES:
    for _sc in (True, False):
        add("c3tail-%dx%dx%d-shortcut%d" % (*_shape, _sc), "c3tail", ["aq_bottleneck_c3tail"], ("c3tail", *_shape), functools.partial(run_c3tail, *_shape, _sc), None, True)
for _n in ASM_LADDER:
    for _lad, _W in (("full", 16 * _n), ("partial", 16 * _n - 5)):
        add(f"ladder-c3tail-{_lad}-{_n}", "c3tail", ["aq_bottleneck_c3tail"], ("c3tail", 1, 16, _W), functools.partial(run_c3tail, 1, 16, _W, True), _lad, True)


# ---- 1x1 kernels -----------------------------------------------------------------------------------------------------------------------
def run_c1direct(cin, cout, B, H, W):
    from aquaculture_amd import engine
    g, x, w, b = conv_inputs(B, H, W, cin, cout, 1, cin + H)
    x = x.bfloat16()
    outs, worst = [], 0.0
    for act in (True, False):
        out = engine.conv1x1_direct_nhwc(x.cuda(), w, b, act)
        ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
        worst = max(worst, bf16_close(out, ref, 2e-3)["max_err"])
        outs.append(out)
    return {"max_err": worst}, outs


F8_STEP = 2.0 ** -9                                          # spacing of e4m3's subnormal codes (below 2^-6)


def f8out_check(got, want, ref, x, w, b, scale):
    """The family's comparator (test_gpu_fp8.py, test_gpu_poison_kernels.py): no NaN code, the largest code 448, more than 99 % of the codes
    equal, every other within 0.126 max(|wanted|, 2^-9).  That bound admits a neighbouring code wherever one code step is at most an
    eighth of the value, which is every normal e4m3 number; below 2^-6 the codes are 2^-9 apart and a neighbouring code is refused.  A
    neighbouring code is what a correct kernel gives when the exact quotient lies on a rounding boundary, so here -- and only here -- an
    element outside the family's bound passes if (a) its code is the wanted code's neighbour and (b) the quotient q computed in float64
    from the same bf16 operands lies within `eps` of the midpoint of the two codes.  eps is what an fp32 evaluation can lose:

      pre-activation z: products of bf16 numbers are exact in fp32; the sum is taken in k-steps of 32 channels, in order.  Every term
        enters one rounded addition and every running sum S_k (after k-step k, the last one with the bias) is rounded once:
        |dz| <= 2^-24 (sum |x_i| |w_i| + |b| + sum_k |S_k|), the S_k computed here in float64;
      y = SiLU(z): |dy| <= |SiLU'(z)| |dz| + |dz|^2 / 2 (|SiLU''| <= 1/2), plus one rounding each for exp2, the add, rcp and the two
        multiplies: 5 x 2^-24 |y|;
      q = y / scale: the reciprocal of the scale and the product round once each: 2 x 2^-24 |q|.

    So that (b) keeps meaning "on a boundary", eps must be at most an eighth of a code step for every admitted element (asserted: a wider
    layer whose bound grows past that fails here instead of passing everything).  The number admitted is bounded too.  torch's fp32
    reference, from which the wanted codes come, errs by at most d_ref = max |ref / scale - q| over the elements below 2^-6 (the
    reference's own error, measured against float64 in this case); allowing the kernel four times that, as the split-mode conv test
    allows four times the fp32 kernel's error, the two straddle a midpoint only if q is within 5 d_ref of it, which of n_sub elements
    spread over a code step 2 x 5 d_ref / 2^-9 are expected to be: admitted <= 1 + ceil(n_sub 10 d_ref / 2^-9).
    Returns (share of equal codes, number admitted under (a) and (b), that number's bound, largest eps of an admitted element in steps)."""
    gv, wv = got.view(torch.float8_e4m3fn).float(), want.float()
    same = (got == want.view(torch.uint8)).float().mean().item()
    assert not torch.isnan(gv).any() and float(gv.max()) == 448.0, float(gv.max())
    bad = (gv - wv).abs() > 0.126 * wv.abs().clamp_min(F8_STEP)
    admitted, allowed, eps_steps = 0, 0, 0.0
    if bad.any():
        c = w.shape[0]
        xd, wd = x.double().reshape(-1, c), w.bfloat16().double().reshape(c, c)
        S, sums, A = torch.zeros(xd.shape[0], c, dtype=torch.float64), 0.0, xd.abs() @ wd.abs().t() + b.double().abs()
        for k in range(0, c, 32):
            S = S + xd[:, k:k + 32] @ wd[:, k:k + 32].t()
            if k + 32 == c:
                S = S + b.double()
            sums = sums + S.abs()
        z = S
        sig = torch.sigmoid(z)
        y = z * sig
        dz = 2.0 ** -24 * (A + sums)
        dy = (sig * (1 + z * (1 - sig))).abs() * dz + dz * dz / 2 + 5 * 2.0 ** -24 * y.abs()
        q = (y / scale).reshape(gv.shape)
        eps = (dy / scale).reshape(gv.shape) + 2 * 2.0 ** -24 * q.abs()
        neighbour = (got.int() - want.view(torch.uint8).int()).abs() == 1          # same sign: the sign bit is 0x80
        on_boundary = (q - (gv.double() + wv.double()) / 2).abs() <= eps
        refused = bad & ~(neighbour & on_boundary)
        assert not refused.any(), (int(refused.sum()), gv[refused][:4].tolist(), wv[refused][:4].tolist(), (q[refused][:4] / F8_STEP).tolist(),
                                   (eps[refused][:4] / F8_STEP).tolist())
        eps_steps = float(eps[bad].max()) / F8_STEP
        assert eps_steps <= 1 / 8, eps_steps
        sub = q.abs() < 2.0 ** -6
        d_ref = float(((ref.double() / scale).reshape(gv.shape) - q)[sub].abs().max())
        admitted, allowed = int(bad.sum()), 1 + int(np.ceil(int(sub.sum()) * 10 * d_ref / F8_STEP))
        assert admitted <= allowed, (admitted, allowed, int(sub.sum()), d_ref / F8_STEP)
    assert same > 0.99, same
    return same, admitted, allowed, eps_steps


def run_c1f8out(c, B, H, W):
    """aq_conv1x1_direct_f8out: the e4m3 codes of SiLU(conv1x1) / scale, under f8out_check."""
    from aquaculture_amd import engine
    lib = engine.load_library()
    g, x, w, b = conv_inputs(B, H, W, c, c, 1, c + H)
    x = x.bfloat16()
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)).permute(0, 2, 3, 1)
    scale = float(ref.abs().max()) / 448.0 * 0.9
    want = (ref / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    wk = np.ascontiguousarray(w.permute(0, 2, 3, 1).float().numpy())
    wp = wk.ctypes.data_as(C.POINTER(C.c_float))
    xd = x.cuda()
    codes = torch.zeros((B, H, W, c), dtype=torch.uint8, device="cuda")
    n = C.c_size_t()
    engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, None, C.byref(n), None))
    wbuf = torch.empty(n.value, dtype=torch.uint8, device="cuda")
    engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, wbuf.data_ptr(), C.byref(n), engine._stream_ptr()))
    bbuf = b.float().cuda()
    engine._check(lib.aq_conv1x1_direct_f8out(xd.data_ptr(), c, 0, codes.data_ptr(), c, 0, c, c, wbuf.data_ptr(), bbuf.data_ptr(), B * H * W, 1, scale,
                                              engine._stream_ptr()))
    torch.cuda.synchronize()
    same, admitted, allowed, eps_steps = f8out_check(codes.cpu(), want, ref, x, w, b, scale)
    return {"same_codes": same, "on_a_rounding_boundary": admitted, "allowed_on_a_boundary": allowed, "eps_in_code_steps": eps_steps}, [codes]


def run_c1asm(cin, cout, family, B, H, W):
    from aquaculture_amd import engine
    env(AQ_C1_ASM_NB=family)
    try:
        g, x, w, b = conv_inputs(B, H, W, cin, cout, 1, cin + H)
        x = x.bfloat16()
        out = engine.conv1x1_asm_nhwc(x.cuda(), w, b)
    finally:
        env(AQ_C1_ASM_NB=None)
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)).permute(0, 2, 3, 1)
    return bf16_close(out, ref, 2e-3), [out]


for _shape in ((1, 5, 7), (2, 37, 41)):
    _npix = _shape[0] * _shape[1] * _shape[2]
    for _cin, _cout in C1_DIRECT_TP:
        add("conv1x1_direct-%d-%d-%dx%dx%d" % (_cin, _cout, *_shape), "conv1x1_direct", ["aq_conv1x1_direct"], ("c1direct", _cin, _cout, _npix),
            functools.partial(run_c1direct, _cin, _cout, *_shape))
    for _c in (192, 384):
        add("conv1x1_direct_f8out-%d-%dx%dx%d" % (_c, *_shape), "conv1x1_direct_f8out", ["aq_conv1x1_direct_f8out"], ("c1direct", _c, _c, _npix),
            functools.partial(run_c1f8out, _c, *_shape))
    for _cin, _cout in ((96, 384), (768, 384), (1536, 768)):
        for _fam in (13, 7):
            add("conv1x1_asm-%d-%d-nb%d-%dx%dx%d" % (_cin, _cout, _fam, *_shape), "conv1x1_asm", ["aq_conv1x1_asm"], ("c1asm", _fam, _cout, _npix),
                functools.partial(run_c1asm, _cin, _cout, _fam, *_shape), None, True)
for _n in LADDER:                                            # one row of pixels: n tiles of TP, the partial ladder's last tile holds TP - 37
    for _lad, _cut in (("full", 0), ("partial", 37)):
        for (_cin, _cout), _tp in C1_DIRECT_TP.items():
            add(f"ladder-conv1x1_direct-{_cin}-{_cout}-{_lad}-{_n}", f"conv1x1_direct-{_cin}-{_cout}", ["aq_conv1x1_direct"],
                ("c1direct", _cin, _cout, _tp * _n - _cut), functools.partial(run_c1direct, _cin, _cout, 1, 1, _tp * _n - _cut), _lad)
        for _c in (192, 384):
            _tp = C1_DIRECT_TP[(_c, _c)]
            add(f"ladder-conv1x1_direct_f8out-{_c}-{_lad}-{_n}", f"conv1x1_direct_f8out-{_c}", ["aq_conv1x1_direct_f8out"],
                ("c1direct", _c, _c, _tp * _n - _cut), functools.partial(run_c1f8out, _c, 1, 1, _tp * _n - _cut), _lad)
        for _fam, _tp in C1_ASM_TPX.items():                 # 96 -> 384: one channel tile, so a pixel tile is a tile
            add(f"ladder-conv1x1_asm-nb{_fam}-{_lad}-{_n}", f"conv1x1_asm-nb{_fam}", ["aq_conv1x1_asm"], ("c1asm", _fam, 384, _tp * _n - _cut),
                functools.partial(run_c1asm, 96, 384, _fam, 1, 1, _tp * _n - _cut), _lad, True)


# ---- planar 3x3 ------------------------------------------------------------------------------------------------------------------------
PL_BUILDS = ("13asm", "13slot-asm", "13pm-asm", "7asm", "8asm", 13, 10, 7)
EXPERIMENTAL_BUILDS = ("7asm", "8asm")                      # built only with AQ_GEN_EXPERIMENTAL=1: their cases are skipped otherwise


def pl_nb(build):
    return int(re.match(r"\d+", build).group()) if isinstance(build, str) else build


def pl_env(build):
    """The switches test_planar_conv3x3_matches_reference sets for a build."""
    env(AQ_PL_ASM="1" if isinstance(build, str) else "0", AQ_PL_PM={"13slot-asm": "0", "13pm-asm": "2"}.get(build), AQ_PL_NB=pl_nb(build))


def pl_clear():
    env(AQ_PL_ASM=None, AQ_PL_PM=None, AQ_PL_NB=None)


def pl_call(call, B, H, W, c, resmode, x, resv):
    """The planar kernels' common case: the shortcut a tensor of its own or the output itself (owned values pre-set)."""
    out = torch.empty((B, H, W, c), dtype=torch.bfloat16, device="cuda")
    res = None
    if resmode == "sep":
        res = resv.cuda()
    elif resmode == "inplace":
        out.copy_(resv)
        res = out
    call(x.cuda(), res, out)
    torch.cuda.synchronize()
    return out


def run_pl(build, B, H, W, cin, c, resmode):
    from aquaculture_amd import engine
    lib = engine.load_library()
    nb = pl_nb(build)
    if isinstance(build, str) and not lib.aq_conv3x3_pl_asm_family(nb):
        return {"skipped": "not built: experimental assembly family (AQ_GEN_EXPERIMENTAL=1)"}, []
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 7 + H * 3 + nb)
    x = x.bfloat16()
    resv = torch.randn(B, H, W, c, generator=g).bfloat16()
    pl_env(build)
    try:
        out = pl_call(lambda xv, res, o: engine.conv3x3_pl_nhwc(xv, w, b, True, residual=res, out=o), B, H, W, c, resmode, x, resv)
    finally:
        pl_clear()
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, padding=1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.float()
    return bf16_close(out, ref, 4e-3), [out]


def run_pl_w8(B, H, W, cin, c, resmode):
    from aquaculture_amd import engine, quant
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 7 + H * 3)
    x = x.bfloat16()
    wq = torch.from_numpy(quant.quantize_rows(w.numpy())[0])
    resv = torch.randn(B, H, W, c, generator=g).bfloat16()
    out = pl_call(lambda xv, res, o: engine.conv3x3_pl_nhwc(xv, wq, b, True, residual=res, out=o, w8=True), B, H, W, c, resmode, x, resv)
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), wq.bfloat16().float(), b, padding=1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.float()
    return bf16_close(out, ref, 4e-3), [out]


def run_pl_f8(B, H, W, cin, c, resmode):
    """fp8 MFMA on both operands; reference and bounds of test_planar_conv3x3_f8_matches_reference."""
    from aquaculture_amd import engine
    g = torch.Generator().manual_seed(c * 3 + H * 5 + cin)
    x = torch.randn(B, H, W, cin, generator=g).abs() * 0.9 - 0.25
    act_scale = float(x.abs().max()) / 448.0
    xq = (x / act_scale).to(torch.float8_e4m3fn)
    w = torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5
    w = w * (10.0 ** torch.linspace(-1, 1, c)).view(-1, 1, 1, 1)
    b = torch.randn(c, generator=g) * 0.2
    ws = w.abs().amax(dim=(1, 2, 3), keepdim=True) / 448.0
    wq = (w / ws).to(torch.float8_e4m3fn)
    resv = torch.randn(B, H, W, c, generator=g).bfloat16()
    out = pl_call(lambda xv, res, o: engine.conv3x3_pl_f8_nhwc(xv, act_scale, w, b, True, residual=res, out=o), B, H, W, c, resmode,
                  xq.view(torch.uint8), resv)
    got = out.float().cpu()
    ref = F.conv2d(xq.float().double().permute(0, 3, 1, 2), wq.float().double(), None, padding=1)
    ref = F.silu(ref * (act_scale * ws.view(1, -1, 1, 1).double()) + b.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.double()
    scale = ref.abs().amax(dim=(0, 1, 2)).clamp_min(1e-6).float()
    rel = ((got - ref.float()).abs() / scale).max().item()
    assert rel <= 2 ** -7, rel
    torch.testing.assert_close(got, ref.float().bfloat16().float(), rtol=2 ** -6, atol=2e-2 * float(scale.max()))
    return {"max_rel_err": rel}, [out]


def run_pl_s2(B, H, W, cin, c, act):
    from aquaculture_amd import engine
    assert engine.load_library().aq_conv3x3_pl_s2_supported(cin, c, B, H, W)
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 5 + H * 3 + cin)
    x = x.bfloat16()
    out = engine.conv3x3_pl_s2_nhwc(x.cuda(), w, b, act)
    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, stride=2, padding=1)
    ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
    return bf16_close(out, ref, 4e-3), [out]


def pl_refused(build, W, c):
    """What the family's tests expect the launcher to refuse: the 8-block build on wide images or where cout / 192 is no power of two."""
    return pl_nb(build) == 8 and (W > 40 or bool((c // 192) & (c // 192 - 1)))


for _shape in PL_SHAPES:
    _B, _H, _W, _cin, _c = _shape
    for _rm in RESMODES:
        for _b in PL_BUILDS:
            if pl_refused(_b, _W, _c):
                continue
            add("conv3x3_pl-%s-%dx%dx%d-%d-%d-res_%s" % (_b, *_shape, _rm), "conv3x3_pl", ["aq_conv3x3_pl"], ("pl", pl_nb(_b), _c, _B * _H * _W),
                functools.partial(run_pl, _b, *_shape, _rm), None, isinstance(_b, str) and not (_c // 192) & (_c // 192 - 1))
        if _c != 576:                                        # cout / 192 is no power of two: both refuse (their own tests pin that)
            add("conv3x3_pl_w8-%dx%dx%d-%d-%d-res_%s" % (*_shape, _rm), "conv3x3_pl_w8", ["aq_conv3x3_pl_w8"], ("pl", 13, _c, _B * _H * _W),
                functools.partial(run_pl_w8, *_shape, _rm), None, True)
            add("conv3x3_pl_f8-%dx%dx%d-%d-%d-res_%s" % (*_shape, _rm), "conv3x3_pl_f8", ["aq_conv3x3_pl_f8"], ("pl", 13, _c, _B * _H * _W),
                functools.partial(run_pl_f8, *_shape, _rm), None, True)
for _case in ((1, 18, 14, 64, 192, True), (2, 4, 4, 64, 192, False), (2, 26, 48, 96, 192, True)):
    add("conv3x3_pl_s2-%dx%dx%d-%d-%d-act%d" % _case, "conv3x3_pl_s2", ["aq_conv3x3_pl_s2"], ("pl", PL_S2_NB, _case[4], _case[0] * (_case[1] // 2) * (_case[2] // 2)),
        functools.partial(run_pl_s2, *_case), None, True)
for _n in LADDER:                                            # a 16-pixel-wide image: a tile of nb pixel blocks is nb rows (128 -> 192 channels: one channel tile)
    for _lad, _cut in (("full", 0), ("partial", 1)):
        for _b in PL_BUILDS:
            _nb = pl_nb(_b)
            add(f"ladder-conv3x3_pl-{_b}-{_lad}-{_n}", f"conv3x3_pl-{_b}", ["aq_conv3x3_pl"], ("pl", _nb, 192, 16 * (_nb * _n - _cut)),
                functools.partial(run_pl, _b, 1, _nb * _n - _cut, 16, 128, 192, "sep"), _lad, isinstance(_b, str))
        add(f"ladder-conv3x3_pl_w8-{_lad}-{_n}", "conv3x3_pl_w8", ["aq_conv3x3_pl_w8"], ("pl", 13, 192, 16 * (13 * _n - _cut)),
            functools.partial(run_pl_w8, 1, 13 * _n - _cut, 16, 128, 192, "sep"), _lad, True)
        add(f"ladder-conv3x3_pl_f8-{_lad}-{_n}", "conv3x3_pl_f8", ["aq_conv3x3_pl_f8"], ("pl", 13, 192, 16 * (13 * _n - _cut)),
            functools.partial(run_pl_f8, 1, 13 * _n - _cut, 16, 128, 192, "sep"), _lad, True)
        add(f"ladder-conv3x3_pl_s2-{_lad}-{_n}", "conv3x3_pl_s2", ["aq_conv3x3_pl_s2"], ("pl", PL_S2_NB, 192, 16 * (13 * _n - _cut)),
            functools.partial(run_pl_s2, 1, 2 * (13 * _n - _cut), 32, 64, 192, True), _lad, True)


# ---- Detect head fused with its decode -------------------------------------------------------------------------------------------------
def run_head(cin, B, ny, nx, aug):
    from aquaculture_amd import engine
    nc = 5
    xw, x, w, b = make_level(B, ny, nx, cin, 3, nc, cin + ny)
    cap, off, thr, stride, scale, flip_w = 3 * ny * nx, 1000, 0.25, 16.0, 0.67, 640.0
    xd = xw.cuda()[..., 8:8 + cin]
    if aug:
        counts, cand, rows = engine.head_decode_level_aug(xd, w, b, off, stride, ANCHORS, nc, thr, cap, scale, flip_w)
    else:
        counts, cand, rows = engine.head_decode_level(xd, w, b, off, stride, ANCHORS, nc, thr, cap)
    torch.cuda.synchronize()
    counts, cand, rows = counts.cpu(), cand.cpu(), rows.cpu()
    ref = head_reference(x, w, b, ANCHORS, nc, stride)
    if aug:                                                  # [UPSTREAM _descale_pred]
        ref[..., :4] /= scale
        ref[..., 0] = flip_w - ref[..., 0]
    stats = check_level(counts, cand, rows, ref, off, thr, cap)
    owned = [counts]
    for bi in range(B):
        n = min(int(counts[bi]), cap)
        assert bool((cand[bi, n:] == -1).all())
        o = torch.argsort(cand[bi, :n])                      # the order within an image follows the atomic counters: sorted by candidate
        owned += [cand[bi, :n][o], rows[bi, :n][o]]
    assert stats[3] > 0.1 * B * cap
    return {"worst_over_bound": stats[0], "max_err": stats[1], "in_band": stats[2], "candidates": stats[3]}, owned


for _cin in WIDTHS:
    for _shape in ((3, 5, 7), (3, 8, 8)):
        for _aug in (False, True):
            _id = "head_decode%s-%d-%dx%dx%d" % ("_aug" if _aug else "", _cin, *_shape)
            add(_id, "head_decode", ["aq_head_decode_aug" if _aug else "aq_head_decode"], ("head", _cin, _shape[0] * _shape[1] * _shape[2]),
                functools.partial(run_head, _cin, *_shape, _aug))
            EXEMPT[_id] = "the candidate list's row order follows atomic counters; digest over the rows sorted by candidate index"


# ---- image-side launchers --------------------------------------------------------------------------------------------------------------
def run_blank_stats():
    import test_gpu_blank_key as K
    images = [im for _, im in K.CASES]
    buf, bases, pitches = K._pack(images)
    got = K._gpu(buf, images, bases, pitches)[0]
    K._check(got, images)
    return {"frames": len(images)}, [got]


def blank_stats_items():
    import test_blank_key as K
    return max(cdiv(im.shape[0], 32) for _, im in K.CASES) * len(K.CASES)       # kBandRows = 32: bands of the tallest frame, per frame


def run_blank_geom():
    import test_gpu_blank_geom as G
    images = [G.image_of(m, k) for k, (_, m) in enumerate(G.MASKS)]
    buf, bases, pitches = G._pack(images)
    rec, maps, edges, _, _ = G._gpu(buf, images, bases, pitches)
    G._check(rec, maps, edges, images)
    owned = [rec]
    for k in range(len(images)):
        owned += [maps[k][0], maps[k][1], edges[k]]
    return {"frames": len(images)}, owned


def blank_geom_items():
    import test_blank_geom as G
    return max(cdiv(m.shape[0] * cdiv(m.shape[1], 64), 4) for _, m in G.MASKS) * len(G.MASKS)    # sweep_grid: row pieces of 64 px, four to a workgroup


@functools.lru_cache(maxsize=1)
def crop_case():
    from aquaculture_amd import engine
    from test_gpu_save_crop import _rects
    rng, r2 = np.random.default_rng(0), np.random.default_rng(1)
    host, bases, pitches, rects, wins, base = [], [], [], [], [], 0
    for h, w in CROP_SIZES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        im[: h // 3] = im[: h // 3] // 64 * 64
        host.append(im.reshape(-1))
        for x1, y1, x2, y2 in _rects(h, w, r2):
            bases.append(base)
            pitches.append(3 * w)
            rects.append((x1, y1, x2, y2))
            wins.append(im[y1:y2, x1:x2])
        base += im.size
    return np.concatenate(host), engine.crop_table(np.asarray(bases), np.asarray(pitches), np.asarray(rects)), wins


def crop_items():
    from test_gpu_save_crop import _rects
    r2, blocks = np.random.default_rng(1), 0
    for h, w in CROP_SIZES:
        blocks += sum(cdiv(x2 - x1, 8) * cdiv(y2 - y1, 8) for x1, y1, x2, y2 in _rects(h, w, r2))
    return cdiv(3 * blocks, 256)                             # three threads per block position, workgroups of 256


def run_crops():
    from aquaculture_amd import engine
    from test_gpu_save_crop import _check_coefs
    host, table, wins = crop_case()
    assert cdiv(3 * int(engine.crop_blocks(table).sum()), 256) == crop_items()
    coef, _ = engine.encode_crops(torch.from_numpy(host).cuda(), table)
    coef = np.asarray(coef.cpu()) if isinstance(coef, torch.Tensor) else np.asarray(coef)
    assert coef.shape[0] == int(engine.crop_blocks(table).sum())
    _check_coefs(coef, table, wins)
    return {"blocks": int(coef.shape[0])}, [coef]


def frame_items():
    return (sum(cdiv(cdiv(w, 16), 4) * cdiv(h, 16) for h, w in MIXED),       # aq_annotate_u8: units of four 16 x 16 cells of a cell row
            cdiv(sum(cdiv(w, 16) * cdiv(h, 16) for h, w in MIXED), 4))      # aq_image_jpeg_coefs: groups of four MCUs


def run_frames():
    """aq_annotate_u8 against Pillow's ImageDraw and aq_image_jpeg_coefs against the restatement of libjpeg's pixel path, on MIXED."""
    from aquaculture_amd import engine
    from test_gpu_save_img import _content, _draw, _random_boxes
    from test_save_img import pillow_box_label, reference_coefs_420, want_labels
    rng = np.random.default_rng(6)
    images = [_content("random", h, w, rng) for h, w in MIXED]
    dets = [_random_boxes(40, h, w, rng) for h, w in MIXED]
    dets[4] = (np.array([[0, 0, 1, 1]]), np.array([3]), np.array([0.5], np.float32))
    got, src, flat, (out, canvases) = _draw(images, dets, 2)
    want = [pillow_box_label(im, b, c, want_labels(c, v, False, False), 2) for im, (b, c, v) in zip(images, dets)]
    for i, (g_, w_) in enumerate(zip(got, want)):
        assert np.array_equal(g_, w_), (i, g_.shape, np.argwhere((g_ != w_).any(2))[:5])
    assert np.array_equal(src.cpu().numpy(), flat)
    table = engine.frame_table(canvases["dst"], canvases["dst_pitch"], list(MIXED))
    coef, _ = engine.encode_frames(out, table)
    coef = np.asarray(coef.cpu()) if isinstance(coef, torch.Tensor) else np.asarray(coef)
    assert coef.shape[0] == int(engine.frame_mcus(table).sum()) and cdiv(coef.shape[0], 4) == frame_items()[1]
    for i, w_ in enumerate(want):
        m = int(table["mcu"][i])
        ref = reference_coefs_420(w_).reshape(-1, 384)
        assert np.array_equal(coef[m:m + ref.shape[0]], ref), (i, w_.shape)
    return {"mcus": int(coef.shape[0])}, list(got) + [coef]


def run_overlaps(which):
    from aquaculture_amd import overlaps
    from test_overlaps import random_case, same_bytes, strips_case
    if which == "random":
        boxes, det_row, dets, literal = random_case()
    else:
        boxes, det_row, dets, want_state = strips_case()
    start, partner = overlaps.partners_gpu(boxes)
    ws, wp = overlaps.partners_numpy(boxes)
    assert start.tobytes() == ws.tobytes() and partner.tobytes() == wp.tobytes()
    got = overlaps.clip_gpu(boxes, start, partner, det_row, dets)
    if which == "random":
        same_bytes(got, literal)
    else:
        same_bytes(got, overlaps.clip_numpy(boxes, start, partner, det_row, dets))
        assert got["state"].tolist() == want_state.tolist()
    return {"detections": int(dets.shape[0])}, [start, partner] + [got[k] for k in ("state", "clip_bounds", "clip_area", "has_region")]


add("blank_stats-mixed", "blank_stats", ["aq_blank_stats_u8"], ("count", blank_stats_items()), run_blank_stats)
add("blank_geom-mixed", "blank_geom", ["aq_blank_components_u8", "aq_blank_ring_edges_u8"], ("count", blank_geom_items()), run_blank_geom)
add("crop_jpeg-sizes", "crop_jpeg", ["aq_crop_jpeg_coefs"], ("count", crop_items()), run_crops)
add("annotate_and_frames-mixed", "frames", ["aq_annotate_u8", "aq_image_jpeg_coefs"], ("count", frame_items()[0]), run_frames)
add("overlap_clip-random", "overlaps", ["aq_overlap_partners_f64", "aq_overlap_clip_f64"], ("count", cdiv(4000, 4)), functools.partial(run_overlaps, "random"))
add("overlap_clip-strips", "overlaps", ["aq_overlap_partners_f64", "aq_overlap_clip_f64"], ("count", cdiv(6, 4)), functools.partial(run_overlaps, "strips"))


# ---- the whole engine, synthetic yolov5m -----------------------------------------------------------------------------------------------
ENGINE_SHAPES = (((96, 160), 5), ((640, 384), 3))
ENGINE_RECORD = {}                                           # case id -> last_launches() and the detections of its call, for the record


@functools.lru_cache(maxsize=1)
def synth_ck():
    from aquaculture_amd import checkpoint
    return checkpoint.synthetic_checkpoint("yolov5m", 5)


def engine_tiles(hw, B):
    """Synthetic tiles cut to H x W, as test_fp32_engine_on_ragged_shapes cuts them."""
    from aquaculture_amd import tiles
    H, W = hw
    return np.ascontiguousarray(tiles.synthetic_batch(list(range(B)), max(640, H, W))[:, :H, :W])


def engine_owned(dets, counts):
    dets, counts = dets.cpu(), counts.cpu()
    return [counts] + [dets[b, :int(counts[b])] for b in range(counts.shape[0])]


def run_engine(id_, precision, hw, B, augment):
    """fp32: the north-star gate of test_gpu_engine.py (identical counts, boxes / confidences within 1e-4 of the oracle's detections).
    bf16: test_infer_bf16_close_to_emulated_oracle's (plain) and test_infer_augment_bf16_close_to_emulated_oracle's (augmented) bounds."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    from test_gpu_augment import oracle_augmented_pred
    from test_gpu_bf16_deviation import BOUNDS as BF16       # the numbers test_infer_bf16_close_to_emulated_oracle writes out
    from test_gpu_engine import _match
    ck = synth_ck()
    x = engine_tiles(hw, B)
    eng = engine.Engine(ck, precision)
    t = torch.from_numpy(x).cuda()
    dets, counts = (v.clone() for v in (eng.infer(t, augment=True) if augment else eng.infer(t)))
    ENGINE_RECORD[id_] = {"last_launches": [list(v) for v in (eng.last_launches(augment_pass=1) if augment else eng.last_launches())],
                          "counts": counts.cpu().tolist(),                                       # (float32 values are exact in JSON's doubles)
                          "detections": [dets[b, :int(counts[b])].cpu().double().tolist() for b in range(B)]}
    if precision == "fp32":
        ref_pred = O.model_from_checkpoint(ck).forward(O.preprocess(x))
        pred = eng.forward_raw(t).cpu()
        m = {"d_conf_max": (pred[..., 4:] - ref_pred[..., 4:]).abs().max().item(), "d_box_max": (pred[..., :4] - ref_pred[..., :4]).abs().max().item(),
             "boxes": int(counts.sum())}
        assert m["d_conf_max"] <= 1e-4 and m["d_box_max"] <= 640 * 1e-4, m       # boxes scale with the anchors (up to 373 px), not the tile
        _match(dets.cpu().numpy(), counts.cpu().numpy(), O.non_max_suppression(ref_pred.numpy()), box_tol=640 * 1e-4, conf_tol=1e-4)
    else:
        mq = O.model_from_checkpoint(ck, O.q_bf16)
        ref = oracle_augmented_pred(mq, x) if augment else mq.forward(O.preprocess(x))
        pred = eng.forward_raw(t, augment=augment).cpu()
        d_conf = (pred[..., 4:] - ref[..., 4:]).abs().flatten()
        m = {"d_conf_mean": d_conf.mean().item(), "d_conf_p999": d_conf.kthvalue(int(0.999 * d_conf.numel()))[0].item(),
             "d_box_mean": (pred[..., :4] - ref[..., :4]).abs().mean().item(), "boxes": int(counts.sum())}
        assert m["d_conf_mean"] <= BF16["dconf_mean"] and m["d_conf_p999"] <= BF16["dconf_p999"] and m["d_box_mean"] <= BF16["dbox_mean_px"], m
        ref_counts = [r.shape[0] for r in O.non_max_suppression(ref.numpy())]
        for got, want in zip(counts.cpu().tolist(), ref_counts):
            assert abs(got - want) <= BF16["count_diff_max"], (counts.cpu().tolist(), ref_counts)
    owned = engine_owned(dets, counts)
    eng.close()
    return m, owned


for _prec in ("bf16", "fp32"):
    for _hw, _B in ENGINE_SHAPES:
        _id = "engine-%s-%dx%d-b%d" % (_prec, *_hw, _B)
        add(_id, "engine", ["aq_engine_infer"], ("count", _B), functools.partial(run_engine, _id, _prec, _hw, _B, False))
add("engine-bf16-augment-96x160-b5", "engine", ["aq_engine_infer_augment"], ("count", 5),
    functools.partial(run_engine, "engine-bf16-augment-96x160-b5", "bf16", (96, 160), 5, True))


# ---- a partial tile in the middle of a walk ---------------------------------------------------------------------------------------------
# The "partial" ladders end in their partial tile.  The families tiled in rows of an image (tile index = row * tiles_x + column) get a third
# ladder, "mid": two tile rows of n tiles whose last column is partial, so tiles n - 1 and 2 n - 1 of 2 n are partial and a workgroup of a
# grid of G < n workgroups goes on from tile n - 1 to the whole tile n - 1 + G (one workgroup: full ... partial, full ... partial).  The
# families tiled over the flattened pixels (1x1, planar 3x3, implicit GEMM) can have no partial tile but the last; the one-column ladders
# of the HIP-source Bottleneck at C = 48 and 96 neither (two columns are the assembly builds').
MID_LADDER = (2, 3, 4, 5, 9)
for _n in MID_LADDER:
    for _fam, _cut in STEM_CUT.items():
        add(f"ladder-stem-{_fam}-mid-{_n}", f"stem-{_fam}", ["aq_stem_conv"], ("stem", 1, 32, 128 * _n - _cut),
            functools.partial(run_stem, 1, 32, 128 * _n - _cut, _fam.split("-")[0]), "mid")
    add(f"ladder-stemdown-mid-{_n}", "stemdown", ["aq_stemdown"], ("stemdown", 1, 64, 64 * _n - 24), functools.partial(run_stemdown, 1, 64, 64 * _n - 24), "mid")
    add(f"ladder-downblock-mid-{_n}", "downblock", ["aq_downblock"], ("downblock", 1, 32, 32 * _n - 10), functools.partial(run_downblock, 1, 32, 32 * _n - 10), "mid")
    add(f"ladder-conv3x3s2_direct-mid-{_n}", "conv3x3s2_direct", ["aq_conv3x3s2_direct"], ("conv3x3s2", 1, 16, 32 * _n - 10),
        functools.partial(run_conv3x3s2, 1, 16, 32 * _n - 10), "mid")
    for _c in (16, 32, 64):
        _tw, _th = btl_tile(_c)
        add_bottleneck(f"ladder-bottleneck-hip-c{_c}-mid-{_n}", f"bottleneck-hip-c{_c}", _c, 1, 2 * _th, _tw * _n - 5, "mid")
    for _c in (48, 96):
        add_bottleneck(f"ladder-bottleneck-asm-c{_c}-mid-{_n}", f"bottleneck-asm-c{_c}", _c, 1, 2 * btl_tile(_c)[1], 16 * _n - 5, "mid")
    add(f"ladder-c3tail-mid-{_n}", "c3tail", ["aq_bottleneck_c3tail"], ("c3tail", 1, 32, 16 * _n - 5), functools.partial(run_c3tail, 1, 32, 16 * _n - 5, True), "mid", True)


# ---- the runner ------------------------------------------------------------------------------------------------------------------------
def digest(owned):
    """sha256 over every owned output: dtype, shape and bytes, in order."""
    h = hashlib.sha256()
    for t in owned:
        if isinstance(t, torch.Tensor):
            t = t.detach().contiguous().cpu()
            a = t.view(torch.uint8).numpy() if t.dtype == torch.bfloat16 else t.numpy()
            h.update(f"{t.dtype}{tuple(t.shape)}".encode())
        else:
            a = np.ascontiguousarray(t)
            h.update(f"{a.dtype}{a.shape}".encode())
        h.update(a.tobytes())
    return h.hexdigest()


def is_gpu_fault(err):
    """Did the device fault?  By the error's text, or because the device no longer synchronises."""
    s = str(err)
    if isinstance(err, RuntimeError) and ("HIP error" in s or "hipError" in s or "illegal memory access" in s):
        return True
    try:
        torch.cuda.synchronize()
    except RuntimeError:
        return True
    return False


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", required=True)
    args = ap.parse_args(argv)
    import time
    from aquaculture_amd import engine
    engine.load_library()
    records = []

    def write():
        with open(args.out + ".part", "w") as f:
            json.dump({"cases": records, "num_cus_env": os.environ.get("AQ_NUM_CUS")}, f)
        os.replace(args.out + ".part", args.out)

    for case in CASES:
        rec = {"id": case.id, "n_tiles": case.n_tiles}
        t0 = time.perf_counter()
        try:
            try:
                metrics, owned = case.run()
                rec.update(metrics, ok=True)
            except AssertionError as err:                    # the comparator's verdict: a finding, the run goes on
                rec.update(ok=False, error=str(err)[:500])
                owned = []
            torch.cuda.synchronize()
            rec["sha256"] = digest(owned)
            rec.update(ENGINE_RECORD.get(case.id, {}))
        except Exception as err:                             # noqa: BLE001
            rec.update(ok=False, error=f"{type(err).__name__}: {err}"[:500], sha256=None)
            records.append(rec)
            if is_gpu_fault(err):                            # nothing more is launched on a faulted device
                print(f"{case.id}: {err}", file=sys.stderr)
                write()
                return 3
            continue
        rec["seconds"] = round(time.perf_counter() - t0, 4)
        records.append(rec)
    write()
    print(f"{len(records)} cases, {sum(not r['ok'] for r in records)} not ok, AQ_NUM_CUS={os.environ.get('AQ_NUM_CUS')}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
