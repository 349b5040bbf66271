"""No kernel's result may depend on bytes it does not own.

Every stand-alone launcher runs twice at its smallest hard shapes: once with every byte it was not given holding 0x00, once 0xFF (NaN in
bf16 / fp16 / fp32 / fp64 / e4m3, -1 in every integer type).  "Not given" is: whatever `torch.empty` returns inside the wrappers (packed
weights, bias tiles, scratch, outputs: tests/poison.py), the channels beside the input / residual / output slices (the tensors are slices
[8 : 8 + c] of wider rows), and one whole image in front of and one behind the batch.  The kernels are deterministic, so the check has no
tolerance: the owned outputs of the two runs are equal bit for bit, the filler still holds its fill, and every guard behind an allocation
is intact.  The 0x00 run also meets the family's own parity check (reference and tolerance imported from its test), which keeps the shapes
from being vacuous, and the 0xFF run's outputs are finite.

Buffers with a documented zero-on-entry contract are zeroed here and say so; nothing else is.
"""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from poison import poisoned
from test_gpu_conv import _bottleneck_reference, _ref
from test_gpu_head_decode import ANCHORS, WIDTHS, check_level, make_level, reference as head_reference

pytestmark = pytest.mark.gpu


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """A failed test is a finding; a faulted device is the end of the session: nothing more is launched on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"the GPU faulted, no further test is run: {err}", 3)


FILLS = (0x00, 0xFF)
PAD = 8                      # channels in front of every slice and behind it (16 for one-byte types: slices start on 16 bytes)


# ---- scaffolding ---------------------------------------------------------------------------------------------------------------------
def bits(t):
    """The tensor's bytes as integers of its element size (NaNs compare equal to themselves)."""
    t = t.contiguous()
    return t.view({1: torch.uint8, 2: torch.int16, 4: torch.int32, 8: torch.int64}[t.element_size()]).cpu()


def filled(shape, dtype, byte):
    t = torch.zeros(shape, dtype=dtype, device="cuda")
    t.view(-1).view(torch.uint8).fill_(byte)
    return t


class Slice:
    """An owned [B, H, W, c] tensor inside a [B + 2, H, W, front + c + back] one whose every other byte is ``byte``."""

    def __init__(self, B, H, W, c, dtype, byte, value=None, back=None):
        self.byte, self.c = byte, c
        self.front = front = PAD if torch.empty(0, dtype=dtype).element_size() > 1 else 16
        self.wide = filled((B + 2, H, W, front + c + (front if back is None else back)), dtype, byte)
        self.view = self.wide[1:1 + B, :, :, front:front + c]
        self.mask = torch.ones(self.wide.shape, dtype=torch.bool, device="cuda")
        self.mask[1:1 + B, :, :, front:front + c] = False
        if value is not None:
            self.view.copy_(value.to(dtype))

    def filler_intact(self):
        raw = self.wide.view(torch.uint8).view(*self.wide.shape, self.wide.element_size())
        return bool((raw[self.mask] == self.byte).all())


def run_both(monkeypatch, run, finite=True):
    """run(byte) -> {name: owned output, a tensor or a numpy array}, under the poisoned allocator of each fill; the outputs of the two runs
    are equal bit for bit and the 0xFF run's floating-point outputs are finite (finite=False: an output whose values include -inf by
    definition).  Returns the 0x00 run's outputs (tensors on the host)."""
    outs = {}
    for byte in FILLS:
        with poisoned(monkeypatch, byte) as p:
            got = run(byte)
            torch.cuda.synchronize()
            outs[byte] = {k: torch.as_tensor(v).detach().clone().cpu() for k, v in got.items()}
            p.check_guards()
            assert not p.passed_through, f"device allocations the helper did not poison: {p.passed_through}"
    assert list(outs[0x00]) == list(outs[0xFF])
    for k, a in outs[0x00].items():
        b = outs[0xFF][k]
        assert a.shape == b.shape and a.dtype == b.dtype, f"{k}: {tuple(a.shape)} {a.dtype} under 0x00, {tuple(b.shape)} {b.dtype} under 0xFF"
        same = bits(a) == bits(b)
        assert bool(same.all()), f"{k}: {int((~same).sum())} of {same.numel()} values depend on unowned bytes (first at {torch.nonzero(~same)[0].tolist()})"
        if finite and b.is_floating_point():
            assert bool(torch.isfinite(b.float()).all()), f"{k}: non-finite outputs under the 0xFF fill"
    return outs[0x00]


def conv_inputs(B, H, W, cin, cout, k, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, cin, generator=g) * 0.8
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.2
    return g, x, w, b


# ---- aq_conv2d: implicit-GEMM and halo kernels, every tile configuration ------------------------------------------------------------
# B, H, W, cin, cout, k, stride, act, residual
CONV_CASES = [(1, 9, 7, 32, 64, 3, 1, True, True),           # ragged; 64 output channels under tiles of up to 384 rows
              (2, 20, 20, 48, 48, 3, 1, True, False),        # the partial K chunk
              (3, 8, 8, 384, 32, 1, 1, False, False),
              (1, 16, 24, 48, 96, 3, 2, True, False)]


def conv_all_configs(lib, monkeypatch, shape, cin, cout, xv, rv, odt, call):
    """call(x slice, residual slice or None, out slice, cfg) under both fills, for every tile configuration and its one-tile-per-workgroup
    form; a configuration the layer cannot run ("halo conv: ...") is left out, as the family's parity test leaves it out.  Returns
    {cfg: output of the 0x00 run}; the one-tile form's bytes are the plain form's."""
    from aquaculture_amd import engine
    B, H, W, Ho, Wo = shape

    def run(byte):
        xs = Slice(B, H, W, cin, xv.dtype, byte, xv)
        rs = Slice(B, Ho, Wo, cout, rv.dtype, byte, rv) if rv is not None else None
        outs = {}
        for cfg in range(lib.aq_conv_num_configs()):
            for one in (0, engine.CONV_CFG_ONE_TILE_PER_WG):
                os_ = Slice(B, Ho, Wo, cout, odt, byte)
                try:
                    call(xs.view, rs.view if rs else None, os_.view, cfg | one)
                except RuntimeError as err:
                    assert "halo conv" in str(err), err
                    continue
                assert os_.filler_intact(), f"cfg {cfg | one} wrote outside its channel slice"
                outs[cfg | one] = os_.view
        assert xs.filler_intact() and (rs is None or rs.filler_intact())
        return outs

    outs = run_both(monkeypatch, run)
    plain = {c: o for c, o in outs.items() if not c & engine.CONV_CFG_ONE_TILE_PER_WG}
    assert len(plain) >= 10 and len(outs) == 2 * len(plain)
    for c, o in plain.items():
        assert torch.equal(bits(outs[c | engine.CONV_CFG_ONE_TILE_PER_WG]), bits(o)), c
    return plain


@pytest.mark.parametrize("case", CONV_CASES)
@pytest.mark.parametrize("precision", ["fp32", "bf16", "f16x3"])
def test_conv2d(lib, monkeypatch, case, precision):
    """References and tolerances: test_conv_matches_reference (fp32, bf16) and test_conv_split_mode_is_fp32_grade (f16x3: an fp64
    reference, the error within 4x the exact-fp32 kernel's on the same layer and tile shape)."""
    from aquaculture_amd import engine
    B, H, W, cin, cout, k, stride, act, use_res = case
    g = torch.Generator().manual_seed(1234 + cin + cout)
    x = torch.randn(B, H, W, cin, generator=g) * (2.0 if precision == "f16x3" else 1.0)
    w = torch.randn(cout, cin, k, k, generator=g) * (2.0 / (cin * k * k)) ** 0.5
    if precision == "f16x3":
        w = w * (10.0 ** torch.linspace(-3, 1, cout)).view(-1, 1, 1, 1)
    b = torch.randn(cout, generator=g) * 0.1
    pad = k // 2
    Ho, Wo = (H + 2 * pad - k) // stride + 1, (W + 2 * pad - k) // stride + 1
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    xv = x.to(dt)
    rv = torch.randn(B, Ho, Wo, cout, generator=g).to(dt) if use_res else None
    outs = conv_all_configs(lib, monkeypatch, (B, H, W, Ho, Wo), cin, cout, xv, rv, dt,
                            lambda xs, res, out, cfg: engine.conv2d_nhwc(xs, w, b, stride=stride, act=act, residual=res, precision=precision, cfg=cfg, out=out))
    if precision == "f16x3":
        y = F.conv2d(x.double().permute(0, 3, 1, 2), w.double(), b.double(), stride=stride, padding=pad)
        y = F.silu(y) if act else y
        ref = (y + rv.double().permute(0, 3, 1, 2) if use_res else y).permute(0, 2, 3, 1)
        scale = ref.abs().amax(dim=(0, 1, 2), keepdim=True).clamp_min(1e-30)
        o32 = engine.conv2d_nhwc(xv.cuda(), w, b, stride=stride, act=act, residual=rv.cuda() if use_res else None, precision="fp32", cfg=min(outs))
        e32 = ((o32.cpu().double() - ref).abs() / scale).max().item()
        for cfg, out in outs.items():
            e3 = ((out.double() - ref).abs() / scale).max().item()
            assert e3 <= max(4.0 * e32, 2e-6), (cfg, e3, e32)
            torch.testing.assert_close(out, ref.float(), rtol=2e-5, atol=2e-5 * float(scale.max()))
        return
    ref = _ref(xv, w, b, stride, pad, act, rv, precision == "bf16")
    for cfg, out in outs.items():
        if precision == "fp32":
            torch.testing.assert_close(out, ref, rtol=2e-5, atol=2e-5)
        else:
            torch.testing.assert_close(out.float(), ref.bfloat16().float(), rtol=2 ** -7, atol=1e-3)


def test_conv2d_f32_out_head(lib, monkeypatch):
    """The Detect-head form of test_conv_f32_out_head: bf16 in, fp32 out, no activation, 30 live rows of 32."""
    from aquaculture_amd import engine
    B, H, W = 2, 5, 7
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, H, W, 192, generator=g).bfloat16()
    w, b = torch.zeros(32, 192, 1, 1), torch.zeros(32)
    w[:30] = torch.randn(30, 192, 1, 1, generator=g) * 0.1
    b[:30] = torch.randn(30, generator=g)
    outs = conv_all_configs(lib, monkeypatch, (B, H, W, H, W), 192, 32, x, None, torch.float32,
                            lambda xs, res, out, cfg: engine.conv2d_nhwc(xs, w, b, act=False, precision="bf16", out_f32=True, cfg=cfg, out=out))
    ref = _ref(x, w, b, 1, 0, False, None, True)
    for cfg, out in outs.items():
        torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)


# ---- stem, stem + down-block ---------------------------------------------------------------------------------------------------------
def tiles_between(B, H, W, byte, seed):
    """uint8 tiles [B, H, W, 3] as images 1 .. B of a batch whose first and last image hold the fill."""
    g = torch.Generator().manual_seed(seed)
    x = torch.randint(0, 256, (B, H, W, 3), generator=g, dtype=torch.uint8)
    wide = filled((B + 2, H, W, 3), torch.uint8, byte)
    wide[1:1 + B] = x.cuda()
    return x, wide


@pytest.mark.parametrize("shape", [(1, 16, 24), (3, 32, 160)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_stem_conv(lib, monkeypatch, shape, precision):
    from aquaculture_amd import engine
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 31 + W)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    b = torch.randn(48, generator=g) * 0.1
    x = tiles_between(B, H, W, 0, H + W)[0]
    xin, wq = x.permute(0, 3, 1, 2).float() / 255, w
    if precision == "bf16":
        xin, wq = xin.bfloat16().float(), w.bfloat16().float()
    ref = F.silu(F.conv2d(xin, wq, b, stride=2, padding=2)).permute(0, 2, 3, 1).contiguous()

    def run(byte):
        wide = tiles_between(B, H, W, byte, H + W)[1]
        out = engine.stem_conv_nhwc(wide[1:1 + B], w, b, precision=precision)
        assert bool((wide[0] == byte).all()) and bool((wide[-1] == byte).all())
        return {"out": out}

    out = run_both(monkeypatch, run)["out"].float()
    if precision == "fp32":
        torch.testing.assert_close(out, ref, rtol=2e-5, atol=2e-5)
    else:
        torch.testing.assert_close(out, ref.bfloat16().float(), rtol=2 ** -7, atol=1e-3)


def downblock_weights(g):
    wa = torch.randn(96, 48, 3, 3, generator=g) * (2.0 / (9 * 48)) ** 0.5
    wb = torch.randn(96, 96, 1, 1, generator=g) * (2.0 / 96) ** 0.5
    return wa, torch.randn(96, generator=g) * 0.2, wb, torch.randn(96, generator=g) * 0.2


@pytest.mark.parametrize("shape", [(1, 16, 24), (3, 148, 92)])
def test_stemdown(lib, monkeypatch, shape):
    """aq_stemdown: bit-identical to aq_stem_conv followed by aq_downblock (its own test's reference), computed here on clean buffers."""
    from aquaculture_amd import engine
    B, Hi, Wi = shape
    g = torch.Generator().manual_seed(Hi + Wi)
    ws = torch.randn(48, 3, 6, 6, generator=g) * 0.25
    bs = torch.randn(48, generator=g) * 0.3
    wa, ba, wb, bb = downblock_weights(g)
    x = tiles_between(B, Hi, Wi, 0, Hi * 3 + Wi)[0].cuda()
    ref = engine.downblock_nhwc(engine.stem_conv_nhwc(x, ws, bs, act=True, precision="bf16"), wa, ba, wb, bb).cpu()

    def run(byte):
        wide = tiles_between(B, Hi, Wi, byte, Hi * 3 + Wi)[1]
        os_ = Slice(B, Hi // 4, Wi // 4, 96, torch.bfloat16, byte)
        engine.stemdown_nhwc(wide[1:1 + B], ws, bs, wa, ba, wb, bb, out=os_.view)
        assert os_.filler_intact() and bool((wide[0] == byte).all()) and bool((wide[-1] == byte).all())
        return {"out": os_.view}

    out = run_both(monkeypatch, run)["out"]
    assert torch.equal(bits(out), bits(ref)) and float(ref.float().abs().mean()) > 0.05


# ---- fused Bottleneck, C3 tail, down-block, direct 3x3/s2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("c", [16, 32, 48, 64, 96])
@pytest.mark.parametrize("shape", [(1, 7, 5), (2, 16, 32)])
def test_bottleneck(lib, monkeypatch, c, shape):
    from aquaculture_amd import engine
    B, H, W = shape
    g = torch.Generator().manual_seed(c * 1000 + H)
    x = (torch.randn(B, H, W, c, generator=g) * 0.8).bfloat16()
    w1 = torch.randn(c, c, 1, 1, generator=g) * (2.0 / c) ** 0.5
    w2 = torch.randn(c, c, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5
    b1, b2 = torch.randn(c, generator=g) * 0.2, torch.randn(c, generator=g) * 0.2

    def run(byte):
        xs = Slice(B, H, W, c, torch.bfloat16, byte, x)
        outs = {}
        for shortcut in (True, False):
            os_ = Slice(B, H, W, c, torch.bfloat16, byte)
            engine.bottleneck_nhwc(xs.view, w1, b1, w2, b2, shortcut, out=os_.view)
            assert os_.filler_intact(), "wrote outside its channel slice"
            outs[f"shortcut {shortcut}"] = os_.view
        assert xs.filler_intact()
        return outs

    outs = run_both(monkeypatch, run)
    for shortcut in (True, False):
        ref = _bottleneck_reference(x, w1, b1, w2, b2, shortcut)
        err = (outs[f"shortcut {shortcut}"].float() - ref).abs()
        assert (err <= 2 ** -7 * ref.abs() + 2e-2).all(), float(err.max())
        assert float(err.mean()) < 3e-3


# the kernel wants two 16 x 16 tiles per row: (1, 1, 17) is the smallest image it takes; (2, 17, 20): a one-row last tile row, batch seam
C3TAIL_SHAPES = [(1, 1, 17), (2, 17, 20)]


@pytest.mark.parametrize("shape", C3TAIL_SHAPES)
@pytest.mark.parametrize("shortcut", [True, False])
def test_bottleneck_c3tail(lib, monkeypatch, shape, shortcut):
    """aq_bottleneck_c3tail against its own test's reference: aq_bottleneck into the concat buffer, then aq_conv1x1_direct over it, bit for bit."""
    from aquaculture_amd import engine
    from test_gpu_c3tail import _weights
    B, H, W = shape
    ld = (PAD + 48 + PAD, PAD + 48 + PAD, PAD + 96 + PAD)
    assert engine.bottleneck_c3tail_supported(B, H, W, *ld) and not engine.bottleneck_c3tail_supported(1, 1, 16, *ld)
    p = _weights(B + H)
    g = torch.Generator().manual_seed(W)
    x = torch.randn(B, H, W, 48, generator=g).bfloat16()
    cv2 = torch.randn(B, H, W, 48, generator=g).bfloat16()
    cat = torch.zeros(B, H, W, 96, dtype=torch.bfloat16, device="cuda")
    cat[..., 48:] = cv2.cuda()
    engine.bottleneck_nhwc(x.cuda(), p["w1"], p["b1"], p["w2"], p["b2"], shortcut, out=cat[..., :48])
    ref = engine.conv1x1_direct_nhwc(cat, p["w3"], p["b3"]).cpu()

    def run(byte):
        xs = Slice(B, H, W, 48, torch.bfloat16, byte, x)
        cs = Slice(B, H, W, 48, torch.bfloat16, byte, cv2)
        os_ = Slice(B, H, W, 96, torch.bfloat16, byte)
        packed = engine.pack_bottleneck_c3tail(p["w1"], p["b1"], p["w2"], p["b2"], p["w3"], p["b3"], "cuda")
        engine.bottleneck_c3tail_nhwc(xs.view, cs.view, packed, shortcut, out=os_.view)
        assert xs.filler_intact() and cs.filler_intact() and os_.filler_intact()
        return {"out": os_.view}

    assert torch.equal(bits(run_both(monkeypatch, run)["out"]), bits(ref))


@pytest.mark.parametrize("shape", [(1, 6, 10), (1, 36, 44)])
def test_downblock(lib, monkeypatch, shape):
    from aquaculture_amd import engine
    B, H, W = shape
    g = torch.Generator().manual_seed(H * 7 + W)
    x = (torch.randn(B, H, W, 48, generator=g) * 0.8).bfloat16()
    wa, ba, wb, bb = downblock_weights(g)

    def run(byte):
        xs = Slice(B, H, W, 48, torch.bfloat16, byte, x)
        os_ = Slice(B, H // 2, W // 2, 96, torch.bfloat16, byte)
        engine.downblock_nhwc(xs.view, wa, ba, wb, bb, out=os_.view)
        assert xs.filler_intact() and os_.filler_intact()
        return {"out": os_.view}

    got = run_both(monkeypatch, run)["out"].float()
    t = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), wa.bfloat16().float(), ba, stride=2, padding=1)).bfloat16().float()
    ref = F.silu(F.conv2d(t, wb.bfloat16().float(), bb)).permute(0, 2, 3, 1).contiguous()
    err = (got - ref).abs()
    assert (err <= 2 ** -7 * ref.abs() + 2e-2).all(), float(err.max())
    assert float(err.mean()) < 3e-3


@pytest.mark.parametrize("shape", [(1, 6, 10), (1, 36, 44)])
def test_conv3x3s2_direct(lib, monkeypatch, shape):
    from aquaculture_amd import engine
    B, H, W = shape
    g, x, w, b = conv_inputs(B, H, W, 96, 192, 3, H * 5 + W)
    x = x.bfloat16()

    def run(byte):
        xs = Slice(B, H, W, 96, torch.bfloat16, byte, x)
        outs = {}
        for act in (True, False):
            os_ = Slice(B, H // 2, W // 2, 192, torch.bfloat16, byte)
            engine.conv3x3s2_direct_nhwc(xs.view, w, b, act, out=os_.view)
            assert os_.filler_intact()
            outs[f"act {act}"] = os_.view
        assert xs.filler_intact()
        return outs

    outs = run_both(monkeypatch, run)
    for act in (True, False):
        ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, stride=2, padding=1)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
        torch.testing.assert_close(outs[f"act {act}"].float(), ref.bfloat16().float(), rtol=2 ** -7, atol=4e-3)


# ---- 1x1 kernels ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cin,cout", [(96, 96), (192, 192), (384, 192), (384, 384)])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 37, 41)])
def test_conv1x1_direct(lib, monkeypatch, cin, cout, shape):
    from aquaculture_amd import engine
    B, H, W = shape
    g, x, w, b = conv_inputs(B, H, W, cin, cout, 1, cin + H)
    x = x.bfloat16()

    def run(byte):
        xs = Slice(B, H, W, cin, torch.bfloat16, byte, x)
        outs = {}
        for act in (True, False):
            os_ = Slice(B, H, W, cout, torch.bfloat16, byte)
            engine.conv1x1_direct_nhwc(xs.view, w, b, act, out=os_.view)
            assert os_.filler_intact()
            outs[f"act {act}"] = os_.view
        assert xs.filler_intact()
        return outs

    outs = run_both(monkeypatch, run)
    for act in (True, False):
        ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)
        ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
        torch.testing.assert_close(outs[f"act {act}"].float(), ref.bfloat16().float(), rtol=2 ** -7, atol=2e-3)


@pytest.mark.parametrize("c", [192, 384])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 37, 41)])
def test_conv1x1_direct_f8out(lib, monkeypatch, c, shape):
    """aq_conv1x1_direct_f8out: the e4m3 codes of SiLU(conv1x1) / scale, checked as its own test checks them."""
    from aquaculture_amd import engine
    B, H, W = shape
    g, x, w, b = conv_inputs(B, H, W, c, c, 1, c + H)
    x = x.bfloat16()
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)).permute(0, 2, 3, 1)
    scale = float(ref.abs().max()) / 448.0 * 0.9
    want = (ref / scale).clamp(-448, 448).to(torch.float8_e4m3fn)
    wk = np.ascontiguousarray(w.permute(0, 2, 3, 1).float().numpy())
    wp = wk.ctypes.data_as(C.POINTER(C.c_float))

    def run(byte):
        xs = Slice(B, H, W, c, torch.bfloat16, byte, x)
        os_ = Slice(B, H, W, c, torch.uint8, byte, back=c + 16)          # codes in the first bytes of a wider (bf16-sized) row
        n = C.c_size_t()
        engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, None, C.byref(n), None))
        wbuf = torch.empty(n.value, dtype=torch.uint8, device="cuda")
        engine._check(lib.aq_pack_conv1x1_direct(wp, c, c, wbuf.data_ptr(), C.byref(n), engine._stream_ptr()))
        bbuf = b.float().cuda()
        engine._check(lib.aq_conv1x1_direct_f8out(xs.view.data_ptr(), xs.wide.shape[3], 0, os_.view.data_ptr(), os_.wide.shape[3], 0, c, c,
                                                  wbuf.data_ptr(), bbuf.data_ptr(), B * H * W, 1, scale, engine._stream_ptr()))
        torch.cuda.synchronize()
        assert xs.filler_intact() and os_.filler_intact()
        return {"codes": os_.view}

    got = run_both(monkeypatch, run)["codes"]
    gv, wv = got.view(torch.float8_e4m3fn).float(), want.float()
    assert not torch.isnan(gv).any() and float(gv.max()) == 448.0
    assert (got == want.view(torch.uint8)).float().mean().item() > 0.99
    assert ((gv - wv).abs() <= 0.126 * wv.abs().clamp_min(2.0 ** -9)).all()


@pytest.mark.parametrize("cin,cout", [(96, 384), (768, 384), (1536, 768)])
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 37, 41)])
@pytest.mark.parametrize("family", [13, 7])
def test_conv1x1_asm(lib, monkeypatch, cin, cout, shape, family):
    from aquaculture_amd import engine
    monkeypatch.setenv("AQ_C1_ASM_NB", str(family))
    B, H, W = shape
    g, x, w, b = conv_inputs(B, H, W, cin, cout, 1, cin + H)
    x = x.bfloat16()

    def run(byte):
        xs = Slice(B, H, W, cin, torch.bfloat16, byte, x)
        os_ = Slice(B, H, W, cout, torch.bfloat16, byte)
        engine.conv1x1_asm_nhwc(xs.view, w, b, out=os_.view)
        assert xs.filler_intact() and os_.filler_intact()
        return {"out": os_.view}

    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b)).permute(0, 2, 3, 1)
    torch.testing.assert_close(run_both(monkeypatch, run)["out"].float(), ref.bfloat16().float(), rtol=2 ** -7, atol=2e-3)


# ---- planar 3x3 ----------------------------------------------------------------------------------------------------------------------
PL_SHAPES = [(1, 9, 7, 192, 192), (2, 13, 24, 128, 192), (4, 12, 12, 128, 576)]
RESMODES = [None, "sep", "inplace"]


def pl_run(monkeypatch, call, B, H, W, cin, c, resmode, x, xdt, res_value):
    """The planar kernels' common case: x a slice, out a slice, the shortcut a slice of its own or the output itself (owned values pre-set)."""
    def run(byte):
        xs = Slice(B, H, W, cin, xdt, byte, x)
        os_ = Slice(B, H, W, c, torch.bfloat16, byte)
        rs, res = None, None
        if resmode == "sep":
            rs = Slice(B, H, W, c, torch.bfloat16, byte, res_value)
            res = rs.view
        elif resmode == "inplace":
            os_.view.copy_(res_value)
            res = os_.view
        call(xs.view, res, os_.view)
        assert xs.filler_intact() and os_.filler_intact() and (rs is None or rs.filler_intact()), "wrote outside its channel slice"
        return {"out": os_.view}
    return run_both(monkeypatch, run)["out"].float()


@pytest.mark.parametrize("shape", PL_SHAPES)
@pytest.mark.parametrize("resmode", RESMODES)
@pytest.mark.parametrize("nb", ["13asm", "13slot-asm", "13pm-asm", "7asm", "8asm", 13, 10, 7])
def test_conv3x3_pl(lib, monkeypatch, shape, resmode, nb):
    """Every build test_planar_conv3x3_matches_reference enumerates (unbuilt experimental families skipped the same way)."""
    from aquaculture_amd import engine
    B, H, W, cin, c = shape
    monkeypatch.setenv("AQ_PL_ASM", "1" if isinstance(nb, str) else "0")
    if nb in ("13slot-asm", "13pm-asm"):
        monkeypatch.setenv("AQ_PL_PM", "0" if nb == "13slot-asm" else "2")
        nb = "13asm"
    if isinstance(nb, str) and not lib.aq_conv3x3_pl_asm_family(int(nb[:-3])):
        pytest.skip("experimental assembly family: built only with AQ_GEN_EXPERIMENTAL=1")
    nb = int(nb[:-3]) if isinstance(nb, str) else nb
    monkeypatch.setenv("AQ_PL_NB", str(nb))
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 7 + H * 3 + nb)
    x = x.bfloat16()
    resv = torch.randn(B, H, W, c, generator=g).bfloat16()
    if nb == 8 and (W > 40 or (c // 192) & (c // 192 - 1)):
        with pytest.raises(RuntimeError, match="no tile of this kernel fits"):
            engine.conv3x3_pl_nhwc(x.cuda(), w, b, True)
        return
    got = pl_run(monkeypatch, lambda xv, res, out: engine.conv3x3_pl_nhwc(xv, w, b, True, residual=res, out=out), B, H, W, cin, c, resmode, x,
                 torch.bfloat16, resv)
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, padding=1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.float()
    torch.testing.assert_close(got, ref.bfloat16().float(), rtol=2 ** -7, atol=4e-3)


@pytest.mark.parametrize("shape", PL_SHAPES)
@pytest.mark.parametrize("resmode", RESMODES)
def test_conv3x3_pl_w8(lib, monkeypatch, shape, resmode):
    """The e4m3 weight stream: weights on the fp8 grid, the reference and tolerance of the bf16 stream (test_gpu_fp8w.py)."""
    from aquaculture_amd import engine, quant
    B, H, W, cin, c = shape
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 7 + H * 3)
    x = x.bfloat16()
    wq = torch.from_numpy(quant.quantize_rows(w.numpy())[0])
    assert bool(lib.aq_conv3x3_pl_w8_supported(cin, c, B, H, W)) == (c != 576)
    if c == 576:                                             # cout / 192 is no power of two: refused, nothing is launched
        with pytest.raises(RuntimeError, match="does not support this shape"):
            engine.conv3x3_pl_nhwc(x.cuda(), wq, b, True, w8=True)
        return
    resv = torch.randn(B, H, W, c, generator=g).bfloat16()
    got = pl_run(monkeypatch, lambda xv, res, out: engine.conv3x3_pl_nhwc(xv, wq, b, True, residual=res, out=out, w8=True), B, H, W, cin, c,
                 resmode, x, torch.bfloat16, resv)
    ref = F.silu(F.conv2d(x.float().permute(0, 3, 1, 2), wq.bfloat16().float(), b, padding=1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.float()
    torch.testing.assert_close(got, ref.bfloat16().float(), rtol=2 ** -7, atol=4e-3)


@pytest.mark.parametrize("shape", PL_SHAPES)
@pytest.mark.parametrize("resmode", RESMODES)
def test_conv3x3_pl_f8(lib, monkeypatch, shape, resmode):
    """fp8 MFMA on both operands; reference and bounds of test_planar_conv3x3_f8_matches_reference."""
    from aquaculture_amd import engine
    B, H, W, cin, c = shape
    assert bool(lib.aq_conv3x3_pl_f8_supported(cin, c, B, H, W)) == (c != 576)
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
    if c == 576:                                             # cout / 192 is no power of two: the launcher refuses, nothing is launched
        with pytest.raises(RuntimeError, match="conv3x3_pl_f8: unsupported"):
            engine.conv3x3_pl_f8_nhwc(xq.view(torch.uint8).cuda(), act_scale, w, b, True)
        return
    got = pl_run(monkeypatch, lambda xv, res, out: engine.conv3x3_pl_f8_nhwc(xv, act_scale, w, b, True, residual=res, out=out), B, H, W, cin, c,
                 resmode, xq.view(torch.uint8), torch.uint8, resv)
    ref = F.conv2d(xq.float().double().permute(0, 3, 1, 2), wq.float().double(), None, padding=1)
    ref = F.silu(ref * (act_scale * ws.view(1, -1, 1, 1).double()) + b.double().view(1, -1, 1, 1)).permute(0, 2, 3, 1)
    if resmode:
        ref = ref + resv.double()
    scale = ref.abs().amax(dim=(0, 1, 2)).clamp_min(1e-6).float()
    assert ((got - ref.float()).abs() / scale).max().item() <= 2 ** -7
    torch.testing.assert_close(got, ref.float().bfloat16().float(), rtol=2 ** -6, atol=2e-2 * float(scale.max()))


@pytest.mark.parametrize("case", [(1, 18, 14, 64, 192, True), (2, 4, 4, 64, 192, False), (2, 26, 48, 96, 192, True)])
def test_conv3x3_pl_s2(lib, monkeypatch, case):
    from aquaculture_amd import engine
    B, H, W, cin, c, act = case
    assert lib.aq_conv3x3_pl_s2_supported(cin, c, B, H, W)
    g, x, w, b = conv_inputs(B, H, W, cin, c, 3, c * 5 + H * 3 + cin)
    x = x.bfloat16()

    def run(byte):
        xs = Slice(B, H, W, cin, torch.bfloat16, byte, x)
        os_ = Slice(B, H // 2, W // 2, c, torch.bfloat16, byte)
        engine.conv3x3_pl_s2_nhwc(xs.view, w, b, act, out=os_.view)
        assert xs.filler_intact() and os_.filler_intact(), "wrote outside its channel slice"
        return {"out": os_.view}

    ref = F.conv2d(x.float().permute(0, 3, 1, 2), w.bfloat16().float(), b, stride=2, padding=1)
    ref = (F.silu(ref) if act else ref).permute(0, 2, 3, 1)
    torch.testing.assert_close(run_both(monkeypatch, run)["out"].float(), ref.bfloat16().float(), rtol=2 ** -7, atol=4e-3)


# ---- Detect head fused with its decode -----------------------------------------------------------------------------------------------
def by_candidate(counts, cand, rows):
    """The candidate list in candidate order (the order within an image is unspecified): per image (indices, rows), and the counters."""
    counts, cand, rows = counts.cpu(), cand.cpu(), rows.cpu()
    out = {"counts": counts}
    for bi in range(cand.shape[0]):
        n = min(int(counts[bi]), cand.shape[1])
        o = torch.argsort(cand[bi, :n])
        out[f"cand {bi}"], out[f"rows {bi}"] = cand[bi, :n][o], rows[bi, :n][o]
    return out


@pytest.mark.parametrize("cin", WIDTHS)
@pytest.mark.parametrize("nc", [5, 4])
@pytest.mark.parametrize("aug", [False, True])
def test_head_decode(lib, monkeypatch, cin, nc, aug):
    """Counters, candidate indices and rows as the wrapper allocates them (zeroed counters, -1 indices, zero rows: the counters' zero on
    entry is the entry point's contract); the packed weights, the channels beside x and the images round the batch are poisoned."""
    from aquaculture_amd import engine
    B, ny, nx = 3, 5, 7
    xw, x, w, b = make_level(B, ny, nx, cin, 3, nc, cin + ny)
    cap, off, thr, stride, scale, flip_w = 3 * ny * nx, 1000, 0.25, 16.0, 0.67, 640.0

    def run(byte):
        xs = Slice(B, ny, nx, cin, torch.bfloat16, byte, x)
        if aug:
            got = engine.head_decode_level_aug(xs.view, w, b, off, stride, ANCHORS, nc, thr, cap, scale, flip_w)
        else:
            got = engine.head_decode_level(xs.view, w, b, off, stride, ANCHORS, nc, thr, cap)
        assert xs.filler_intact()
        for bi in range(B):
            assert bool((got[1][bi, int(got[0][bi]):] == -1).all())
        return by_candidate(*got)

    outs = run_both(monkeypatch, run)
    ref = head_reference(x, w, b, ANCHORS, nc, stride)
    if aug:                                                  # [UPSTREAM _descale_pred]
        ref[..., :4] /= scale
        ref[..., 0] = flip_w - ref[..., 0]
    cand = torch.full((B, cap), -1, dtype=torch.int32)
    rows = torch.zeros((B, cap, nc + 5))
    for bi in range(B):
        n = outs[f"cand {bi}"].numel()
        cand[bi, :n], rows[bi, :n] = outs[f"cand {bi}"], outs[f"rows {bi}"]
    assert check_level(outs["counts"], cand, rows, ref, off, thr, cap)[3] > 0.1 * B * cap


# ---- pointwise kernels ---------------------------------------------------------------------------------------------------------------
POINT_SHAPES = [(1, 5, 3, 8), (3, 13, 17, 16)]


@pytest.mark.parametrize("shape", POINT_SHAPES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sppf_pool(lib, monkeypatch, shape, precision):
    """aq_sppf_pool in place on [x | y1 | y2 | y3]: bit-exact against three chained MaxPool2d(5, 1, 2); the y slices enter holding the fill."""
    from aquaculture_amd import engine
    B, H, W, c = shape
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    g = torch.Generator().manual_seed(H * 31 + c)
    x = torch.randn(B, H, W, c, generator=g).to(dt)

    def run(byte):
        s = Slice(B, H, W, 4 * c, dt, byte)
        s.view[..., :c] = x.cuda()
        engine._check(lib.aq_sppf_pool(s.wide[1:].data_ptr(), s.wide.shape[3], s.front, c, B, H, W, 0 if precision == "bf16" else 1, engine._stream_ptr()))
        torch.cuda.synchronize()
        assert s.filler_intact()
        return {"buf": s.view}

    got = run_both(monkeypatch, run)["buf"]
    y = x.float().permute(0, 3, 1, 2)
    assert torch.equal(got[..., :c], x)
    for i in range(1, 4):
        y = F.max_pool2d(y, 5, 1, 2)
        assert torch.equal(got[..., i * c:(i + 1) * c].float(), y.permute(0, 2, 3, 1)), i


@pytest.mark.parametrize("shape", POINT_SHAPES)
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_upsample2x(lib, monkeypatch, shape, precision):
    from aquaculture_amd import engine
    B, H, W, c = shape
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    x = torch.randn(B, H, W, c, generator=torch.Generator().manual_seed(H + c)).to(dt)

    def run(byte):
        xs = Slice(B, H, W, c, dt, byte, x)
        os_ = Slice(B, 2 * H, 2 * W, c, dt, byte)
        engine._check(lib.aq_upsample2x(xs.view.data_ptr(), xs.wide.shape[3], 0, os_.view.data_ptr(), os_.wide.shape[3], 0, c, B, H, W,
                                        0 if precision == "bf16" else 1, engine._stream_ptr()))
        torch.cuda.synchronize()
        assert xs.filler_intact() and os_.filler_intact()
        return {"out": os_.view}

    got = run_both(monkeypatch, run)["out"]
    assert torch.equal(got, x.repeat_interleave(2, 1).repeat_interleave(2, 2))       # nearest: copies, no rounding


def s2d_reference(xin):
    """(B, 3, H, W) float -> space-to-depth [B, H/2, W/2, 12] in the kernels' channel order (dy, dx, c)."""
    B, _, H, W = xin.shape
    return F.pixel_unshuffle(xin, 2).view(B, 3, 2, 2, H // 2, W // 2).permute(0, 4, 5, 2, 3, 1).reshape(B, H // 2, W // 2, 12)


@pytest.mark.parametrize("shape", [(1, 10, 6), (3, 26, 34)])                        # outputs (1, 5, 3) and (3, 13, 17), 16 channels
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_preprocess_s2d(lib, monkeypatch, shape, precision):
    from aquaculture_amd import engine
    B, H, W = shape
    dt = torch.bfloat16 if precision == "bf16" else torch.float32
    x = tiles_between(B, H, W, 0, H * W)[0]

    def run(byte):
        wide = tiles_between(B, H, W, byte, H * W)[1]
        out = torch.empty((B, H // 2, W // 2, 16), dtype=dt, device="cuda")
        engine._check(lib.aq_preprocess_s2d(wide[1:1 + B].data_ptr(), out.data_ptr(), B, H, W, 0 if precision == "bf16" else 1, engine._stream_ptr()))
        torch.cuda.synchronize()
        return {"out": out}

    got = run_both(monkeypatch, run)["out"]
    ref = s2d_reference(x.permute(0, 3, 1, 2).float() / 255)
    assert (got[..., 12:] == 0).all()
    if precision == "fp32":
        assert (got[..., :12] - ref).abs().max().item() <= 2 * np.finfo(np.float32).eps
    else:
        assert ((got[..., :12].float() - ref.bfloat16().float()).abs() <= 2 ** -7 * ref.abs()).all()


def scaled_pass(H, W, flip):
    """An --augment pass geometry at a small tile: the 0.67 pass of augment.geometry, flipped or not."""
    from aquaculture_amd import augment
    return augment.geometry(H, W)[0][2]._replace(flip=flip)


@pytest.mark.parametrize("shape", [(1, 64, 64), (3, 96, 160)])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("flip", [False, True])
def test_scaled_preprocess_and_stem(lib, monkeypatch, shape, precision, flip):
    """aq_preprocess_s2d_scaled and aq_stem_conv_scaled against the reference scaled image, at the bounds of test_gpu_augment.py."""
    from aquaculture_amd import engine
    from test_gpu_augment import scaled_input
    B, H, W = shape
    ps = scaled_pass(H, W, flip)
    g = torch.Generator().manual_seed(H + 2 * flip)
    w = torch.randn(48, 3, 6, 6, generator=g) * 0.2
    b = torch.randn(48, generator=g) * 0.1
    x = tiles_between(B, H, W, 0, H + W + flip)[0]
    xin = scaled_input(x.permute(0, 3, 1, 2).float() / 255, ps, W)

    def run(byte):
        wide = tiles_between(B, H, W, byte, H + W + flip)[1]
        s2d = engine.preprocess_s2d_scaled(wide[1:1 + B], ps.h, ps.w, ps.hp, ps.wp, flip, precision)
        stem = engine.stem_conv_scaled_nhwc(wide[1:1 + B], w, b, ps.h, ps.w, ps.hp, ps.wp, flip, precision=precision)
        return {"s2d": s2d, "stem": stem}

    outs = run_both(monkeypatch, run)
    ref = s2d_reference(xin)
    s2d, stem = outs["s2d"], outs["stem"].float()
    assert (s2d[..., 12:] == 0).all()
    xq, wq = (xin.bfloat16().float(), w.bfloat16().float()) if precision == "bf16" else (xin, w)
    sref = F.silu(F.conv2d(xq, wq, b, stride=2, padding=2)).permute(0, 2, 3, 1).contiguous()
    if precision == "fp32":
        assert (s2d[..., :12] - ref).abs().max().item() <= 2 * np.finfo(np.float32).eps
        assert (stem - sref).abs().max().item() <= 1e-5
    else:
        assert ((s2d[..., :12].float() - ref.bfloat16().float()).abs() <= 2 ** -7 * ref.abs()).all()
        torch.testing.assert_close(stem, sref.bfloat16().float(), rtol=2 ** -7, atol=1e-3)


# ---- NMS, augmented decode -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,seed", [(300, 2), (2049, 4)])
def test_nms(lib, monkeypatch, n, seed):
    """engine.nms with its key / box / bit-matrix scratch, detections and counts under the poisoned allocator; against the oracle as
    test_random_dense_matches_oracle checks it.  2049 candidates take the sort path, whose keys are padded to a power of two."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    from test_gpu_nms import _random_pred
    pred = _random_pred(np.random.default_rng(seed), n, spread=600.0 if n <= 300 else 3000.0)
    pred[0, :, 4] = np.maximum(pred[0, :, 4], 0.9)           # every row passes: n candidates
    pred[0, :, 5] = 0.95
    ref = O.non_max_suppression(pred, 0.25, 0.45, 1000)

    def run(byte):
        dets, counts = engine.nms(torch.from_numpy(pred).cuda().contiguous(), 5, 0.25, 0.45, 1000)
        counts = counts.cpu()
        return {"counts": counts, "dets": dets[0, :int(counts[0])]}

    outs = run_both(monkeypatch, run)
    assert int(outs["counts"][0]) == ref[0].shape[0] and np.array_equal(outs["dets"].numpy(), ref[0])


def test_detect_decode_aug(lib, monkeypatch):
    """aq_detect_decode_aug in pred mode on fp32 head maps (pass 2 of a 64 x 64 tile; the rows outside the pass stay zero: the wrapper
    allocates pred zeroed).  The head maps are dense (the wrapper takes no channel slice), between two filler images; compared between
    the two fills."""
    from aquaculture_amd import augment, engine
    H = W = 64
    passes, n = augment.geometry(H, W)
    ps = passes[2]
    g = torch.Generator().manual_seed(5)
    heads = [torch.randn(2, ps.hp // s, ps.wp // s, 30, generator=g) for s in (8, 16, 32)]
    ag = [[(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)], [(30.0, 61.0), (62.0, 45.0), (59.0, 119.0)], [(116.0, 90.0), (156.0, 198.0), (373.0, 326.0)]]

    def run(byte):
        batch = [filled((4,) + tuple(h.shape[1:]), torch.float32, byte) for h in heads]      # images 1, 2 of four are the heads'
        for t, h in zip(batch, heads):
            t[1:3] = h.cuda()
        pred = engine.detect_decode_aug([t[1:3] for t in batch], ps.hp, ps.wp, 5, ag, [8.0, 16.0, 32.0], ps.level_mask, ps.out_first - ps.keep_first, n,
                                        ps.scale, float(W) if ps.flip else 0.0)
        return {"pred": pred}

    pred = run_both(monkeypatch, run)["pred"]
    outside = torch.ones(n, dtype=torch.bool)
    outside[ps.out_first:ps.out_first + ps.keep_count] = False
    assert (pred[:, outside] == 0).all() and float(pred[:, ~outside].abs().sum()) > 0


# ---- JPEG decode, blank key and geometry, crop and frame encoders, annotation, facilities, evaluate, land filter, tonnage --------------
# Each at the smallest input its own GPU test uses, compared between the two fills: what the wrappers take from `torch.empty` (outputs,
# scratch, arenas, pinned arenas, status words) is poisoned; where the input is images in one buffer, the bytes round them hold the fill.

def test_jpeg_huffman_decode_and_idct_rgb(lib, monkeypatch):
    """aq_jpeg_huffman_decode into aq_jpeg_idct_rgb on 70 files of 33 x 17 (more than one wave of segments): the segment status, the
    coefficients and the pixels; the 0x00 run decodes every segment."""
    from aquaculture_amd import engine, jpeg
    from test_jpeg import _jpeg
    H, W = 33, 17
    data = _jpeg(np.random.default_rng(11).integers(0, 255, (H, W, 3), dtype=np.uint8), quality=80)
    B, n = 70, jpeg.coef_count(H, W)
    batch = jpeg.GpuDecodeBatch(B, H, W, bytes_per_image=jpeg.stream_capacity(H, W, 12))
    for i in range(B):
        assert batch.add(i, data) == 0
    segs, sets, _ = batch.finish()
    streams, segs, qt = batch.streams.copy(), segs.view(np.uint8).reshape(-1, 32).copy(), batch.qt.view(np.int16).copy()

    def run(byte):
        # csrc/jpeg_huff.hip: "coef_dev ... zeroed by the caller" (the kernel stores only non-zero coefficients): the one zero-on-entry
        # contract of these entry points, so exactly this buffer is zeroed; the status words and the IDCT scratch are poisoned
        coef = torch.zeros(B * n, dtype=torch.int16, device="cuda")
        st = engine.jpeg_huffman_decode(torch.from_numpy(streams).cuda(), torch.from_numpy(segs).cuda(), torch.from_numpy(sets).cuda(), coef)
        off = torch.arange(B, dtype=torch.int64, device="cuda") * n
        rgb = engine.jpeg_idct_rgb(coef, off, torch.from_numpy(qt).cuda(), H, W)
        return {"status": st, "coef": coef, "rgb": rgb}

    outs = run_both(monkeypatch, run)
    assert int(outs["status"].abs().max()) == 0 and bool((outs["rgb"] == outs["rgb"][0]).all()) and int(outs["rgb"].max()) > 200


def test_blank_stats(lib, monkeypatch):
    """aq_blank_stats_u8 on the branch cases in one buffer of mixed sizes; the 0x00 run is blank.stats_numpy's, field for field."""
    import test_gpu_blank_key as K
    images = [im for _, im in K.CASES]

    def run(byte):
        buf, bases, pitches = K._pack(images, fill=byte)
        return {"stats": K._gpu(buf, images, bases, pitches)[0]}

    K._check(run_both(monkeypatch, run)["stats"].numpy(), images)


def test_blank_components_and_ring_edges(lib, monkeypatch):
    """aq_blank_components_u8 and aq_blank_ring_edges_u8 on the constructed and random masks in one buffer: records, both label maps and
    the winner's edges."""
    import test_gpu_blank_geom as G
    images = [G.image_of(m, k) for k, (_, m) in enumerate(G.MASKS)]

    def run(byte):
        buf, bases, pitches = G._pack(images, fill=byte)
        rec, maps, edges, _, _ = G._gpu(buf, images, bases, pitches)
        out = {"records": rec}
        for k in range(len(images)):
            out[f"fg {k}"], out[f"bg {k}"], out[f"edges {k}"] = maps[k][0].copy(), maps[k][1].copy(), edges[k]
        return out

    outs = run_both(monkeypatch, run)
    assert {0, 1}.issubset(set(outs["records"][:, 1].tolist())) and int(outs["records"][:, 10].max()) > 0


def test_encode_crops(lib, monkeypatch):
    """aq_crop_jpeg_coefs through its device and pinned arenas, in one piece and in pieces of the largest crop."""
    from aquaculture_amd import engine
    from test_gpu_save_crop import SIZES, _rects
    rng, r2 = np.random.default_rng(0), np.random.default_rng(1)
    host, bases, pitches, rects, base = [], [], [], [], 16
    for h, w in SIZES:
        im = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        im[: h // 3] = im[: h // 3] // 64 * 64
        host.append(im.reshape(-1))
        for rect in _rects(h, w, r2):
            bases.append(base)
            pitches.append(3 * w)
            rects.append(rect)
        base += im.size
    table = engine.crop_table(np.asarray(bases), np.asarray(pitches), np.asarray(rects))
    largest = int(engine.crop_blocks(table).max())

    def run(byte):
        edge = np.full(16, byte, np.uint8)
        buf = torch.from_numpy(np.concatenate([edge] + host + [edge])).cuda()
        return {"one piece": engine.encode_crops(buf, table)[0], "pieces": engine.encode_crops(buf, table, arena_blocks=largest)[0]}

    outs = run_both(monkeypatch, run)
    assert torch.equal(outs["one piece"], outs["pieces"]) and outs["pieces"].shape == (int(engine.crop_blocks(table).sum()), 192)


def test_annotate_images_and_encode_frames(lib, monkeypatch):
    """aq_annotate_u8 on images of mixed sizes in one buffer, then aq_image_jpeg_coefs on the annotated copies (its arenas poisoned): each
    image's pixels (the bytes between two copies belong to nobody) and the coefficients, in one piece and in pieces of the largest frame."""
    from aquaculture_amd import engine
    from test_gpu_save_img import MIXED, _content, _draw, _random_boxes
    rng = np.random.default_rng(6)
    images = [_content("random", h, w, rng) for h, w in MIXED]
    dets = [_random_boxes(40, h, w, rng) for h, w in MIXED]

    def run(byte):
        got, _, _, (out, canvases) = _draw(images, dets, 2)
        table = engine.frame_table(canvases["dst"], canvases["dst_pitch"], list(MIXED))
        res = {f"image {k}": g for k, g in enumerate(got)}
        res["one piece"] = engine.encode_frames(out, table)[0]
        res["pieces"] = engine.encode_frames(out, table, arena_mcus=int(engine.frame_mcus(table).max()))[0]
        return res

    outs = run_both(monkeypatch, run)
    assert torch.equal(outs["one piece"], outs["pieces"]) and any(not np.array_equal(outs[f"image {k}"].numpy(), im) for k, im in enumerate(images))


@pytest.mark.parametrize("name", ["blobs_0", "two_groups", "border_b_first", "chain_9.99"])
def test_facility_dbscan(lib, monkeypatch, name):
    from aquaculture_amd import engine
    from test_facilities import CASES
    xy, group, eps, ms = CASES[name]

    def run(byte):
        core, root = engine.facility_dbscan(torch.from_numpy(xy).cuda(), torch.from_numpy(group).cuda(), eps, ms)
        return {"core": core, "root": root}

    outs = run_both(monkeypatch, run)
    assert int(outs["core"].sum()) > 0 and int(outs["root"].max()) >= 0


@pytest.mark.parametrize("name,K", [("one_point", 3), ("four_coincident", 6), ("blobs_0", 1), ("blobs_0", 10), ("blobs_0", 16)])
def test_eval_member_conf(lib, monkeypatch, name, K):
    from test_facilities import CASES
    from test_gpu_evaluate import confidences, member_gpu
    xy, group, eps, _ = CASES[name]
    conf = confidences(xy.shape[0], 7)
    M = run_both(monkeypatch, lambda byte: {"M": member_gpu(xy, group, conf, eps, K)}, finite=False)["M"]
    assert M.shape == (xy.shape[0], K) and bool(torch.isfinite(M[:, 0]).all())


def test_box_match(lib, monkeypatch):
    """aq_box_match_f64 on the edge / corner / degenerate boxes: with a payload, without one, with groups that have no keys, with no keys."""
    from test_gpu_evaluate import match_gpu
    k = np.array([[1.0, 0.0, 2.0, 1.0], [5.0, 4.0, 6.0, 5.0], [0.0, 0.0, 9.0, 9.0], [7.0, 7.0, 7.0, 7.0]])
    kg = np.array([0, 0, 1, 0], np.int32)
    pay = np.array([[0.25, 1.0], [0.5, 2.0], [0.75, 3.0], [0.125, 4.0]])
    q = np.array([[0.0, 0.0, 1.0, 1.0], [2.0, 1.0, 3.0, 2.0], [5.0, 5.0, 5.0, 5.0], [7.0, 7.0, 7.0, 7.0], [3.0, 0.0, 4.0, 1.0], [np.nextafter(2.0, 3.0), 0.0, 3.0, 1.0]])

    def run(byte):
        out = {}
        out["hit"], out["max"] = match_gpu(q, np.zeros(6, np.int32), k, kg, 2, pay)
        out["hit, no payload"] = match_gpu(q, np.ones(6, np.int32), k, kg, 2)[0]
        out["hit, no group"], out["max, no group"] = match_gpu(q, np.array([2, 3, -1, 4, 1 << 30, -(1 << 31)], np.int32), k, kg, 4, pay)
        out["hit, no keys"], out["max, no keys"] = match_gpu(q, np.zeros(6, np.int32), np.zeros((0, 4)), np.zeros(0, np.int32), 2, np.zeros((0, 3)))
        return out

    outs = run_both(monkeypatch, run, finite=False)
    assert outs["hit"].tolist() == [True, True, True, True, False, False] and outs["max"][:4].tolist() == [[0.25, 1.0], [0.25, 1.0], [0.5, 2.0], [0.125, 4.0]]
    assert not outs["hit, no group"].any() and not outs["hit, no keys"].any() and bool(torch.isneginf(outs["max, no keys"]).all())


@pytest.mark.parametrize("band_height", [None, 1000.0, 0.37])
def test_land_flags(lib, monkeypatch, band_height):
    """aq_land_filter_f64 on the named cases: the default bands, one band, bands thinner than the sliver is wide; without land the flags
    are the launcher's own zeros."""
    from test_gpu_land_filter import gpu_flags
    from test_land_filter import named_boxes, named_expected, named_land
    boxes, segs = named_boxes(), named_land()
    outs = run_both(monkeypatch, lambda byte: {"flags": gpu_flags(boxes, segs, band_height), "no land": gpu_flags(boxes, np.zeros((0, 4)))})
    assert outs["flags"].tolist() == named_expected().tolist() and not outs["no land"].any()


@pytest.mark.parametrize("name", ["one", "four", "resample"])
def test_tonnage_simulate_and_reduce(lib, monkeypatch, name):
    """aq_tonnage_simulate_f64 and aq_tonnage_reduce_f64, K = 65 in one chunk and in chunks of 30: ton, the passes' totals (the empty pass
    of "four" is the reduce kernel's own +0) and the moments, which the caller zeroes once and the chunks add to."""
    from test_gpu_tonnage import TABLES, run_gpu

    def run(byte):
        a, b = run_gpu(TABLES[name], 65, 0), run_gpu(TABLES[name], 65, 0, chunk=30)
        return {f"{k}{tag}": r[k] for tag, r in (("", a), (", chunks", b)) for k in ("ton", "T", "moments")}

    outs = run_both(monkeypatch, run)
    for k in ("ton", "T", "moments"):
        assert torch.equal(bits(outs[k]), bits(outs[k + ", chunks"])), k
    assert float(outs["ton"].abs().sum()) > 0
