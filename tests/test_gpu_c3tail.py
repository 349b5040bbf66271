"""The C3 tail (aq_bottleneck_c3tail): a C3 block's last Bottleneck (C = 48) with the block's cv3 1x1 (96 -> 96 + SiLU) in its epilogue.

The fused kernel rounds y to bf16 exactly where the two-launch form stores it, and runs cv3 in conv1x1_direct_kernel's order (accumulators
from zero, k-steps of 32 channels in order, bias after, the same SiLU sequence), so it must give the two launches' bits: aq_bottleneck into
the concat buffer, then aq_conv1x1_direct over it."""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _weights(seed, C=48):
    g = torch.Generator().manual_seed(seed)

    def w(*shape):
        fan_in = shape[1] * shape[2] * shape[3]
        return torch.randn(*shape, generator=g) * (1.5 / fan_in ** 0.5)

    return dict(w1=w(C, C, 1, 1), b1=torch.randn(C, generator=g) * 0.1, w2=w(C, C, 3, 3), b2=torch.randn(C, generator=g) * 0.1,
                w3=w(2 * C, 2 * C, 1, 1), b3=torch.randn(2 * C, generator=g) * 0.1)


def _inputs(B, H, W, seed, in_ld=48):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(B, H, W, in_ld, generator=g).to(torch.bfloat16).cuda()
    cat = torch.randn(B, H, W, 96, generator=g).to(torch.bfloat16).cuda()      # [m.1 out (overwritten by the two-launch form) | cv2 out]
    return x, cat


def _two_launches(x, cat, p, shortcut):
    from aquaculture_amd import engine
    cat2 = cat.clone()
    engine.bottleneck_nhwc(x[..., :48], p["w1"], p["b1"], p["w2"], p["b2"], shortcut, out=cat2[..., :48])
    return engine.conv1x1_direct_nhwc(cat2, p["w3"], p["b3"])


def _fused(x, cat, p, shortcut, out=None):
    from aquaculture_amd import engine
    packed = engine.pack_bottleneck_c3tail(p["w1"], p["b1"], p["w2"], p["b2"], p["w3"], p["b3"], x.device)
    return engine.bottleneck_c3tail_nhwc(x[..., :48], cat[..., 48:], packed, shortcut, out=out)


def _assert_same(got, ref, what):
    if not torch.equal(got, ref):
        d = (got.float() - ref.float()).abs()
        bad = torch.nonzero(d.reshape(-1, d.shape[-1]).amax(1)).flatten()
        pytest.fail(f"{what}: {bad.numel()} pixels differ (first {bad[:8].tolist()}), max |diff| {d.max().item():.4g}")


@pytest.mark.parametrize("B,H,W,shortcut", [(64, 160, 160, True),      # the benchmark's geometry (640 px tiles, batch 64)
                                            (3, 50, 70, True),          # ragged: odd batch, partial tiles at the right and bottom edges
                                            (2, 33, 32, False)])        # two tiles per row exactly, one-row last tile row, no shortcut
def test_fused_equals_two_launches(lib, B, H, W, shortcut):
    from aquaculture_amd import engine
    assert engine.bottleneck_c3tail_supported(B, H, W)
    p = _weights(B + H)
    x, cat = _inputs(B, H, W, seed=W)
    _assert_same(_fused(x, cat, p, shortcut), _two_launches(x, cat, p, shortcut), f"{B} x {H} x {W}")


def test_output_channel_offset_and_strided_inputs(lib):
    """x a slice of a wider tensor, out at channel 24 of a 128-channel tensor: the channels around it stay untouched."""
    B, H, W = 2, 48, 64
    p = _weights(7)
    x, cat = _inputs(B, H, W, seed=8, in_ld=64)
    x = x[..., 16:]                                     # 48 channels at offset 16 of a 64-channel row
    out = torch.full((B, H, W, 128), 3.0, dtype=torch.bfloat16, device="cuda")
    _fused(x, cat, p, True, out=out[..., 24:120])
    _assert_same(out[..., 24:120], _two_launches(x, cat, p, True), "out at channel 24")
    assert bool((out[..., :24] == 3.0).all()) and bool((out[..., 120:] == 3.0).all())


def test_narrow_image_is_unsupported(lib):
    """One tile per row: the assembly kernel's magic-number tile decode does not apply; the entry point refuses without a launch (the
    engine then runs the two launches)."""
    from aquaculture_amd import engine
    assert not engine.bottleneck_c3tail_supported(2, 64, 16)
    p = _weights(3)
    x, cat = _inputs(2, 64, 16, seed=3)
    with pytest.raises(Exception):
        _fused(x, cat, p, True)


def test_two_streams_match_one_stream(lib):
    """Two launches in flight on two streams (two workspaces, as two engine slots run them) give the one-stream results."""
    from aquaculture_amd import engine
    B, H, W = 16, 160, 160
    p = _weights(11)
    packed = engine.pack_bottleneck_c3tail(p["w1"], p["b1"], p["w2"], p["b2"], p["w3"], p["b3"], "cuda")
    ins = [_inputs(B, H, W, seed=s) for s in (21, 22)]
    ref = [engine.bottleneck_c3tail_nhwc(x[..., :48], cat[..., 48:], packed) for x, cat in ins]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    torch.cuda.synchronize()
    outs = []
    for rep in range(3):
        for (x, cat), st in zip(ins, streams):
            with torch.cuda.stream(st):
                outs.append(engine.bottleneck_c3tail_nhwc(x[..., :48], cat[..., 48:], packed, sync=False))
    torch.cuda.synchronize()
    for i, o in enumerate(outs):
        _assert_same(o, ref[i % 2], f"stream {i % 2}, repetition {i // 2}")


def _tail_pair(eng):
    from aquaculture_amd import spec
    ops = eng.plan.ops
    pairs = [i for i in range(len(ops) - 1) if ops[i].kind == spec.OP_BOTTLENECK and ops[i].src.channels == 48 and ops[i + 1].kind == spec.OP_CONV
             and ops[i + 1].k == 1 and ops[i + 1].src.tensor == ops[i].dst.tensor]
    assert len(pairs) == 1, pairs                       # yolov5m: model.2.m.1 -> model.2.cv3 (model.4 / model.17 have C = 96)
    return pairs[0]


@pytest.mark.parametrize("precision", ["bf16", "fp8w"])
def test_engine_detections_with_and_without_the_tail(lib, synth_ck, precision):
    """Whole engine, AQ_C3TAIL=0 against =1 (cv3 on the direct 1x1, as the shipped tuned tables run it): model.2's output, every later
    tensor and the detections are the same bits; stepping one op at a time runs the two launches and agrees too."""
    from aquaculture_amd import engine, tiles
    x = torch.from_numpy(tiles.synthetic_batch([0, 1, 2], 640)).cuda()
    old = os.environ.get("AQ_C3TAIL")
    engs = {}
    try:
        for v in ("0", "1"):
            os.environ["AQ_C3TAIL"] = v
            engs[v] = engine.Engine(synth_ck, precision)
    finally:
        if old is None:
            os.environ.pop("AQ_C3TAIL", None)
        else:
            os.environ["AQ_C3TAIL"] = old
    res = {}
    for v, eng in engs.items():
        i = _tail_pair(eng)
        eng.set_conv_config(i + 1, engine.CONV_CFG_DIRECT1X1)
        d, c = eng.infer(x, 0.25, 0.45, 300)
        torch.cuda.synchronize()
        res[v] = (d.clone(), c.clone(), eng.tensor_by_name("out2", 3).clone(), eng.tensor_by_name("out3", 3).clone(), eng.last_launches())
    (d0, c0, o20, o30, f0), (d1, c1, o21, o31, f1) = res["0"], res["1"]
    _assert_same(o21, o20, "model.2 output")
    _assert_same(o31, o30, "model.3 output")
    assert torch.equal(c0, c1)
    for j in range(3):
        assert torch.equal(d0[j, :c0[j]], d1[j, :c1[j]]), j
    assert f0 == f1                                     # the fused form reports the two launches' kernel families
    # stepping through the plan one op at a time (the two-launch form) == one infer call with the tail
    eng = engs["1"]
    n = len(eng.plan.ops)
    for k in range(n):
        ds, cs = eng.run_ops(x, k, k + 1, 0.25, 0.45, 300)
    torch.cuda.synchronize()
    _assert_same(eng.tensor_by_name("out2", 3), o20, "model.2 output, stepped")
    assert torch.equal(cs, c1)
    for j in range(3):
        assert torch.equal(ds[j, :cs[j]], d1[j, :c1[j]]), j
