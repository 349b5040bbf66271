"""The detection tail and the engines at 6 to 128 classes.  Every other GPU test builds its checkpoint, its head maps or its pred rows with
5, 4 or 1 classes, while the library takes any nc from 1 to 128 (a stock 80-class YOLOv5 checkpoint loads and runs).  From nc = 6 upwards
na * (nc + 5) > 32: the fused head refuses, every engine takes the unfused tail (head conv -> aq_detect_decode -> aq_nms_opts) with head
tensors of 64, 256 or 416 channels, rows of up to 133 floats, class offsets of up to 127 * 7680 and the high word of the class filter.

Where the code under test is reached (readable without a GPU):
  * `grep -n cls_hi aquaculture_amd/csrc/detect_nms.hip` names the branch of candidate_row that only a best class >= 64 takes;
    test_class_filter_words_and_agnostic's classes=[64] and classes=[63, 64, nc - 1] are the cases that need it to be right, and
    engine.class_mask's upper word (m >> 64) with them: with the two words of class_mask swapped those cases fail at the oracle
    comparison in test_gpu_nms._run (see the measurements below);
  * head_ld > 32 in decode_kernel: test_detect_decode_at_wide_heads (64, 256 and 416 channels, garbage behind na * no);
  * several M tiles of the fp32-out conv epilogue: test_head_conv_form_at_its_real_widths (cout 64 .. 416 on every tile configuration);
  * engine.cpp's AQ_OP_DECODE / AQ_OP_NMS with rows of 11, 85 and 133 floats: the engine tests.

Each test restates the check of a test at nc <= 5 (named in its docstring) with that test's own reference and tolerances; where a check
needs detections it first requires them of the oracle's output alone (at least 50 per tile, at nc >= 65 at least 20 of them of a class
>= 64), so that "nothing passed anywhere" cannot pass.  The synthetic head is calibrated per class count in a fixture
(tests/golden/make_synth_calib.py::calibrate, passed as calib=); aquaculture_amd/data/synth_head_calib.json is not touched.

Measured on MI355X (all 55 cases pass, 14 s together; the two command-line runs take 6 s, no other case 1 s):
  * oracle detections per tile (of those with a class >= 64; distinct classes over the tiles), conf 0.25, IoU 0.45 --
        nc 6,   128 px, tiles 0 / 3 / 19:   55 /  99 /  88  (-; 6)
        nc 80,  128 px:                    103 / 125 / 112  (34 / 54 / 47; 42)       augmented: 260 / 293 / 276 (78 / 113 / 96; 52)
        nc 128, 128 px:                     64 /  78 /  73  (31 / 37 / 35; 35)
        nc 80,  256 px, tiles 1 / 6 / 12:  233 / 205 / 200  (84 / 83 / 79; 47);  --classes 3 64 70 79: 19 / 4 / 4 (classes 64 and 79);
                                           --agnostic-nms: 215 / 188 / 166;  bf16-emulating oracle: 228 / 202 / 204 (83 / 77 / 88; 48)
  * NMS alone, survivors per image (class >= 64): n = 300: 300, 300 at nc 65 (8, 6), nc 80 (42, 65), nc 128 (150, 145) -- with this many
    classes hardly any two dense rows share one; n = 2049 and 6000: max_det = 1000 at every nc (nc 65: 19, 23; nc 80: about 205; nc 128:
    about 500); the 100,800-row tile at nc 80: 1000 (203).  The rows of test_class_filter_words_and_agnostic have 6 or 7 best classes
    only, so that boxes of one class do overlap: 163 to 181 survivors per image of 600 rows under classes=[63, 64, nc - 1].
  * engine.class_mask with its two words swapped (tried on a scratch edit, reverted): test_class_filter_words_and_agnostic fails at all
    three nc in test_gpu_nms._run's count comparison (179 against the oracle's 181 at nc 65, 90 / 166 at 80, 163 / 170 at 128), so do
    test_first_maximum_wins_across_the_words (0 / 8), test_max_det_and_the_five_class_layout (0 / 2),
    test_engine_classes_and_agnostic_at_80_classes (23 boxes against 19) and the --classes run of the command-line test (8 lines / 3).
  * decode against the oracle's, largest |d| (bound 1e-6 of the largest value): nc 6 1.2e-4 (1.3e-3), nc 11 6.1e-5 (1.1e-3), nc 80 1.5e-5
    (1.3e-3), nc 128 6.1e-5 (1.3e-3); confidences 1.2e-7 at every nc (bound 2.4e-7); 4 to 5 % of the values differ at all.  The bf16
    engine's forward_raw against the decode of its own head tensors: 1.2e-4 (bound 1.5e-3) at nc 6 and 80, confidences 1.2e-7.
  * head conv form, 21 configurations per case, largest |d| against rtol = atol = 1e-4: 7.2e-7 (cin 192, cout 64, 35 pixels) to 3.3e-6
    (cin 768, cout 416, 800 pixels); at worst 0.023 of the bound (cin 768, cout 256).  No configuration refuses cout = 416.
  * fp32 engine against the oracle's pred: max |d conf| 1.1e-5 / 2.1e-5 / 1.6e-5 at nc 6 / 80 / 128 (bound 1e-4), max |d box| 9.2e-3 /
    7.6e-3 / 4.5e-3 px (bound 6.4e-2); equal detection counts everywhere, the augmented call and both NMS options included.
  * bf16 engine at nc 80, 256 px, against the emulated-bf16 oracle: |d conf| mean 6.6e-3 (bound 1.04e-2), p99.9 4.2e-2 (7.3e-2), |d box|
    mean 0.49 px (1.02); counts 228 / 205 / 201 against 228 / 202 / 204 (bound +- 8).
  * command line: 444 of 444 label lines agree with the oracle writer's (102 / 122 / 114 / 106 per file, each with two-digit class
    ids), 23 of 23 under --classes 3 64 70 79.
No test exposed a wrong result.  The one change to the library: aq_engine_create refuses nc > 128 itself.
"""
import ctypes as C
import functools
import importlib.util
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from poison import poisoned
from test_gpu_augment import oracle_augmented_pred
from test_gpu_conv import _ref
from test_gpu_engine import _match
from test_gpu_nms import (_agnostic_and_class_filter, _assert_decode_bounds, _detect_decode_case, _large_tile, _max_det_truncation,
                          _oracle_decode, _pred, _random_dense, _random_pred, _run)

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MIN_DETS = 50            # per tile, as tests/test_gpu_nc4.py
MIN_HIGH = 20            # per tile with a class >= 64, at nc >= 65


@pytest.fixture(autouse=True)
def stop_at_a_gpu_fault():
    """As tests/test_gpu_poison_kernels.py: a failed test is a finding, a faulted device ends the session -- nothing more is launched on it."""
    yield
    try:
        torch.cuda.synchronize()
    except RuntimeError as err:
        pytest.exit(f"the GPU faulted, no further test is run: {err}", 3)


AG = [[(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)], [(30.0, 61.0), (62.0, 45.0), (59.0, 119.0)], [(116.0, 90.0), (156.0, 198.0), (373.0, 326.0)]]


# ---- 1. NMS alone ----------------------------------------------------------------------------------------------------------------------
def _survivors(nc, floor):
    """What a dense case requires of the oracle's result before the launch: more than `floor` rows per image, and one of a class >= 64."""
    def check(ref):
        assert all(r.shape[0] > floor for r in ref), [r.shape[0] for r in ref]
        high = [int((r[:, 5] >= 64).sum()) for r in ref]
        if nc >= 65:
            assert all(h >= 1 for h in high), high
        print(f"nms nc {nc}: {[r.shape[0] for r in ref]} survivors, {high} of a class >= 64")
    return check


@pytest.mark.parametrize("nc,n", [(nc, n) for nc in (6, 64, 65, 80, 128) for n in (300, 2049)] + [(80, 6000), (128, 6000)])
def test_random_dense_matches_oracle(lib, nc, n):
    """tests/test_gpu_nms.py::test_random_dense_matches_oracle: 300 rows take the bit-matrix path, 2049 the path past 2048 candidates, 6000
    the bitonic sort in global memory; rows of 11 to 133 floats."""
    _random_dense(nc, n, 1000 * nc + n, precheck=_survivors(nc, 10))


def test_large_tile_at_80_classes(lib):
    """tests/test_gpu_nms.py::test_large_tiles_take_the_4096_candidate_bit_matrix: 100,800 rows of 85 floats, 4097 candidates."""
    _large_tile(80, 4097, precheck=_survivors(80, 100))


@pytest.mark.parametrize("nc", [65, 80, 128])
def test_max_det_and_the_five_class_layout(lib, nc):
    """tests/test_gpu_nms.py::test_max_det_truncation and ::test_agnostic_and_class_filter on rows of nc + 5 floats (classes 0 .. 4 used)."""
    _max_det_truncation(nc)
    _agnostic_and_class_filter(nc)


def _rows_with_given_best_classes(nc, n=600, B=2, seed=0):
    """Dense overlapping rows whose best class is drawn from {0, 3, 62, 63, 64, nc - 1} (and 70 where it exists): the named class scores
    0.8 .. 1, every other class 0.3 .. 0.6."""
    rng = np.random.default_rng(seed + nc)
    p = _random_pred(rng, n, spread=400.0, B=B, nc=nc)
    p[..., 4] = rng.uniform(0.5, 1.0, (B, n))
    p[..., 5:] = rng.uniform(0.3, 0.6, (B, n, nc))
    pool = [0, 3, 62, 63, 64, nc - 1] + ([70] if nc > 71 else [])
    best = np.asarray(pool)[rng.integers(0, len(pool), (B, n))]
    np.put_along_axis(p[..., 5:], best[..., None], rng.uniform(0.8, 1.0, (B, n, 1)).astype(np.float32), 2)
    return p, pool


@pytest.mark.parametrize("nc", [65, 80, 128])
def test_class_filter_words_and_agnostic(lib, nc):
    """detect.py --classes / --agnostic-nms on both words of the class mask (tests/test_gpu_nms.py::test_agnostic_and_class_filter has five
    classes: the word above bit 63 is all ones or unused there).  classes=[64] and [63, 64, nc - 1] keep rows only if bit c - 64 of the
    upper word is read for a best class c >= 64; [0, 63] must drop every such row; classes no row has as its best leave nothing."""
    p, pool = _rows_with_given_best_classes(nc)
    best = p[..., 5:].argmax(2)
    for c in (63, 64, nc - 1):
        assert all(int((best[b] == c).sum()) >= 20 for b in range(p.shape[0])), c          # on the array, before any launch
    empties = [1] + ([66] if nc > 67 else [])
    assert not np.isin(best, empties).any()
    full = _run(p)
    for agnostic in (False, True):
        for classes in ([0, 63], [64], [63, 64, nc - 1], list(range(nc))):
            def check(ref, classes=classes):
                for r in ref:
                    assert r.shape[0] > 5 and set(r[:, 5]) == {float(c) for c in set(classes) & set(pool)}, (classes, sorted(set(r[:, 5])))
            r = _run(p, agnostic=agnostic, classes=classes, precheck=check)
            if len(classes) == nc and not agnostic:
                assert all(np.array_equal(a, b) for a, b in zip(r, full))
        for c in empties:
            assert all(r.shape[0] == 0 for r in _run(p, agnostic=agnostic, classes=[c]))


@pytest.mark.parametrize("pair", [(3, 70), (64, 65)])
def test_first_maximum_wins_across_the_words(lib, pair):
    """tests/test_gpu_nms.py::test_confidence_ties_are_ordered_by_index at 80 classes: the best score is shared by two classes, the lower
    index is reported -- across the two words of the class mask, and inside the upper one."""
    lo, hi = pair
    boxes = [[100 + 50 * i, 100, 20, 20] for i in range(8)]
    p = _pred(boxes, 0.9, {0: 0.1, lo: 0.8, hi: 0.8, 79: 0.2, 40: 0.1}, 80)
    r = _run(p)[0]
    assert r.shape[0] == 8 and np.all(r[:, 5] == lo) and np.all(np.diff(r[:, 0]) > 0)
    assert _run(p, classes=[hi])[0].shape[0] == 0 and _run(p, classes=[lo])[0].shape[0] == 8


@pytest.mark.parametrize("pair", [(0, 127), (126, 127), (127, 126)])
def test_cross_class_overlap_at_high_class_ids(lib, pair):
    """tests/test_gpu_nms.py::test_cross_class_overlap_is_not_suppressed near x = y = 1270 with classes up to 127: the class offset
    (cls * 7680) puts the coordinates at 9.7e5, where an fp32 ulp is 1/16 px; bit for bit with the oracle, which adds it the same way."""
    a, b = pair
    boxes = [[1270, 1270, 50, 50], [1270, 1270, 50, 50], [1271, 1270, 50, 50]]
    p = _pred(boxes, 0.9, {a: [0.9, 0, 0.8], b: [0, 0.9, 0]}, 128)
    r = _run(p)[0]
    assert r.shape[0] == 2 and set(r[:, 5]) == {float(a), float(b)}
    r = _run(p, agnostic=True)[0]
    assert r.shape[0] == 1


def test_nms_refuses_129_classes_and_writes_nothing(lib):
    """The pattern of tests/test_gpu_head_decode.py::test_unsupported_heads_are_refused_and_nothing_is_written."""
    from aquaculture_amd import engine
    nc, B, n = 129, 2, 64
    pred = torch.from_numpy(_random_pred(np.random.default_rng(129), n, B=B, nc=nc)).cuda()
    scratch = torch.zeros(lib.aq_nms_scratch_bytes(B, n), dtype=torch.uint8, device="cuda")
    dets = torch.full((B, 100, 6), -3.0, dtype=torch.float32, device="cuda")
    counts = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    ones = (1 << 64) - 1
    rc = lib.aq_nms_opts(pred.data_ptr(), n, B, n, nc, 0.25, 0.45, 100, None, None, 0, scratch.data_ptr(), dets.data_ptr(), counts.data_ptr(), 0,
                         ones, ones, engine._stream_ptr())
    assert rc != 0 and b"nms: the class filter covers 128 classes (nc = 129)" in lib.aq_last_error()
    with pytest.raises(RuntimeError, match="128 classes"):
        engine.nms(pred, nc)
    torch.cuda.synchronize()
    assert (dets == -3.0).all() and (counts == -3).all()


# ---- 2. the unfused decode at wide heads -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("nc,head_ld,small_cap", [(6, 64, False), (11, 64, False), (80, 256, False), (128, 416, False), (80, 256, True)])
def test_detect_decode_at_wide_heads(lib, nc, head_ld, small_cap):
    """tests/test_gpu_nms.py::test_detect_decode_at_four_and_one_classes, its procedure and bounds, on head maps of the widths
    spec.build_plan gives 6, 11, 80 and 128 classes; every channel past na * no holds garbage (at 80 classes that is one channel)."""
    from aquaculture_amd import spec
    assert spec.make_divisible(3 * (nc + 5), 32) == head_ld
    _detect_decode_case(lib, nc, small_cap, head_ld)


def test_detect_decode_aug_at_80_classes(lib):
    """tests/test_gpu_augment.py::test_detect_decode_aug_matches_descaled_oracle, its criterion, on random head maps of 256 channels (255
    true ones) at the pass geometries of a 64 x 96 tile: pass 1 (0.83, flipped) and pass 2 (0.67, P3 dropped)."""
    from aquaculture_amd import augment, checkpoint, engine
    from oracle import yolov5_oracle as O
    ck = checkpoint.synthetic_checkpoint("yolov5m", 5)
    nc, na, H, W, B = 80, 3, 64, 96, 2
    no = nc + 5
    passes, n = augment.geometry(H, W)
    for pi in (1, 2):
        ps = passes[pi]
        g = torch.Generator().manual_seed(80 + pi)
        heads = [torch.randn(B, ps.hp // s, ps.wp // s, 256, generator=g) * 1.5 for s in (8, 16, 32)]
        assert all((h[..., na * no:] != 0).all() for h in heads)
        y = _oracle_decode(O.OracleModel({}, nc, ck.anchors, ck.stride, ck.bn_eps), [h[..., :na * no] for h in heads])
        assert y.shape[1] == ps.rows
        y[..., :4] /= augment.SCALES[pi]
        if ps.flip:
            y[..., 0] = W - y[..., 0]
        pred = engine.detect_decode_aug([h.cuda() for h in heads], ps.hp, ps.wp, nc, ck.anchor_grid_px().numpy().tolist(), ck.stride, ps.level_mask,
                                        ps.out_first - ps.keep_first, n, ps.scale, float(W) if ps.flip else 0.0).cpu()
        got = pred[:, ps.out_first:ps.out_first + ps.keep_count]
        want = y[:, ps.keep_first:ps.keep_first + ps.keep_count]
        assert ps.keep_count > 0 and got.shape == want.shape
        assert (got - want).abs().max().item() <= 1e-6 * max(1.0, want.abs().max().item())
        outside = torch.ones(n, dtype=torch.bool)
        outside[ps.out_first:ps.out_first + ps.keep_count] = False
        assert (pred[:, outside] == 0).all()


# ---- 3. the head conv form at its real widths ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 5, 7), (2, 20, 20)])
@pytest.mark.parametrize("cin,cout,true_cout", [(192, 64, 33), (384, 64, 48), (192, 256, 255), (384, 256, 255), (768, 256, 255), (768, 416, 399)])
def test_head_conv_form_at_its_real_widths(lib, cin, cout, true_cout, shape):
    """tests/test_gpu_conv.py::test_conv_f32_out_head (bf16 in, fp32 out, no activation; `_ref` on bf16-rounded operands, rtol = atol =
    1e-4) at the head widths of 6, 11, 80 and 128 classes and the three yolov5m head inputs, on every tile configuration that takes a 1x1
    layer (as test_conv_matches_reference loops them): up to 13 M tiles of 32 rows, 2 of 256.  The padding channels are the zero bias."""
    from aquaculture_amd import engine
    B, H, W = shape
    g = torch.Generator().manual_seed(cin + cout + true_cout)
    x = torch.randn(B, H, W, cin, generator=g).bfloat16()
    w = torch.zeros(cout, cin, 1, 1)
    w[:true_cout] = torch.randn(true_cout, cin, 1, 1, generator=g) * cin ** -0.5
    b = torch.zeros(cout)
    b[:true_cout] = torch.randn(true_cout, generator=g)
    ref = _ref(x, w, b, 1, 0, False, None, True)
    xd = x.cuda()
    ran, worst, worst_abs = 0, 0.0, 0.0
    for cfg in range(lib.aq_conv_num_configs()):
        try:
            out = engine.conv2d_nhwc(xd, w, b, act=False, precision="bf16", out_f32=True, cfg=cfg).cpu()
        except RuntimeError as err:          # tile shape not applicable to this layer (the halo kernel on a 1x1 conv)
            assert "halo conv" in str(err), err
            continue
        ran += 1
        assert out.dtype == torch.float32 and out.shape == ref.shape
        worst = max(worst, ((out - ref).abs() / (1e-4 + 1e-4 * ref.abs())).max().item())
        worst_abs = max(worst_abs, (out - ref).abs().max().item())
        torch.testing.assert_close(out, ref, rtol=1e-4, atol=1e-4)
        assert (out[..., true_cout:] == 0).all(), cfg
    print(f"head conv cin {cin} cout {cout} ({true_cout}) {shape}: {ran} configurations, max |d| {worst_abs:.2e}, worst error {worst:.3f} of the "
          f"bound (1e-4 + 1e-4 |ref|)")
    assert ran >= 10


# ---- 4. engines ------------------------------------------------------------------------------------------------------------------------
def _enough(dets, nc, label):
    """The conditions every engine test puts on the oracle's detections before it looks at the engine's."""
    n = [d.shape[0] for d in dets]
    high = [int((d[:, 5] >= 64).sum()) for d in dets]
    distinct = len({int(c) for d in dets for c in d[:, 5]})
    print(f"oracle {label}: {n} detections, {high} of a class >= 64, {distinct} distinct classes")
    assert all(v >= MIN_DETS for v in n), n
    assert all((d[:, 5] < nc).all() for d in dets) and distinct > 1
    if nc >= 65:
        assert all(h >= MIN_HIGH for h in high), high


class _Zoo:
    """Checkpoints, tiles and oracle results of this module, each computed once and read-only."""

    def __init__(self):
        spec = importlib.util.spec_from_file_location("make_synth_calib", os.path.join(ROOT, "tests", "golden", "make_synth_calib.py"))
        self.calib = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(self.calib)
        self.checkpoint = functools.lru_cache(maxsize=None)(self._checkpoint)
        self.tiles = functools.lru_cache(maxsize=None)(self._tiles)
        self.oracle = functools.lru_cache(maxsize=None)(self._oracle)

    def _checkpoint(self, nc):
        """(the seeded synthetic yolov5m checkpoint with nc classes, the calibration table computed for it): the committed table has 4 and 5."""
        from aquaculture_amd import checkpoint
        table = self.calib.calibrate("yolov5m", nc, 640, 8)
        return checkpoint.synthetic_checkpoint("yolov5m", nc, calib=table), table

    def _tiles(self, size):
        from aquaculture_amd import tiles
        return tiles.synthetic_batch([0, 3, 19] if size == 128 else [1, 6, 12], size)

    def _oracle(self, nc, size):
        """(pred, detections) of the fp32 oracle on the 128-px tiles 0 / 3 / 19 or the 256-px tiles 1 / 6 / 12."""
        from oracle import yolov5_oracle as O
        pred = O.model_from_checkpoint(self.checkpoint(nc)[0]).forward(O.preprocess(self.tiles(size)))
        dets = O.non_max_suppression(pred.numpy())
        _enough(dets, nc, f"nc {nc} at {size} px")
        return pred, dets


@pytest.fixture(scope="module")
def zoo():
    """The calibrated checkpoints (1 s each) and oracle results of the engine tests, shared among them and released with the module."""
    return _Zoo()


@pytest.mark.parametrize("nc", [6, 80, 128])
def test_fp32_engine_matches_oracle(lib, zoo, nc):
    """tests/test_gpu_engine.py::test_infer_fp32_matches_oracle_detections (equal counts, boxes and confidences within 1e-4) and
    ::test_forward_raw_fp32_640's tolerance on the prediction, on the 128-px tiles."""
    from aquaculture_amd import engine
    ref_pred, ref = zoo.oracle(nc, 128)
    eng = engine.Engine(zoo.checkpoint(nc)[0], "fp32")
    t = torch.from_numpy(zoo.tiles(128)).cuda()
    dets, counts = eng.infer(t)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    assert "head_decode" not in [f for f, _ in eng.last_launches()]
    _match(dets, counts, ref, box_tol=640 * 1e-4, conf_tol=1e-4)
    for b in range(3):
        cls = dets[b, :counts[b], 5]
        assert ((cls >= 0) & (cls < nc) & (cls == np.round(cls))).all()
    pred = eng.forward_raw(t).cpu()
    assert pred.shape == ref_pred.shape == (3, 1008, nc + 5)
    d_conf, d_box = (pred[..., 4:] - ref_pred[..., 4:]).abs().max().item(), (pred[..., :4] - ref_pred[..., :4]).abs().max().item()
    print(f"fp32 nc {nc}: max |d conf| {d_conf:.2e} (bound 1e-4), max |d box| {d_box:.2e} px (bound 6.4e-2)")
    assert d_conf <= 1e-4 and d_box <= 640 * 1e-4
    eng.close()


def test_the_fused_head_ends_at_five_classes(lib, zoo, synth_ck):
    """na * (nc + 5) <= 32 pinned from both sides: the bf16 engine runs the fused head at 5 classes and conv + decode at 6."""
    from aquaculture_amd import engine
    t = torch.from_numpy(zoo.tiles(128)).cuda()
    for ck, fused in ((synth_ck, True), (zoo.checkpoint(6)[0], False)):
        assert lib.aq_head_decode_supported(192, 3, ck.nc) == int(fused)
        eng = engine.Engine(ck, "bf16")
        eng.infer(t)
        torch.cuda.synchronize()
        assert ("head_decode" in [f for f, _ in eng.last_launches()]) == fused, ck.nc
        eng.close()


@pytest.mark.parametrize("nc", [6, 80])
def test_bf16_engine_tail(lib, zoo, nc):
    """The tail of the bf16 engine apart from its backbone's bf16 noise: `infer` equals aq_nms_opts on `forward_raw` bit for bit
    (tests/test_gpu_nms.py::test_engine_decode_plus_nms_equals_nms_on_raw_pred: the compact-candidate path against the full pred), and
    `forward_raw` is the oracle's Detect decode of the engine's OWN fp32 head tensors (64 and 256 channels, read through tensor_ptr) under
    the bounds of test_detect_decode_at_four_and_one_classes."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    ck = zoo.checkpoint(nc)[0]
    zoo.oracle(nc, 128)                                                           # (its conditions on the detections)
    eng = engine.Engine(ck, "bf16")
    t = torch.from_numpy(zoo.tiles(128)).cuda()
    d0, c0 = eng.infer(t)
    assert "head_decode" not in [f for f, _ in eng.last_launches()]
    raw = eng.forward_raw(t)
    d1, c1 = engine.nms(raw, nc)
    assert torch.equal(c0, c1) and int(c0.min()) >= MIN_DETS // 2
    for b in range(3):
        assert torch.equal(d0[b, :c0[b]], d1[b, :c1[b]])
    if nc >= 65:
        assert all(int((d0[b, :c0[b], 5] >= 64).sum()) >= MIN_HIGH // 2 for b in range(3))
    torch.cuda.synchronize()
    heads = [eng.tensor_by_name(f"head{lvl}", 3).float().cpu() for lvl in range(3)]
    width = 64 if nc == 6 else 256
    assert all(h.shape[3] == width and h.dtype == torch.float32 for h in heads)
    want = _oracle_decode(O.OracleModel({}, nc, ck.anchors, ck.stride, ck.bn_eps), [h[..., :3 * (nc + 5)] for h in heads])
    _assert_decode_bounds(raw.cpu(), want, f"bf16 engine nc {nc}: forward_raw against the decode of its own heads")
    eng.close()


def test_bf16_engine_close_to_emulated_oracle_at_80_classes(lib, zoo):
    """tests/test_gpu_nc4.py::test_infer_bf16_close_to_emulated_oracle, its check and bounds (the nc = 5 test's own), on the 256-px tiles:
    the per-logit error does not depend on how many logits there are."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    nc = 80
    ck = zoo.checkpoint(nc)[0]
    eng = engine.Engine(ck, "bf16")
    ref = O.model_from_checkpoint(ck, O.q_bf16).forward(O.preprocess(zoo.tiles(256)))
    t = torch.from_numpy(zoo.tiles(256)).cuda()
    pred = eng.forward_raw(t).cpu()
    assert pred.shape == ref.shape == (3, 4032, nc + 5)
    d_conf = (pred[..., 4:] - ref[..., 4:]).abs().flatten()
    print(f"nc {nc} bf16: |d conf| mean {d_conf.mean().item():.3e}, p99.9 {d_conf.kthvalue(int(0.999 * d_conf.numel()))[0].item():.3e}, "
          f"|d box| mean {(pred[..., :4] - ref[..., :4]).abs().mean().item():.3f} px")
    assert d_conf.mean().item() <= 1.04e-2
    assert d_conf.kthvalue(int(0.999 * d_conf.numel()))[0].item() <= 7.3e-2
    assert (pred[..., :4] - ref[..., :4]).abs().mean().item() <= 1.02
    ref_dets = O.non_max_suppression(ref.numpy())
    _enough(ref_dets, nc, f"(bf16-emulating) nc {nc} at 256 px")
    _, counts = eng.infer(t)
    print(f"nc {nc} bf16: counts {counts.cpu().tolist()} against {[r.shape[0] for r in ref_dets]}")
    for got, want in zip(counts.cpu().tolist(), [r.shape[0] for r in ref_dets]):
        assert abs(got - want) <= 8
    eng.close()


def test_engine_classes_and_agnostic_at_80_classes(lib, zoo):
    """tests/test_gpu_augment.py::test_infer_augment_classes_and_agnostic's comparison on plain calls: detect.py --classes 3 64 70 79 and
    --agnostic-nms through Engine.set_nms_options on the 256-px tiles, against the oracle's NMS with the same options."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    nc, keep = 80, [3, 64, 70, 79]
    ref_pred, plain = zoo.oracle(nc, 256)
    eng = engine.Engine(zoo.checkpoint(nc)[0], "fp32")
    t = torch.from_numpy(zoo.tiles(256)).cuda()
    for classes, agnostic in ((keep, False), (None, True), (keep, True)):
        ref = O.non_max_suppression(ref_pred.numpy(), agnostic=agnostic, classes=classes)
        print(f"oracle nc {nc} at 256 px, classes {classes}, agnostic {agnostic}: {[r.shape[0] for r in ref]} detections")
        if classes is not None:
            assert all(r.shape[0] >= 1 and set(r[:, 5]) <= {float(c) for c in keep} for r in ref)
            assert all((r[:, 5] >= 64).any() for r in ref) and sum(r.shape[0] for r in ref) < 0.1 * sum(p.shape[0] for p in plain)
        else:
            assert all(MIN_DETS <= r.shape[0] < p.shape[0] for r, p in zip(ref, plain))        # agnostic suppresses more
        eng.set_nms_options(agnostic=agnostic, classes=classes)
        dets, counts = eng.infer(t)
        _match(dets.cpu().numpy(), counts.cpu().numpy(), ref, box_tol=640 * 1e-4, conf_tol=1e-4)
    eng.set_nms_options()
    dets, counts = eng.infer(t)
    _match(dets.cpu().numpy(), counts.cpu().numpy(), plain, box_tol=640 * 1e-4, conf_tol=1e-4)
    eng.close()


def test_infer_augment_at_80_classes(lib, zoo):
    """tests/test_gpu_augment.py::test_infer_augment_matches_oracle_nms on the 128-px tiles: aq_detect_decode_aug appends three passes of
    85-float rows to one list."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    nc = 80
    ck = zoo.checkpoint(nc)[0]
    ref = O.non_max_suppression(oracle_augmented_pred(O.model_from_checkpoint(ck), zoo.tiles(128)).numpy())
    _enough(ref, nc, f"nc {nc} at 128 px, augmented")
    assert sum(r.shape[0] for r in ref) > 100
    eng = engine.Engine(ck, "fp32")
    dets, counts = eng.infer(torch.from_numpy(zoo.tiles(128)).cuda(), augment=True)
    _match(dets.cpu().numpy(), counts.cpu().numpy(), ref, box_tol=640 * 1e-4, conf_tol=1e-4)
    eng.close()


def test_engine_create_refuses_129_classes(lib):
    """aq_engine_create names nc and the limit of 128 (the class filter's two words) and returns no engine -- before this check an
    nc = 129 engine was built, ran the whole network and was refused by the NMS launcher."""
    from aquaculture_amd import checkpoint, engine
    tens = (engine.aq_tensor_desc * 1)()
    ops = (engine.aq_op_desc * 1)()
    for nc, refused in ((129, True), (1 << 20, True)):
        desc = engine.aq_model_desc()
        desc.precision, desc.nc, desc.na, desc.nl = engine.ENGINE_PRECISIONS["fp32"], nc, 3, 3
        desc.n_tensors, desc.n_ops, desc.tensors, desc.ops = 1, 1, tens, ops
        h = C.c_void_p()
        rc = lib.aq_engine_create(C.byref(desc), 0, C.byref(h))
        msg = lib.aq_last_error().decode()
        assert rc != 0 and h.value is None
        assert f"nc = {nc}" in msg and "128" in msg, msg
    with pytest.raises(RuntimeError, match=r"engine_create: nc = 129.* 128 classes"):
        engine.Engine(checkpoint.synthetic_checkpoint("yolov5m", 129, calib=None), "fp32")


# ---- 5. poison and the command line ----------------------------------------------------------------------------------------------------
def test_decode_and_nms_at_80_classes_own_their_results(lib, monkeypatch):
    """In the style of tests/test_gpu_poison_kernels.py::test_nms and ::test_detect_decode_aug: aq_detect_decode on head maps of 256
    channels between two filler images, then aq_nms_opts on its compact list and on its full pred, with pred, list, rows, counters,
    scratch, detections and counts all from the poisoned allocator (0xFF: NaN / -1); guards intact, and every owned result equal to the
    unpoisoned run's bytes."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    from test_gpu_poison_kernels import bits, filled
    nc, na, B, H, W, ld, conf, max_det = 80, 3, 2, 64, 96, 256, 0.25, 300
    no = nc + 5
    g = torch.Generator().manual_seed(85)
    heads = [torch.randn(B, H // s, W // s, ld, generator=g) * 1.5 for s in (8, 16, 32)]
    N = sum(na * h.shape[1] * h.shape[2] for h in heads)
    anch = (C.c_float * (3 * na * 2))(*[float(v) for lvl in AG for a in lvl for v in a])
    st = (C.c_float * 3)(8.0, 16.0, 32.0)
    ones = (1 << 64) - 1

    def run(byte):
        batch = [filled((B + 2,) + tuple(h.shape[1:]), torch.float32, byte) for h in heads]
        for t, h in zip(batch, heads):
            t[1:1 + B] = h.cuda()
        pred = torch.empty((B, N, no), dtype=torch.float32, device="cuda")
        cand = torch.empty((B, N), dtype=torch.int32, device="cuda")
        rows = torch.empty((B, N, no), dtype=torch.float32, device="cuda")
        ncand = torch.empty((B,), dtype=torch.int32, device="cuda")
        hp = (C.c_void_p * 3)(*[t[1:1 + B].data_ptr() for t in batch])
        engine._check(lib.aq_detect_decode(hp, ld, B, H, W, nc, na, anch, st, pred.data_ptr(), conf, cand.data_ptr(), rows.data_ptr(), ncand.data_ptr(),
                                           N, engine._stream_ptr()))
        scratch = torch.empty(lib.aq_nms_scratch_bytes(B, N), dtype=torch.uint8, device="cuda")
        dets = torch.empty((B, max_det, 6), dtype=torch.float32, device="cuda")
        counts = torch.empty((B,), dtype=torch.int32, device="cuda")
        engine._check(lib.aq_nms_opts(rows.data_ptr(), N, B, N, nc, conf, 0.45, max_det, cand.data_ptr(), ncand.data_ptr(), N, scratch.data_ptr(),
                                      dets.data_ptr(), counts.data_ptr(), 0, ones, ones, engine._stream_ptr()))
        dets2, counts2 = engine.nms(pred, nc, conf, 0.45, max_det)
        torch.cuda.synchronize()
        for t in batch:                                                        # the filler images still hold their fill
            raw = t.view(torch.uint8).view(B + 2, -1)
            assert (raw[0] == byte).all() and (raw[-1] == byte).all()
        out = {"pred": pred.cpu(), "ncand": ncand.cpu(), "counts": counts.cpu(), "counts2": counts2.cpu()}
        for b in range(B):
            k = int(ncand[b])
            order = torch.argsort(cand[b, :k])
            out[f"cand{b}"], out[f"rows{b}"] = cand[b, :k][order].cpu(), rows[b, :k][order].cpu()
            out[f"dets{b}"], out[f"dets2_{b}"] = dets[b, :int(counts[b])].cpu(), dets2[b, :int(counts2[b])].cpu()
        return out

    plain = run(0x00)
    with poisoned(monkeypatch, 0xFF) as p:
        got = run(0xFF)
        p.check_guards()
        assert p.intercepted >= 10 and not p.passed_through, p.passed_through
    assert list(plain) == list(got)
    for k, a in plain.items():
        assert a.shape == got[k].shape and bool((bits(a) == bits(got[k])).all()), k
        assert bool(torch.isfinite(got[k].float()).all()), k
    ref = O.non_max_suppression(plain["pred"].numpy(), conf, 0.45, max_det)        # ... and they are the right bytes
    for b, r in enumerate(ref):
        assert r.shape[0] > 10 and (r[:, 5] >= 64).sum() >= 1
        assert np.array_equal(plain[f"dets{b}"].numpy(), r) and np.array_equal(plain[f"dets2_{b}"].numpy(), r)
        assert torch.equal(plain[f"rows{b}"], plain["pred"][b, plain[f"cand{b}"].long()])
        assert plain[f"cand{b}"].tolist() == torch.nonzero(plain["pred"][b, :, 4] > conf).flatten().tolist()


def _agreeing_lines(path, lines):
    """(label lines of the file at `path`, how many of the oracle writer's `lines` have a partner among them): `cls xc yc w h` identical
    as text, the confidence (printed to 6 digits) within 1e-4 -- tests/test_gpu_nc4.py::test_cli_writes_four_class_labels' comparison."""
    got = open(path).read().splitlines() if os.path.exists(path) else []
    pool = {}
    for l in got:
        f = l.split()
        pool.setdefault(" ".join(f[:5]), []).append(float(f[5]))
    same = 0
    for l in lines:
        f = l.split()
        cands = pool.get(" ".join(f[:5]), [])
        hit = [c for c in cands if abs(c - float(f[5])) <= 1e-4]
        if hit:
            cands.remove(hit[0])
            same += 1
    return got, same


def test_cli_writes_two_digit_class_ids(lib, zoo, tmp_path):
    """tests/test_gpu_nc4.py::test_cli_writes_four_class_labels with an 80-class checkpoint file on four 128-px JPEGs, in child processes:
    yolov5/detect.py --save-txt --save-conf, and once more with --classes 3 64 70 79; per tile the oracle writer's lines."""
    from aquaculture_amd import checkpoint, dataloader, tiles
    from oracle import yolov5_oracle as O
    nc, keep, idx = 80, [3, 64, 70, 79], [0, 3, 19, 6]
    tiles.write_synthetic_jpegs(str(tmp_path / "jpegs"), idx, size=128)
    w = tmp_path / "synth_nc80.pt"
    checkpoint.write_synthetic_checkpoint(str(w), "yolov5m", nc, calib=zoo.checkpoint(nc)[1])
    loaded = checkpoint.load_checkpoint(str(w))
    assert loaded.nc == nc and len(loaded.names) == nc
    model = O.model_from_checkpoint(loaded)
    want, want_kept = {}, {}
    for i in idx:
        stem = tiles.tile_name(i)[:-5]
        im = dataloader.read_rgb(str(tmp_path / "jpegs" / (stem + ".jpeg")))
        assert im.shape == (128, 128, 3)
        pred = model.forward(O.preprocess(im[None])).numpy()
        det = O.non_max_suppression(pred)[0]
        _enough([det], nc, f"nc {nc}, {stem}.jpeg")
        want[stem] = O.label_lines(det, (128, 128), (128, 128))
        assert any(len(l.split()[0]) == 2 for l in want[stem])                 # a two-digit class id in every file
        want_kept[stem] = O.label_lines(O.non_max_suppression(pred, classes=keep)[0], (128, 128), (128, 128))
    assert sum(len(v) for v in want_kept.values()) >= 4 and any(int(l.split()[0]) >= 64 for v in want_kept.values() for l in v)
    base = [sys.executable, os.path.join(ROOT, "yolov5", "detect.py"), "--weights", str(w), "--source", str(tmp_path / "jpegs"), "--imgsz", "128",
            "--nosave", "--save-txt", "--save-conf", "--project", str(tmp_path / "runs"), "--batch-size", "4"]
    for name, extra, lines_of in (("nc80", [], want), ("nc80_kept", ["--classes"] + [str(c) for c in keep], want_kept)):
        r = subprocess.run(base + ["--name", name] + extra, capture_output=True, text=True, timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        labels = tmp_path / "runs" / name / "labels"
        written = sorted(os.listdir(labels)) if labels.exists() else []
        assert written == sorted(s + ".txt" for s, v in lines_of.items() if v)
        same = total = 0
        for stem, lines in lines_of.items():
            got, n = _agreeing_lines(labels / (stem + ".txt"), lines)
            assert len(got) == len(lines), (name, stem, len(got), len(lines))
            arr = np.array([[float(v) for v in l.split()] for l in got]).reshape(-1, 6)
            assert set(arr[:, 0]) <= ({float(c) for c in keep} if extra else {float(c) for c in range(nc)})
            assert np.all(np.diff(arr[:, 5]) >= -1e-6) and (not len(arr) or (arr[:, 1:5].min() >= 0 and arr[:, 1:5].max() <= 1))
            same += n
            total += len(lines)
        print(f"nc 80 labels ({name}): {same}/{total} lines agree with the oracle writer's")
        assert total >= (4 if extra else 4 * MIN_DETS) and same >= 0.995 * total
