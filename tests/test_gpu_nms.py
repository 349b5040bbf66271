"""S2 alone: the HIP NMS (aq_nms through the C ABI) must reproduce the oracle's non_max_suppression BIT FOR BIT
on hand-built pred tensors that hit the edge cases: empty input, confidence ties, the strict '>'
IoU boundary, cross-class overlap (class-offset trick), n > max_det, the > 2048-candidate path, the 30,000 cap.
The checkpoints of the product have 4 or 5 classes (nc is read from the checkpoint): the dense, max_det, agnostic / class-filter
and 4096-candidate cases run at nc = 5, 4 and 1 (rows of 10, 9 and 6 floats), the decode that feeds the NMS (aq_detect_decode) at 4 and 1."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
NC = 5


def _pred(boxes_xywh, obj, cls_conf, nc=NC):
    """cls_conf: rows written for five classes, cut to the first nc -- or, for more classes than columns, a dict {class: scores of the
    rows} (the other classes score 0), or rows of fewer than nc columns (the classes past them score 0)."""
    n = len(boxes_xywh)
    p = np.zeros((1, n, 5 + nc), np.float32)
    p[0, :, :4] = boxes_xywh
    p[0, :, 4] = obj
    if isinstance(cls_conf, dict):
        for c, v in cls_conf.items():
            assert 0 <= c < nc
            p[0, :, 5 + c] = v
        return p
    rows = np.asarray(cls_conf, np.float32)[:, :nc]
    p[0, :, 5:5 + rows.shape[1]] = rows
    return p


def _run(pred, conf=0.25, iou=0.45, max_det=1000, agnostic=False, classes=None, precheck=None):
    """precheck(ref): what the caller requires of the oracle's result alone, asserted before anything is launched."""
    from aquaculture_amd import engine
    from oracle import yolov5_oracle as O
    ref = O.non_max_suppression(pred, conf, iou, max_det, agnostic=agnostic, classes=classes)
    if precheck is not None:
        precheck(ref)
    dets, counts = engine.nms(torch.from_numpy(pred).cuda().contiguous(), pred.shape[2] - 5, conf, iou, max_det, agnostic=agnostic, classes=classes)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    for b, r in enumerate(ref):
        assert counts[b] == r.shape[0], (counts[b], r.shape[0])
        assert np.array_equal(dets[b, :counts[b]], r)
    return ref


def _random_pred(rng, n, spread=600.0, B=1, nc=NC):
    p = np.zeros((B, n, 5 + nc), np.float32)
    p[..., 0:2] = rng.uniform(20, spread, (B, n, 2))
    p[..., 2:4] = rng.uniform(4, 80, (B, n, 2))
    p[..., 4] = rng.uniform(0, 1, (B, n))
    p[..., 5:] = rng.uniform(0, 1, (B, n, nc))
    return p.astype(np.float32)


def test_empty_and_below_threshold(lib):
    rng = np.random.default_rng(0)
    p = _random_pred(rng, 500)
    p[..., 4] = 0.2                      # nothing passes obj > 0.25
    assert _run(p)[0].shape[0] == 0
    p[..., 4] = 0.3
    p[..., 5:] = 0.5                     # obj*cls = 0.15: passes the first threshold, fails the second
    assert _run(p)[0].shape[0] == 0


def test_confidence_ties_are_ordered_by_index(lib):
    boxes = [[100 + 50 * i, 100, 20, 20] for i in range(8)]
    p = _pred(boxes, 0.9, np.tile([[0.1, 0.8, 0.8, 0.2, 0.1]], (8, 1)))   # every row: conf 0.72, first max class = 1
    r = _run(p)[0]
    assert r.shape[0] == 8 and np.all(r[:, 5] == 1) and np.all(np.diff(r[:, 0]) > 0)


def test_strict_iou_boundary(lib):
    # IoU of the second box with the first is exactly 0.5: kept at thr 0.5 (strict '>'), suppressed at 0.45
    boxes = [[100, 100, 40, 40], [100, 110, 40, 20]]
    p = _pred(boxes, [0.9, 0.8], np.tile([[0.9, 0, 0, 0, 0]], (2, 1)))
    assert _run(p, iou=0.5)[0].shape[0] == 2
    assert _run(p, iou=0.45)[0].shape[0] == 1


def test_cross_class_overlap_is_not_suppressed(lib):
    boxes = [[200, 200, 50, 50], [200, 200, 50, 50], [201, 200, 50, 50]]
    cls = np.array([[0.9, 0, 0, 0, 0], [0, 0.9, 0, 0, 0], [0.8, 0, 0, 0, 0]], np.float32)
    r = _run(_pred(boxes, 0.9, cls))[0]
    assert r.shape[0] == 2 and set(r[:, 5]) == {0.0, 1.0}


def _agnostic_and_class_filter(nc):
    boxes = [[200, 200, 50, 50], [200, 200, 50, 50], [201, 200, 50, 50], [400, 400, 30, 30]]
    cls = np.array([[0.9, 0, 0, 0, 0], [0, 0.95, 0, 0, 0], [0.8, 0, 0, 0, 0], [0, 0, 0, 0.7, 0]], np.float32)
    if nc == 1:                                                       # one class: every row's class 0, as the only column has it
        cls[:, 0] = [0.9, 0.95, 0.8, 0.7]
    p = _pred(boxes, 0.9, cls, nc)
    r = _run(p, agnostic=True)[0]
    if nc >= 4:
        assert r.shape[0] == 2 and list(r[:, 5]) == [1.0, 3.0]        # the class-1 box wins the spot, the far class-3 box stays
        r = _run(p, classes=[0, 3])[0]
        assert r.shape[0] == 2 and set(r[:, 5]) == {0.0, 3.0}
        assert _run(p, classes=[nc - 1 if nc > 4 else 2])[0].shape[0] == 0
        r = _run(p, agnostic=True, classes=[0, 3])[0]
        assert r.shape[0] == 2 and set(r[:, 5]) == {0.0, 3.0}
    else:
        assert r.shape[0] == 2 and list(r[:, 5]) == [0.0, 0.0]
        assert _run(p, classes=[0])[0].shape[0] == 2
    rng = np.random.default_rng(11)
    keep = [1, 2] if nc > 2 else [0]
    for n in (700, 3000):                                             # both the bit-matrix path and the greedy fallback
        q = _random_pred(rng, n, B=2, nc=nc)
        q[..., 4] = rng.uniform(0.5, 1.0, q.shape[:2])
        q[..., 5:] = rng.uniform(0.6, 1.0, q.shape[:2] + (nc,))
        assert all(x.shape[0] > 5 for x in _run(q, agnostic=True))
        assert all(x.shape[0] > 5 and set(x[:, 5]) <= {float(k) for k in keep} for x in _run(q, classes=keep))


def test_agnostic_and_class_filter(lib):
    """detect.py --agnostic-nms / --classes [UPSTREAM non_max_suppression(classes, agnostic)]: with agnostic the class-0 and class-1 boxes on
    the same spot suppress each other; a class filter removes the other classes' candidates before the suppression."""
    _agnostic_and_class_filter(NC)


@pytest.mark.parametrize("nc", [4, 1])
def test_agnostic_and_class_filter_other_class_counts(lib, nc):
    _agnostic_and_class_filter(nc)


def test_max_det_truncation(lib):
    _max_det_truncation(NC)


@pytest.mark.parametrize("nc", [4, 1])
def test_max_det_truncation_other_class_counts(lib, nc):
    _max_det_truncation(nc)


def _max_det_truncation(nc):
    rng = np.random.default_rng(1)
    p = _random_pred(rng, 1500, spread=3000.0, nc=nc)
    p[..., 2:4] = 3.0                    # tiny boxes: almost nothing suppressed
    p[..., 4] = rng.uniform(0.6, 1.0, p.shape[:2])
    p[..., 5] = 0.99
    assert _run(p, max_det=300)[0].shape[0] == 300
    assert _run(p, max_det=1000)[0].shape[0] == 1000


@pytest.mark.parametrize("n,seed", [(300, 2), (2048, 3), (2049, 4), (6000, 5)])
def test_random_dense_matches_oracle(lib, n, seed):
    """Dense overlapping boxes across both the bit-matrix path (n <= 2048) and the greedy fallback."""
    _random_dense(NC, n, seed)


@pytest.mark.parametrize("nc", [4, 1])
@pytest.mark.parametrize("n,seed", [(300, 2), (2048, 3), (2049, 4), (6000, 5)])
def test_random_dense_matches_oracle_other_class_counts(lib, n, seed, nc):
    _random_dense(nc, n, seed)


def _random_dense(nc, n, seed, precheck=None):
    rng = np.random.default_rng(seed)
    p = _random_pred(rng, n, B=2, nc=nc)
    p[..., 4] = rng.uniform(0.5, 1.0, p.shape[:2])
    p[..., 5:] = rng.uniform(0.6, 1.0, p.shape[:2] + (nc,))
    r = _run(p, precheck=precheck)
    assert all(x.shape[0] > 10 for x in r)


def test_max_nms_cap_30000(lib):
    """More than 30,000 rows pass both thresholds: only the 30,000 most confident enter NMS [UPSTREAM max_nms]."""
    rng = np.random.default_rng(6)
    n = 33000
    p = np.zeros((1, n, 5 + NC), np.float32)
    p[0, :, 0] = (np.arange(n) % 200) * 10 + 5
    p[0, :, 1] = (np.arange(n) // 200) * 10 + 5
    p[0, :, 2:4] = 6.0
    p[0, :, 4] = rng.uniform(0.5, 1.0, n)
    p[0, :, 5] = 0.99
    r = _run(p, max_det=40000)[0]
    assert r.shape[0] == 30000


def test_engine_decode_plus_nms_equals_nms_on_raw_pred(lib, synth_ck, monkeypatch):
    """The compact-candidate path (decode writes only rows with obj > conf_thres) and S1 -> S2 through the full pred tensor agree bit for
    bit.  (With the Detect heads fused with their decode -- csrc/head_decode.hip, the default of `infer` -- the head convs sum K in a
    different order, so that comparison is one of tolerances: tests/test_gpu_head_decode.py.)"""
    from aquaculture_amd import engine, tiles
    monkeypatch.setenv("AQ_DISABLE_HEAD_FUSION", "1")
    eng = engine.Engine(synth_ck, "bf16")
    t = torch.from_numpy(tiles.synthetic_batch([3, 4], 640)).cuda()
    d0, c0 = eng.infer(t)
    d1, c1 = engine.nms(eng.forward_raw(t), synth_ck.nc)
    assert torch.equal(c0, c1)
    for b in range(2):
        assert torch.equal(d0[b, :c0[b]], d1[b, :c1[b]])


@pytest.mark.parametrize("n_cand", [1500, 2049, 3500, 4096, 4097, 6000])
def test_large_tiles_take_the_4096_candidate_bit_matrix(lib, n_cand):
    """1280-px tiles (100,800 rows; BASELINE.json configs[4]) are launched on nms_kernel<4096> (round 3): candidate counts on both sides
    of the old 2,048 and the new 4,096 limit (beyond it: the bitonic path), all bit for bit the oracle's."""
    _large_tile(NC, n_cand)


@pytest.mark.parametrize("nc", [4, 1])
@pytest.mark.parametrize("n_cand", [1500, 2049, 3500, 4096, 4097, 6000])
def test_large_tiles_take_the_4096_candidate_bit_matrix_other_class_counts(lib, n_cand, nc):
    _large_tile(nc, n_cand)


def _large_tile(nc, n_cand, precheck=None):
    rng = np.random.default_rng(n_cand)
    N = 100800
    p = _random_pred(rng, N, spread=1240.0, nc=nc)
    p[..., 4] = 0.1                                           # nothing passes ...
    idx = rng.choice(N, n_cand, replace=False)
    p[0, idx, 4] = rng.uniform(0.5, 1.0, n_cand)              # ... but n_cand rows
    p[0, idx, 5:] = rng.uniform(0.6, 1.0, (n_cand, nc))
    r = _run(p, max_det=1000, precheck=precheck)[0]
    assert r.shape[0] > 100


# ---- the unfused decode (aq_detect_decode) away from nc = 5 ---------------------------------------------------------------------------
def _decode(lib, heads, H, W, nc, na, anchors_px, strides, conf, cap, head_ld=32):
    """aq_detect_decode on fp32 head maps [B, ny, nx, head_ld]: (pred [B, N, no], counts [B], cand [B, cap + guard], rows [B, cap + guard, no]);
    the guard slots behind an image's cap are part of the next image's -- the buffers are allocated with a sentinel tail instead."""
    from aquaculture_amd import engine
    B, no = heads[0].shape[0], nc + 5
    assert all(h.shape[3] == head_ld and h.is_contiguous() for h in heads)
    N = sum(na * h.shape[1] * h.shape[2] for h in heads)
    pred = torch.full((B, N, no), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((B + 64,), -7, dtype=torch.int32, device="cuda")
    cand = torch.full((B * cap + 1024,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((B * cap * no + 1024,), -7.0, dtype=torch.float32, device="cuda")
    hp = (C.c_void_p * 3)(*[h.data_ptr() for h in heads])
    anch = (C.c_float * (3 * na * 2))(*[float(v) for lvl in anchors_px for a in lvl for v in a])
    st = (C.c_float * 3)(*[float(s) for s in strides])
    engine._check(lib.aq_detect_decode(hp, head_ld, B, H, W, nc, na, anch, st, pred.data_ptr(), conf, cand.data_ptr(), rows.data_ptr(), counts.data_ptr(),
                                       cap, engine._stream_ptr()))
    torch.cuda.synchronize()
    assert (counts[B:] == -7).all() and (cand[B * cap:] == -7).all() and (rows[B * cap * no:] == -7.0).all()
    return pred.cpu(), counts[:B].cpu(), cand[:B * cap].view(B, cap).cpu(), rows[:B * cap * no].view(B, cap, no).cpu()


@pytest.mark.parametrize("nc,small_cap", [(4, False), (1, False), (4, True)])
def test_detect_decode_at_four_and_one_classes(lib, nc, small_cap):
    """Random fp32 head maps of 32 channels whose channels past na * no hold garbage, 64 x 96 px (levels 8 x 12, 4 x 6, 2 x 3), B = 3: the
    full pred against the oracle's Detect decode to fp32 rounding (1e-6 of the largest value); the compact list names exactly the rows with obj > conf_thres (all of them, or the
    first cap when there are more), its rows are bitwise the pred rows they name, its counters are exact."""
    _detect_decode_case(lib, nc, small_cap)


def _detect_decode_case(lib, nc, small_cap, head_ld=32):
    """The procedure of test_detect_decode_at_four_and_one_classes on head maps of head_ld channels (tests/test_gpu_many_classes.py runs it
    at the widths of 6 to 128 classes)."""
    from aquaculture_amd import checkpoint
    from oracle import yolov5_oracle as O
    ck = checkpoint.synthetic_checkpoint("yolov5m", 5)
    B, H, W, na, no, conf = 3, 64, 96, 3, nc + 5, 0.25
    g = torch.Generator().manual_seed(40 + nc)
    heads = [torch.randn(B, H // s, W // s, head_ld, generator=g) * 1.5 for s in (8, 16, 32)]
    assert na * no < head_ld and all((h[..., na * no:] != 0).all() for h in heads)
    m = O.OracleModel({}, nc, ck.anchors, ck.stride, ck.bn_eps)
    want = _oracle_decode(m, [h[..., :na * no] for h in heads])
    N = want.shape[1]
    passing = (want[..., 4] > conf).sum(1)
    assert int(passing.min()) > 20
    cap = int(passing.max()) // 2 if small_cap else N
    pred, counts, cand, rows = _decode(lib, [h.cuda().contiguous() for h in heads], H, W, nc, na, ck.anchor_grid_px().numpy().tolist(), ck.stride,
                                       conf, cap, head_ld)
    assert pred.shape == want.shape == (B, 3 * (96 + 24 + 6), no)
    _assert_decode_bounds(pred, want, f"detect_decode nc {nc}")
    assert torch.equal(pred[..., 4] > conf, want[..., 4] > conf)
    assert counts.tolist() == passing.tolist()
    for b in range(B):
        stored = min(int(counts[b]), cap)
        got = cand[b, :stored]
        ok = set(torch.nonzero(pred[b, :, 4] > conf).flatten().tolist())
        assert len(set(got.tolist())) == stored and (set(got.tolist()) == ok if not small_cap else set(got.tolist()) < ok)
        assert torch.equal(rows[b, :stored], pred[b, got.long()])
        assert (cand[b, stored:] == -7).all() and (rows[b, stored:] == -7.0).all()


def _assert_decode_bounds(pred, want, label):
    """A decoded pred against the oracle's Detect decode of the same head maps; returns (largest |d|, its bound)."""
    # the criterion of tests/test_gpu_augment.py::test_detect_decode_aug_matches_descaled_oracle: the oracle's sigmoid is torch's vectorised
    # CPU exp, the kernel's is the device expf -- both correctly rounded to within an ulp, not the same function, so the two decodes agree
    # to fp32 rounding and not in every bit (measured on MI355X: 403 of 10,206 values differ at nc = 4, 229 of 6,804 at nc = 1, by a few
    # units in the last place -- at most 9.2e-5 px on a box side)
    diff = (pred - want).abs()
    bound = 1e-6 * max(1.0, want.abs().max().item())
    print(f"{label}: {int((diff > 0).sum())} of {diff.numel()} values differ from the oracle's, max |d| {diff.max().item():.3e} "
          f"(bound {bound:.3e}), max |d conf| {diff[..., 4:].max().item():.3e} (bound {4 * 2.0 ** -24:.3e})")
    assert diff.max().item() <= bound
    # ... and value by value: each sigmoid is exp (1 ulp) + an add and a divide (half an ulp each), so two of them are at most 4 ulp apart
    # (2.4e-7 below 1); wh squares it (twice the relative error, two more roundings: 12 ulp), xy adds at most 2 * stride * 2.4e-7 <= 1e-5 px
    assert diff[..., 4:].max().item() <= 4 * 2.0 ** -24
    assert (diff[..., :4] <= 12 * 2.0 ** -23 * want[..., :4].abs() + 1e-5).all()
    return diff.max().item(), bound


def _oracle_decode(m, heads_nhwc):
    """[UPSTREAM Detect.forward, inference branch] of oracle/yolov5_oracle.py on given head maps: OracleModel.detect with the head
    convolutions as identities (weights eye, bias zero), so that only its decode arithmetic runs."""
    feats = [h.permute(0, 3, 1, 2).contiguous() for h in heads_nhwc]
    for i, f in enumerate(feats):
        c = f.shape[1]
        m.state[f"model.24.m.{i}.weight"] = torch.eye(c).view(c, c, 1, 1)
        m.state[f"model.24.m.{i}.bias"] = torch.zeros(c)
    return m.detect(feats)
