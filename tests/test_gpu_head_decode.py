"""Detect head fused with its decode (csrc/head_decode.hip; [UPSTREAM models/yolo.py Detect.forward] + the candidate filter of
[UPSTREAM utils/general.py non_max_suppression], reached through reference README.md:77): the kernel against a plain restatement on the
same bf16-rounded operands with the matrix product and the bias in fp64, and the engine's `infer` with and without the fusion
(AQ_DISABLE_HEAD_FUSION=1 = conv + decode).

Every instantiation of the kernel table is run (k-steps cin / 32 = 4, 6, 8, 10, 12, 16, 20, 24, 32, 40), on pixel counts where a
workgroup iteration covers one image, two images, or both by turns; at batches where every workgroup loops; at class / anchor counts
other than 5 / 3; with fewer slots than candidates; with strided counters and several levels appending to one list.

Criteria (the project's, unchanged): candidate sets agree outside a +-2e-4 band round the threshold; rows agree at rtol 2e-4, atol 2e-3.

Measured on MI355X, per width, over the (3, 5, 7) and (3, 8, 8) cases at nc = 5, na = 3 -- worst row error as a fraction of its bound
(|got - ref| / (2e-3 + 2e-4 |ref|)), worst absolute row error, candidates inside the band:
    cin    (3, 5, 7)                          (3, 8, 8)
    128    0.001 of the bound, 1.5e-5, 0      0.001, 3.1e-5, 1
    192    0.001, 1.5e-5, 0                   0.002, 1.5e-5, 0
    256    0.001, 1.9e-5, 0                   0.001, 2.3e-5, 1
    320    0.002, 1.9e-5, 0                   0.001, 2.3e-5, 0
    384    0.001, 1.5e-5, 1                   0.001, 2.3e-5, 1
    512    0.002, 1.5e-5, 0                   0.002, 1.5e-5, 0
    640    0.001, 2.3e-5, 0                   0.002, 1.9e-5, 1
    768    0.001, 2.3e-5, 0                   0.002, 2.3e-5, 0
    1024   0.001, 1.5e-5, 0                   0.002, 2.3e-5, 0
    1280   0.002, 2.3e-5, 0                   0.002, 2.3e-5, 0
(315 and 576 candidates per case, 178 .. 471 of them passing.)  The loop cases, 37 x 41 pixels per image: cin 256, B = 109 (2584 iterations
on 1024 workgroups): 0.003 of the bound, 6.1e-5, 347 of 496,059 candidates in the band; cin 512, B = 55 (2608 iterations): 0.004, 6.1e-5,
127 of 250,305; cin 1280, B = 28 (2655 iterations): 0.003, 6.1e-5, 67 of 127,428.  The class / anchor cases (nc, na) = (4, 3), (1, 3),
(3, 4), (11, 2), (11, 1) at cin 384 and 128: at most 0.002 of the bound, 3.1e-5, at most 1 candidate in the band.  No width comes within
two orders of magnitude of the tolerance: the errors are those of fp32 accumulation and of expf against the fp64 sigmoid.
"""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

ANCHORS = [(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)]
ANCHORS4 = ANCHORS + [(61.0, 45.0)]
KSTEPS = [4, 6, 8, 10, 12, 16, 20, 24, 32, 40]               # kHead[] of csrc/head_decode.hip
WIDTHS = [128, 192, 256, 320, 384, 512, 640, 768, 1024, 1280]
RTOL, ATOL, BAND = 2e-4, 2e-3, 2e-4


def ksplit(cin):
    """Waves that share a 16-pixel block (kHead[].split): a workgroup iteration covers 64 / split pixels."""
    return 1 if cin <= 256 else 2 if cin <= 512 else 4


def make_level(B, ny, nx, cin, na, nc, seed, pad=8):
    """x bf16 [B, ny, nx, cin] as a channel slice of a wider tensor (`pad` channels before it, as many after), w [na * no, cin], bias."""
    no = nc + 5
    g = torch.Generator().manual_seed(seed)
    xw = (torch.randn(B, ny, nx, cin + 2 * pad, generator=g) * 0.7).bfloat16()
    w = torch.randn(na * no, cin, generator=g) * (1.5 / cin ** 0.5)
    b = torch.randn(na * no, generator=g) * 0.5
    b[4::no] -= 0.5                                          # roughly a third of the candidates pass
    return xw, xw[..., pad:pad + cin], w, b


def reference(x, w, b, anchors, nc, stride):
    """Detect.forward of one level on bf16-rounded operands: product and bias in fp64, sigmoid in fp64, the box arithmetic in fp32.
    Returns rows [B, na * ny * nx, no] in candidate order (a, y, x)."""
    B, ny, nx, cin = x.shape
    na, no = len(anchors), nc + 5
    wd = w.bfloat16().double().t().contiguous()
    xf = x.reshape(-1, cin)
    raw = torch.cat([xf[i:i + 16384].double() @ wd for i in range(0, xf.shape[0], 16384)]) + b.double()
    sig = torch.sigmoid(raw).float().reshape(B, ny, nx, na, no)
    yy, xx = torch.meshgrid(torch.arange(ny, dtype=torch.float32), torch.arange(nx, dtype=torch.float32), indexing="ij")
    ref = torch.empty_like(sig)
    ref[..., 0] = (sig[..., 0] * 2 + (xx - 0.5)[None, :, :, None]) * stride
    ref[..., 1] = (sig[..., 1] * 2 + (yy - 0.5)[None, :, :, None]) * stride
    ref[..., 2:4] = (sig[..., 2:4] * 2) ** 2 * torch.tensor(anchors)[None, None, None]
    ref[..., 4:] = sig[..., 4:]
    return ref.permute(0, 3, 1, 2, 4).reshape(B, na * ny * nx, no)


def check_level(counts, cand, rows, ref, off, thr, cap):
    """counts [B], cand [B, cap], rows [B, cap, no] of one level against its reference rows.  Per image: the counter is the number of passing
    candidates (up to the band), the first min(count, cap) slots hold distinct candidates of this image's passing set -- all of it when it
    fits -- and their rows are the reference's.  Returns (worst error / bound, worst absolute error, candidates in the band, total count)."""
    counts, cand, rows = counts.cpu(), cand.cpu(), rows.cpu()
    worst_rel = worst_abs = 0.0
    in_band = total = 0
    for bi in range(ref.shape[0]):
        obj = ref[bi, :, 4]
        sure = (obj - thr).abs() > BAND                      # away from the threshold the pass / fail decision must agree
        want = set((off + torch.nonzero(sure & (obj > thr)).flatten()).tolist())
        maybe = set((off + torch.nonzero(~sure).flatten()).tolist())
        n = int(counts[bi])
        assert len(want) <= n <= len(want | maybe), (bi, n, len(want), len(maybe))
        stored = min(n, cap)
        got = cand[bi, :stored].tolist()
        assert len(set(got)) == stored and set(got) <= want | maybe, (bi, n, len(want))
        if n <= cap:
            assert want <= set(got), (bi, n, len(want))
        if stored:
            sel = torch.tensor(got) - off
            d = (rows[bi, :stored] - ref[bi, sel]).abs()
            worst_abs = max(worst_abs, float(d.max()))
            worst_rel = max(worst_rel, float((d / (ATOL + RTOL * ref[bi, sel].abs())).max()))
            torch.testing.assert_close(rows[bi, :stored], ref[bi, sel], rtol=RTOL, atol=ATOL)
        in_band += len(maybe)
        total += n
    return worst_rel, worst_abs, in_band, total


def run_case(B, ny, nx, cin, anchors=ANCHORS, nc=5, seed=None, off=1000, stride=16.0, thr=0.25, pad=8):
    from aquaculture_amd import engine
    na = len(anchors)
    xw, x, w, b = make_level(B, ny, nx, cin, na, nc, cin + ny if seed is None else seed, pad)
    cap = na * ny * nx
    counts, cand, rows = engine.head_decode_level(xw.cuda()[..., pad:pad + cin], w, b, off, stride, anchors, nc, thr, cap)
    ref = reference(x, w, b, anchors, nc, stride)
    stats = check_level(counts, cand, rows, ref, off, thr, cap)
    cand = cand.cpu()
    for bi in range(B):
        assert (cand[bi, int(counts[bi]):] == -1).all()
    assert stats[3] > 0.1 * B * cap
    return stats


def test_the_parametrisation_reaches_every_kernel_of_the_table(lib):
    assert sorted(c // 32 for c in WIDTHS) == KSTEPS and all(c % 32 == 0 for c in WIDTHS)
    assert sorted({ksplit(c) for c in WIDTHS}) == [1, 2, 4]
    for cin in WIDTHS:
        assert lib.aq_head_decode_supported(cin, 3, 5) == 1 and lib.aq_head_decode_supported(cin, 3, 4) == 1, cin


@pytest.mark.parametrize("case", [
    # B, ny, nx, cin: the three yolov5m levels at 640 px (batch cut down), a ragged one (pixel count not a multiple of 16), yolov5s widths
    (3, 80, 80, 192), (5, 40, 40, 384), (7, 20, 20, 768), (2, 13, 9, 256), (1, 5, 7, 128), (2, 12, 12, 1024),
])
def test_head_decode_matches_reference(lib, case):
    B, ny, nx, cin = case
    run_case(B, ny, nx, cin)


@pytest.mark.parametrize("shape", [(3, 5, 7), (3, 8, 8)])
@pytest.mark.parametrize("cin", WIDTHS)
def test_every_width_on_straddling_and_one_image_iterations(lib, cin, shape):
    """(3, 5, 7): 105 pixels, 35 per image -- no multiple of 16, 32 or 64: with 64 pixels per iteration every iteration straddles two
    images, with 32 and 16 one-image and straddling iterations both occur.  (3, 8, 8): 64 pixels per image, every iteration is one-image."""
    B, ny, nx = shape
    assert lib.aq_head_decode_supported(cin, 3, 5) == 1
    pxi, hw = 64 // ksplit(cin), ny * nx
    kinds = {it * pxi // hw == min(it * pxi + pxi - 1, B * hw - 1) // hw for it in range((B * hw + pxi - 1) // pxi)}
    assert kinds == ({True} if hw == 64 else {False} if pxi == 64 else {True, False})
    rel, ab, band, total = run_case(B, ny, nx, cin)
    print(f"head_decode cin {cin} {shape}: worst row error {rel:.3f} of the bound ({ab:.2e} abs), {band} candidates in the band, {total} pass")


@pytest.mark.parametrize("cin", [256, 512, 1280])
def test_persistent_loop_runs_every_workgroup_more_than_twice(lib, cin):
    """One case per K split (1, 2, 4; cin 1280 is the two-workgroups-per-CU build): at least 2.5 iterations per workgroup of the 4 x CUs
    grid, images of 37 x 41 pixels, so that a workgroup meets straddling and one-image iterations by turns with its LDS tile, wave counts
    and base reused from one to the next."""
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    pxi, hw = 64 // ksplit(cin), 37 * 41
    B = -(-int(2.5 * 4 * cus * pxi) // hw)
    npix = B * hw
    nit = (npix + pxi - 1) // pxi
    assert npix >= 2.5 * 4 * cus * pxi and nit > 2 * 4 * cus
    kinds = {it * pxi // hw == min(it * pxi + pxi - 1, npix - 1) // hw for it in range(nit)}
    assert kinds == {True, False}
    rel, ab, band, total = run_case(B, 37, 41, cin, seed=cin + 1, pad=0)
    print(f"head_decode loop cin {cin} B {B} ({nit} iterations, {4 * cus} workgroups): worst row error {rel:.3f} of the bound ({ab:.2e} abs), "
          f"{band} candidates in the band, {total} pass")


@pytest.mark.parametrize("cin", [384, 128])
@pytest.mark.parametrize("nc,na", [(4, 3), (1, 3), (3, 4), (11, 2), (11, 1)])
def test_class_and_anchor_counts(lib, nc, na, cin):
    """Row lengths 9, 6, 8 and 16; (3, 4) and (11, 2) fill all 32 rows of the head tile, (3, 4) uses the fourth lane quarter; with the others
    the rows past na * no are padding, whose channels must not reach any candidate row."""
    assert lib.aq_head_decode_supported(cin, na, nc) == 1
    rel, ab, band, total = run_case(3, 5, 7, cin, anchors=ANCHORS4[:na], nc=nc, seed=100 * nc + na)
    print(f"head_decode cin {cin} nc {nc} na {na}: worst row error {rel:.3f} of the bound ({ab:.2e} abs), {band} in the band, {total} pass")


REFUSED = [(384, 3, 6), (384, 1, 12), (384, 5, 1), (96, 3, 5), (352, 3, 5), (100, 3, 5)]      # cin, na, nc


@pytest.mark.parametrize("aug", [False, True])
@pytest.mark.parametrize("cin,na,nc", REFUSED)
def test_unsupported_heads_are_refused_and_nothing_is_written(lib, cin, na, nc, aug):
    """na (nc + 5) > 32, nc = 12, na = 5, 3 and 11 k-steps (below / not in the table), cin no multiple of 32: an error, no launch."""
    from aquaculture_amd import engine
    assert lib.aq_head_decode_supported(cin, na, nc) == 0
    B, ny, nx, cap = 2, 4, 4, 64
    x = torch.zeros((B, ny, nx, 512), dtype=torch.bfloat16, device="cuda")
    packed = torch.zeros(1 << 16, dtype=torch.uint8, device="cuda")
    counts = torch.full((B,), -3, dtype=torch.int32, device="cuda")
    cand = torch.full((B, cap), -3, dtype=torch.int32, device="cuda")
    rows = torch.full((B, cap, 32), -3.0, dtype=torch.float32, device="cuda")
    anch = (C.c_float * 16)(*([8.0] * 16))
    if aug:                                                  # (this entry point has ctypes argument types, the plain one does not)
        rc = lib.aq_head_decode_aug(x.data_ptr(), 512, 0, cin, packed.data_ptr(), B, ny, nx, 0, 8.0, anch, nc, na, 0.25, 0.67, 640.0, cand.data_ptr(),
                                    rows.data_ptr(), counts.data_ptr(), 1, cap, engine._stream_ptr())
    else:
        vp = C.c_void_p
        rc = lib.aq_head_decode(vp(x.data_ptr()), 512, 0, cin, vp(packed.data_ptr()), B, ny, nx, 0, C.c_float(8.0), anch, nc, na, C.c_float(0.25),
                                vp(cand.data_ptr()), vp(rows.data_ptr()), vp(counts.data_ptr()), 1, cap, vp(engine._stream_ptr()))
    assert rc != 0 and b"head_decode" in lib.aq_last_error()
    torch.cuda.synchronize()
    assert (counts == -3).all() and (cand == -3).all() and (rows == -3.0).all()


@pytest.mark.parametrize("cin", [192, 512])
def test_fewer_slots_than_candidates(lib, cin):
    """cap = about half the passing candidates of the fullest image: the counters still count every passing candidate, the first cap slots
    of an image hold distinct candidates of its own passing set with the reference's rows, nothing is written past an image's slots or
    behind the buffers."""
    from aquaculture_amd import engine
    B, ny, nx, nc, off, stride, thr, guard = 3, 9, 11, 5, 77, 16.0, 0.25, 4096
    xw, x, w, b = make_level(B, ny, nx, cin, 3, nc, 31 + cin)
    ref = reference(x, w, b, ANCHORS, nc, stride)
    passing = (ref[..., 4] > thr).sum(1)
    cap = int(passing.max()) // 2
    assert cap >= 16 and int(passing.min()) > cap                                   # every image overflows its slots
    cand = torch.full((B * cap + guard,), -7, dtype=torch.int32, device="cuda")
    rows = torch.full((B * cap * (nc + 5) + guard,), -7.0, dtype=torch.float32, device="cuda")
    counts = torch.full((B + guard,), -7, dtype=torch.int32, device="cuda")
    counts[:B] = 0
    engine.head_decode_level(xw.cuda()[..., 8:8 + cin], w, b, off, stride, ANCHORS, nc, thr, cap, counts=counts, cand=cand, rows=rows)
    assert (cand[B * cap:] == -7).all() and (rows[B * cap * (nc + 5):] == -7.0).all() and (counts[B:] == -7).all()
    cand2, rows2 = cand[:B * cap].view(B, cap), rows[:B * cap * (nc + 5)].view(B, cap, nc + 5)
    assert (cand2 != -7).all()                                                       # every slot of every image was filled ...
    check_level(counts[:B], cand2, rows2, ref, off, thr, cap)                        # ... with a candidate of that image, whose row is the reference's
    # a candidate index alone does not name its image: the rows do -- no row of image b equals image b + 1's reference at its index
    rows2, cand2 = rows2.cpu(), cand2.cpu()
    for bi in range(B):
        other = ref[(bi + 1) % B, (cand2[bi] - off).long()]
        assert ((rows2[bi] - other).abs().amax(1) > 10 * ATOL).all()


def test_three_levels_append_to_one_list_with_counters_1024_ints_apart(lib):
    """Three levels of different size, width, stride and anchors into one candidate list, counters 1024 ints apart as the engine keeps
    them, then aq_head_counts_gather: per image the union of the three references; the ints between the counters stay as they were; and the
    same three levels with adjacent counters give the same candidates and bit-identical rows."""
    from aquaculture_amd import engine
    B, nc, thr, cs = 3, 4, 0.25, 1024
    no = nc + 5
    levels = [(8, 12, 192, 8.0, [(10.0, 13.0), (16.0, 30.0), (33.0, 23.0)]), (4, 6, 384, 16.0, [(30.0, 61.0), (62.0, 45.0), (59.0, 119.0)]),
              (2, 3, 768, 32.0, [(116.0, 90.0), (156.0, 198.0), (373.0, 326.0)])]
    offs = np.cumsum([0] + [3 * ny * nx for ny, nx, *_ in levels]).tolist()
    N = offs[-1]
    data = [make_level(B, ny, nx, cin, 3, nc, 7 + cin) for ny, nx, cin, _, _ in levels]
    refs = [reference(d[1], d[2], d[3], anch, nc, stride) for d, (_, _, _, stride, anch) in zip(data, levels)]
    outs = []
    for stride_ints in (cs, 1):
        wide = torch.full(((B - 1) * stride_ints + 1 + 64,), -9, dtype=torch.int32, device="cuda")
        wide[0:(B - 1) * stride_ints + 1:stride_ints] = 0
        cand = torch.full((B, N), -1, dtype=torch.int32, device="cuda")
        rows = torch.zeros((B, N, no), dtype=torch.float32, device="cuda")
        for d, (ny, nx, cin, stride, anch), off in zip(data, levels, offs):
            engine.head_decode_level(d[0].cuda()[..., 8:8 + cin], d[2], d[3], off, stride, anch, nc, thr, N, count_stride=stride_ints, counts=wide,
                                     cand=cand, rows=rows)
        counts = engine.head_counts_gather(wide, stride_ints, B).cpu()
        w = wide.cpu()
        assert torch.equal(counts, w[0:(B - 1) * stride_ints + 1:stride_ints])
        untouched = torch.ones(w.numel(), dtype=torch.bool)
        untouched[0:(B - 1) * stride_ints + 1:stride_ints] = False
        assert (w[untouched] == -9).all()
        outs.append((counts, cand.cpu(), rows.cpu()))
    counts, cand, rows = outs[0]
    for bi in range(B):
        n = int(counts[bi])
        got = cand[bi, :n]
        assert len(set(got.tolist())) == n and (cand[bi, n:] == -1).all()
        assert int(got.min()) >= 0 and int(got.max()) < N
        for ref, off, nxt in zip(refs, offs, offs[1:]):              # the level's share of the list, as a list of its own
            m = (got >= off) & (got < nxt)
            assert int(m.sum()) > 0
            check_level(m.sum()[None], got[m][None], rows[bi, :n][m][None], ref[bi:bi + 1], off, thr, N)
    c1, i1, r1 = outs[1]
    assert torch.equal(counts, c1)
    for bi in range(B):
        n = int(counts[bi])
        o0, o1 = torch.argsort(cand[bi, :n]), torch.argsort(i1[bi, :n])
        assert torch.equal(cand[bi, :n][o0], i1[bi, :n][o1]) and torch.equal(rows[bi, :n][o0], r1[bi, :n][o1])


def assert_same_detections(d0, c0, d1, c1):
    """Two runs of `infer` that differ in the summation order of the head convs only (fp32 accumulate, K split differently)."""
    assert (c0 - c1).abs().max() <= 1                                 # a box within 1e-6 of a threshold may flip
    for bi in range(c0.shape[0]):
        if c0[bi] != c1[bi]:
            continue
        n = int(c0[bi])
        if n == 0:
            continue
        # the lists are sorted by confidence: two detections whose confidences differ by less than the two paths' rounding may swap places, so
        # match every row to its nearest row of the other list (one to one) instead of comparing position by position
        a, b = d0[bi, :n], d1[bi, :n]
        dist = (a[:, None, :4] - b[None, :, :4]).abs().amax(-1)
        nearest = dist.argmin(1)
        assert sorted(nearest.tolist()) == list(range(n)), "not a one-to-one match"
        b = b[nearest]
        assert (nearest - torch.arange(n)).abs().max() <= 2          # ... and only neighbours swap
        torch.testing.assert_close(a[:, :4], b[:, :4], rtol=0, atol=2e-2)
        torch.testing.assert_close(a[:, 4], b[:, 4], rtol=0, atol=1e-4)
        assert torch.equal(a[:, 5], b[:, 5])


def infer_fused_and_unfused(ck, x, monkeypatch):
    """[(dets, counts, raw candidate counts)] of a bf16 engine without and with the fused heads."""
    from aquaculture_amd import engine
    outs = []
    for off in ("1", "0"):
        monkeypatch.setenv("AQ_DISABLE_HEAD_FUSION", off)
        eng = engine.Engine(ck, "bf16")
        dets, counts = eng.infer(x)
        torch.cuda.synchronize()
        fused = "head_decode" in [f for f, _ in eng.last_launches()]
        assert fused == (off == "0")
        outs.append((dets.cpu().clone(), counts.cpu().clone(), eng.candidates(x.shape[0])[2].cpu().clone()))
        eng.close()
        del eng
    return outs


def test_engine_infer_with_and_without_head_fusion(lib, synth_ck, monkeypatch):
    """Same detections either way, up to the summation order of the head convs (fp32 accumulate, K split differently)."""
    from aquaculture_amd import tiles
    x = torch.from_numpy(tiles.synthetic_batch([1, 6, 12], 256)).cuda()
    (d0, c0, _), (d1, c1, _) = infer_fused_and_unfused(synth_ck, x, monkeypatch)
    assert int(c0.sum()) > 20
    assert_same_detections(d0, c0, d1, c1)


@pytest.fixture(scope="module")
def synth_ck_nc4():
    from aquaculture_amd import checkpoint
    return checkpoint.synthetic_checkpoint("yolov5m", 4)


@pytest.mark.parametrize("nc", [5, 4])
@pytest.mark.parametrize("shape,batch", [((384, 640), 1), ((640, 384), 3), ((32, 32), 2), ((96, 160), 5)])
def test_bf16_engine_on_ragged_shapes_with_and_without_head_fusion(lib, synth_ck, synth_ck_nc4, monkeypatch, shape, batch, nc):
    """The shapes of tests/test_gpu_engine.py::test_fp32_engine_on_ragged_shapes through the bf16 engine, whose P5 level (1 x 1 to
    20 x 12 pixels) runs the fused head's straddling iterations: fused against unfused heads, the criteria of the test above; where there
    are no detections at all, the raw candidate counts must be equal."""
    from aquaculture_amd import tiles
    H, W = shape
    ck = synth_ck if nc == 5 else synth_ck_nc4
    big = tiles.synthetic_batch(range(batch), max(640, H, W))
    x = torch.from_numpy(np.ascontiguousarray(big[:, :H, :W, :])).cuda()
    (d0, c0, n0), (d1, c1, n1) = infer_fused_and_unfused(ck, x, monkeypatch)
    assert_same_detections(d0, c0, d1, c1)
    assert ((d0[..., 5] < nc) | (torch.arange(d0.shape[1])[None] >= c0[:, None])).all()
    if int(c0.sum()) == 0 or int(c1.sum()) == 0:
        assert torch.equal(n0, n1)
