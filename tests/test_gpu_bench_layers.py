"""The benchmark's own path, layer by layer: every kernel bench.py launches, at the benchmark's batch, against an fp64 reference.

Each engine is built as bench.py builds it (same fused-op switches, the shipped tuned table, the benchmark's tiles, fp8 calibrated on
the first 16 tiles), and the plan is stepped through one op at a time (Engine.run_ops), which launches exactly what one `infer` call
launches.  Just before op i runs, its inputs are copied to the host for a sample of images (the first and last images and both sides of
a mid-batch seam); just after, its output.  So the in-place Bottleneck chains and the ping-pong buffers are checked with their true
inputs, and a kernel that goes wrong deep inside a batch of 64 or 128 -- a persistent workgroup's tenth tile, an image seam inside a
tile, a tuned configuration that no smaller test selects -- is named by op.  References are fp64 on the engine's own bf16 input values
and the folded weights rounded as the engine's packer rounds them; bounds are those the kernels' own parity tests state.

Then the same stepping pass again: every op's full output (all images) must be bit-identical between the two passes, and the first
op that is not names a run-to-run race.  Finally the benchmark's two batches in flight: two streams, two workspace slots, four distinct
batches, eight steps, each bit-identical to the same batch run alone.

BASELINE.json configs[4] (yolov5x, 1280 px, batch 16) is not here: its fp64 references take minutes of CPU per image.
"""
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

OP_CONV, OP_SPPF_POOL, OP_UPSAMPLE2X, OP_DECODE, OP_NMS, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK = 1, 2, 3, 4, 5, 6, 7, 8
CONF, IOU, MAX_DET = 0.25, 0.45, 1000            # bench.py step()

CONFIGS = {
    # BASELINE.json configs[1] / configs[3]: model, precision, batch, tile size, sampled images (first, last, both sides of a seam)
    "configs1": ("yolov5m", "bf16", 64, 640, [0, 31, 32, 63]),
    "configs3": ("yolov5m", "fp8", 128, 640, [0, 63, 64, 127]),
}

# Kernel families of each plan op at the benchmark's geometry (Engine.last_launches, run-length encoded in plan order): a change in
# which kernels the benchmark runs shows up here as a test change.
FAMILIES = {
    "configs1": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3s2', 1),
        ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 2),
        ('none', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 2), ('none', 1),
        ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('asm1x1', 1), ('head_decode', 3), ('none', 2),
    ],
    "configs3": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 2), ('none', 1), ('direct1x1', 1),
        ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 1), ('head_decode', 3), ('none', 2),
    ],
}


def _rle(fams):
    out = []
    for f in fams:
        if out and out[-1][0] == f:
            out[-1][1] += 1
        else:
            out.append([f, 1])
    return [(f, n) for f, n in out]


def _bf16(t):
    return t.double().to(torch.bfloat16).double()


def _nchw(t):
    return t.permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1)


class _Setup:
    def __init__(self, name):
        import bench
        from aquaculture_amd import checkpoint
        from aquaculture_amd.engine import Engine
        variant, precision, B, size, sample = CONFIGS[name]
        self.name, self.B, self.size, self.sample = name, B, size, sample
        self.ck = checkpoint.synthetic_checkpoint(variant, 5)
        self.x = torch.from_numpy(bench.make_tiles(0, B, 1, size)[0]).cuda()
        self.eng = Engine(self.ck, precision, 0, fused_stem=True, fused_bottleneck=precision in ("bf16", "fp8w", "fp8"),
                          fp8_calibration=self.x[:min(B, 16)] if precision == "fp8" else None)
        self.eng.autotune(self.x, cache=None, shipped=True)
        assert self.eng.tuned_from == "shipped table", "the benchmark's kernels, not a fresh timing"
        self.packed = {}
        ci = 0
        packed = checkpoint.pack_plan_weights(self.ck, self.eng.plan, "native")
        for i, o in enumerate(self.eng.plan.ops):
            if o.kind in (OP_CONV, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK):
                self.packed[i] = packed[ci]
                ci += 1
        # fp8 pairs: producer op -> scale of the codes it writes, consumer op -> scale of the codes it reads
        self.f8_scale = {}
        for prod, cons in self.eng.fp8_pairs():
            s = self.eng.fp8_scales.get(self.eng.plan.ops[cons].name)
            if s:
                self.f8_scale[prod] = self.f8_scale[cons] = float(s)

    def slice_view(self, s, dtype=None):
        """Device view of plan slice `s` [B, h, w, C] (the input tensor: the tiles); dtype uint8 = the e4m3 codes of an fp8 slice."""
        if s.tensor == self.eng.plan.input_tensor:
            return self.x
        t = self.eng.tensor(s.tensor, self.B)
        if dtype == torch.uint8:                      # codes in the first bytes of each pixel's bf16 slot
            return t.view(torch.uint8)[..., 2 * s.ch_off:2 * s.ch_off + s.channels]
        return t[..., s.ch_off:s.ch_off + s.channels]


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request, lib):
    import bench
    threads = torch.get_num_threads()
    torch.set_num_threads(bench.host_threads())     # the references' fp64 GEMMs: more threads than the host really has cost 10x
    s = _Setup(request.param)
    yield s
    s.eng.close()
    torch.set_num_threads(threads)


# ---------------------------------------------------------------------------------------------------------------------------------
# references (fp64, CPU) on one op's snapshot of its inputs
def _conv_ref(x, w_krsc, b, stride, pad, act, res=None, scale=None):
    """x: [n, h, w, cin] float64 values the kernel reads; w_krsc: the values the kernel multiplies (already rounded); scale: per-Cout
    factor of an fp8 consumer (act scale x weight scale)."""
    w = torch.as_tensor(w_krsc).double().permute(0, 3, 1, 2)
    y = F.conv2d(_nchw(x), w, None, stride=stride, padding=pad)
    if scale is not None:
        y = y * scale.view(1, -1, 1, 1)
    y = y + torch.as_tensor(b).double().view(1, -1, 1, 1)
    if act:
        y = F.silu(y)
    y = _nhwc(y)
    if res is not None:
        y = y + res
    return y


def _err_report(got, ref, rel, abs_):
    """(ok, max err, mean err, worst (image slot, y, x, c), ratio) of |got - ref| against rel |ref| + abs."""
    err = (got - ref).abs()
    ratio = err / (rel * ref.abs() + abs_)
    k = int(torch.argmax(ratio))
    idx = np.unravel_index(k, tuple(ratio.shape))
    return bool((ratio <= 1).all()), float(err.max()), float(err.mean()), idx, float(ratio.max())


def _decode_ref(setup, xs_by_level, head_ops):
    """fp64 head conv + decode of every level for the sampled images -> per image: {cand index: row (xywh px, obj, cls)}."""
    ck = setup.ck
    na, no = ck.na, ck.nc + 5
    anchors = ck.anchor_grid_px()
    out = [dict() for _ in setup.sample]
    off = 0
    for lvl, oi in enumerate(head_ops):
        x = xs_by_level[lvl]                                          # [n, ny, nx, cin] float64
        n, ny, nx, cin = x.shape
        pc = setup.packed[oi]
        w = _bf16(torch.from_numpy(pc.weight[:na * no, 0, 0, :]))      # (head rows past na * no are padding)
        b = torch.from_numpy(pc.bias[:na * no]).double()
        raw = (x.reshape(-1, cin) @ w.t() + b).reshape(n, ny, nx, na, no)
        sig = torch.sigmoid(raw)
        yy, xx = torch.meshgrid(torch.arange(ny, dtype=torch.float64), torch.arange(nx, dtype=torch.float64), indexing="ij")
        stride = float(ck.stride[lvl])
        ref = torch.empty_like(sig)
        ref[..., 0] = (sig[..., 0] * 2 + (xx - 0.5)[None, :, :, None]) * stride
        ref[..., 1] = (sig[..., 1] * 2 + (yy - 0.5)[None, :, :, None]) * stride
        ref[..., 2:4] = (sig[..., 2:4] * 2) ** 2 * anchors[lvl].double()[None, None, None]
        ref[..., 4:] = sig[..., 4:]
        flat = ref.permute(0, 3, 1, 2, 4).reshape(n, -1, no)          # candidate order: a, y, x
        for j in range(n):
            out[j][off] = flat[j]
        off += na * ny * nx
    return [torch.cat([v for _, v in sorted(d.items())], 0) for d in out]


def _check_candidates(setup, ref_rows, cand, rows, counts):
    """Same candidate set as the fp64 reference (but for candidates within 1e-4 of the threshold), rows within 1e-3 relative."""
    msgs, stats = [], []
    for j, img in enumerate(setup.sample):
        ref = ref_rows[j]
        obj = ref[:, 4]
        sure = (obj - CONF).abs() > 1e-4
        want = set(torch.nonzero(sure & (obj > CONF)).flatten().tolist())
        maybe = set(torch.nonzero(~sure).flatten().tolist())
        n = int(counts[j])
        got = cand[j, :n].long()
        gs = set(got.tolist())
        if len(gs) != n or not (want <= gs <= want | maybe):
            msgs.append(f"image {img}: {n} candidates ({len(gs)} distinct), reference {len(want)} (+{len(maybe)} at the threshold): "
                        f"missing {sorted(want - gs)[:5]}, extra {sorted(gs - want - maybe)[:5]}")
            continue
        r = ref[got]
        g = rows[j, :n].double()
        err = (g - r).abs()
        bound = 1e-3 * r.abs() + 1e-6
        stats.append((float(err.max()) if n else 0.0, float(err.mean()) if n else 0.0))
        if n and not (err <= bound).all():
            k = int(torch.argmax(err / bound))
            cidx, col = divmod(k, r.shape[1])
            msgs.append(f"image {img}: candidate {int(got[cidx])} column {col}: {float(g[cidx, col])} vs fp64 {float(r[cidx, col])}")
    return msgs, stats


# ---------------------------------------------------------------------------------------------------------------------------------
def _stepping_pass(setup, check, keep):
    """One pass over the plan, op by op.  check: compare every op with its fp64 reference on the sampled images (returns failures and
    the per-op table); keep: full-batch copies of every op's output on the device (returns them)."""
    eng, plan, B, sample = setup.eng, setup.eng.plan, setup.B, setup.sample
    dets = torch.zeros((B, MAX_DET, 6), dtype=torch.float32, device="cuda")
    counts = torch.zeros((B,), dtype=torch.int32, device="cuda")
    idx = torch.tensor(sample, device="cuda")
    head_ops = [i for i, o in enumerate(plan.ops) if o.kind == OP_CONV and o.level >= 0]
    head_x = {}
    failures, table, full = [], [], {}
    t_ref, t_op = 0.0, None                          # host time spent on the references (from the output copy to the next op)
    for i, op in enumerate(plan.ops):
        if t_op is not None:
            t_ref += time.perf_counter() - t_op
            t_op = None
        code = i in setup.f8_scale
        pre = {}
        if check and op.src is not None and op.kind != OP_NMS:
            pre["src"] = setup.slice_view(op.src, torch.uint8 if code and op.kind == OP_CONV and op.k == 3 else None)[idx].cpu()
            if op.res is not None and op.res.tensor >= 0:
                pre["res"] = setup.slice_view(op.res)[idx].cpu()
        if check and op.kind == OP_NMS:
            c, r, n = eng.candidates(B)
            pre["cand"], pre["rows"], pre["counts"] = c[idx].cpu(), r[idx].cpu(), n[idx].cpu()
        eng.run_ops(setup.x, i, i + 1, CONF, IOU, MAX_DET, out=(dets, counts))
        fam = eng.last_launches()[i]
        dst_codes = code and op.kind == OP_CONV and op.k == 1
        if keep:
            if op.kind == OP_CONV and op.level >= 0:
                if i == head_ops[-1]:
                    c, r, n = eng.candidates(B)
                    full[i] = (c.clone(), r.clone(), n.clone())
            elif op.kind == OP_NMS:
                full[i] = (dets.clone(), counts.clone())
            elif op.dst is not None:
                full[i] = setup.slice_view(op.dst, torch.uint8 if dst_codes else None).clone()
        if not check:
            continue
        t_op = time.perf_counter()
        label = f"op {i} {op.name} ({fam[0]}, cfg {fam[1]})"
        if op.kind == OP_CONV and op.level >= 0:
            head_x[op.level] = pre["src"].double()
            if i == head_ops[-1]:
                ref_rows = _decode_ref(setup, [head_x[l] for l in range(3)], head_ops)
                c, r, n = eng.candidates(B)
                msgs, stats = _check_candidates(setup, ref_rows, c[idx].cpu(), r[idx].cpu(), n[idx].cpu())
                failures += [f"{label}: {m}" for m in msgs]
                mx = max([s[0] for s in stats], default=0.0)
                table.append((i, "model.24.m.0-2 + decode", fam, mx, float(np.mean([s[1] for s in stats])) if stats else 0.0))
            continue
        if op.kind == OP_NMS:
            from oracle import yolov5_oracle as O
            N = pre["rows"].shape[1]
            got_d, got_c = dets[idx].cpu().numpy(), counts[idx].cpu().numpy()
            for j, img in enumerate(sample):
                n = int(pre["counts"][j])
                pred = np.zeros((1, N, setup.ck.nc + 5), np.float32)
                pred[0, pre["cand"][j, :n].long().numpy()] = pre["rows"][j, :n].numpy()
                want = O.non_max_suppression(pred, CONF, IOU, MAX_DET)[0]
                if int(got_c[j]) != want.shape[0] or not np.array_equal(got_d[j, :got_c[j]], want):
                    failures.append(f"{label}: image {img}: {int(got_c[j])} boxes vs the oracle's {want.shape[0]} on the engine's candidates "
                                    f"(first differing row {next((k for k in range(min(int(got_c[j]), want.shape[0])) if not np.array_equal(got_d[j, k], want[k])), None)})")
            table.append((i, op.name, fam, 0.0, 0.0))
            continue
        if op.kind == OP_DECODE:
            assert fam[0] == "none", f"{label}: the benchmark's engine decodes behind the head convs"
            continue
        got = setup.slice_view(op.dst, torch.uint8 if dst_codes else None)[idx].cpu()
        rel, abs_, mean_lim, exact = 2.0 ** -7, 4e-3, None, False
        if op.kind == OP_SPPF_POOL:
            x = pre["src"].double()
            ys, y = [], _nchw(x)
            for _ in range(3):
                y = F.max_pool2d(y, 5, 1, 2)
                ys.append(y)
            ref, exact = _nhwc(torch.cat(ys, 1)), True
        elif op.kind == OP_UPSAMPLE2X:
            ref, exact = pre["src"].double().repeat_interleave(2, 1).repeat_interleave(2, 2), True
        elif op.kind == OP_STEM:
            x = _bf16(pre["src"].double() / 255.0)
            pc = setup.packed[i]
            ref = _conv_ref(x, _bf16(torch.from_numpy(pc.weight)), pc.bias, op.stride, op.pad, op.act)
        elif op.kind == OP_BOTTLENECK:
            c = op.src.channels
            pc = setup.packed[i]
            w1 = _bf16(torch.from_numpy(pc.weight[:c * c]).view(c, 1, 1, c))
            w2 = _bf16(torch.from_numpy(pc.weight[c * c:]).view(c, 3, 3, c))
            x = pre["src"].double()
            t = _bf16(_conv_ref(x, w1, pc.bias[:c], 1, 0, True))
            ref = _conv_ref(t, w2, pc.bias[c:], 1, 1, True, res=x if op.res is not None and op.res.tensor >= 0 else None)
            abs_, mean_lim = 2e-2, 3e-3
        elif op.kind == OP_DOWNBLOCK:
            pc = setup.packed[i]
            ci, cm = op.src.channels, op.dst.channels
            wa = _bf16(torch.from_numpy(pc.weight[:cm * 9 * ci]).view(cm, 3, 3, ci))
            wb = _bf16(torch.from_numpy(pc.weight[cm * 9 * ci:]).view(cm, 1, 1, cm))
            t = _bf16(_conv_ref(pre["src"].double(), wa, pc.bias[:cm], 2, 1, True))
            ref = _conv_ref(t, wb, pc.bias[cm:], 1, 0, True)
            abs_, mean_lim = 2e-2, 3e-3
        elif op.kind == OP_CONV and fam[0] == "direct1x1_f8out":
            pc = setup.packed[i]
            y = _conv_ref(pre["src"].double(), _bf16(torch.from_numpy(pc.weight)), pc.bias, op.stride, op.pad, op.act)
            q = y / setup.f8_scale[i]
            want = q.clamp(-448, 448).float().to(torch.float8_e4m3fn).view(torch.uint8)
            gv, wv = got.view(torch.float8_e4m3fn).double(), want.view(torch.float8_e4m3fn).double()

            def order(c):                             # position on the e4m3 number line: neighbouring codes are 1 apart (+0 == -0)
                m = (c & 0x7f).long()
                return torch.where(c >= 0x80, -m, m)
            steps = (order(got) - order(want)).abs()
            same = float((steps == 0).double().mean())
            table.append((i, op.name, fam, float((gv - wv).abs().max()), 1.0 - same))
            if same <= 0.99 or int(steps.max()) > 1 or bool(torch.isnan(gv).any()):
                k = np.unravel_index(int(torch.argmax(steps)), tuple(steps.shape))
                failures.append(f"{label}: {same:.4%} of the e4m3 codes equal the reference's, worst {int(steps.max())} codes apart at "
                                f"(image {sample[k[0]]}, y {k[1]}, x {k[2]}, c {k[3]}): code {int(got[k]):#04x} = {float(gv[k])} vs "
                                f"{int(want[k]):#04x} = {float(wv[k])} for y / scale = {float(q[k])}")
            continue
        elif op.kind == OP_CONV:
            pc = setup.packed[i]
            w = torch.from_numpy(pc.weight)
            scale = None
            if fam[0] == "pl3x3_f8":
                s_act = setup.f8_scale[i]
                x = pre["src"].view(torch.float8_e4m3fn).double()
                wf = torch.from_numpy(pc.weight).float()
                ws = wf.abs().amax(dim=(1, 2, 3)) / 448.0
                ws = torch.where(ws > 0, ws, torch.ones_like(ws))
                w = (wf / ws.view(-1, 1, 1, 1)).to(torch.float8_e4m3fn).double()
                scale = s_act * ws.double()
            else:
                assert fam[0] in ("igemm_or_halo", "pl3x3", "pl3x3s2", "direct1x1", "asm1x1", "direct3x3s2"), label
                x = pre["src"].double()
                w = _bf16(w)
            ref = _conv_ref(x, w, pc.bias, op.stride, op.pad, op.act, res=pre["res"].double() if "res" in pre else None, scale=scale)
        else:
            raise AssertionError(f"{label}: op kind {op.kind} has no reference here")
        got = got.double()
        if exact:
            ok = torch.equal(got, ref)
            err = (got - ref).abs()
            k = np.unravel_index(int(torch.argmax(err)), tuple(err.shape))
            table.append((i, op.name, fam, float(err.max()), float(err.mean())))
            if not ok:
                failures.append(f"{label}: not bit-identical, worst at (image {sample[k[0]]}, y {k[1]}, x {k[2]}, c {k[3]}): "
                                f"{float(got[k])} vs {float(ref[k])}")
            continue
        ok, mx, mean, k, ratio = _err_report(got, ref, rel, abs_)
        table.append((i, op.name, fam, mx, mean))
        if not ok or (mean_lim is not None and mean >= mean_lim):
            failures.append(f"{label}: max err {mx:.3g} ({ratio:.2f} x the bound {rel:.3g} |ref| + {abs_:g}), mean {mean:.3g}"
                            f"{'' if mean_lim is None else f' (limit {mean_lim:g})'}; worst at (image {sample[k[0]]}, y {k[1]}, x {k[2]}, "
                            f"c {k[3]}): {float(got[k])} vs fp64 {float(ref[k])}")
    if t_op is not None:
        t_ref += time.perf_counter() - t_op
    torch.cuda.synchronize()
    return failures, table, full, (dets, counts), t_ref


def test_bench_path_layer_by_layer(setup):
    """Per-op fp64 references on the sampled images, run-to-run bit-identity of every op's full output, and stepping == infer."""
    eng, B = setup.eng, setup.B
    t0 = time.perf_counter()
    failures, table, full1, _, t_ref = _stepping_pass(setup, check=True, keep=True)
    t1 = time.perf_counter()
    fams = eng.last_launches()
    print(f"\n{setup.name}: B = {B}, images {setup.sample}: stepping pass with fp64 references {t1 - t0:.1f} s "
          f"(references {t_ref:.1f} s on {torch.get_num_threads()} threads)")
    print(f"{'op':>4} {'name':<28} {'family':<16} {'cfg':>5} {'max err':>10} {'mean err':>10}")
    for i, name, fam, mx, mean in table:
        print(f"{i:>4} {name:<28} {fam[0]:<16} {fam[1]:>5} {mx:>10.3g} {mean:>10.3g}")
    print(f"families: {_rle([f for f, _ in fams])}")
    assert not failures, "\n".join(failures)

    # the family list (what the benchmark runs)
    want = FAMILIES[setup.name]
    if want is not None:
        assert _rle([f for f, _ in fams]) == want, _rle([f for f, _ in fams])
    assert all(f != "none" for (f, _), o in zip(fams, eng.plan.ops) if o.kind in (OP_CONV, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK))
    if eng.precision_name == "fp8":
        pairs = eng.fp8_pairs()
        assert len(pairs) == 14 and all(fams[c][0] == "pl3x3_f8" and fams[p][0] == "direct1x1_f8out" for p, c in pairs)

    # layer-level determinism: the whole pass again, every op's full output bit-identical (a race names its op here)
    _, _, full2, (d2, c2), _ = _stepping_pass(setup, check=False, keep=True)
    for i, op in enumerate(eng.plan.ops):
        if i not in full1:
            continue
        a, b = full1[i], full2[i]
        if isinstance(a, tuple) and len(a) == 3:                 # candidate list: same set per image, any order (atomics)
            ca, ra, na_ = a
            cb, rb, nb = b
            same = torch.equal(na_, nb)
            if same:
                for j in range(B):
                    n = int(na_[j])
                    oa, ob = torch.argsort(ca[j, :n]), torch.argsort(cb[j, :n])
                    if not (torch.equal(ca[j, :n][oa], cb[j, :n][ob]) and torch.equal(ra[j, :n][oa], rb[j, :n][ob])):
                        same = False
                        break
        elif isinstance(a, tuple):
            same = torch.equal(a[1], b[1]) and all(torch.equal(a[0][j, :a[1][j]], b[0][j, :a[1][j]]) for j in range(B))
        else:
            same = torch.equal(a, b)
        if not same:
            bad = ""
            if not isinstance(a, tuple):
                diff = torch.nonzero((a != b).reshape(a.shape[0], -1).any(1)).flatten().tolist()
                bad = f" (images {diff[:8]}{' ...' if len(diff) > 8 else ''})"
            pytest.fail(f"op {i} {op.name} ({fams[i][0]}, cfg {fams[i][1]}) changed between two identical passes{bad}: "
                        f"the first op whose output is not run-to-run deterministic")
    del full1, full2

    # stepping == one infer call: same detections, counts and kernels
    d1, c1 = eng.infer(setup.x, CONF, IOU, MAX_DET)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2)
    for j in range(B):
        assert torch.equal(d1[j, :c1[j]], d2[j, :c2[j]]), j
    assert eng.last_launches() == fams
    print(f"{setup.name}: determinism + stepping == infer {time.perf_counter() - t1:.1f} s")


def test_run_ops_pieces_equal_infer(setup):
    """Uneven pieces (every split point of the fused-head bookkeeping included) give infer's detections, counts and launches."""
    eng, B = setup.eng, setup.B
    d1, c1 = eng.infer(setup.x, CONF, IOU, MAX_DET)
    d1, c1, f1 = d1.clone(), c1.clone(), eng.last_launches()
    n = len(eng.plan.ops)
    heads = [i for i, o in enumerate(eng.plan.ops) if o.kind == OP_CONV and o.level >= 0]
    cuts = sorted({0, 1, 2, 3, n // 2, heads[0], heads[1], heads[1] + 1, heads[2], n - 1, n})
    dets = torch.zeros((B, MAX_DET, 6), dtype=torch.float32, device="cuda")
    counts = torch.zeros((B,), dtype=torch.int32, device="cuda")
    for a, b in zip(cuts[:-1], cuts[1:]):
        eng.run_ops(setup.x, a, b, CONF, IOU, MAX_DET, out=(dets, counts))
    torch.cuda.synchronize()
    assert torch.equal(counts, c1)
    for j in range(B):
        assert torch.equal(dets[j, :c1[j]], d1[j, :c1[j]]), j
    assert eng.last_launches() == f1
    with pytest.raises(RuntimeError):
        eng.run_ops(setup.x, 3, n + 1, CONF, IOU, MAX_DET, out=(dets, counts))


def test_two_batches_in_flight_as_the_benchmark_runs_them(lib):
    """bench.py step(): batches alternate over two HIP streams with a workspace slot each.  Four distinct 64-tile batches, eight
    steps with their own output buffers: every step equals the same batch run alone on one stream."""
    import bench
    from aquaculture_amd import checkpoint
    from aquaculture_amd.engine import Engine
    variant, precision, B, size, _ = CONFIGS["configs1"]
    ck = checkpoint.synthetic_checkpoint(variant, 5)
    pool = torch.from_numpy(bench.make_tiles(0, B, 4, size)).cuda()
    eng = Engine(ck, precision, 0, fused_stem=True, fused_bottleneck=True)
    eng.autotune(pool[0], cache=None, shipped=True)
    assert eng.tuned_from == "shipped table"
    alone = []
    for k in range(4):
        d, c = eng.infer(pool[k], CONF, IOU, MAX_DET, slot=0)
        alone.append((d.clone(), c.clone()))
    torch.cuda.synchronize()
    K = 8
    dets = torch.zeros((K, B, MAX_DET, 6), dtype=torch.float32, device="cuda")
    counts = torch.zeros((K, B), dtype=torch.int32, device="cuda")
    streams = [torch.cuda.Stream() for _ in range(2)]
    for st in streams:
        st.wait_stream(torch.cuda.current_stream())
    for k in range(K):
        with torch.cuda.stream(streams[k % 2]):
            eng.infer(pool[k % 4], CONF, IOU, MAX_DET, out=(dets[k], counts[k]), slot=k % 2)
    for st in streams:
        torch.cuda.current_stream().wait_stream(st)
    torch.cuda.synchronize()
    for k in range(K):
        d, c = alone[k % 4]
        assert torch.equal(counts[k], c), f"step {k} (batch {k % 4}, stream {k % 2}): counts differ from the batch run alone"
        for j in range(B):
            assert torch.equal(dets[k, j, :c[j]], d[j, :c[j]]), f"step {k} (batch {k % 4}, stream {k % 2}): image {j} differs"
    assert int(counts.sum()) > 0
    eng.close()
