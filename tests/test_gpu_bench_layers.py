"""The benchmark's own path, layer by layer: every kernel bench.py and the shipped tuned tables launch, at their own batch, against an fp64
reference.

CONFIGS is the table of engines: BASELINE.json configs[1], [3] and [4], the two parity-mode engines every default bench.py run times
(fp32 on heuristic tile shapes, f16x3 on its shipped table) and every other shipped tuned table (tests/test_layer_windows.py checks that
each key of aquaculture_amd/data/tuned_tables.json has an entry here).  Each engine is built as its user builds it, and the plan is
stepped through one op at a time (Engine.run_ops), which launches exactly what one `infer` call launches.  Just before op i runs, its
inputs are copied to the host for a sample of images (the first and last images, and both sides of a mid-batch seam); just after, its
output.  So the in-place Bottleneck chains and the ping-pong buffers are checked with their true inputs, and a kernel that goes wrong deep
inside a batch -- a persistent workgroup's tenth tile, an image seam inside a tile, a tuned configuration that no smaller test selects --
is named by op.  References are fp64 on the engine's own input values and the folded weights as the engine stores them (rounded to bf16
for bf16 engines, fp32 for the fp32 and f16x3 parity engines); bounds are those the kernels' own parity tests state, and north_star's
1e-4 gate on the candidate rows of the fp32-grade engines.

configs[4] (yolov5x, 1280 px, batch 16) has convolutions too large for whole-image fp64 references: every conv is checked on windows of
8 x 8 output pixels with all output channels (oracle/windowed_ref.py) -- the four corners, the middle of each edge, the last rows of
image 7 and the first rows of image 8, tile boundaries of the kernel's own pixel tiles, two seeded interior windows -- each computed
from only the input region it reads, copied from the device window by window.  Planes the windows would mostly cover (the 40 x 40
level) are checked whole, as are the cheap ops: preprocess, SPPF, upsample, the head convs + decode and NMS.

Then the same stepping pass again: every op's full output (all images) must be bit-identical between the two passes, and the first
op that is not names a run-to-run race.  A third pass runs a ragged batch, the first B' (odd) images: every op that launches what the
full batch launches, and whose upstream ops do too, must give the full batch's outputs for those images bit for bit, and every op is
checked against fp64 on image B' - 1, where the last image ends inside every kernel's last pixel tile.  Finally the benchmark's two
batches in flight: two streams, two workspace slots, four distinct batches, eight steps, each bit-identical to the same batch run alone.
"""
import time
from typing import List, NamedTuple, Optional

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

OP_PREPROCESS, OP_CONV, OP_SPPF_POOL, OP_UPSAMPLE2X, OP_DECODE, OP_NMS, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK = 0, 1, 2, 3, 4, 5, 6, 7, 8
CONF, IOU, MAX_DET = 0.25, 0.45, 1000            # bench.py step()


class Entry(NamedTuple):
    variant: str
    precision: str
    batch: int
    size: int
    sample: List[int]             # images checked against fp64 (first, last, and both sides of a seam where there are four)
    tuning: Optional[str]         # Engine.tuned_from after the engine is built as its user builds it; None = no autotune call
    ragged: int                   # B' of the ragged-batch pass
    built_as: str


CONFIGS = {
    "configs1": Entry("yolov5m", "bf16", 64, 640, [0, 31, 32, 63], "shipped table", 37, "bench.py"),
    "configs3": Entry("yolov5m", "fp8", 128, 640, [0, 63, 64, 127], "shipped table", 101, "bench.py --precision fp8 --batch 128"),
    # bench.py's parity legs (every default run): Engine(ck, "fp32") with no autotune call, Engine(ck, "f16x3") + autotune(shipped=True)
    "parity_fp32": Entry("yolov5m", "fp32", 64, 640, [0, 31, 32, 63], None, 37, "bench.py parity leg (fp32)"),
    "parity_f16x3": Entry("yolov5m", "f16x3", 64, 640, [0, 31, 32, 63], "shipped table", 37, "bench.py parity leg (f16x3)"),
    # the other shipped tables (detect.py --batch-size 16 / 32, bench.py --batch 128, bench.py --precision fp8): first and last image
    "table_bf16_b16": Entry("yolov5m", "bf16", 16, 640, [0, 15], "shipped table", 11, "bench.py --batch 16"),
    "table_bf16_b32": Entry("yolov5m", "bf16", 32, 640, [0, 31], "shipped table", 21, "bench.py --batch 32"),
    "table_bf16_b128": Entry("yolov5m", "bf16", 128, 640, [0, 127], "shipped table", 101, "bench.py --batch 128"),
    "table_fp8_b64": Entry("yolov5m", "fp8", 64, 640, [0, 63], "shipped table", 37, "bench.py --precision fp8"),
    "configs4": Entry("yolov5x", "bf16", 16, 1280, [0, 7, 8, 15], "shipped table", 5, "bench.py --variant yolov5x --size 1280 --batch 16"),
    # the engine's batch limits, on heuristic tile shapes: fp32 (detect.py's default precision) with out0 past 2^31 bytes (image 109 holds
    # byte 2^31); bf16 across both points where Bottleneck launches leave the assembly builds (219: model.2.m.0, 437: the others at 2^30
    # input bytes), so the ragged batch (217) runs the assembly builds and the full batch the HIP-source ones
    "fp32_b128": Entry("yolov5m", "fp32", 128, 640, [0, 109, 127], None, 101, "detect.py --batch-size 128"),
    "bf16_b448": Entry("yolov5m", "bf16", 448, 640, [0, 218, 219, 436, 437, 447], None, 217, "detect.py --half --batch-size 448, untuned"),
}

# conv tolerances (rel, abs) of the kernels' own parity tests: bf16 storage; fp32 (tests/test_gpu_conv.py); f16x3 = 4 x fp32
# (tests/test_gpu_conv.py::test_conv_split_mode_is_fp32_grade)
CONV_TOL = {"bf16": (2.0 ** -7, 4e-3), "fp8": (2.0 ** -7, 4e-3), "fp32": (2e-5, 2e-5), "f16x3": (8e-5, 8e-5)}

# A conv whose error exceeds CONV_TOL passes only on evidence that the excess is fp32 accumulation (_accumulation_evidence): on the
# same inputs, an fp32 CPU computation of the op must be at most ACC_VS_CPU32 times less accurate than the kernel, and every element's
# error must stay within CONV_TOL + ACC_C x 2^-24 sqrt(K) sum_k |x_k w_k|, the random-walk size of K fp32 roundings.  configs1 and
# configs3 keep their bounds as they were.
ACC_VS_CPU32, ACC_C = 4.0, 1.0
ACC_EXEMPT = ("configs1", "configs3")

# Kernel families of each plan op at the benchmark's geometry (Engine.last_launches, run-length encoded in plan order): a change in
# which kernels the benchmark runs shows up here as a test change.
FAMILIES = {
    "configs1": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('asm1x1', 2), ('none', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 2), ('none', 1), ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1),
        ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('asm1x1', 1), ('head_decode', 3), ('none', 2),
    ],
    "configs3": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 2),
        ('none', 1), ('asm1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1),
        ('direct1x1', 2), ('none', 1), ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1),
        ('asm1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 1),
        ('head_decode', 3), ('none', 2),
    ],
    "parity_fp32": [
        ('stem', 1), ('igemm_or_halo', 41), ('none', 1), ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 7), ('none', 1),
        ('igemm_or_halo', 23), ('none', 2),
    ],
    "parity_f16x3": [
        ('stem', 1), ('igemm_or_halo', 41), ('none', 1), ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 7), ('none', 1),
        ('igemm_or_halo', 23), ('none', 2),
    ],
    "table_bf16_b16": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3s2', 1), ('igemm_or_halo', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 2), ('none', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 2), ('none', 1), ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1),
        ('igemm_or_halo', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('igemm_or_halo', 2),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('igemm_or_halo', 1), ('head_decode', 3), ('none', 2),
    ],
    "table_bf16_b32": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('igemm_or_halo', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('asm1x1', 1), ('igemm_or_halo', 1), ('none', 1), ('asm1x1', 1), ('igemm_or_halo', 1), ('none', 1), ('asm1x1', 1),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 2), ('none', 1), ('direct1x1', 1),
        ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1), ('igemm_or_halo', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('asm1x1', 1), ('head_decode', 3), ('none', 2),
    ],
    "table_bf16_b128": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1),
        ('asm1x1', 2), ('none', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1),
        ('pl3x3', 1), ('direct1x1', 2), ('none', 1), ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1),
        ('direct1x1', 2), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1),
        ('direct1x1', 1), ('pl3x3', 1), ('direct1x1', 1), ('pl3x3', 1), ('asm1x1', 1), ('head_decode', 3), ('none', 2),
    ],
    "table_fp8_b64": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('direct1x1', 1), ('direct3x3s2', 1), ('direct1x1', 1), ('bottleneck', 4),
        ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1),
        ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1), ('asm1x1', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 2), ('none', 1), ('asm1x1', 2),
        ('none', 1), ('asm1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1),
        ('direct1x1', 2), ('none', 1), ('direct1x1', 1), ('bottleneck', 2), ('direct1x1', 1), ('pl3x3s2', 1), ('direct1x1', 1),
        ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1', 1), ('pl3x3s2', 1),
        ('asm1x1', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('direct1x1_f8out', 1), ('pl3x3_f8', 1), ('asm1x1', 1),
        ('head_decode', 3), ('none', 2),
    ],
    "fp32_b128": [
        ('stem', 1), ('igemm_or_halo', 41), ('none', 1), ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 7), ('none', 1),
        ('igemm_or_halo', 23), ('none', 2),
    ],
    "bf16_b448": [
        ('stem', 1), ('downblock', 1), ('bottleneck', 2), ('igemm_or_halo', 3), ('bottleneck', 4), ('igemm_or_halo', 24), ('none', 1),
        ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 7), ('none', 1), ('igemm_or_halo', 1), ('bottleneck', 2),
        ('igemm_or_halo', 15), ('head_decode', 3), ('none', 2),
    ],
    "configs4": [
        ('none', 1), ('igemm_or_halo', 70), ('none', 1), ('igemm_or_halo', 2), ('none', 1), ('igemm_or_halo', 11), ('none', 1),
        ('igemm_or_halo', 32), ('head_decode', 3), ('none', 2),
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


def _fp32(t):
    return t.float().double()


class _Setup:
    def __init__(self, name):
        import bench
        from aquaculture_amd import checkpoint
        from aquaculture_amd.engine import Engine
        e = CONFIGS[name]
        self.name, self.entry, self.B, self.size, self.sample = name, e, e.batch, e.size, e.sample
        self.precision = e.precision
        self.fp32_grade = e.precision in ("fp32", "f16x3")
        self.rnd = _fp32 if self.fp32_grade else _bf16           # how the engine stores activations and conv weights
        self.tol = CONV_TOL[e.precision]
        self.windowed = e.size >= 1280                          # conv references on windows (oracle/windowed_ref.py)
        self.ck = checkpoint.synthetic_checkpoint(e.variant, 5)
        self.x = torch.from_numpy(bench.make_tiles(0, self.B, 1, e.size)[0]).cuda()
        if self.fp32_grade:                                     # bench.py's parity legs
            self.eng = Engine(self.ck, e.precision, 0)
        else:                                                   # bench.py's main engine
            self.eng = Engine(self.ck, e.precision, 0, fused_stem=True, fused_bottleneck=e.precision in ("bf16", "fp8w", "fp8"),
                              fp8_calibration=self.x[:min(self.B, 16)] if e.precision == "fp8" else None)
        if e.tuning is not None:
            self.eng.autotune(self.x, cache=None, shipped=True)
        assert getattr(self.eng, "tuned_from", None) == e.tuning, "the kernels its user runs, not a fresh timing"
        self.packed = {}
        ci = 0
        packed = checkpoint.pack_plan_weights(self.ck, self.eng.plan, "native")
        for i, o in enumerate(self.eng.plan.ops):
            if o.kind in (OP_CONV, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK):
                self.packed[i] = packed[ci]
                ci += 1
        # fp8 pairs: producer op -> scale of the codes it writes, consumer op -> scale of the codes it reads
        self.f8_scale, self.f8_producer = {}, {}
        for prod, cons in self.eng.fp8_pairs():
            s = self.eng.fp8_scales.get(self.eng.plan.ops[cons].name)
            if s:
                self.f8_scale[prod] = self.f8_scale[cons] = float(s)
                self.f8_producer[cons] = prod

    def slice_view(self, s, dtype=None, B=None):
        """Device view of plan slice `s` [B, h, w, C] (the input tensor: the tiles); dtype uint8 = the e4m3 codes of an fp8 slice."""
        B = self.B if B is None else B
        if s.tensor == self.eng.plan.input_tensor:
            return self.x[:B]
        t = self.eng.tensor(s.tensor, B)
        if dtype == torch.uint8:                      # codes in the first bytes of each pixel's bf16 slot
            return t.view(torch.uint8)[..., 2 * s.ch_off:2 * s.ch_off + s.channels]
        return t[..., s.ch_off:s.ch_off + s.channels]

    def tile_pixels(self, launch):
        """Pixel-tile width (bn) of a conv launch (family, cfg): the implicit-GEMM / halo tiles walk the flattened [B, h, w] pixel range
        in steps of bn (aq_conv_config_tiles).  The windowed checks run on those families only."""
        import ctypes as C
        bm, bn = C.c_int(), C.c_int()
        assert launch[0] == "igemm_or_halo" and self.eng.lib.aq_conv_config_tiles(launch[1], C.byref(bm), C.byref(bn)) == 0, \
            f"no pixel-tile geometry for {launch}"
        return bn.value


@pytest.fixture(scope="module", params=list(CONFIGS))
def setup(request, lib):
    import bench
    threads = torch.get_num_threads()
    torch.set_num_threads(bench.host_threads())     # the references' fp64 GEMMs: more threads than the host really has cost 10x
    t0 = time.perf_counter()
    s = _Setup(request.param)
    print(f"\n{s.name} ({s.entry.built_as}): {s.entry.variant} {s.precision} batch {s.B} {s.size} px, tile configs "
          f"{getattr(s.eng, 'tuned_from', 'heuristic (no autotune)')}; engine built in {time.perf_counter() - t0:.1f} s")
    yield s
    s.eng.close()
    torch.set_num_threads(threads)


def _upstream(plan):
    """Per op: every op whose output it reads, directly or through other ops (last writer of each channel slice, in plan order)."""
    writers, ups = {}, []
    for i, o in enumerate(plan.ops):
        deps = set()
        if o.kind in (OP_DECODE, OP_NMS):                # the head outputs / the candidate list: everything before
            deps = set(range(i))
        for sl in (o.src, o.res):
            if sl is None or sl.tensor < 0:
                continue
            for lo, hi, j in writers.get(sl.tensor, []):
                if lo < sl.ch_off + sl.channels and sl.ch_off < hi:
                    deps |= {j} | ups[j]
        ups.append(deps)
        if o.dst is not None and o.dst.tensor >= 0:
            d = o.dst
            keep = [w for w in writers.get(d.tensor, []) if not (d.ch_off <= w[0] and w[1] <= d.ch_off + d.channels)]
            writers[d.tensor] = keep + [(d.ch_off, d.ch_off + d.channels, i)]
    return ups


# ---------------------------------------------------------------------------------------------------------------------------------
# references (fp64, CPU) on one op's snapshot of its inputs
def _conv_ref(x, w_krsc, b, stride, pad, act, res=None, scale=None, dtype=torch.float64):
    """x: [n, h, w, cin] float64 values the kernel reads; w_krsc: the values the kernel multiplies (already rounded); scale: per-Cout
    factor of an fp8 consumer (act scale x weight scale).  dtype float32: the same op computed in fp32 on the CPU."""
    w = torch.as_tensor(w_krsc).to(dtype).permute(0, 3, 1, 2)
    y = F.conv2d(_nchw(x.to(dtype)), w, None, stride=stride, padding=pad)
    if scale is not None:
        y = y * scale.to(dtype).view(1, -1, 1, 1)
    y = y + torch.as_tensor(b).to(dtype).view(1, -1, 1, 1)
    if act:
        y = F.silu(y)
    y = _nhwc(y)
    if res is not None:
        y = y + res.to(dtype)
    return y


def _accumulation_evidence(setup, conv, x, w, b, act, scale, res, got, ref, rel, abs_):
    """For a conv that exceeds its CONV_TOL bound: is the excess the op's own fp32 accumulation?  conv(x, w, b, act, res, scale, dtype)
    computes the op on the snapshot.  Returns (ok, note): the kernel's max error against fp64, the same op computed in fp32 on the CPU
    (stored as the engine stores it) against fp64, K, and the worst error in units of 2^-24 sqrt(K) sum |x w|."""
    cpu = setup.rnd(conv(x, w, b, act, res, scale, torch.float32).double())
    e_cpu = float((cpu - ref).abs().max())
    err = (got - ref).abs()
    K = int(np.prod(tuple(torch.as_tensor(w).shape[1:])))
    mag = conv(x.abs(), torch.as_tensor(w).abs(), torch.as_tensor(b).abs(), False, None, None if scale is None else scale.abs(),
               torch.float64)
    acc = 2.0 ** -24 * K ** 0.5 * mag
    units = float(((err - rel * ref.abs() - abs_).clamp(min=0) / acc.clamp(min=1e-30)).max())    # the excess over CONV_TOL
    ok = bool((err <= rel * ref.abs() + abs_ + ACC_C * acc).all()) and float(err.max()) <= ACC_VS_CPU32 * max(e_cpu, 1e-30)
    return ok, (f"K = {K}: max err {float(err.max()):.3g}, fp32 CPU {e_cpu:.3g} (ratio {float(err.max()) / max(e_cpu, 1e-30):.2f}, "
                f"limit {ACC_VS_CPU32:g}), excess over the bound at most {units:.2f} x 2^-24 sqrt(K) sum|xw| (limit {ACC_C:g})")


def _err_report(got, ref, rel, abs_):
    """(ok, max err, mean err, worst (image slot, y, x, c), ratio) of |got - ref| against rel |ref| + abs."""
    err = (got - ref).abs()
    ratio = err / (rel * ref.abs() + abs_)
    k = int(torch.argmax(ratio))
    idx = np.unravel_index(k, tuple(ratio.shape))
    return bool((ratio <= 1).all()), float(err.max()), float(err.mean()), idx, float(ratio.max())


def _decode_ref(setup, xs_by_level, head_ops, sample):
    """fp64 head conv + decode of every level for the sampled images -> per image: {cand index: row (xywh px, obj, cls)}."""
    ck = setup.ck
    na, no = ck.na, ck.nc + 5
    anchors = ck.anchor_grid_px()
    out = [dict() for _ in sample]
    off = 0
    for lvl, oi in enumerate(head_ops):
        x = xs_by_level[lvl]                                          # [n, ny, nx, cin] float64
        n, ny, nx, cin = x.shape
        pc = setup.packed[oi]
        w = setup.rnd(torch.from_numpy(pc.weight[:na * no, 0, 0, :]))  # (head rows past na * no are padding)
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


def _check_candidates(setup, ref_rows, cand, rows, counts, sample):
    """Same candidate set as the fp64 reference (but for candidates within 1e-4 of the threshold), rows within 1e-3 relative (bf16
    engines) or within north_star's gate (fp32-grade engines: boxes within 1e-4 x tile px, objectness and class scores within 1e-4)."""
    msgs, stats = [], []
    for j, img in enumerate(sample):
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
        if setup.fp32_grade:
            bound = torch.full_like(r, 1e-4)
            bound[:, :4] = 1e-4 * setup.size
        else:
            bound = 1e-3 * r.abs() + 1e-6
        stats.append((float(err.max()) if n else 0.0, float(err.mean()) if n else 0.0))
        if n and not (err <= bound).all():
            k = int(torch.argmax(err / bound))
            cidx, col = divmod(k, r.shape[1])
            msgs.append(f"image {img}: candidate {int(got[cidx])} column {col}: {float(g[cidx, col])} vs fp64 {float(r[cidx, col])}")
    return msgs, stats


# ---------------------------------------------------------------------------------------------------------------------------------
def _conv_weights(setup, i, fam, src_codes):
    """(input transform, weights the kernel multiplies, per-Cout scale or None) of conv op i as it ran (family fam)."""
    pc = setup.packed[i]
    if fam[0] == "pl3x3_f8":
        s_act = setup.f8_scale[i]
        wf = torch.from_numpy(pc.weight).float()
        ws = wf.abs().amax(dim=(1, 2, 3)) / 448.0
        ws = torch.where(ws > 0, ws, torch.ones_like(ws))
        w = (wf / ws.view(-1, 1, 1, 1)).to(torch.float8_e4m3fn).double()
        assert src_codes
        return (lambda t: t.view(torch.float8_e4m3fn).double()), w, s_act * ws.double()
    assert fam[0] in ("igemm_or_halo", "pl3x3", "pl3x3s2", "direct1x1", "asm1x1", "direct3x3s2"), fam
    assert not src_codes, "a bf16 consumer of e4m3 codes"
    return (lambda t: t.double()), setup.rnd(torch.from_numpy(pc.weight)), None


def _preprocess_ref(setup, u8):
    """OP_PREPROCESS, bit-exact: space-to-depth of u8 / 255 in fp32, channel (dy*2 + dx)*3 + c, channels 12-15 zero, stored rounded."""
    n, H, W, _ = u8.shape
    v = (u8.float() / 255.0).view(n, H // 2, 2, W // 2, 2, 3).permute(0, 1, 3, 2, 4, 5).reshape(n, H // 2, W // 2, 12)
    v = torch.cat([v, torch.zeros((n, H // 2, W // 2, 4))], -1)
    return setup.rnd(v)


def _stepping_pass(setup, check, keep, B=None, sample=None, keep_images=None):
    """One pass over the plan, op by op, on the first B tiles.  check: compare every op with its fp64 reference on the images `sample`
    (returns failures and the per-op table); keep: full-batch copies of every op's output on the device (returns them), of the first
    keep_images images only if given."""
    from oracle import windowed_ref as WR
    B = setup.B if B is None else B
    sample = setup.sample if sample is None else sample
    x_in = setup.x[:B]
    eng, plan = setup.eng, setup.eng.plan
    dets = torch.zeros((B, MAX_DET, 6), dtype=torch.float32, device="cuda")
    counts = torch.zeros((B,), dtype=torch.int32, device="cuda")
    idx = torch.tensor(sample, device="cuda")
    head_ops = [i for i, o in enumerate(plan.ops) if o.kind == OP_CONV and o.level >= 0]
    seam = (sample[1], sample[2]) if len(sample) == 4 else ()
    head_x, fused_heads, codes_written = {}, None, set()
    failures, table, full = [], [], {}
    t_ref, t_op = 0.0, None                          # host time spent on the references (from the output copy to the next op)
    n_win = 0
    if check and setup.windowed:                     # the kernels (and tile shapes) this batch size launches, for the windows' tile seams
        eng.infer(x_in, CONF, IOU, MAX_DET)
        launches = eng.last_launches()
    for i, op in enumerate(plan.ops):
        if t_op is not None:
            t_ref += time.perf_counter() - t_op
            t_op = None
        src_codes = setup.f8_producer.get(i) in codes_written
        windowed = setup.windowed and op.kind == OP_CONV and op.level < 0
        pre, wins = {}, None
        if check and windowed:
            # only the input region each window reads, cut out on the device (a whole 640 x 640 x 160 plane is 131 MB per image)
            H, W = setup.slice_view(op.src, B=B).shape[1:3]
            Ho, Wo = setup.slice_view(op.dst, B=B).shape[1:3]
            wins = WR.pick_windows(B, Ho, Wo, sample, bn=setup.tile_pixels(launches[i]), seam=seam, seed=i)
            sv = setup.slice_view(op.src, B=B)
            rv = setup.slice_view(op.res, B=B) if op.res is not None and op.res.tensor >= 0 else None
            pre["win"] = []
            for w in wins:
                r = WR.input_region(w, op.k, op.stride, op.pad, H, W)
                xr = sv[w.image, r.y0:r.y1, r.x0:r.x1].contiguous().cpu()
                rr = rv[w.image, w.y0:w.y1, w.x0:w.x1].contiguous().cpu() if rv is not None else None
                pre["win"].append((w, r, xr, rr))
        elif check and op.src is not None and op.kind != OP_NMS:
            pre["src"] = setup.slice_view(op.src, torch.uint8 if src_codes else None, B=B)[idx].cpu()
            if op.res is not None and op.res.tensor >= 0:
                pre["res"] = setup.slice_view(op.res, B=B)[idx].cpu()
        if check and op.kind == OP_NMS:
            c, r, n = eng.candidates(B)
            pre["cand"], pre["rows"], pre["counts"] = c[idx].cpu(), r[idx].cpu(), n[idx].cpu()
        eng.run_ops(x_in, i, i + 1, CONF, IOU, MAX_DET, out=(dets, counts))
        fam = eng.last_launches()[i]
        dst_codes = fam[0] == "direct1x1_f8out"
        if dst_codes:
            codes_written.add(i)
        is_head = op.kind == OP_CONV and op.level >= 0
        if is_head:
            fused_heads = fam[0] == "head_decode"
        cand_op = (is_head and fused_heads and i == head_ops[-1]) or (op.kind == OP_DECODE and not fused_heads)
        if keep:
            nk = B if keep_images is None else keep_images
            if cand_op:
                c, r, n = eng.candidates(B)
                full[i] = (c[:nk].clone(), r[:nk].clone(), n[:nk].clone())
            elif op.kind == OP_NMS:
                full[i] = (dets[:nk].clone(), counts[:nk].clone())
            elif op.dst is not None and not (is_head and fused_heads):
                full[i] = setup.slice_view(op.dst, torch.uint8 if dst_codes else None, B=B)[:nk].clone()
        if not check:
            continue
        t_op = time.perf_counter()
        label = f"op {i} {op.name} ({fam[0]}, cfg {fam[1]})"
        if is_head:
            head_x[op.level] = pre["src"].double()
            if fused_heads:
                if i != head_ops[-1]:
                    continue
        if cand_op:
            ref_rows = _decode_ref(setup, [head_x[l] for l in range(3)], head_ops, sample)
            c, r, n = eng.candidates(B)
            msgs, stats = _check_candidates(setup, ref_rows, c[idx].cpu(), r[idx].cpu(), n[idx].cpu(), sample)
            failures += [f"{label}: {m}" for m in msgs]
            mx = max([s[0] for s in stats], default=0.0)
            table.append((i, "model.24.m.0-2 + decode" if fused_heads else op.name, fam, mx,
                          float(np.mean([s[1] for s in stats])) if stats else 0.0))
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
            assert fam[0] == "none", f"{label}: the engine decodes behind the head convs"
            continue
        rel, abs_ = setup.tol
        if windowed:
            xf, w, scale = _conv_weights(setup, i, fam, src_codes)
            pc = setup.packed[i]
            dv = setup.slice_view(op.dst, B=B)
            errs, worst, evidence = [], None, []
            for w_, r, xr, rr in pre["win"]:
                got = dv[w_.image, w_.y0:w_.y1, w_.x0:w_.x1].contiguous().cpu().double()
                res_w = rr.double() if rr is not None else None
                ref = WR.conv_window(xf(xr), r, w, pc.bias, op.stride, op.act, res=res_w, scale=scale)
                ok, mx, mean, k, ratio = WR.compare(got, ref, rel, abs_)
                errs.append((mx, mean, got.numel()))
                if not ok and setup.name not in ACC_EXEMPT:
                    def conv(x_, w2, b2, act, res_, sc, dt, r=r):
                        return WR.conv_window(x_, r, w2, b2, op.stride, act, res=res_, scale=sc, dtype=dt)
                    acc_ok, note = _accumulation_evidence(setup, conv, xf(xr), w, pc.bias, op.act, scale, res_w, got, ref, rel, abs_)
                    evidence.append((acc_ok, f"window '{w_.tag}' of image {w_.image}: {ratio:.2f} x the bound; {note}"))
                    ratio = ratio if not acc_ok else 0.0
                if worst is None or ratio > worst[0]:
                    worst = (ratio, w_, k, float(got[k]), float(ref[k]), mx)
            n_win += len(pre["win"])
            mx = max(e[0] for e in errs)
            mean = sum(e[1] * e[2] for e in errs) / sum(e[2] for e in errs)
            table.append((i, op.name, fam, mx, mean))
            for acc_ok, note in evidence:
                print(f"  {label}: {'accumulation' if acc_ok else 'NOT accumulation'}: {note}")
            if worst[0] > 1:
                ratio, w_, k, g, rf, _ = worst
                failures.append(f"{label}: max err {mx:.3g} ({ratio:.2f} x the bound {rel:.3g} |ref| + {abs_:g}); worst in window "
                                f"'{w_.tag}' of image {w_.image} at (y {w_.y0 + k[0]}, x {w_.x0 + k[1]}, c {k[2]}): {g} vs fp64 {rf}")
            continue
        got = setup.slice_view(op.dst, torch.uint8 if dst_codes else None, B=B)[idx].cpu()
        mean_lim, exact = None, False
        if op.kind == OP_PREPROCESS:
            ref, exact = _preprocess_ref(setup, pre["src"]), True
        elif op.kind == OP_SPPF_POOL:
            x = pre["src"].double()
            ys, y = [], _nchw(x)
            for _ in range(3):
                y = F.max_pool2d(y, 5, 1, 2)
                ys.append(y)
            ref, exact = _nhwc(torch.cat(ys, 1)), True
        elif op.kind == OP_UPSAMPLE2X:
            ref, exact = pre["src"].double().repeat_interleave(2, 1).repeat_interleave(2, 2), True
        elif op.kind == OP_STEM:
            x = setup.rnd((pre["src"].float() / 255.0).double())         # the stem's x / 255 in fp32, then stored
            pc = setup.packed[i]
            ref = _conv_ref(x, setup.rnd(torch.from_numpy(pc.weight)), pc.bias, op.stride, op.pad, op.act)
        elif op.kind == OP_BOTTLENECK:
            assert not setup.fp32_grade, label
            c = op.src.channels
            pc = setup.packed[i]
            w1 = _bf16(torch.from_numpy(pc.weight[:c * c]).view(c, 1, 1, c))
            w2 = _bf16(torch.from_numpy(pc.weight[c * c:]).view(c, 3, 3, c))
            x = pre["src"].double()
            t = _bf16(_conv_ref(x, w1, pc.bias[:c], 1, 0, True))
            ref = _conv_ref(t, w2, pc.bias[c:], 1, 1, True, res=x if op.res is not None and op.res.tensor >= 0 else None)
            abs_, mean_lim = 2e-2, 3e-3
        elif op.kind == OP_DOWNBLOCK:
            assert not setup.fp32_grade, label
            pc = setup.packed[i]
            ci, cm = op.src.channels, op.dst.channels
            wa = _bf16(torch.from_numpy(pc.weight[:cm * 9 * ci]).view(cm, 3, 3, ci))
            wb = _bf16(torch.from_numpy(pc.weight[cm * 9 * ci:]).view(cm, 1, 1, cm))
            t = _bf16(_conv_ref(pre["src"].double(), wa, pc.bias[:cm], 2, 1, True))
            ref = _conv_ref(t, wb, pc.bias[cm:], 1, 0, True)
            abs_, mean_lim = 2e-2, 3e-3
        elif op.kind == OP_CONV and dst_codes:
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
            xf, w, scale = _conv_weights(setup, i, fam, src_codes)
            pc = setup.packed[i]
            conv_args = (xf(pre["src"]), w, pc.bias, op.act, scale, pre["res"].double() if "res" in pre else None)
            ref = _conv_ref(xf(pre["src"]), w, pc.bias, op.stride, op.pad, op.act, res=conv_args[5], scale=scale)
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
        if not ok and op.kind == OP_CONV and setup.name not in ACC_EXEMPT:
            def conv(x_, w2, b2, act, res_, sc, dt):
                return _conv_ref(x_, w2, b2, op.stride, op.pad, act, res=res_, scale=sc, dtype=dt)
            xv, wv, bv, act, sc, rv = conv_args
            ok, note = _accumulation_evidence(setup, conv, xv, wv, bv, act, sc, rv, got, ref, rel, abs_)
            print(f"  {label}: {ratio:.2f} x the bound, {'accumulation' if ok else 'NOT accumulation'}: {note}")
        if not ok or (mean_lim is not None and mean >= mean_lim):
            failures.append(f"{label}: max err {mx:.3g} ({ratio:.2f} x the bound {rel:.3g} |ref| + {abs_:g}), mean {mean:.3g}"
                            f"{'' if mean_lim is None else f' (limit {mean_lim:g})'}; worst at (image {sample[k[0]]}, y {k[1]}, x {k[2]}, "
                            f"c {k[3]}): {float(got[k])} vs fp64 {float(ref[k])}")
    if t_op is not None:
        t_ref += time.perf_counter() - t_op
    torch.cuda.synchronize()
    return failures, table, full, (dets, counts), (t_ref, n_win)


def _print_table(table):
    print(f"{'op':>4} {'name':<28} {'family':<16} {'cfg':>5} {'max err':>10} {'mean err':>10}")
    for i, name, fam, mx, mean in table:
        print(f"{i:>4} {name:<28} {fam[0]:<16} {fam[1]:>5} {mx:>10.3g} {mean:>10.3g}")


def _same_output(a, b, n_img):
    """Bit-identity of one op's kept outputs on images [0, n_img): a tensor, a candidate list (same set per image, any order: atomics)
    or the NMS detections and counts.  Returns (same, the images that differ where known)."""
    if isinstance(a, tuple) and len(a) == 3:
        ca, ra, na_ = a
        cb, rb, nb = b
        if not torch.equal(na_[:n_img], nb[:n_img]):
            return False, torch.nonzero(na_[:n_img] != nb[:n_img]).flatten().tolist()
        for j in range(n_img):
            n = int(na_[j])
            oa, ob = torch.argsort(ca[j, :n]), torch.argsort(cb[j, :n])
            if not (torch.equal(ca[j, :n][oa], cb[j, :n][ob]) and torch.equal(ra[j, :n][oa], rb[j, :n][ob])):
                return False, [j]
        return True, []
    if isinstance(a, tuple):
        if not torch.equal(a[1][:n_img], b[1][:n_img]):
            return False, torch.nonzero(a[1][:n_img] != b[1][:n_img]).flatten().tolist()
        bad = [j for j in range(n_img) if not torch.equal(a[0][j, :a[1][j]], b[0][j, :a[1][j]])]
        return not bad, bad
    a, b = a[:n_img], b[:n_img]
    if torch.equal(a, b):
        return True, []
    return False, torch.nonzero((a != b).reshape(a.shape[0], -1).any(1)).flatten().tolist()


def test_bench_path_layer_by_layer(setup):
    """Per-op fp64 references on the sampled images, run-to-run bit-identity of every op's full output, and stepping == infer."""
    eng, B = setup.eng, setup.B
    t0 = time.perf_counter()
    failures, table, full1, _, (t_ref, n_win) = _stepping_pass(setup, check=True, keep=True)
    t1 = time.perf_counter()
    fams = eng.last_launches()
    print(f"\n{setup.name}: B = {B}, images {setup.sample}: stepping pass with fp64 references {t1 - t0:.1f} s "
          f"(references {t_ref:.1f} s on {torch.get_num_threads()} threads{f', {n_win} windows' if n_win else ''})")
    _print_table(table)
    print(f"families: {_rle([f for f, _ in fams])}")
    worst = max(table, key=lambda r: r[3])
    print(f"{setup.name}: worst op {worst[0]} {worst[1]} ({worst[2][0]}, cfg {worst[2][1]}) max err {worst[3]:.3g}")
    assert not failures, "\n".join(failures)

    # the family list (what the engine runs)
    assert _rle([f for f, _ in fams]) == FAMILIES[setup.name], _rle([f for f, _ in fams])
    assert all(f != "none" for (f, _), o in zip(fams, eng.plan.ops) if o.kind in (OP_CONV, OP_STEM, OP_BOTTLENECK, OP_DOWNBLOCK))
    if eng.precision_name == "fp8":
        pairs = eng.fp8_pairs()
        assert len(pairs) == 14 and all(fams[c][0] == "pl3x3_f8" and fams[p][0] == "direct1x1_f8out" for p, c in pairs)
    if setup.name == "configs4":             # as tests/test_gpu_baseline_configs.py::test_configs4_yolov5x_bf16_at_batch_16_1280px
        ops3 = [i for i, o in enumerate(eng.plan.ops) if o.kind == OP_CONV and o.k == 3]
        assert len(ops3) >= 49 and {fams[i][0] for i in ops3} <= {"igemm_or_halo", "pl3x3", "pl3x3s2", "direct3x3s2"}

    # layer-level determinism: the whole pass again, every op's full output bit-identical (a race names its op here)
    _, _, full2, (d2, c2), _ = _stepping_pass(setup, check=False, keep=True)
    for i, op in enumerate(eng.plan.ops):
        if i not in full1:
            continue
        same, bad = _same_output(full1[i], full2[i], B)
        if not same:
            pytest.fail(f"op {i} {op.name} ({fams[i][0]}, cfg {fams[i][1]}) changed between two identical passes (images {bad[:8]}"
                        f"{' ...' if len(bad) > 8 else ''}): the first op whose output is not run-to-run deterministic")
    del full1, full2

    # stepping == one infer call: same detections, counts and kernels
    d1, c1 = eng.infer(setup.x, CONF, IOU, MAX_DET)
    torch.cuda.synchronize()
    assert torch.equal(c1, c2)
    for j in range(B):
        assert torch.equal(d1[j, :c1[j]], d2[j, :c2[j]]), j
    assert eng.last_launches() == fams
    print(f"{setup.name}: determinism + stepping == infer {time.perf_counter() - t1:.1f} s; total {time.perf_counter() - t0:.1f} s")


def test_ragged_last_batch(setup):
    """The first B' (odd) tiles as a batch of their own -- a sweep's ragged last batch, on the same tuned table: every op that launches
    what the full batch launches, and whose upstream ops do too, gives the full batch's outputs bit for bit on those images; every op,
    fallbacks included, matches fp64 on image B' - 1 (the tail of every kernel's pixel-tile walk)."""
    eng, B, Bp = setup.eng, setup.B, setup.entry.ragged
    t0 = time.perf_counter()
    _, _, fullB, _, _ = _stepping_pass(setup, check=False, keep=True, keep_images=Bp)
    famB = eng.last_launches()
    t1 = time.perf_counter()
    failures, table, fullR, _, (t_ref, n_win) = _stepping_pass(setup, check=True, keep=True, B=Bp, sample=[Bp - 1])
    famR = eng.last_launches()
    t2 = time.perf_counter()
    print(f"\n{setup.name}: ragged batch B' = {Bp} of {B}, image {Bp - 1}: full pass {t1 - t0:.1f} s, stepping pass with fp64 references "
          f"{t2 - t1:.1f} s (references {t_ref:.1f} s{f', {n_win} windows' if n_win else ''})")
    changed = [i for i in range(len(famB)) if famB[i] != famR[i]]
    print(f"ops launching other kernels at B' = {Bp}: "
          f"{[(i, eng.plan.ops[i].name, famB[i], famR[i]) for i in changed] if changed else 'none'}")
    _print_table(table)
    assert not failures, "\n".join(failures)
    ups = _upstream(eng.plan)
    n_same = 0
    for i, op in enumerate(eng.plan.ops):
        if i not in fullB or i in changed or ups[i] & set(changed):
            continue
        same, bad = _same_output(fullB[i], fullR[i], Bp)
        if not same:
            pytest.fail(f"op {i} {op.name} ({famR[i][0]}, cfg {famR[i][1]}): images {bad[:8]} of a batch of {Bp} differ from the same images "
                        f"in the batch of {B}, on the same kernels: the first op whose output depends on the batch size")
        n_same += 1
    print(f"{setup.name}: {n_same} ops bit-identical to the full batch on images [0, {Bp}); total {time.perf_counter() - t0:.1f} s")
    excluded = [i for i in fullB if i in changed or ups[i] & set(changed)]
    assert n_same + len(excluded) == len(fullB) and (n_same > 0 or changed)


def test_bottleneck_form_follows_its_guard(setup):
    """Which build each Bottleneck launch ran (aq_engine_last_launch's cfg: 1 = generated assembly, 0 = HIP source) at the full and the
    ragged batch equals the assembly builds' guard (32-bit offsets: input under 2^30 bytes, output under 2^31), so the switch points --
    bf16_b448: model.2.m.0 at 219, the other assembly-eligible launches at 437 -- are asserted, not inferred from the family list."""
    from oracle.guards import btl_asm_fits
    eng, plan = setup.eng, setup.eng.plan
    ops = [(i, o) for i, o in enumerate(plan.ops) if o.kind == OP_BOTTLENECK]
    forms = {}
    for Bx in (setup.B, setup.entry.ragged):
        eng.infer(setup.x[:Bx], CONF, IOU, MAX_DET)
        torch.cuda.synchronize()
        fams = eng.last_launches()
        for i, o in ops:
            h = setup.size // plan.tensors[o.src.tensor].down
            want = int(btl_asm_fits(o.src.channels, Bx, h, h, plan.tensors[o.src.tensor].channels, plan.tensors[o.dst.tensor].channels))
            assert fams[i] == ("bottleneck", want), (o.name, Bx, fams[i], want)
            forms[(o.name, Bx)] = want
    print(f"\n{setup.name}: Bottleneck forms (1 = assembly) {forms}")
    if setup.name == "bf16_b448":
        assert forms[("model.2.m.0", 448)] == 0 and forms[("model.2.m.1", 448)] == 0 and forms[("model.4.m.1", 448)] == 1
        assert all(forms[(o.name, 217)] == 1 for _, o in ops)


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
    variant, precision, B, size = CONFIGS["configs1"][:4]
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
