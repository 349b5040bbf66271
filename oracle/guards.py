"""Size guards of the HIP launchers restated in Python, so that tests derive their batch limits from the formulas instead of copying
numbers (and catch a launcher whose guard drifts from what it documents).  Host arithmetic only.

Three parts:
  * one line per predicate of csrc/size_guards.h, under the same name (tests/test_size_guards.py compares the two at every edge);
  * PLAN_TERMS: which predicates the engine's batch check (plan_unfit_op in csrc/engine.cpp) applies to each op family;
  * PARENT_PLAN_TERMS: the limits plan_unfit_op wrote out itself before it called the predicates, kept to show that handing the check to
    the launchers' predicates moved no limit an engine can reach (B <= 65535).
"""

B23, B24, B30, B31, B32 = 1 << 23, 1 << 24, 1 << 30, 1 << 31, 1 << 32
BATCH_CAP = 65535                     # plan_unfit_op: the decode and NMS grids


def cdiv(a: int, b: int) -> int:
    return (a + b - 1) // b


def largest(pred, hi: int = 1 << 40) -> int:
    """The largest B in [0, hi] with pred(B), for a predicate that only gets harder to meet as B grows (0: not even B = 1)."""
    lo = 0
    while lo < hi:
        mid = (lo + hi + 1) // 2
        if pred(mid):
            lo = mid
        else:
            hi = mid - 1
    return lo


# ---- csrc/size_guards.h, line for line ----
def btl_tile_w(C): return 32 if C == 16 else 16
def btl_tile_h(C): return 8 if C == 96 else 16
def preprocess_fits(B, H, W): return B * (H // 2) * (W // 2) < B31
def sppf_pool_fits(B, H, W, groups): return B * H * W * groups < B31
def upsample2x_fits(B, H, W, groups): return B * 4 * H * W * groups < B31
def upsample2x_rows_fit(B, H): return B * H < 65536
def tile_bytes_fit(B, H, W): return B * H * W * 3 < (1 << 40)
def stem_out_fits(B, Ho, Wo): return B * Ho * Wo < B31 and B * cdiv(Wo, 64) * cdiv(Ho, 8) < B31
def stem_fits(B, H, W): return B * H * W * 3 < B32 and stem_out_fits(B, H // 2, W // 2)
def down_fits(B, H, W, th): return B * H * W < B31 and B * cdiv(W // 2, 16) * cdiv(H // 2, th) < B30
def downblock_fits(B, H, W): return down_fits(B, H, W, 8)
def conv3x3s2_direct_fits(B, H, W): return down_fits(B, H, W, 4)
def bottleneck_fits(C, B, H, W): return B * H * W < B31 and B * cdiv(W, btl_tile_w(C)) * cdiv(H, btl_tile_h(C)) < B30
def c3tail_cat_fits(B, H, W, cat_ld): return B * H * W * cat_ld * 2 < B31
def conv1x1_direct_fits(npix): return npix < B31
def conv1x1_asm_fits(npix, in_ld, out_ld): return npix * in_ld * 2 < B31 - (1 << 22) and npix * out_ld * 2 < B32 - (1 << 22)
def pl3x3_index_fits(B, H, W): return B * (H + 1) * (W + 1) + W + 2 < B23
def pl3x3_offsets_fit(B, H, W, out_ld, res_ld): return B * H * W * out_ld * 2 < B31 and B * H * W * res_ld * 2 < B31
def igemm_index_fits(npix, kgroups_pad, G): return npix < B24 and kgroups_pad < (1 << 15) and 0 < G < (1 << 15)
def igemm_tiles_fit(npix, cout, bm, bn): return cdiv(cout, bm) ** 2 * cdiv(npix, bn) < B31
def igemm_fits(npix, kgroups_pad, G, cout, bm, bn): return igemm_index_fits(npix, kgroups_pad, G) and igemm_tiles_fit(npix, cout, bm, bn)
def head_decode_fits(B, ny, nx): return B * ny * nx < B30


def btl_asm_tiles_fit(C, B, H, W, in_ld, out_ld):
    tx = cdiv(W, 16)
    tpi = tx * cdiv(H, btl_tile_h(C))
    nt = tpi * B
    return tx >= 2 and tpi >= 2 and nt < B24 and nt * tpi < B32 and B * H * W * in_ld * 2 < B30 and B * H * W * out_ld * 2 < B31


def pl3x3s2_fits(B, H, W, in_ld, out_ld):
    return (pl3x3_index_fits(B, H // 2, W // 2) and B * (H // 2) * (W // 2) * out_ld * 2 < B31 and B * H * W * in_ld * 2 < B31
            and in_ld * 2 < B24)


def pl3x3_f8_offsets_fit(B, H, W, in_ld_bytes, out_ld, res_ld):
    return pl3x3_offsets_fit(B, H, W, out_ld, res_ld) and B * H * W * in_ld_bytes < B31 and in_ld_bytes < B24


def btl_asm_fits(C: int, B: int, H: int, W: int, in_ld: int, out_ld: int) -> bool:
    """csrc/bottleneck.hip btl_asm_fits with its switches at their defaults: does aq_bottleneck run a generated-assembly build (C = 48:
    16 x 16 tiles, C = 96: 8 x 16)?"""
    return C in (48, 96) and btl_asm_tiles_fit(C, B, H, W, in_ld, out_ld)


# ---- the engine's batch check, per op family ----
# g: the op's geometry at one tile size -- H, W (network input), hs, ws / hd, wd (source / destination tensor), ld_s, ld_d, ld_r (row
# lengths in elements; ld_r = 0: no residual), c_src, cout, groups (16-byte groups of the source slice), kgroups_pad, G and bm, bn (the
# implicit-GEMM packing and tile shape).  The planar 3x3/s2 entry leaves out aq_conv3x3_pl_s2_supported's region-row test, which both
# versions ask of the library itself.
PLAN_TERMS = {
    "preprocess": lambda B, g: preprocess_fits(B, g["H"], g["W"]),
    "stem": lambda B, g: stem_fits(B, g["H"], g["W"]),
    "downblock": lambda B, g: downblock_fits(B, g["hs"], g["ws"]),
    "bottleneck": lambda B, g: bottleneck_fits(g["c_src"], B, g["hs"], g["ws"]),
    "sppf_pool": lambda B, g: sppf_pool_fits(B, g["hs"], g["ws"], g["groups"]),
    "upsample2x": lambda B, g: upsample2x_rows_fit(B, g["hs"]) and upsample2x_fits(B, g["hs"], g["ws"], g["groups"]),
    "head_decode": lambda B, g: head_decode_fits(B, g["hd"], g["wd"]),
    "conv1x1_direct": lambda B, g: conv1x1_direct_fits(B * g["hd"] * g["wd"]),
    "conv1x1_asm": lambda B, g: conv1x1_asm_fits(B * g["hd"] * g["wd"], g["ld_s"], g["ld_d"]),
    "conv3x3s2_direct": lambda B, g: conv3x3s2_direct_fits(B, g["hs"], g["ws"]),
    "pl3x3": lambda B, g: pl3x3_index_fits(B, g["hs"], g["ws"]) and pl3x3_offsets_fit(B, g["hs"], g["ws"], g["ld_d"], g["ld_r"]),
    "pl3x3s2": lambda B, g: pl3x3s2_fits(B, g["hs"], g["ws"], g["ld_s"], g["ld_d"]),
    "igemm": lambda B, g: igemm_fits(B * g["hd"] * g["wd"], g["kgroups_pad"], g["G"], g["cout"], g["bm"], g["bn"]),
}

# plan_unfit_op's own terms before it called the predicates (the text of the commit before csrc/size_guards.h existed)
PARENT_PLAN_TERMS = {
    "preprocess": lambda B, g: not B * (g["H"] // 2) * (g["W"] // 2) >= B31,
    "stem": lambda B, g: not (B * g["H"] * g["W"] * 3 >= B32 or B * g["hd"] * g["wd"] >= B31),
    "downblock": lambda B, g: not B * g["hs"] * g["ws"] >= B31,
    "bottleneck": lambda B, g: not B * g["hs"] * g["ws"] >= B31,
    "sppf_pool": lambda B, g: not B * g["hs"] * g["ws"] * g["groups"] >= B31,
    "upsample2x": lambda B, g: not B * g["hs"] >= 65536 and not B * 4 * g["hs"] * g["ws"] * g["groups"] >= B31,
    "head_decode": lambda B, g: not B * g["hd"] * g["wd"] >= B30,
    "conv1x1_direct": lambda B, g: B * g["hd"] * g["wd"] < B31,
    "conv1x1_asm": lambda B, g: B * g["hd"] * g["wd"] * g["ld_s"] * 2 < B31 - (1 << 22) and B * g["hd"] * g["wd"] * g["ld_d"] * 2 < B32 - (1 << 22),
    "conv3x3s2_direct": lambda B, g: B * g["hs"] * g["ws"] < B31,
    "pl3x3": lambda B, g: (B * (g["hs"] + 1) * (g["ws"] + 1) + g["ws"] + 2 < B23 and B * g["hd"] * g["wd"] * g["ld_d"] * 2 < B31
                           and B * g["hd"] * g["wd"] * g["ld_r"] * 2 < B31),
    "pl3x3s2": lambda B, g: (B * (g["hs"] // 2 + 1) * (g["ws"] // 2 + 1) + g["ws"] // 2 + 2 < B23       # (aq_conv3x3_pl_s2_supported)
                             and B * g["hd"] * g["wd"] * g["ld_d"] * 2 < B31 and B * g["hs"] * g["ws"] * g["ld_s"] * 2 < B31),
    "igemm": lambda B, g: B * g["hd"] * g["wd"] < B24,
}


# ---- a plan's ops as guard families (aquaculture_amd/spec.py plans) ----
IGEMM_SMALLEST_TILE = (32, 128)       # the smallest bm and bn of any implicit-GEMM / halo tile shape (aq_conv_config_tiles): the most tiles


def op_families(op, direct_forms: bool = True):
    """The families plan_unfit_op can ask of this op.  A conv: the implicit-GEMM fallback, the fused head + decode of a Detect level and,
    with direct_forms, every direct form its kernel size has (an engine without a tuned table runs none of them)."""
    from aquaculture_amd import spec
    if op.kind == spec.OP_CONV:
        fam = {(1, 1): ["conv1x1_direct", "conv1x1_asm"], (3, 1): ["pl3x3"], (3, 2): ["conv3x3s2_direct", "pl3x3s2"]}.get((op.k, op.stride), [])
        return (fam if direct_forms else []) + ["igemm"] + (["head_decode"] if op.level >= 0 else [])
    return {spec.OP_PREPROCESS: ["preprocess"], spec.OP_STEM: ["stem"], spec.OP_DOWNBLOCK: ["downblock"], spec.OP_BOTTLENECK: ["bottleneck"],
            spec.OP_SPPF_POOL: ["sppf_pool"], spec.OP_UPSAMPLE2X: ["upsample2x"]}.get(op.kind, [])


def op_geometry(plan, op, H: int, W: int, eb: int) -> dict:
    """The `g` of PLAN_TERMS for one op at H x W tiles; eb: bytes per activation element (2: bf16, 4: fp32)."""
    ts, td = plan.tensors[op.src.tensor], plan.tensors[op.dst.tensor]
    G = op.src.channels * eb // 16
    return dict(H=H, W=W, hs=H // ts.down, ws=W // ts.down, hd=H // td.down, wd=W // td.down, ld_s=ts.channels, ld_d=td.channels,
                ld_r=plan.tensors[op.res.tensor].channels if op.res else 0, c_src=op.src.channels, cout=op.dst.channels, groups=G, G=G,
                kgroups_pad=(op.k * op.k * G + 7) // 8 * 8, bm=IGEMM_SMALLEST_TILE[0], bn=IGEMM_SMALLEST_TILE[1])


def plan_batch_limit(plan, H: int, W: int, eb: int):
    """(largest batch the sizing call takes for an engine without a tuned table, name of the first op that sets it; None: the batch cap)."""
    limit, name = BATCH_CAP, None
    for op in plan.ops:
        for fam in op_families(op, direct_forms=False):
            g = op_geometry(plan, op, H, W, eb)
            b = largest(lambda B: PLAN_TERMS[fam](B, g))
            if b < limit:
                limit, name = b, op.name
    return limit, name
