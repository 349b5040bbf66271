"""The launchers' size limits are written once, in csrc/size_guards.h; the launchers, the exported queries and the engine's batch check
(plan_unfit_op) all call those predicates.  CPU only: nothing here launches a kernel.

  * no limit an engine can reach moved when plan_unfit_op handed its own arithmetic to the predicates: for every op of the yolov5m and
    yolov5x plans (their strides, row lengths and channel counts), at square tiles of 32 .. 1024 px, the largest batch under the check's
    earlier terms equals the largest batch under the predicates wherever the earlier limit is at most the 65535 batch cap;
  * every C predicate agrees with its line in oracle/guards.py at its edge and one past it (aq_size_guard, and the exported queries).
"""
import ctypes as C

import pytest

from aquaculture_amd import spec
from oracle import guards

TILES = (32, 64, 320, 640, 1024)
# (variant, fused stem and Bottlenecks, bytes per element): the bf16 plans bench.py runs and the unfused fp32 ones
PLANS = (("yolov5m", True, 2), ("yolov5m", False, 4), ("yolov5x", True, 2), ("yolov5x", False, 4))


def _cases():
    for variant, fused, eb in PLANS:
        plan = spec.build_plan(variant, fused_stem=fused, fused_bottleneck=fused)
        for op in plan.ops:
            for fam in guards.op_families(op):
                for T in TILES:
                    yield f"{variant} {'bf16' if eb == 2 else 'fp32'} {op.name} {fam} {T} px", fam, guards.op_geometry(plan, op, T, T, eb)


def test_no_reachable_limit_moved(lib):
    bm, bn = C.c_int(), C.c_int()
    shapes = []
    for cfg in range(lib.aq_conv_num_configs()):
        assert lib.aq_conv_config_tiles(cfg, C.byref(bm), C.byref(bn)) == 0
        shapes.append((bm.value, bn.value))
    assert guards.IGEMM_SMALLEST_TILE == (min(s[0] for s in shapes), min(s[1] for s in shapes)), shapes
    seen, moved, beyond = set(), [], {}
    for what, fam, g in _cases():
        seen.add(fam)
        old = guards.largest(lambda B: guards.PARENT_PLAN_TERMS[fam](B, g))
        new = guards.largest(lambda B: guards.PLAN_TERMS[fam](B, g))
        assert new <= old, f"{what}: the predicates take {new} images, more than the check's earlier terms ({old})"
        if old != new:
            (moved if old <= guards.BATCH_CAP else beyond.setdefault(fam, [])).append(f"{what}: {old} -> {new}")
    assert seen == set(guards.PLAN_TERMS), set(guards.PLAN_TERMS) - seen
    # families whose limit differs only above the batch cap (DESIGN.md names them): listed, not a failure
    print("limits that differ above the batch cap:", {f: v[:3] for f, v in beyond.items()} or "none")
    assert not moved, "limits at or below the 65535 batch cap moved:\n" + "\n".join(moved) + f"\n(above the cap: {beyond})"
    assert set(beyond) <= {"stem", "downblock", "bottleneck", "conv3x3s2_direct", "pl3x3s2", "igemm"}, beyond


# ---- every predicate of size_guards.h against its Python line ----
# (enum value of include/aq_engine.h, the Python line, the arguments with None where the batch goes, the same with a larger geometry)
SG = {
    "preprocess": (0, guards.preprocess_fits, [(None, 640, 640), (None, 32, 32)]),
    "sppf_pool": (1, guards.sppf_pool_fits, [(None, 20, 20, 48), (None, 1, 1, 80)]),
    "upsample2x": (2, guards.upsample2x_fits, [(None, 20, 20, 48), (None, 2, 2, 40)]),
    "upsample2x_rows": (3, guards.upsample2x_rows_fit, [(None, 40), (None, 1)]),
    "stem": (4, guards.stem_fits, [(None, 640, 640), (None, 32, 32), (None, 2, 2)]),
    "downblock": (5, guards.downblock_fits, [(None, 320, 320), (None, 16, 16), (None, 2, 2)]),
    "conv3x3s2_direct": (6, guards.conv3x3s2_direct_fits, [(None, 160, 160), (None, 8, 8), (None, 2, 2)]),
    "bottleneck": (7, guards.bottleneck_fits, [(48, None, 160, 160), (96, None, 80, 80), (16, None, 1, 1), (96, None, 8, 16)]),
    "btl_asm_tiles": (8, guards.btl_asm_tiles_fit, [(48, None, 160, 160, 96, 48), (48, None, 160, 160, 48, 96), (96, None, 80, 80, 192, 96),
                                                    (96, None, 80, 80, 96, 192), (48, None, 16, 17, 48, 48), (96, None, 8, 32, 96, 96)]),
    "c3tail_cat": (9, guards.c3tail_cat_fits, [(None, 160, 160, 96)]),
    "conv1x1_direct": (10, guards.conv1x1_direct_fits, [(None,)]),
    "conv1x1_asm": (11, guards.conv1x1_asm_fits, [(None, 96, 384), (None, 1536, 384)]),
    "pl3x3_index": (12, guards.pl3x3_index_fits, [(None, 40, 40), (None, 20, 20), (None, 1, 1)]),
    "pl3x3_offsets": (13, guards.pl3x3_offsets_fit, [(None, 40, 40, 192, 0), (None, 40, 40, 192, 384)]),
    "pl3x3s2": (14, guards.pl3x3s2_fits, [(None, 80, 80, 384, 384), (None, 2, 2, 64, 192), (None, 80, 80, 96, 768)]),
    "pl3x3_f8_offsets": (15, guards.pl3x3_f8_offsets_fit, [(None, 40, 40, 384, 192, 0), (None, 40, 40, 384, 192, 384), (None, 20, 20, 768, 96, 0)]),
    "igemm": (16, guards.igemm_fits, [(None, 440, 48, 96, 64, 128), (None, 8, 1, 65536, 64, 128)]),
    "head_decode": (17, guards.head_decode_fits, [(None, 80, 80), (None, 1, 1)]),
    "tile_bytes": (18, guards.tile_bytes_fit, [(None, 640, 640), (None, 32, 32)]),
}


def _c_guard(lib, which, args):
    v = (C.c_longlong * len(args))(*args)
    return lib.aq_size_guard(which, v, len(args))


@pytest.mark.parametrize("name", sorted(SG))
def test_c_predicate_equals_its_python_line(lib, name):
    which, py, shapes = SG[name]
    for shape in shapes:
        at = lambda B: tuple(B if a is None else a for a in shape)
        Bmax = guards.largest(lambda B: py(*at(B)))
        assert 0 < Bmax < 1 << 40, (name, shape, Bmax)
        for B in (1, Bmax - 1, Bmax, Bmax + 1, 2 * Bmax):
            assert _c_guard(lib, which, at(B)) == int(py(*at(B))) == int(B <= Bmax), (name, at(B))
    assert _c_guard(lib, which, at(1)[:-1]) == -1 and _c_guard(lib, which, at(1) + (1,)) == -1, "a wrong argument count must give -1"


def test_size_guard_hook_rejects_unknown_ids(lib):
    v = (C.c_longlong * 6)(1, 1, 1, 1, 1, 1)
    assert lib.aq_size_guard(-1, v, 3) == -1 and lib.aq_size_guard(len(SG), v, 3) == -1 and lib.aq_size_guard(0, None, 3) == -1
    assert sorted(s[0] for s in SG.values()) == list(range(len(SG)))


def test_row_lengths_past_the_pixel_stride_limits_are_refused(lib):
    """The two terms with no batch in them: a planar 3x3/s2 input row of 2^23 elements, an fp8 input row of 2^24 bytes."""
    for ld in ((1 << 23) - 8, 1 << 23):
        assert _c_guard(lib, SG["pl3x3s2"][0], (1, 2, 2, ld, 192)) == int(guards.pl3x3s2_fits(1, 2, 2, ld, 192)) == int(ld < 1 << 23)
    for ld in ((1 << 24) - 16, 1 << 24):
        assert _c_guard(lib, SG["pl3x3_f8_offsets"][0], (1, 2, 2, ld, 192, 0)) == int(guards.pl3x3_f8_offsets_fit(1, 2, 2, ld, 192, 0)) == int(ld < 1 << 24)


# ---- the exported, pure queries against the restatement (shapes of tests/test_gpu_large_offsets.py) ----
@pytest.mark.parametrize("C_,H,in_ld,out_ld", [(48, 160, 96, 48), (48, 160, 48, 96), (96, 80, 96, 192)])
def test_bottleneck_asm_form_query(lib, C_, H, in_ld, out_ld):
    Bmax = guards.largest(lambda B: guards.btl_asm_fits(C_, B, H, H, in_ld, out_ld))
    for B in (Bmax, Bmax + 1):
        assert lib.aq_bottleneck_asm_form(C_, B, H, H, in_ld, out_ld) == int(B <= Bmax), B


@pytest.mark.parametrize("H,in_ld,cat_ld,out_ld", [(160, 48, 96, 96), (160, 96, 96, 96), (80, 48, 192, 96)])
def test_c3tail_query(lib, H, in_ld, cat_ld, out_ld):
    fits = lambda B: guards.btl_asm_fits(48, B, H, H, in_ld, out_ld) and guards.c3tail_cat_fits(B, H, H, cat_ld)
    Bmax = guards.largest(fits)
    for B in (Bmax, Bmax + 1):
        assert lib.aq_bottleneck_c3tail_supported(B, H, H, in_ld, cat_ld, out_ld) == int(B <= Bmax), B


@pytest.mark.parametrize("cin,cout,H", [(192, 384, 80), (192, 192, 80), (384, 768, 40)])
def test_planar3x3s2_query(lib, cin, cout, H):
    """The query holds the index range only (the launcher adds the byte offsets), and the region rows of the image width."""
    Bmax = guards.largest(lambda B: guards.pl3x3_index_fits(B, H // 2, H // 2))
    for B in (Bmax, Bmax + 1):
        assert lib.aq_conv3x3_pl_s2_supported(cin, cout, B, H, H) == int(B <= Bmax), B


@pytest.mark.parametrize("query", ["aq_conv3x3_pl_f8_supported", "aq_conv3x3_pl_w8_supported"])
@pytest.mark.parametrize("cin,cout,H", [(192, 192, 40), (384, 384, 20), (384, 384, 40)])
def test_planar3x3_f8_and_w8_queries(lib, query, cin, cout, H):
    """f8: the query holds the index range, as the bf16 launcher does.  w8: the query has no size term of its own and says yes on both
    sides; the limit is the launcher's (pl_conv), whose predicate is asked directly."""
    Bmax = guards.largest(lambda B: guards.pl3x3_index_fits(B, H, H))
    for B in (Bmax, Bmax + 1):
        if query.endswith("w8_supported"):
            assert getattr(lib, query)(cin, cout, B, H, H) == 1, B
            assert _c_guard(lib, SG["pl3x3_index"][0], (B, H, H)) == int(B <= Bmax), B
        else:
            assert getattr(lib, query)(cin, cout, B, H, H) == int(B <= Bmax), B
