"""The case table of tests/cu_cases.py, checked without a GPU: tile counts recomputed from the launchers' own constants, the ladders'
coverage, a case for every launcher that sizes its grid from aq_cus(), and the block -> first-tile map of the persistent grids.

The tile constants are read from the sources (csrc/size_guards.h through oracle/guards.py where it restates them, else the launcher's
.hip file), so a launcher whose tile changes makes the table's counts fail here rather than silently thin out the GPU test."""
import os
import re

import pytest

import cu_cases
from oracle import guards as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "aquaculture_amd", "csrc")

# Every exported launcher that calls aq_cus() (csrc/*.hip), by the entry point a caller binds
LAUNCHERS = {
    "aq_stem_conv", "aq_stem_conv_scaled", "aq_stemdown", "aq_downblock", "aq_conv3x3s2_direct", "aq_bottleneck", "aq_bottleneck_c3tail",
    "aq_conv1x1_direct", "aq_conv1x1_direct_f8out", "aq_conv1x1_asm", "aq_conv3x3_pl", "aq_conv3x3_pl_w8", "aq_conv3x3_pl_f8", "aq_conv3x3_pl_s2",
    "aq_conv2d", "aq_head_decode", "aq_head_decode_aug", "aq_blank_stats_u8", "aq_blank_components_u8", "aq_blank_ring_edges_u8",
    "aq_crop_jpeg_coefs", "aq_image_jpeg_coefs", "aq_annotate_u8", "aq_overlap_partners_f64", "aq_overlap_clip_f64",
}
# .hip files that call aq_cus() -> the launchers above that live in them (launch_state.hip defines it)
FILES = {
    "stem_conv.hip": {"aq_stem_conv", "aq_stem_conv_scaled"}, "downblock.hip": {"aq_stemdown", "aq_downblock", "aq_conv3x3s2_direct"},
    "bottleneck.hip": {"aq_bottleneck", "aq_bottleneck_c3tail"}, "conv1x1_direct.hip": {"aq_conv1x1_direct", "aq_conv1x1_direct_f8out"},
    "conv1x1_asm.hip": {"aq_conv1x1_asm"}, "conv3x3_pl.hip": {"aq_conv3x3_pl", "aq_conv3x3_pl_w8", "aq_conv3x3_pl_f8", "aq_conv3x3_pl_s2"},
    "conv_igemm.hip": {"aq_conv2d"}, "conv_halo.hip": {"aq_conv2d"}, "head_decode.hip": {"aq_head_decode", "aq_head_decode_aug"},
    "blank_stats.hip": {"aq_blank_stats_u8"}, "blank_geom.hip": {"aq_blank_components_u8", "aq_blank_ring_edges_u8"},
    "crop_jpeg.hip": {"aq_crop_jpeg_coefs", "aq_image_jpeg_coefs"}, "annotate.hip": {"aq_annotate_u8"},
    "overlaps.hip": {"aq_overlap_partners_f64", "aq_overlap_clip_f64"},
}


def src(name):
    with open(os.path.join(CSRC, name)) as f:
        return f.read()


def const(text, name):
    return int(re.search(rf"\b{name}\s*=\s*(\d+)", text).group(1))


@pytest.fixture(scope="module")
def tiles():
    """The launchers' tile constants, from their sources."""
    sg, c1, c1a, pl = src("size_guards.h"), src("conv1x1_direct.hip"), src("conv1x1_asm.hip"), src("conv3x3_pl.hip")
    t = {k: const(sg, k) for k in ("kStemTW", "kStemTH", "kDownTW", "kDownblockTH", "kConv3x3s2TH")}
    nw = const(c1, "kNW")
    tp = {}
    for ks, mbt, mbw, nbw in re.findall(r"launch_c1<(\d+), (\d+), (\d+), (\d+)>\(p, st\)", c1):
        tp[(32 * int(ks), 16 * int(mbt))] = nw // (int(mbt) // int(mbw)) * int(nbw) * 16       # C1Geom: CIN, COUT -> TP = PG * NBW * 16
    assert len(tp) == 4
    t["c1"] = tp
    t["c1asm"] = dict(zip((13, 7), (int(v) for v in re.search(r"kTPX\[2\] = \{(\d+), (\d+)\}", c1a).groups())))
    t["c1asm_nt"] = const(c1a, "kNT")
    t["pl_bm"], t["pl_s2_nb"] = const(pl, "PL_BM"), const(pl, "PL_S2_NB")
    assert re.search(r"\(long long\)a\.npix \+ 207\) / 208 \* n_mt", pl)                        # the fp8 family's tile: 13 pixel blocks
    cfg = [(int(a), int(b)) for a, b in re.findall(r"^\s*CFG\((\d+), (\d+),", src("conv_igemm.hip"), re.M)]
    halo = [(int(a), int(b)) for a, b in re.findall(r"^\s*HCFG\((\d+), (\d+),", src("conv_halo.hip"), re.M)]
    t["conv"] = cfg + halo
    return t


def recount(g, t):
    """tiles_of restated against the constants read from the sources."""
    k = g[0]
    if k == "stem":
        return g[1] * G.cdiv(g[3] // 2, t["kStemTW"]) * G.cdiv(g[2] // 2, t["kStemTH"])
    if k == "stemdown":
        return g[1] * G.cdiv(g[3] // 4, t["kDownTW"]) * G.cdiv(g[2] // 4, t["kDownblockTH"])
    if k == "downblock":
        return g[1] * G.cdiv(g[3] // 2, t["kDownTW"]) * G.cdiv(g[2] // 2, t["kDownblockTH"])
    if k == "conv3x3s2":
        return g[1] * G.cdiv(g[3] // 2, t["kDownTW"]) * G.cdiv(g[2] // 2, t["kConv3x3s2TH"])
    if k == "bottleneck":
        return g[2] * G.cdiv(g[4], G.btl_tile_w(g[1])) * G.cdiv(g[3], G.btl_tile_h(g[1]))
    if k == "c3tail":
        return g[1] * G.cdiv(g[3], G.btl_tile_w(48)) * G.cdiv(g[2], G.btl_tile_h(48))
    if k == "c1direct":
        return G.cdiv(g[3], t["c1"][(g[1], g[2])])
    if k == "c1asm":
        return G.cdiv(g[3], t["c1asm"][g[1]]) * (g[2] // t["c1asm_nt"])
    if k == "pl":
        return G.cdiv(g[3], 16 * g[1]) * (g[2] // t["pl_bm"])
    if k == "conv2d":
        bm, bn = t["conv"][g[1]]
        return G.cdiv(g[2], bm) * G.cdiv(g[3], bn)
    if k == "head":
        return G.cdiv(g[2], 64 // (1 if g[1] <= 256 else 2 if g[1] <= 512 else 4))
    assert k == "count"
    return g[1]


def last_tile_is_partial(g, t):
    """Does the tiled extent of a ladder case end inside a tile?"""
    k = g[0]
    if k == "stem":
        return (g[3] // 2) % t["kStemTW"] != 0
    if k == "stemdown":
        return (g[3] // 4) % t["kDownTW"] != 0
    if k in ("downblock", "conv3x3s2"):
        return (g[3] // 2) % t["kDownTW"] != 0
    if k == "bottleneck":
        return g[4] % G.btl_tile_w(g[1]) != 0 or g[3] % G.btl_tile_h(g[1]) != 0
    if k == "c3tail":
        return g[3] % 16 != 0
    if k == "c1direct":
        return g[3] % t["c1"][(g[1], g[2])] != 0
    if k == "c1asm":
        return g[3] % t["c1asm"][g[1]] != 0
    if k == "pl":
        return g[3] % (16 * g[1]) != 0
    if k == "conv2d":
        return g[3] % t["conv"][g[1]][1] != 0
    raise AssertionError(k)


def test_tile_constants_of_the_table_are_the_sources(tiles):
    assert (cu_cases.STEM_TW, cu_cases.STEM_TH) == (tiles["kStemTW"], tiles["kStemTH"])
    assert (cu_cases.DOWN_TW, cu_cases.DOWNBLOCK_TH, cu_cases.CONV3X3S2_TH) == (tiles["kDownTW"], tiles["kDownblockTH"], tiles["kConv3x3s2TH"])
    assert cu_cases.C1_DIRECT_TP == tiles["c1"] and cu_cases.C1_ASM_TPX == tiles["c1asm"] and cu_cases.C1_ASM_NT == tiles["c1asm_nt"]
    assert (cu_cases.PL_BM, cu_cases.PL_S2_NB) == (tiles["pl_bm"], tiles["pl_s2_nb"]) and cu_cases.PL_F8_BN == 16 * 13
    assert cu_cases.CONV_TILES == tiles["conv"] and len(cu_cases.IGEMM_TILES) == 21 and len(cu_cases.HALO_TILES) == 13
    for c in (16, 32, 48, 64, 96):
        assert cu_cases.btl_tile(c) == (G.btl_tile_w(c), G.btl_tile_h(c))


def test_every_tile_count_is_what_the_constants_give(tiles):
    ids = [c.id for c in cu_cases.CASES]
    assert len(set(ids)) == len(ids)
    for c in cu_cases.CASES:
        assert c.n_tiles == recount(c.geom, tiles) >= 1, c.id
        if c.geom[0] == "bottleneck":                        # which build takes the launch: the size predicate of csrc/size_guards.h
            assert c.asm == G.btl_asm_fits(c.geom[1], *c.geom[2:], c.geom[1], c.geom[1]), c.id
        if c.geom[0] == "c3tail":
            assert G.btl_asm_tiles_fit(48, *c.geom[1:], 48, 96), c.id
    frames, mcus = cu_cases.frame_items()
    assert frames > 32 * 32 and mcus > 32 * 32               # more than one trip at 32 workgroups per CU and 32 CUs (a partitioned device)


def test_ladders_reach_every_trip_count_and_end_in_a_partial_tile(tiles):
    ladders = {}
    for c in cu_cases.CASES:
        if c.ladder:
            assert c.id.startswith("ladder-") and c.ladder in ("full", "partial", "mid")
            ladders.setdefault(c.family, {"full": [], "partial": [], "mid": [], "asm": set()})[c.ladder].append(c)
            ladders[c.family]["asm"].add(c.asm)
    assert len(ladders) >= 30
    for fam, l in ladders.items():
        # the assembly Bottleneck and C3-tail kernels need two tiles per row and image: 2 stands in for 1 (cu_cases.ASM_LADDER)
        needs_two = fam.startswith("bottleneck-asm") or fam == "c3tail"
        want = {2, 3, 4, 5, 9, 17} if needs_two else {1, 2, 3, 4, 5, 9, 17}
        # (the plain bf16 stem kernel runs only widths that are no multiple of 4: it can have no ladder of whole tiles)
        for kind in ("partial",) if fam == "stem-bf16-plain" else ("full", "partial"):
            counts = {c.n_tiles for c in l[kind]}
            assert want <= counts, (fam, kind, sorted(counts))
            assert counts == set(cu_cases.ASM_LADDER if needs_two else cu_cases.LADDER), (fam, kind)
        assert all(not last_tile_is_partial(c.geom, tiles) for c in l["full"]), fam
        assert l["partial"] and all(last_tile_is_partial(c.geom, tiles) for c in l["partial"]), fam
        if needs_two or "asm" in fam:
            assert l["asm"] == {True}, fam
        if fam.startswith("bottleneck-hip"):
            assert l["asm"] == {False}, fam
    # a partial tile in the middle of the walk, for every family tiled in image rows: two tile rows whose last column is partial
    row_tiled = {"stem-fp32", "stem-bf16", "stem-bf16-plain", "stemdown", "downblock", "conv3x3s2_direct", "c3tail", "bottleneck-asm-c48", "bottleneck-asm-c96",
                 "bottleneck-hip-c16", "bottleneck-hip-c32", "bottleneck-hip-c64"}
    assert {f for f, l in ladders.items() if l["mid"]} == row_tiled
    for fam in row_tiled:
        assert {c.n_tiles for c in ladders[fam]["mid"]} == {2 * n for n in cu_cases.MID_LADDER} and 2 in cu_cases.MID_LADDER and 3 in cu_cases.MID_LADDER
        for c in ladders[fam]["mid"]:
            g = list(c.geom)
            h = {"bottleneck": 3}.get(g[0], 2)               # where the geometry holds the image height
            g[h] //= 2
            assert last_tile_is_partial(c.geom, tiles) and 2 * recount(tuple(g), tiles) == c.n_tiles, c.id       # two rows of n, the nth partial
    # which stem kernel a ladder runs: the launcher's own condition, read from the source.  The bf16 ladders stay on the LDS-DMA kernel
    # (the two-deep pipeline with the counted waits) in whole, partial and mid-walk tiles alike; the other two families on the plain one.
    assert "const bool dma = !f32 && (W % 4) == 0 && ((uintptr_t)tiles_dev & 3) == 0" in src("stem_conv.hip")
    for fam, dma in (("stem-bf16", True), ("stem-bf16-plain", False), ("stem-fp32", False)):
        prec = fam.split("-")[1]
        for kind in ("full", "partial", "mid"):
            assert ladders[fam][kind] or (fam, kind) == ("stem-bf16-plain", "full")
            for c in ladders[fam][kind]:
                assert (prec == "bf16" and c.geom[3] % 4 == 0) == dma == cu_cases.stem_uses_dma(prec, c.geom[3]), c.id
    assert {k for k in ("partial", "mid") for c in ladders["stem-bf16"][k] if (c.geom[3] // 2) % tiles["kStemTW"] == 40} == {"partial", "mid"}
    families = set(ladders)
    assert set(cu_cases.EXPERIMENTAL_BUILDS) < set(cu_cases.PL_BUILDS)      # (their ladders run only in a build that holds them: the GPU test lists them)
    for want in ("stem-bf16", "stem-fp32", "stemdown", "downblock", "conv3x3s2_direct", "c3tail", "conv2d-igemm", "conv2d-halo", "conv1x1_asm-nb13",
                 "conv1x1_asm-nb7", "conv1x1_direct_f8out-192", "conv1x1_direct_f8out-384", "conv3x3_pl_w8", "conv3x3_pl_f8", "conv3x3_pl_s2",
                 "bottleneck-asm-c48", "bottleneck-asm-c96"):
        assert want in families, want
    assert {f"bottleneck-hip-c{c}" for c in (16, 32, 48, 64, 96)} <= families
    assert {f"conv1x1_direct-{a}-{b}" for a, b in tiles["c1"]} <= families
    assert {f"conv3x3_pl-{b}" for b in cu_cases.PL_BUILDS} <= families


def test_every_launcher_that_reads_the_cu_count_has_a_case():
    covered = {name for c in cu_cases.CASES for name in c.launchers}
    assert LAUNCHERS <= covered, sorted(LAUNCHERS - covered)
    with open(os.path.join(ROOT, "aquaculture_amd", "engine.py")) as f:
        bound = set(re.findall(r"lib\.(aq_\w+)\b", f.read()))        # (some are called with explicit ctypes values, without argtypes)
    assert LAUNCHERS <= bound, sorted(LAUNCHERS - bound)
    assert covered - LAUNCHERS <= {"aq_engine_infer", "aq_engine_infer_augment"} and covered - LAUNCHERS <= bound
    # the files that call aq_cus() are the ones the list was read from, and each of their launchers is exported there
    calling = {n for n in os.listdir(CSRC) if n.endswith(".hip") and re.search(r"\baq_cus\(&", src(n))}
    assert calling == set(FILES), sorted(calling ^ set(FILES))
    assert set().union(*FILES.values()) == LAUNCHERS
    for name, launchers in FILES.items():
        text = src(name) + (src("engine.cpp") if "aq_conv2d" in launchers else "")       # aq_conv2d: exported by engine.cpp over both files' launchers
        for fn in launchers:
            assert re.search(rf'extern "C" int {fn}\(', text), (name, fn)


def test_exemptions_are_the_head_decode_candidate_lists():
    ids = {c.id for c in cu_cases.CASES}
    assert set(cu_cases.EXEMPT) <= ids and all(i.startswith("head_decode") and reason for i, reason in cu_cases.EXEMPT.items())
    assert {c.id for c in cu_cases.CASES if c.family == "head_decode"} == set(cu_cases.EXEMPT)


def first_tile(G_, bid):
    """csrc/conv_device.h first_tile, restated."""
    q, r, xcd = G_ >> 3, G_ & 7, bid & 7
    return (xcd * (q + 1) if xcd < r else r * (q + 1) + (xcd - r) * q) + (bid >> 3)


def test_first_tile_is_a_bijection():
    text = src("conv_device.h")
    assert "const int q = G >> 3, r = G & 7, xcd = bid & 7;" in text
    assert "return (xcd < r ? xcd * (q + 1) : r * (q + 1) + (xcd - r) * q) + (bid >> 3);" in text
    for G_ in range(1, 2049):
        assert sorted(first_tile(G_, b) for b in range(G_)) == list(range(G_)), G_
    assert first_tile(13, 8) == 1 and [first_tile(13, b) for b in range(8)] == [0, 2, 4, 6, 8, 10, 11, 12]    # G & 7 != 0, G >> 3 >= 1
