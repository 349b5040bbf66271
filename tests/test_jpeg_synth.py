"""The acceptance rule of the split / GPU JPEG decode (oracle/jpeg_oracle.py: |pass-1 workspace| <= WS_MAX), pinned to Pillow's
libjpeg-turbo on files built from chosen coefficients (tests/jpeg_synth.py), and the host entropy decoder on coefficients an encoder never
produces.  CPU only; the device side is tests/test_gpu_jpeg_synth.py."""
import io

import numpy as np
import pytest
from PIL import Image

import jpeg_synth as S
from oracle import jpeg_oracle as J


@pytest.fixture(scope="module")
def jpeg_lib():
    from aquaculture_amd import build, jpeg
    build.build()
    return jpeg


def _oracle_rgb(jpeg_lib, data, h, w):
    coef, qt, info = S.host_decode(jpeg_lib, data, h, w)
    return J.decode_from_coeffs(coef, qt, w, h, info.mcu_cols, info.mcu_rows), coef, qt, info


def _enc(img, **kw):
    bio = io.BytesIO()
    Image.fromarray(img).save(bio, format="JPEG", **kw)
    return bio.getvalue()


def test_limit_constants_agree():
    """One limit: AQ_JPEG_WS_MAX of include/aq_engine.h (what the kernel compares with), engine.JPEG_WS_MAX (what detect.py's message
    quotes) and the oracle's WS_MAX; and the kernel's bound on dequantised values, AQ_JPEG_DEQ_MAX, is the oracle's DEQ_MAX."""
    import os
    import re
    from aquaculture_amd import engine
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "aq_engine.h")).read()
    assert [int(v) for v in re.findall(r"^#define AQ_JPEG_WS_MAX (\d+)\s*$", hdr, re.M)] == [J.WS_MAX]
    assert [int(v) for v in re.findall(r"^#define AQ_JPEG_DEQ_MAX (\d+)\s*$", hdr, re.M)] == [J.DEQ_MAX]
    assert engine.JPEG_WS_MAX == J.WS_MAX


def test_accepted_blocks_keep_their_dequantised_values_under_deq_max():
    """DEQ_MAX is a consequence of the rule, not a second rule: the largest |coef q| of an accepted block is reached by a single coefficient of row 0 or
    row 4 of the block (ws = 4 c: 4095), those of the other rows stay under 3785, and a value above DEQ_MAX anywhere is refused whatever else the block
    holds (200,000 random blocks with one coefficient just above the bound)."""
    one = np.ones(64, np.int64)
    for k in range(64):
        v = np.zeros((J.DEQ_MAX + 2, 64), np.int64)
        v[:, k] = np.arange(J.DEQ_MAX + 2)
        ok = J.accepted(v, one)
        assert not ok[J.DEQ_MAX + 1] and ((int(np.nonzero(ok)[0].max()) == 4095) if k // 8 in (0, 4) else (int(np.nonzero(ok)[0].max()) < 3785)), k
    rng = np.random.default_rng(6)
    blk = rng.integers(-60, 61, (200000, 64))
    blk[np.arange(200000), rng.integers(0, 64, 200000)] = rng.choice([-1, 1], 200000) * rng.integers(J.DEQ_MAX + 1, J.DEQ_MAX + 40, 200000)
    assert not J.accepted(blk, one).any()


def test_the_rule_is_pinned_to_pillow_on_624_files_up_to_the_limit(jpeg_lib):
    """Every size of S.SIZES x every table kind (all ones, random 1..255, all 255, 16-bit random 1..1000) x every pattern x 3 seeds = 624
    files whose blocks are pushed right up to WS_MAX: each is accepted by the rule (as the generator promises -- none is left out) and the
    oracle equals Pillow byte for byte.  The files reach the limit: blocks within 7 of WS_MAX occur, and the largest dequantised coefficient
    is above 3500 (inside the rule |coef q| cannot exceed 4096: see the comment beside WS_MAX)."""
    n, near, top, top_deq, bad = 0, 0, 0, 0, []
    for si, (h, w) in enumerate(S.SIZES):
        rows, cols = S.mcus(h, w)
        for ki, kind in enumerate(S.TABLE_KINDS):
            for pi, pattern in enumerate(S.PATTERNS):
                for seed in range(3):
                    rng = np.random.default_rng([si, ki, pi, seed])
                    tables, pq = S.make_tables(kind, rng)
                    coef = S.gen_blocks(rng, rows * cols, tables, pattern, J.WS_MAX)
                    data = S.file_from_coeffs(coef, w, h, tables, pq)
                    got, dec, qt, info = _oracle_rgb(jpeg_lib, data, h, w)
                    assert np.array_equal(dec, S.expected_layout(coef, cols, rows))
                    assert np.array_equal(qt, np.stack([tables[0], tables[1], tables[1]]))
                    assert S.file_accepted(dec, qt, cols, rows), (h, w, kind, pattern, seed)
                    m = S.file_ws_max(dec, qt, cols, rows)
                    top, near = max(top, m), near + (m >= J.WS_MAX - 7)
                    top_deq = max(top_deq, int(np.abs(dec[:4 * rows * cols * 64].reshape(-1, 64).astype(np.int64) * qt[0].astype(np.int64)).max()))
                    ref = S.pil_rgb(data)
                    if not np.array_equal(got, ref):
                        bad.append(((h, w), kind, pattern, seed, m, int((got != ref).sum())))
                    n += 1
    print(f"{n} files, {near} with a block within 7 of WS_MAX = {J.WS_MAX}, largest |ws| {top}, largest |coef q| {top_deq}; {len(bad)} differ from Pillow")
    assert n >= 600 and top <= J.WS_MAX and near >= 100 and 3500 < top_deq <= J.DEQ_MAX
    assert not bad, bad[:10]


def _corpus():
    """Encoder-made files at the extremes of 8-bit content: checkerboard, binary noise, one-pixel stripes in both directions, saturated
    8 x 8 colour squares, uniform noise -- at qualities 1, 4, ..., 100."""
    rng = np.random.default_rng(3)
    checker = np.zeros((48, 80, 3), np.uint8)
    checker[::2, ::2] = 255
    checker[1::2, 1::2] = 255
    binary = rng.integers(0, 2, (48, 80, 3)).astype(np.uint8) * 255
    stripes = np.zeros((48, 80, 3), np.uint8)
    stripes[:, ::2] = 255
    rows = np.zeros((48, 80, 3), np.uint8)
    rows[::2] = 255
    sat = np.tile(np.array([[[255, 0, 0], [0, 255, 0]], [[0, 0, 255], [255, 255, 255]]], np.uint8).repeat(8, 0).repeat(8, 1), (3, 5, 1))
    rnd = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    for name, img in (("checker", checker), ("binary", binary), ("stripes", stripes), ("rows", rows), ("saturated", sat), ("noise", rnd)):
        for q in list(range(1, 101, 3)):
            yield f"{name} q{q}", _enc(img, quality=q)


def test_real_files_stay_inside_half_the_limit(jpeg_lib):
    """The rule must not refuse real tiles: every encoder-made file of the corpus and every file of test_jpeg._cases() is accepted with
    max |ws| <= WS_MAX / 2.  (Largest measured: 5058, the saturated colour squares at quality 1.)"""
    import test_jpeg
    top = ("", 0)
    for name, data in list(_corpus()) + test_jpeg._cases():
        ref = S.pil_rgb(data)
        h, w = ref.shape[:2]
        coef, qt, info = S.host_decode(jpeg_lib, data, h, w)
        assert S.file_accepted(coef, qt, info.mcu_cols, info.mcu_rows), name
        m = S.file_ws_max(coef, qt, info.mcu_cols, info.mcu_rows)
        top = max(top, (name, m), key=lambda t: t[1])
        assert m <= J.WS_MAX // 2, (name, m)
    print(f"largest |ws| of an encoder-made file: {top[1]} ({top[0]})")


def test_refused_files_are_refused_for_a_reason(jpeg_lib):
    """Why the rule exists: files outside it that Pillow's libjpeg-turbo and the oracle's exact arithmetic decode DIFFERENTLY -- a flat image
    of DC 1000 with a table of 16 (|ws| = 64000: every byte differs) and a quality-30 noise image whose DQT entries were set to 255 (quantised
    coefficients of at most a few dozen; one damaged table byte is enough).  The same flat image with a table of 4 is inside the rule and
    equal."""
    h, w = 32, 48
    rows, cols = S.mcus(h, w)
    flat = np.zeros((rows * cols, 6, 64), np.int64)
    flat[:, :, 0] = 1000
    for q, inside in ((4, True), (16, False)):
        data = S.file_from_coeffs(flat, w, h, (np.full(64, q), np.full(64, q)))
        got, coef, qt, info = _oracle_rgb(jpeg_lib, data, h, w)
        assert S.file_accepted(coef, qt, cols, rows) == inside and S.file_ws_max(coef, qt, cols, rows) == 4000 * q
        assert np.array_equal(got, S.pil_rgb(data)) == inside, q
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (48, 80, 3), dtype=np.uint8)
    img[::2] = 255 - img[::2] // 8
    base = _enc(img, quality=30)
    assert np.array_equal(_oracle_rgb(jpeg_lib, base, 48, 80)[0], S.pil_rgb(base))
    data = S.set_tables(base, (np.full(64, 255), np.full(64, 255)))
    got, coef, qt, info = _oracle_rgb(jpeg_lib, data, 48, 80)
    assert np.abs(coef).max() < 64 and not S.file_accepted(coef, qt, info.mcu_cols, info.mcu_rows)
    assert not np.array_equal(got, S.pil_rgb(data))


def test_host_entropy_decoder_returns_the_coefficients_that_went_in(jpeg_lib):
    """Writer -> aq_jpeg_decode_coeffs is the identity on coefficients at the limits of the standard Huffman tables, Pillow reads every
    such file, and the tables come back as written (16-bit entries too)."""
    ones = (np.ones(64, np.int64), np.ones(64, np.int64))
    for k, (name, (h, w), c) in enumerate(S.extreme_coefficient_files()):
        rows, cols = S.mcus(h, w)
        tables, pq = (ones, 0) if k % 2 else S.make_tables("random16", np.random.default_rng(k))
        data = S.file_from_coeffs(c, w, h, tables, pq)
        coef, qt, info = S.host_decode(jpeg_lib, data, h, w)
        assert (info.mcu_rows, info.mcu_cols) == (rows, cols)
        assert np.array_equal(coef, S.expected_layout(c, cols, rows)), name
        assert np.array_equal(qt, np.stack([tables[0], tables[1], tables[1]])), name
        assert S.pil_rgb(data).shape == (h, w, 3), name


def test_generator_reaches_both_sides_of_the_limit():
    """The window search the device test of the rule relies on: blocks with max |ws| in [WS_MAX - 7, WS_MAX] and in [WS_MAX + 1, WS_MAX + 8],
    and accepted() says so."""
    rng = np.random.default_rng(8)
    for pattern in S.PATTERNS:
        q = rng.integers(1, 9, 64)
        a = S.block_in_window(rng, q, J.WS_MAX - 7, J.WS_MAX, pattern)
        b = S.block_in_window(rng, q, J.WS_MAX + 1, J.WS_MAX + 8, pattern)
        assert J.accepted(a, q) and not J.accepted(b, q)
        assert J.WS_MAX - 7 <= int(S.ws_max(a, q)) <= J.WS_MAX < int(S.ws_max(b, q)) <= J.WS_MAX + 8
