"""JPEG files built from CHOSEN quantised coefficients and chosen quantisation tables -- test infrastructure (a plain module, imported by
tests/test_jpeg_synth.py and tests/test_gpu_jpeg_synth.py).

Files a JPEG encoder makes from 8-bit images reach a small corner of what the decoders accept.  Here the ground truth of the entropy
decoders is the coefficient array that went in, and the pixel half sees amplitudes right up to the acceptance rule of
oracle/jpeg_oracle.py (|pass-1 workspace| <= WS_MAX) with any tables.  The files are written by the project's own baseline coder
(engine.image_jpeg_bytes: 4:2:0, the standard Huffman tables -- which code |AC| <= 1023 and DC differences up to 2047), then their DQT
segments are replaced.  aq_jpeg_scan and Pillow both read them.
"""
import io

import numpy as np
from PIL import Image

from oracle import jpeg_oracle as J

# (H, W): a chroma plane one sample wide or high, both branches of the pixel kernel's 12-byte store (3 W a multiple of 4 or not, fewer
# than 4 pixels left in a row), more than one MCU in both directions.  libjpeg replicates chroma planes up to 2 samples wide instead of
# filtering them (jdsample.c), so (40, 1) and (2, 2) do NOT reach the replication of the component's real edge in the triangle filter:
# (40, 6) does, at the bottom and at the right, and (6, 5) at the bottom (an even H or W below a multiple of 16: the last row / column
# filters towards the component's real edge, which lies inside its padded block, and the padding holds other values; (1, 40) at the right
# only); (5, 4) and (6, 5) sit on either side of the 2-sample threshold.
SIZES = [(1, 1), (1, 40), (40, 1), (2, 2), (9, 9), (15, 16), (16, 17), (17, 16), (31, 33), (64, 32), (40, 6), (6, 5), (5, 4)]
PATTERNS = ("sparse", "column", "row", "dense")
TABLE_KINDS = ("ones", "random", "255", "random16")


def _zigzag():
    out = []
    for s in range(15):
        pts = [(i, s - i) for i in range(max(0, s - 7), min(7, s) + 1)]
        out += [y * 8 + x for y, x in (pts[::-1] if s % 2 == 0 else pts)]
    return np.array(out)


ZIGZAG = _zigzag()                      # ZIGZAG[k] = natural index (8 row + column) of zigzag position k


def mcus(h, w):
    """(mcu_rows, mcu_cols) of a 4:2:0 image."""
    return (h + 15) // 16, (w + 15) // 16


def set_tables(data: bytes, tables, pq: int = 0) -> bytes:
    """The file with every DQT segment replaced by one segment per table: tables = (luma, chroma), 64 natural-order entries each, written in
    zigzag order as 8-bit (pq = 0) or 16-bit (pq = 1) entries."""
    out, i, done = bytearray(data[:2]), 2, False
    while True:
        assert data[i] == 0xFF, i
        m, ln = data[i + 1], int.from_bytes(data[i + 2:i + 4], "big")
        if m == 0xDA:
            out += data[i:]
            break
        if m != 0xDB:
            out += data[i:i + 2 + ln]
        elif not done:
            done = True
            for tid, qt in enumerate(tables):
                zz = np.asarray(qt, np.int64)[ZIGZAG]
                assert zz.min() >= 1 and zz.max() <= (65535 if pq else 255)
                body = bytes([(pq << 4) | tid]) + (zz.astype(">u2").tobytes() if pq else zz.astype(np.uint8).tobytes())
                out += b"\xff\xdb" + (2 + len(body)).to_bytes(2, "big") + body
        i += 2 + ln
    assert done
    return bytes(out)


def file_from_coeffs(coef, w: int, h: int, tables, pq: int = 0) -> bytes:
    """coef int [MCUs, 6, 64]: quantised coefficients in natural order, the MCUs in raster order, blocks Y00 Y01 Y10 Y11 Cb Cr -> the bytes
    of a baseline 4:2:0 JPEG of w x h pixels with the quantisation tables (luma, chroma)."""
    from aquaculture_amd import engine
    coef = np.asarray(coef)
    rows, cols = mcus(h, w)
    assert coef.shape == (rows * cols, 6, 64), coef.shape
    assert np.abs(coef[..., 1:]).max(initial=0) <= 1023 and np.abs(coef[..., 0]).max(initial=0) <= 2047
    zz = np.ascontiguousarray(coef[..., ZIGZAG].reshape(-1, 384).astype(np.int16))
    return set_tables(engine.image_jpeg_bytes(zz, w, h), tables, pq)


def expected_layout(coef, mcu_cols: int, mcu_rows: int) -> np.ndarray:
    """The aq_jpeg_decode_coeffs buffer the coefficients [MCUs, 6, 64] must decode to: the Y blocks in raster order of the padded image
    ([2 mcu_rows][2 mcu_cols][64]), then Cb, then Cr ([mcu_rows][mcu_cols][64] each), natural order, int16."""
    c = np.asarray(coef).reshape(mcu_rows, mcu_cols, 6, 64)
    y = c[:, :, :4].reshape(mcu_rows, mcu_cols, 2, 2, 64).transpose(0, 2, 1, 3, 4)           # [my][dy][mx][dx]
    return np.concatenate([y.reshape(-1), c[:, :, 4].reshape(-1), c[:, :, 5].reshape(-1)]).astype(np.int16)


def make_tables(kind: str, rng):
    """-> ((luma, chroma), pq) for a table kind of TABLE_KINDS."""
    if kind == "ones":
        return (np.ones(64, np.int64), np.ones(64, np.int64)), 0
    if kind == "random":
        return (rng.integers(1, 256, 64), rng.integers(1, 256, 64)), 0
    if kind == "255":
        return (np.full(64, 255), np.full(64, 255)), 0
    if kind == "random16":
        return (rng.integers(1, 1001, 64), rng.integers(1, 1001, 64)), 1
    raise ValueError(kind)


def ws_max(blocks, q) -> np.ndarray:
    """max |pass-1 workspace| of every block: blocks int [..., 64], q [64] or broadcastable [..., 64]."""
    blocks = np.asarray(blocks, np.int64)
    ws = J.pass1_workspace(blocks * np.asarray(q, np.int64), np.ones(64, np.int64))
    return np.abs(ws).reshape(ws.shape[:-2] + (64,)).max(-1)


def _raw_blocks(rng, n, pattern):
    """n blocks of a pattern, float, |v| in [0.5, 1] on the pattern's support."""
    sup = np.zeros((n, 64), bool)
    for b in range(n):
        if pattern == "sparse":
            sup[b, rng.choice(64, int(rng.integers(1, 6)), replace=False)] = True
        elif pattern == "column":
            sup[b, np.arange(8) * 8 + int(rng.integers(8))] = True
        elif pattern == "row":
            sup[b, np.arange(8) + 8 * int(rng.integers(8))] = True
        elif pattern == "dense":
            sup[b] = True
        else:
            raise ValueError(pattern)
    return sup * rng.choice([-1.0, 1.0], (n, 64)) * rng.uniform(0.5, 1.0, (n, 64))


def gen_blocks(rng, n_mcu: int, tables, pattern: str, bound: int, fractions=(1.0, 1.0, 1.0, 0.5, 0.1)) -> np.ndarray:
    """Seeded block generator: int64 [n_mcu, 6, 64], |c| <= 1023, every block with max |ws| <= its target = bound x a fraction drawn per
    block.  A block starts as large as the Huffman tables allow and is SHRUNK (bisection on a scale factor, 14 steps) until it is inside its
    target, then pushed towards it again by single steps of single coefficients -- so with fine tables most blocks of fraction 1 end
    within a few units of the bound."""
    q = np.stack([np.asarray(tables[0 if k < 4 else 1], np.int64) for k in range(6)])
    q = np.broadcast_to(q, (n_mcu, 6, 64)).reshape(-1, 64)
    n = q.shape[0]
    raw = _raw_blocks(rng, n, pattern) * 1023.0
    target = bound * rng.choice(np.asarray(fractions), n)
    inside = lambda blk: ws_max(blk, q) <= target
    lo, hi = np.zeros(n), np.ones(n)
    for _ in range(14):
        mid = (lo + hi) / 2
        ok = inside(np.trunc(raw * mid[:, None]).astype(np.int64))
        lo, hi = np.where(ok, mid, lo), np.where(ok, hi, mid)
    full = inside(np.trunc(raw).astype(np.int64))
    blk = np.trunc(raw * np.where(full, 1.0, lo)[:, None]).astype(np.int64)
    sgn = np.where(raw < 0, -1, 1) * (raw != 0)
    for _ in range(24):                                                # push: one step of one coefficient of the support, kept where still inside
        k = rng.integers(0, 64, n)
        cand = blk.copy()
        cand[np.arange(n), k] += sgn[np.arange(n), k]
        cand = np.clip(cand, -1023, 1023)
        ok = inside(cand)
        blk = np.where(ok[:, None], cand, blk)
    assert inside(blk).all() and np.abs(blk).max() <= 1023
    return blk.reshape(n_mcu, 6, 64)


def block_in_window(rng, q, lo: int, hi: int, pattern: str = "sparse", tries: int = 200) -> np.ndarray:
    """Search: one block int64 [64], |c| <= 1023, with lo <= max |ws| <= hi for the table q [64]."""
    q = np.asarray(q, np.int64)
    for _ in range(tries):
        blk = gen_blocks(rng, 1, (q, q), pattern, hi, fractions=(1.0,))[0, 0]
        sup = np.nonzero(blk)[0]
        for _ in range(400):
            m = int(ws_max(blk, q))
            if lo <= m <= hi:
                return blk
            if not sup.size:
                break
            k = int(rng.choice(sup))
            step = (1 if blk[k] > 0 else -1) * (1 if m < lo else -1)
            blk[k] = int(np.clip(blk[k] + step, -1023, 1023))
    raise RuntimeError(f"no block with max |ws| in [{lo}, {hi}] found")


def extreme_coefficient_files():
    """[(name, (h, w), coef [MCUs, 6, 64])]: symbols natural files rarely reach -- category-10 AC values of +-1023, category-11 DC differences
    (DC alternating +-1023: 2046; a DC ramp in steps of 2047), blocks with all 64 coefficients non-zero, only index 63 non-zero (three ZRLs,
    no EOB), long zero runs, empty blocks.  For both entropy decoders."""
    out = []
    for h, w in ((16, 16), (33, 17), (64, 64)):
        rows, cols = mcus(h, w)
        n = rows * cols
        rng = np.random.default_rng([h, w])
        sign = np.where((np.arange(n)[:, None] + np.arange(6)[None, :]) % 2 == 0, 1, -1)
        c = rng.choice([-1023, 1023], (n, 6, 64))
        c[:, :, 0] = 1023 * sign                                        # within a component successive DCs alternate: differences of 2046
        out.append((f"{h}x{w} all 64 at +-1023, DC alternating", (h, w), c))
        c = np.zeros((n, 6, 64), np.int64)
        tri = np.array([-2047, 0, 2047, 0])
        c[:, :4, 0] = tri[(np.arange(4 * n) % 4)].reshape(n, 4)         # Y: -2047, 0, 2047, 0, ... in scan order; Cb, Cr: one step per MCU
        c[:, 4, 0] = tri[np.arange(n) % 4]
        c[:, 5, 0] = -tri[np.arange(n) % 4]
        out.append((f"{h}x{w} DC ramp in steps of 2047", (h, w), c))
        c = np.zeros((n, 6, 64), np.int64)
        c[:, :, 63] = rng.choice([-1023, -1, 1, 1023], (n, 6))
        c[:, 1::2, 63] = 0                                              # every other block empty
        out.append((f"{h}x{w} only index 63, every other block empty", (h, w), c))
        c = rng.integers(-1023, 1024, (n, 6, 64))
        c[c == 0] = 1
        c[:, :, 0] = rng.integers(-1023, 1024, (n, 6))
        out.append((f"{h}x{w} dense random, no zero", (h, w), c))
        c = np.zeros((n, 6, 64), np.int64)
        c[:, :, 17] = 5
        c[:, :, 50] = -1023                                             # a run of 32 zeros: two ZRLs
        c[:, ::3, 50] = 0
        c[:, :, 0] = rng.integers(-3, 4, (n, 6))
        out.append((f"{h}x{w} long zero runs", (h, w), c))
    return out


def pil_rgb(data: bytes) -> np.ndarray:
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))


def host_decode(jpeg_lib, data: bytes, h: int, w: int):
    """aq_jpeg_decode_coeffs on the file: (coef int16 [coef_count], qt uint16 [3, 64], info); asserts that it is accepted and of h x w."""
    coef = np.zeros(jpeg_lib.coef_count(h, w), np.int16)
    qt = np.zeros((3, 64), np.uint16)
    assert jpeg_lib.scan(data) is not None
    rc, info = jpeg_lib.decode_coeffs(data, coef, qt)
    assert rc == 0 and (info.height, info.width) == (h, w), (rc, info.height, info.width)
    return coef, qt, info


def file_ws_max(coef, qt, mcu_cols: int, mcu_rows: int) -> int:
    """max |ws| over all blocks of an aq_jpeg_decode_coeffs buffer."""
    ny, nc = 4 * mcu_cols * mcu_rows * 64, mcu_cols * mcu_rows * 64
    parts = (coef[:ny], coef[ny:ny + nc], coef[ny + nc:ny + 2 * nc])
    return max(int(ws_max(p.reshape(-1, 64), qt[i]).max()) for i, p in enumerate(parts))


def file_accepted(coef, qt, mcu_cols: int, mcu_rows: int) -> bool:
    """The oracle's rule for a whole image: every block of every component accepted."""
    ny, nc = 4 * mcu_cols * mcu_rows * 64, mcu_cols * mcu_rows * 64
    parts = (coef[:ny], coef[ny:ny + nc], coef[ny + nc:ny + 2 * nc])
    return all(bool(J.accepted(p.reshape(-1, 64), qt[i]).all()) for i, p in enumerate(parts))
