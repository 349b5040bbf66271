"""Size guards of the HIP launchers restated in Python, so that tests derive their batch limits from the formulas instead of copying
numbers (and catch a launcher whose guard drifts from what it documents).  Host arithmetic only."""


def btl_asm_fits(C: int, B: int, H: int, W: int, in_ld: int, out_ld: int) -> bool:
    """csrc/bottleneck.hip btl_asm_fits (C = 48, 16 x 16 tiles) / btl96_asm_fits (C = 96, 8 x 16 tiles): does aq_bottleneck run the
    generated-assembly build?  32-bit buffer offsets (input under 2^30 bytes, output under 2^31), magic-number tile decode (>= 2 tiles per
    row and image, tile counts under 2^24 / 2^32)."""
    if C not in (48, 96):
        return False
    th = 16 if C == 48 else 8
    tx, ty = (W + 15) // 16, (H + th - 1) // th
    nt = tx * ty * B
    return (tx >= 2 and tx * ty >= 2 and nt < (1 << 24) and nt * tx * ty < (1 << 32)
            and B * H * W * in_ld * 2 < (1 << 30) and B * H * W * out_ld * 2 < (1 << 31))
