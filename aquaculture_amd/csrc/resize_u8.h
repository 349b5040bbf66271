// OpenCV's 8-bit INTER_LINEAR in fixed point (resize.cpp: HResizeLinear into int at scale 2^11, VResizeLinear<uchar, int, short>), one
// channel of one output pixel from its four taps.  Shared by aq_letterbox_u8 (pointwise.hip) and aq_val_mosaic_u8 (mosaic.hip); the
// coefficient tables (source index pair + weights per destination column / row) are dataloader._axis_coeffs' on the host.
//   p00 p01: the two column taps on the first row tap, p10 p11: on the second;  a0 a1: column weights, b0 b1: row weights (2^11 units).
#pragma once

__device__ __forceinline__ unsigned char aq_resize_linear_u8(int p00, int p01, int p10, int p11, int a0, int a1, int b0, int b1) {
    const int h0 = p00 * a0 + p01 * a1;
    const int h1 = p10 * a0 + p11 * a1;
    const int v = (((b0 * (h0 >> 4)) >> 16) + ((b1 * (h1 >> 4)) >> 16) + 2) >> 2;
    return (unsigned char)(v < 0 ? 0 : (v > 255 ? 255 : v));
}
