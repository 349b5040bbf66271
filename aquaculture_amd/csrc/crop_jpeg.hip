// --save-crop: detection crops as baseline JPEGs, the encoder of the split JPEG decode run in reverse.
//
// Upstream saves every crop with Pillow, `Image.fromarray(rgb).save(f, quality=95, subsampling=0)` [UPSTREAM utils/plots.py save_one_box]:
// libjpeg(-turbo), baseline 4:4:4, islow DCT, the standard Huffman tables.  The pixel half of that encoder runs here on the device, bit for
// bit: edge replication to whole 8x8 blocks (jcprepct.c expand_right_edge / expand_bottom_edge), rgb_ycc_convert (jccolor.c: 16-bit fixed
// point), the level shift, jpeg_fdct_islow (jfdctint.c: 13-bit constants, rows then columns, DESCALE roundings) and quantisation by the
// quality-95 tables (jcparam.c jpeg_set_quality: Annex K scaled by (q 10 + 50) / 100, clamped to [1, 255]; jcdctmgr.c divides by q 8 with
// the rounding half away from zero).  Integer arithmetic only.  The host half (Huffman coding, markers, files) is further down: plain C++
// on the caller's thread and on threads of its own, no interpreter lock held.
//
// Layout: crop i covers block positions [crops[i].block, crops[i].block + ceil(w / 8) ceil(h / 8)) of the coefficient arena, raster order;
// a block position holds 3 x 64 int16 (Y, Cb, Cr), each block in zigzag order -- the order the entropy coder walks.
// Kernel: one thread per (block position, component); the three threads of a position read the same 192 bytes of pixels.
//
// Whole frames (the annotated images of detect.py without --nosave) go through a second kernel further down: 4:2:0, what cv2.imwrite's
// libjpeg writes for a .jpg, sharing fdct8, the tables and the host coder (a sampling argument) with the crops.
#include "aq_common.h"
#include <errno.h>
#include <stdio.h>
#include <string.h>
#include <sys/stat.h>
#include <unistd.h>
#include <atomic>
#include <string>
#include <thread>
#include <vector>

namespace {

// Annex K tables (natural order) and jpeg_natural_order
constexpr unsigned char kStdLuma[64] = {16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56,
                                        14, 17, 22, 29, 51, 87, 80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92,
                                        49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100, 103, 99};
constexpr unsigned char kStdChroma[64] = {17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99,
                                          47, 66, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99,
                                          99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99, 99};
constexpr unsigned char kNatural[64] = {0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                                        35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

// jpeg_set_quality (jcparam.c jpeg_quality_scaling, jpeg_add_quant_table with force_baseline): scale factor 5000 / q below 50, 200 - 2 q from
// there; (base scale + 50) / 100 clamped to [1, 255]
__host__ __device__ constexpr int q_scaled(int base, int quality) {
    const int s = quality < 50 ? 5000 / quality : 200 - 2 * quality, v = (base * s + 50) / 100;
    return v < 1 ? 1 : (v > 255 ? 255 : v);
}
__host__ __device__ constexpr int q95(int base) { return q_scaled(base, 95); }   // the crops' quality, and the frames' default: scale factor 10

constexpr int CB = 13, P1 = 2;
constexpr int F_0_298631336 = 2446, F_0_390180644 = 3196, F_0_541196100 = 4433, F_0_765366865 = 6270, F_0_899976223 = 7373,
              F_1_175875602 = 9633, F_1_501321110 = 12299, F_1_847759065 = 15137, F_1_961570560 = 16069, F_2_053119869 = 16819,
              F_2_562915447 = 20995, F_3_072711026 = 25172;

// jfdctint.c, one dimension over d[0], d[S], ..., d[7 S]; pass 1 (rows) keeps PASS1_BITS of extra precision, pass 2 (columns) removes them
template <int S, bool PASS2>
__device__ __forceinline__ void fdct8(int* d) {
    const int tmp0 = d[0] + d[7 * S], tmp7 = d[0] - d[7 * S];
    const int tmp1 = d[S] + d[6 * S], tmp6 = d[S] - d[6 * S];
    const int tmp2 = d[2 * S] + d[5 * S], tmp5 = d[2 * S] - d[5 * S];
    const int tmp3 = d[3 * S] + d[4 * S], tmp4 = d[3 * S] - d[4 * S];
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    constexpr int SH = PASS2 ? CB + P1 : CB - P1, R = 1 << (SH - 1);
    if (PASS2) {
        d[0] = (tmp10 + tmp11 + (1 << (P1 - 1))) >> P1;
        d[4 * S] = (tmp10 - tmp11 + (1 << (P1 - 1))) >> P1;
    } else {
        d[0] = (tmp10 + tmp11) * (1 << P1);
        d[4 * S] = (tmp10 - tmp11) * (1 << P1);
    }
    const int z1e = (tmp12 + tmp13) * F_0_541196100;
    d[2 * S] = (z1e + tmp13 * F_0_765366865 + R) >> SH;
    d[6 * S] = (z1e + tmp12 * (-F_1_847759065) + R) >> SH;
    int z1 = tmp4 + tmp7, z2 = tmp5 + tmp6, z3 = tmp4 + tmp6, z4 = tmp5 + tmp7;
    const int z5 = (z3 + z4) * F_1_175875602;
    const int t4 = tmp4 * F_0_298631336, t5 = tmp5 * F_2_053119869, t6 = tmp6 * F_3_072711026, t7 = tmp7 * F_1_501321110;
    z1 *= -F_0_899976223; z2 *= -F_2_562915447; z3 *= -F_1_961570560; z4 *= -F_0_390180644;
    z3 += z5; z4 += z5;
    d[7 * S] = (t4 + z1 + z3 + R) >> SH;
    d[5 * S] = (t5 + z2 + z4 + R) >> SH;
    d[3 * S] = (t6 + z2 + z3 + R) >> SH;
    d[S] = (t7 + z1 + z4 + R) >> SH;
}

struct CropParams {
    const unsigned char* img;
    long long img_bytes;
    const aq_crop* crops;
    int n_crops;
    long long n_threads;          // 3 x block positions of this piece
    short* coef;                  // block position crops[0].block of the batch is arena position 0
};

__global__ __launch_bounds__(256) void crop_jpeg_kernel(const CropParams p) {
    const int pos0 = p.crops[0].block;
    for (long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x; t < p.n_threads; t += (long long)gridDim.x * blockDim.x) {
        const long long pos = t / 3;
        const int comp = (int)(t - pos * 3);
        const long long g = pos0 + pos;
        int lo = 0, hi = p.n_crops - 1;                       // the crop that holds block position g: the last one that starts at or before it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.crops[mid].block <= g) lo = mid; else hi = mid - 1;
        }
        const aq_crop c = p.crops[lo];
        const int w = c.x2 - c.x1, h = c.y2 - c.y1;
        short* out = p.coef + (pos * 3 + comp) * 64;
        const bool ok = w > 0 && h > 0 && c.x1 >= 0 && c.y1 >= 0 && c.base >= 0 && c.pitch >= 3 * c.x2 &&
                        c.base + (long long)(c.y2 - 1) * c.pitch + 3LL * c.x2 <= p.img_bytes;
        if (!ok) {                                            // refused by the launcher's caller already; never read outside the images
            for (int k = 0; k < 64; k += 8) *(uint4*)(out + k) = make_uint4(0, 0, 0, 0);
            continue;
        }
        const int bw = (w + 7) >> 3, k = (int)(g - c.block), by = k / bw, bx = k - by * bw;
        // rgb_ycc_convert: the three table sums of the component, >> 16 (Cb / Cr carry CBCR_OFFSET + ONE_HALF - 1, Y carries ONE_HALF)
        const int cr = comp == 0 ? 19595 : (comp == 1 ? -11059 : 32768);
        const int cg = comp == 0 ? 38470 : (comp == 1 ? -21709 : -27439);
        const int cb = comp == 0 ? 7471 : (comp == 1 ? 32768 : -5329);
        const int add = comp == 0 ? 32768 : (128 << 16) + 32767;
        int ws[64];
#pragma unroll
        for (int r = 0; r < 8; ++r) {
            const int y = c.y1 + min(8 * by + r, h - 1);      // edge replication: the last row and column of the crop
            const unsigned char* row = p.img + c.base + (long long)y * c.pitch;
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int x = c.x1 + min(8 * bx + e, w - 1);
                const unsigned char* px = row + 3 * x;
                ws[8 * r + e] = ((cr * px[0] + cg * px[1] + cb * px[2] + add) >> 16) - 128;
            }
        }
#pragma unroll
        for (int r = 0; r < 8; ++r) fdct8<1, false>(ws + 8 * r);
#pragma unroll
        for (int e = 0; e < 8; ++e) fdct8<8, true>(ws + e);
        short q[64];
#pragma unroll
        for (int z = 0; z < 64; ++z) {                        // quantise (divisor = quantval << 3, round half away from zero), zigzag order
            const int n = kNatural[z];
            const int div = 8 * (comp ? q95(kStdChroma[n]) : q95(kStdLuma[n]));
            const int v = ws[n], a = ((v < 0 ? -v : v) + (div >> 1)) / div;
            q[z] = (short)(v < 0 ? -a : a);
        }
#pragma unroll
        for (int z = 0; z < 64; z += 8) {
            uint4 v;
            v.x = (unsigned short)q[z] | ((unsigned)(unsigned short)q[z + 1] << 16);
            v.y = (unsigned short)q[z + 2] | ((unsigned)(unsigned short)q[z + 3] << 16);
            v.z = (unsigned short)q[z + 4] | ((unsigned)(unsigned short)q[z + 5] << 16);
            v.w = (unsigned short)q[z + 6] | ((unsigned)(unsigned short)q[z + 7] << 16);
            *(uint4*)(out + z) = v;
        }
    }
}


// ---- whole frames, 4:2:0 (annotated images; cv2.imwrite's libjpeg defaults) ----
//
// One wave per 16 x 16 MCU, four MCUs per workgroup.  The wave's 64 lanes read the MCU's 256 pixels once (four neighbours each), convert them
// and keep Y and the full-resolution Cb / Cr in LDS; h2v2_downsample (jcsample.c) makes the two chroma blocks there; 48 lanes run the row
// pass and the column pass of the six blocks (one row or column each) through LDS, quantise into zigzag order, and 48 lanes store the MCU's
// 768 bytes, 16 each.  What lies outside the image: pixels are replicated to the right and down (expand_right_edge, expand_bottom_edge),
// the chroma rows below the last downsampled row repeat THAT row, and a Y block wholly outside the component's ceil(w / 8) x ceil(h / 8)
// blocks is libjpeg's dummy block (jccoefct.c compress_data: all zero but the DC of the block before it in the MCU).

// natural order: quantisation divisor (q << 3) of every quality 1 .. 100 (luma, chroma), zigzag position
struct FrameTab { unsigned short div[100][2][64]; unsigned char zz[64]; };
constexpr FrameTab make_frame_tab() {
    FrameTab t{};
    for (int z = 0; z < 64; ++z) t.zz[kNatural[z]] = (unsigned char)z;
    for (int q = 1; q <= 100; ++q)
        for (int n = 0; n < 64; ++n) {
            t.div[q - 1][0][n] = (unsigned short)(8 * q_scaled(kStdLuma[n], q));
            t.div[q - 1][1][n] = (unsigned short)(8 * q_scaled(kStdChroma[n], q));
        }
    return t;
}
__constant__ FrameTab kFrameTab = make_frame_tab();

struct FrameParams {
    const unsigned char* img;
    long long img_bytes;
    const aq_frame* frames;
    int n_frames;
    int n_mcus;                   // of this piece
    short* coef;                  // MCU frames[0].mcu of the batch is arena MCU 0
    int quality;                  // 1 .. 100
};

__global__ __launch_bounds__(256) void frame_jpeg_kernel(const FrameParams p) {
    __shared__ int s_blk[4][6][8][9];                         // level-shifted samples, then row-pass values (rows padded: column reads spread over banks)
    __shared__ unsigned char s_c[4][2][16][16];               // Cb, Cr at full resolution
    __shared__ __attribute__((aligned(16))) short s_q[4][6][64];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int mcu0 = p.frames[0].mcu;
    const int groups = (p.n_mcus + 3) >> 2;
    for (int grp = blockIdx.x; grp < groups; grp += gridDim.x) {          // (the same trip count for all four waves: they share the barriers)
        const int m = grp * 4 + wave;
        const bool live = m < p.n_mcus;
        const int g = mcu0 + m;
        int lo = 0, hi = p.n_frames - 1;                      // the frame that holds MCU g: the last one that starts at or before it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.frames[mid].mcu <= g) lo = mid; else hi = mid - 1;
        }
        const aq_frame f = p.frames[lo];
        const int w = f.w, h = f.h, mw = (w + 15) >> 4, k = g - f.mcu, my = k / max(mw, 1), mx = k - my * mw;
        const bool ok = live && w > 0 && h > 0 && f.base >= 0 && f.pitch >= 3LL * w && my < ((h + 15) >> 4) &&
                        f.base + (long long)(h - 1) * f.pitch + 3LL * w <= p.img_bytes;
        if (ok) {
            // rgb_ycc_convert (jccolor.c): lane = (row, four pixels)
            const int r = lane >> 2, c0 = (lane & 3) * 4;
            const int y = min(16 * my + r, h - 1), x0 = 16 * mx + c0;
            const unsigned char* row = p.img + f.base + (long long)y * f.pitch;
            unsigned char px[12];
            if (x0 + 3 < w && (((uintptr_t)(row + 3 * x0)) & 3) == 0) {
                const uint3 v = *(const uint3*)(row + 3 * x0);
                const unsigned u[3] = {v.x, v.y, v.z};
#pragma unroll
                for (int i = 0; i < 12; ++i) px[i] = (unsigned char)(u[i >> 2] >> (8 * (i & 3)));
            } else {
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const unsigned char* q = row + 3 * min(x0 + e, w - 1);
                    px[3 * e] = q[0]; px[3 * e + 1] = q[1]; px[3 * e + 2] = q[2];
                }
            }
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int R = px[3 * e], G = px[3 * e + 1], B = px[3 * e + 2], c = c0 + e;
                s_blk[wave][(r >> 3) * 2 + (c >> 3)][r & 7][c & 7] = ((19595 * R + 38470 * G + 7471 * B + 32768) >> 16) - 128;
                s_c[wave][0][r][c] = (unsigned char)((-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16);
                s_c[wave][1][r][c] = (unsigned char)((32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16);
            }
        }
        __syncthreads();
        if (ok) {
            // h2v2_downsample: lane = (chroma row, chroma column); bias 1, 2, 1, 2 ... along the row
            const int cy = lane >> 3, cx = lane & 7;
            const int cyl = min(8 * my + cy, ((h + 1) >> 1) - 1) - 8 * my;      // below the last downsampled row: that row again
            const int bias = 1 + (cx & 1);
#pragma unroll
            for (int c = 0; c < 2; ++c) {
                const unsigned char* a = &s_c[wave][c][2 * cyl][2 * cx];
                s_blk[wave][4 + c][cy][cx] = ((a[0] + a[1] + a[16] + a[17] + bias) >> 2) - 128;
            }
        }
        __syncthreads();
        const int b = lane >> 3, i = lane & 7;
        if (ok && lane < 48) {                                // rows
            int v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = s_blk[wave][b][i][e];
            fdct8<1, false>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e) s_blk[wave][b][i][e] = v[e];
        }
        __syncthreads();
        if (ok && lane < 48) {                                // columns, quantisation (divisor q << 3, half away from zero), zigzag order
            int v[8];
#pragma unroll
            for (int e = 0; e < 8; ++e) v[e] = s_blk[wave][b][e][i];
            fdct8<1, true>(v);
#pragma unroll
            for (int e = 0; e < 8; ++e) {
                const int n = 8 * e + i, div = kFrameTab.div[p.quality - 1][b >= 4][n];
                const int a = ((v[e] < 0 ? -v[e] : v[e]) + (div >> 1)) / div;
                s_q[wave][b][kFrameTab.zz[n]] = (short)(v[e] < 0 ? -a : a);
            }
        }
        __syncthreads();
        // dummy blocks of the Y component
        const int wib = (w + 7) >> 3, hib = (h + 7) >> 3;
        const bool row1 = 2 * my + 1 < hib, col1 = 2 * mx + 1 < wib;
        if (ok) {
            if (!col1) s_q[wave][1][lane] = 0;
            if (!row1 || !col1) s_q[wave][3][lane] = 0;
            if (!row1) s_q[wave][2][lane] = 0;
        }
        __syncthreads();
        if (ok && lane == 0) {
            if (!col1) s_q[wave][1][0] = s_q[wave][0][0];
            if (!row1) { s_q[wave][2][0] = s_q[wave][1][0]; s_q[wave][3][0] = s_q[wave][1][0]; }
            else if (!col1) s_q[wave][3][0] = s_q[wave][2][0];
        }
        __syncthreads();
        if (live && lane < 48) {                              // (a frame the launcher would have refused: zeros, never a read outside the images)
            const uint4 v = ok ? *(const uint4*)(&s_q[wave][0][0] + 8 * lane) : make_uint4(0, 0, 0, 0);
            *(uint4*)(p.coef + (long long)m * 384 + 8 * lane) = v;
        }
        __syncthreads();
    }
}

// ---- host half: Huffman coding and the JFIF stream (jchuff.c, jcmarker.c) ----

// Annex K.3 tables: code counts per length 1..16, then the symbols
const unsigned char kDcLumaBits[16] = {0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0};
const unsigned char kDcChromaBits[16] = {0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0};
const unsigned char kDcVals[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 11};
const unsigned char kAcLumaBits[16] = {0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d};
const unsigned char kAcLumaVals[162] = {
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};
const unsigned char kAcChromaBits[16] = {0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77};
const unsigned char kAcChromaVals[162] = {
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa};

struct HuffCode { unsigned short code[256]; unsigned char size[256]; };

// jpeg_make_c_derived_tbl: canonical codes in order of length
HuffCode derive(const unsigned char* bits, const unsigned char* vals) {
    HuffCode t;
    memset(&t, 0, sizeof(t));
    unsigned code = 0;
    int k = 0;
    for (int len = 1; len <= 16; ++len) {
        for (int i = 0; i < bits[len - 1]; ++i, ++k) {
            t.code[vals[k]] = (unsigned short)code++;
            t.size[vals[k]] = (unsigned char)len;
        }
        code <<= 1;
    }
    return t;
}

const HuffCode kDc[2] = {derive(kDcLumaBits, kDcVals), derive(kDcChromaBits, kDcVals)};
const HuffCode kAc[2] = {derive(kAcLumaBits, kAcLumaVals), derive(kAcChromaBits, kAcChromaVals)};

struct BitWriter {
    std::vector<unsigned char>& out;
    unsigned long long buf = 0;
    int n = 0;                                                // bits held in buf (< 8 between calls)
    explicit BitWriter(std::vector<unsigned char>& o) : out(o) {}
    void put(unsigned code, int size) {
        buf = (buf << size) | (code & ((1u << size) - 1));
        n += size;
        while (n >= 8) {
            n -= 8;
            const unsigned char b = (unsigned char)(buf >> n);
            out.push_back(b);
            if (b == 0xFF) out.push_back(0);                  // byte stuffing
        }
    }
    void flush() {                                            // the last byte padded with 1-bits
        if (n > 0) put(0x7F, 8 - n);
    }
};

inline int nbits(int v) { return v ? 32 - __builtin_clz((unsigned)v) : 0; }

// h2v2: 4:2:0 (Y sampled 2 x 2) instead of 4:4:4
void marker_header(std::vector<unsigned char>& o, int w, int h, bool h2v2, int quality) {
    auto u8 = [&](int v) { o.push_back((unsigned char)v); };
    auto u16 = [&](int v) { u8(v >> 8); u8(v & 255); };
    u16(0xFFD8);                                              // SOI
    u16(0xFFE0); u16(16);                                     // APP0: JFIF 1.01, no units, density 1:1, no thumbnail
    for (const char ch : {'J', 'F', 'I', 'F', '\0'}) u8(ch);
    u8(1); u8(1); u8(0); u16(1); u16(1); u8(0); u8(0);
    for (int t = 0; t < 2; ++t) {                             // DQT x 2, 8-bit entries in zigzag order
        u16(0xFFDB); u16(67); u8(t);
        for (int z = 0; z < 64; ++z) u8(q_scaled(t ? kStdChroma[kNatural[z]] : kStdLuma[kNatural[z]], quality));
    }
    u16(0xFFC0); u16(17); u8(8); u16(h); u16(w); u8(3);       // SOF0: components 1, 2, 3, sampling 1x1 each (or 2x2 / 1x1 / 1x1), tables 0 / 1 / 1
    for (int c = 0; c < 3; ++c) { u8(c + 1); u8(h2v2 && c == 0 ? 0x22 : 0x11); u8(c ? 1 : 0); }
    const unsigned char* bits[4] = {kDcLumaBits, kAcLumaBits, kDcChromaBits, kAcChromaBits};
    const unsigned char* vals[4] = {kDcVals, kAcLumaVals, kDcVals, kAcChromaVals};
    const int cls[4] = {0x00, 0x10, 0x01, 0x11};
    for (int t = 0; t < 4; ++t) {                             // DHT x 4 in the order the scan header sends them: DC 0, AC 0, DC 1, AC 1
        int n = 0;
        for (int i = 0; i < 16; ++i) n += bits[t][i];
        u16(0xFFC4); u16(2 + 1 + 16 + n); u8(cls[t]);
        for (int i = 0; i < 16; ++i) u8(bits[t][i]);
        for (int i = 0; i < n; ++i) u8(vals[t][i]);
    }
    u16(0xFFDA); u16(12); u8(3);                              // SOS: all three components, Ss 0, Se 63, Ah / Al 0
    for (int c = 0; c < 3; ++c) { u8(c + 1); u8(c ? 0x11 : 0x00); }
    u8(0); u8(63); u8(0);
}

// One block: DC difference, AC run lengths (jchuff.c encode_one_block)
inline void encode_block(BitWriter& bw, const int16_t* blk, int& last_dc, const HuffCode& dc, const HuffCode& ac) {
    int diff = blk[0] - last_dc;
    last_dc = blk[0];
    int nb = nbits(diff < 0 ? -diff : diff);
    bw.put(dc.code[nb], dc.size[nb]);
    if (nb) bw.put((unsigned)(diff < 0 ? diff - 1 : diff), nb);
    int run = 0;
    for (int k = 1; k < 64; ++k) {
        const int v = blk[k];
        if (v == 0) { ++run; continue; }
        while (run > 15) { bw.put(ac.code[0xF0], ac.size[0xF0]); run -= 16; }   // ZRL
        nb = nbits(v < 0 ? -v : v);
        const int sym = (run << 4) + nb;
        bw.put(ac.code[sym], ac.size[sym]);
        bw.put((unsigned)(v < 0 ? v - 1 : v), nb);
        run = 0;
    }
    if (run > 0) bw.put(ac.code[0], ac.size[0]);             // EOB
}

// One image -> the whole file.  4:4:4 (a crop): coef = its block positions, raster order, Y / Cb / Cr each.  h2v2 (a frame): coef = its
// 16 x 16 MCUs, raster order, Y00 Y01 Y10 Y11 Cb Cr each: the interleaved scan's own order.  Blocks in zigzag order; DC prediction per component.
void encode_jpeg(const int16_t* coef, int w, int h, std::vector<unsigned char>& o, bool h2v2 = false, int quality = 95) {
    o.clear();
    const int unit = h2v2 ? 16 : 8, per = h2v2 ? 6 : 3;
    const long long n = (long long)((w + unit - 1) / unit) * ((h + unit - 1) / unit);
    o.reserve(700 + (size_t)n * per * 32);
    marker_header(o, w, h, h2v2, quality);
    BitWriter bw(o);
    int last_dc[3] = {0, 0, 0};
    for (long long u = 0; u < n; ++u) {
        for (int b = 0; b < per; ++b) {
            const int c = h2v2 ? (b < 4 ? 0 : b - 3) : b;
            encode_block(bw, coef + (u * per + b) * 64, last_dc[c], kDc[c ? 1 : 0], kAc[c ? 1 : 0]);
        }
    }
    bw.flush();
    o.push_back(0xFF);
    o.push_back(0xD9);                                        // EOI
}

// mkdir -p of rel's directories under dir; EEXIST is success (several ranks and threads create the same class directories)
bool make_parents(const std::string& dir, const char* rel) {
    std::string p = dir;
    for (const char* s = rel; *s; ++s) {
        if (*s == '/' && s != rel) {
            p.assign(dir);
            p += '/';
            p.append(rel, (size_t)(s - rel));
            if (mkdir(p.c_str(), 0777) != 0 && errno != EEXIST) return false;
        }
    }
    return true;
}

// n files on threads of their own: encode(i, bytes) -> <dir>/<rel_paths[i]>, truncating; the directories on the way are created.  n_threads
// threads take the files in turn; do_fsync: fsync every file before closing it.  Returns n, or -1 - i when file i could not be written.
template <class Encode>
long write_files(const char* dir, const char* const* rel_paths, int n, int n_threads, int do_fsync, Encode encode) {
    const std::string root(dir);
    std::atomic<int> next{0};
    std::atomic<long> failed{-1};
    auto work = [&]() {
        std::vector<unsigned char> o;
        std::string path;
        for (int i; (i = next.fetch_add(1)) < n && failed.load() < 0;) {
            if (!encode(i, o)) { failed = i; return; }
            path.assign(root);
            path += '/';
            path += rel_paths[i];
            FILE* f = fopen(path.c_str(), "wb");
            if (!f && errno == ENOENT && make_parents(root, rel_paths[i])) f = fopen(path.c_str(), "wb");
            if (!f) { failed = i; return; }
            const bool ok = fwrite(o.data(), 1, o.size(), f) == o.size() && fflush(f) == 0 && (!do_fsync || fsync(fileno(f)) == 0);
            if (fclose(f) != 0 || !ok) { failed = i; return; }
        }
    };
    const int nt = n_threads < 1 ? 1 : (n_threads > 64 ? 64 : (n_threads > n ? (n > 0 ? n : 1) : n_threads));
    std::vector<std::thread> ts;
    for (int t = 1; t < nt; ++t) ts.emplace_back(work);
    work();
    for (auto& t : ts) t.join();
    return failed.load() >= 0 ? -1 - failed.load() : (long)n;
}

}  // namespace

// One piece of a batch's crops: coefficient blocks of every block position of crops_dev[0 .. n_crops) into coef_dev (n_blocks positions,
// the first crop's first position at coef_dev).  crops_dev: sorted by block, back to back (crop i + 1 starts where crop i ends).
extern "C" int aq_crop_jpeg_coefs(const uint8_t* images_dev, long long image_bytes, const aq_crop* crops_dev, int n_crops, int n_blocks,
                                  int16_t* coef_dev, void* stream) {
    AQ_REQUIRE(images_dev && crops_dev && coef_dev, "crop_jpeg_coefs: null pointer");
    AQ_REQUIRE(n_crops > 0 && n_blocks > 0 && image_bytes > 0, "crop_jpeg_coefs: bad sizes (%d crops, %d blocks)", n_crops, n_blocks);
    AQ_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)crops_dev & 7) == 0, "crop_jpeg_coefs: unaligned buffer");
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    CropParams p;
    p.img = images_dev; p.img_bytes = image_bytes; p.crops = crops_dev; p.n_crops = n_crops; p.n_threads = 3LL * n_blocks;
    p.coef = (short*)coef_dev;
    const long long groups = (p.n_threads + 255) / 256;
    const unsigned grid = (unsigned)(groups < 16LL * cus ? groups : 16LL * cus);
    hipLaunchKernelGGL(crop_jpeg_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

// The JPEG file of one w x h crop from its coefficient blocks; bytes written, or -(bytes needed) when buflen is too small.
extern "C" long aq_crop_jpeg_bytes(const int16_t* coef, int w, int h, uint8_t* buf, size_t buflen) {
    if (!coef || w <= 0 || h <= 0 || w > 65535 || h > 65535) return 0;
    std::vector<unsigned char> o;
    encode_jpeg(coef, w, h, o);
    if (!buf || o.size() > buflen) return -(long)o.size();
    memcpy(buf, o.data(), o.size());
    return (long)o.size();
}

// A batch of crop files: crop i (coefficients from block position crops[i].block of coef) -> <dir>/<rel_paths[i]>, truncating; the
// directories on the way are created.  n_threads threads take the crops in turn; do_fsync: fsync every file before closing it (the
// fallback where syncfs is unavailable).  Returns the number of files written, or -1 - i when crop i could not be written.
extern "C" long aq_write_crop_files(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_crop* crops, int n_crops,
                                    int n_threads, int do_fsync) {
    if (!dir || !rel_paths || !coef || !crops || n_crops < 0) return -1;
    return write_files(dir, rel_paths, n_crops, n_threads, do_fsync, [&](int i, std::vector<unsigned char>& o) {
        const aq_crop& c = crops[i];
        const int w = c.x2 - c.x1, h = c.y2 - c.y1;
        if (w <= 0 || h <= 0 || w > 65535 || h > 65535) return false;
        encode_jpeg(coef + (size_t)c.block * 192, w, h, o);
        return true;
    });
}
// One piece of a batch's frames, 4:2:0: the MCUs of frames_dev[0 .. n_frames) into coef_dev (n_mcus MCUs of 6 x 64 int16, the first frame's
// first MCU at coef_dev).  frames: sorted by mcu, back to back; frames_host = the same table in host memory, checked here: a frame that
// leaves [images_dev, images_dev + image_bytes) is refused before anything is launched.
// quality: libjpeg's 1 .. 100 (jpeg_set_quality; the DQT segments aq_image_jpeg_bytes_q writes follow the same tables).
extern "C" int aq_image_jpeg_coefs_q(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host,
                                     int n_frames, int n_mcus, int quality, int16_t* coef_dev, void* stream) {
    AQ_REQUIRE(images_dev && frames_dev && frames_host && coef_dev, "image_jpeg_coefs: null pointer");
    AQ_REQUIRE(quality >= 1 && quality <= 100, "image_jpeg_coefs: quality %d (1 to 100)", quality);
    AQ_REQUIRE(n_frames > 0 && n_mcus > 0 && image_bytes > 0, "image_jpeg_coefs: bad sizes (%d frames, %d MCUs)", n_frames, n_mcus);
    AQ_REQUIRE(((uintptr_t)coef_dev & 15) == 0 && ((uintptr_t)frames_dev & 7) == 0, "image_jpeg_coefs: unaligned buffer");
    long long next = frames_host[0].mcu;
    for (int i = 0; i < n_frames; ++i) {
        const aq_frame& f = frames_host[i];
        AQ_REQUIRE(f.w > 0 && f.h > 0 && f.w <= 65535 && f.h <= 65535 && f.base >= 0 && f.pitch >= 3LL * f.w &&
                   f.base + (long long)(f.h - 1) * f.pitch + 3LL * f.w <= image_bytes,
                   "image_jpeg_coefs: frame %d (%d x %d, pitch %d, at byte %lld) is empty or leaves its buffer of %lld bytes", i, f.w, f.h, f.pitch,
                   (long long)f.base, image_bytes);
        AQ_REQUIRE(f.mcu == next, "image_jpeg_coefs: frame %d starts at MCU %d, not where frame %d ends (%lld)", i, f.mcu, i - 1, next);
        next += (long long)((f.w + 15) / 16) * ((f.h + 15) / 16);
    }
    AQ_REQUIRE(next - frames_host[0].mcu == n_mcus, "image_jpeg_coefs: the frames hold %lld MCUs, not %d", next - frames_host[0].mcu, n_mcus);
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    FrameParams p;
    p.img = images_dev; p.img_bytes = image_bytes; p.frames = frames_dev; p.n_frames = n_frames; p.n_mcus = n_mcus; p.coef = (short*)coef_dev;
    p.quality = quality;
    const long long groups = ((long long)n_mcus + 3) / 4;
    const unsigned grid = (unsigned)(groups < 32LL * cus ? groups : 32LL * cus);
    hipLaunchKernelGGL(frame_jpeg_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_image_jpeg_coefs(const uint8_t* images_dev, long long image_bytes, const aq_frame* frames_dev, const aq_frame* frames_host,
                                   int n_frames, int n_mcus, int16_t* coef_dev, void* stream) {
    return aq_image_jpeg_coefs_q(images_dev, image_bytes, frames_dev, frames_host, n_frames, n_mcus, 95, coef_dev, stream);
}

// The JPEG file of one w x h frame, 4:2:0, from its MCUs; bytes written, or -(bytes needed) when buflen is too small (0: bad arguments).
extern "C" long aq_image_jpeg_bytes_q(const int16_t* coef, int w, int h, int quality, uint8_t* buf, size_t buflen) {
    if (!coef || w <= 0 || h <= 0 || w > 65535 || h > 65535 || quality < 1 || quality > 100) return 0;
    std::vector<unsigned char> o;
    encode_jpeg(coef, w, h, o, true, quality);
    if (!buf || o.size() > buflen) return -(long)o.size();
    memcpy(buf, o.data(), o.size());
    return (long)o.size();
}

extern "C" long aq_image_jpeg_bytes(const int16_t* coef, int w, int h, uint8_t* buf, size_t buflen) {
    return aq_image_jpeg_bytes_q(coef, w, h, 95, buf, buflen);
}

// A batch of frame files: frame i (coefficients from MCU frames[i].mcu of coef) -> <dir>/<rel_paths[i]>, as aq_write_crop_files writes crops.
// Returns the number of files written, or -1 - i when frame i could not be written.
extern "C" long aq_write_image_files_q(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_frame* frames, int n_frames,
                                       int quality, int n_threads, int do_fsync) {
    if (!dir || !rel_paths || !coef || !frames || n_frames < 0 || quality < 1 || quality > 100) return -1;
    return write_files(dir, rel_paths, n_frames, n_threads, do_fsync, [&](int i, std::vector<unsigned char>& o) {
        const aq_frame& f = frames[i];
        if (f.w <= 0 || f.h <= 0 || f.w > 65535 || f.h > 65535) return false;
        encode_jpeg(coef + (size_t)f.mcu * 384, f.w, f.h, o, true, quality);
        return true;
    });
}

extern "C" long aq_write_image_files(const char* dir, const char* const* rel_paths, const int16_t* coef, const aq_frame* frames, int n_frames,
                                     int n_threads, int do_fsync) {
    return aq_write_image_files_q(dir, rel_paths, coef, frames, n_frames, 95, n_threads, do_fsync);
}
