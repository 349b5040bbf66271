// Test-time augmentation (detect.py --augment): the geometry of the three passes, the bilinear tap tables and the scaled space-to-depth
// preprocess.  [UPSTREAM models/yolo.py DetectionModel._forward_augment, _descale_pred, _clip_augmented; utils/torch_utils.py scale_img]
// Compiled with -ffp-contract=off: the tap arithmetic is PyTorch's CPU fp32 sequence, and the host and device copies of it must agree.
#include "aq_common.h"
#include <cmath>

namespace {

constexpr float kAugScale[3] = {1.0f, 0.83f, 0.67f};   // [UPSTREAM _forward_augment: s = [1, 0.83, 0.67]]
constexpr int kAugFlip[3] = {0, 1, 0};                  // [UPSTREAM: f = [None, 3, None]] (3 = left-right)
constexpr double kAugScaleD[3] = {1.0, 0.83, 0.67};     // the Python floats scale_img multiplies by
constexpr int kGs = 32;                                 // [UPSTREAM scale_img(gs=32)]

// [UPSTREAM aten UpSample.h area_pixel_compute_scale / area_pixel_compute_source_index, UpSampleKernel.cpp compute_indices_weights_linear]
__host__ __device__ inline aq_tap make_tap(int in, int out, int d, int flip) {
    const float scale = (float)in / (float)out;
    float src = fmaf(scale, (float)d + 0.5f, -0.5f);   // PyTorch's CPU build contracts scale * (d + 0.5) - 0.5 into one fused multiply-add
    if (src < 0.0f) src = 0.0f;
    aq_tap t;
    t.i0 = (int)src;
    t.i1 = t.i0 + (t.i0 < in - 1 ? 1 : 0);
    float l1 = src - (float)t.i0;
    l1 = l1 < 0.0f ? 0.0f : (l1 > 1.0f ? 1.0f : l1);
    t.l1 = l1;
    t.l0 = 1.0f - l1;
    if (flip) { t.i0 = in - 1 - t.i0; t.i1 = in - 1 - t.i1; }
    return t;
}

__global__ void fill_taps_kernel(aq_tap* taps, int in, int out, int flip) {
    const int d = blockIdx.x * blockDim.x + threadIdx.x;
    if (d < out) taps[d] = make_tap(in, out, d, flip);
}

// out[b][Y][X][(dy*2+dx)*3 + c] = value of (2Y+dy, 2X+dx, c) of the scaled network input, channels 12..15 = 0 (aq_preprocess_s2d's layout)
template <bool F32>
__global__ __launch_bounds__(256) void preprocess_s2d_scaled_kernel(const uint8_t* __restrict__ in, char* __restrict__ out, int B, int H0, int W0,
                                                                   const aq_tap* __restrict__ ytab, const aq_tap* __restrict__ xtab,
                                                                   int h, int w, int hp, int wp) {
    const int H2 = hp >> 1, W2 = wp >> 1;
    const unsigned n = (unsigned)B * H2 * W2;
    for (unsigned i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) {
        const unsigned t = i / (unsigned)W2;
        const int X = (int)(i - t * W2);
        const int b = (int)(t / (unsigned)H2), Y = (int)(t - (unsigned)b * H2);
        const uint8_t* img = in + (size_t)b * H0 * W0 * 3;
        float v[16];
#pragma unroll
        for (int dy = 0; dy < 2; ++dy)
#pragma unroll
            for (int e = 0; e < 6; ++e) v[dy * 6 + e] = aq_aug_value(img, W0, ytab, xtab, h, w, hp, wp, 2 * Y + dy, 2 * X + e / 3, e % 3);
        v[12] = v[13] = v[14] = v[15] = 0.0f;
        if (F32) {
            f32x4* o = (f32x4*)(out + (size_t)i * 64);
#pragma unroll
            for (int q = 0; q < 4; ++q) { f32x4 x = {v[4 * q], v[4 * q + 1], v[4 * q + 2], v[4 * q + 3]}; o[q] = x; }
        } else {
            uint4* o = (uint4*)(out + (size_t)i * 32);
#pragma unroll
            for (int q = 0; q < 2; ++q) {
                uint4 x;
                x.x = aq_f2bf(v[8 * q + 0]) | ((uint32_t)aq_f2bf(v[8 * q + 1]) << 16);
                x.y = aq_f2bf(v[8 * q + 2]) | ((uint32_t)aq_f2bf(v[8 * q + 3]) << 16);
                x.z = aq_f2bf(v[8 * q + 4]) | ((uint32_t)aq_f2bf(v[8 * q + 5]) << 16);
                x.w = aq_f2bf(v[8 * q + 6]) | ((uint32_t)aq_f2bf(v[8 * q + 7]) << 16);
                o[q] = x;
            }
        }
    }
}

}  // namespace

extern "C" int aq_augment_geometry(int H, int W, int na, aq_augment_pass* passes, int* n_aug) {
    AQ_REQUIRE(passes && n_aug, "augment_geometry: null pointer");
    AQ_REQUIRE(H >= kGs && W >= kGs && H % kGs == 0 && W % kGs == 0 && na >= 1 && na <= 8,
               "augment_geometry: tile size must be a positive multiple of %d (got %dx%d), na in [1, 8]", kGs, H, W);
    constexpr int kLevels = 21;                         // [UPSTREAM _clip_augmented: g = sum(4 ** x for x in range(nl)), nl = 3]
    int out = 0;
    for (int i = 0; i < 3; ++i) {
        aq_augment_pass& p = passes[i];
        const double s = kAugScaleD[i];
        p.scale = kAugScale[i];
        p.flip = kAugFlip[i];
        if (i == 0) {                                   // [UPSTREAM scale_img: `if ratio == 1.0: return img`]
            p.h = p.hp = H;
            p.w = p.wp = W;
        } else {
            p.h = (int)(H * s);
            p.w = (int)(W * s);
            p.hp = (int)std::ceil(H * s / kGs) * kGs;
            p.wp = (int)std::ceil(W * s / kGs) * kGs;
        }
        const int p5 = na * (p.hp / 32) * (p.wp / 32);
        p.rows = p5 * kLevels;                          // na (16 + 4 + 1) x the P5 grid
        p.keep_first = 0;
        p.keep_count = p.rows;
        p.level_mask = 7;
        if (i == 0) {                                   // y[0] = y[0][:, :-(N0 // g) * 1]: the P5 level
            p.keep_count = p.rows - (p.rows / kLevels);
            p.level_mask = 3;
        } else if (i == 2) {                            // y[-1] = y[-1][:, (N2 // g) * 16:]: the P3 level
            p.keep_first = (p.rows / kLevels) * 16;
            p.keep_count = p.rows - p.keep_first;
            p.level_mask = 6;
        }
        p.out_first = out;
        out += p.keep_count;
    }
    *n_aug = out;
    return AQ_OK;
}

extern "C" int aq_augment_taps(int in, int out, int flip, aq_tap* taps) {
    AQ_REQUIRE(taps && in > 0 && out > 0, "augment_taps: bad arguments");
    for (int d = 0; d < out; ++d) taps[d] = make_tap(in, out, d, flip);
    return AQ_OK;
}

int aq_augment_fill_taps(aq_tap* taps_dev, int in, int out, int flip, hipStream_t stream) {
    AQ_REQUIRE(taps_dev && in > 0 && out > 0, "augment_fill_taps: bad arguments");
    hipLaunchKernelGGL(fill_taps_kernel, dim3((unsigned)((out + 255) / 256)), dim3(256), 0, stream, taps_dev, in, out, flip);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_preprocess_s2d_scaled(const uint8_t* tiles_dev, int H0, int W0, const aq_tap* ytab_dev, const aq_tap* xtab_dev, int h, int w,
                                        void* out_dev, int B, int hp, int wp, int precision, void* stream) {
    AQ_REQUIRE(tiles_dev && ytab_dev && xtab_dev && out_dev, "preprocess_scaled: null pointer");
    AQ_REQUIRE(B > 0 && H0 > 0 && W0 > 0 && hp > 0 && wp > 0 && hp % 2 == 0 && wp % 2 == 0 && h > 0 && w > 0 && h <= hp && w <= wp,
               "preprocess_scaled: bad shape B=%d %dx%d -> %dx%d in %dx%d", B, H0, W0, h, w, hp, wp);
    const long long n = (long long)B * (hp / 2) * (wp / 2);
    AQ_REQUIRE(n < (1LL << 31) && (long long)B * H0 * W0 * 3 < (1LL << 40), "preprocess_scaled: batch too large");
    long long g = (n + 255) / 256;
    if (g > 256 * 16) g = 256 * 16;
    if (precision == AQ_FP32 || precision == AQ_F16X3)
        hipLaunchKernelGGL(preprocess_s2d_scaled_kernel<true>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, tiles_dev, (char*)out_dev,
                           B, H0, W0, ytab_dev, xtab_dev, h, w, hp, wp);
    else
        hipLaunchKernelGGL(preprocess_s2d_scaled_kernel<false>, dim3((unsigned)g), dim3(256), 0, (hipStream_t)stream, tiles_dev, (char*)out_dev,
                           B, H0, W0, ytab_dev, xtab_dev, h, w, hp, wp);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
