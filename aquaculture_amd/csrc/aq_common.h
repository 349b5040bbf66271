// Shared declarations for the HIP translation units of libaqengine.so (gfx950 only).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stddef.h>
#include <stdlib.h>
#include "../../include/aq_engine.h"
#include "size_guards.h"   // the launchers' size limits (host arithmetic)

typedef unsigned short bf16_t;  // raw bf16 bits
typedef __attribute__((ext_vector_type(8))) short bf16x8;
typedef __attribute__((ext_vector_type(4))) float f32x4;
typedef __attribute__((ext_vector_type(16))) float f32x16;

void aq_set_error(const char* fmt, ...);
#define AQ_CHECK_HIP(expr)                                                              \
    do {                                                                                \
        hipError_t _e = (expr);                                                         \
        if (_e != hipSuccess) {                                                         \
            aq_set_error("%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__, __LINE__); \
            return AQ_ERR_HIP;                                                          \
        }                                                                               \
    } while (0)
#define AQ_REQUIRE(cond, ...)                                                           \
    do {                                                                                \
        if (!(cond)) {                                                                  \
            aq_set_error(__VA_ARGS__);                                                  \
            return AQ_ERR_INVALID;                                                      \
        }                                                                               \
    } while (0)

static inline int aq_elem_bytes(int precision) { return (precision == AQ_FP32 || precision == AQ_F16X3) ? 4 : 2; }

// f32 -> bf16 round-to-nearest-even (finite inputs; NaN stays NaN via the quiet bit)
__host__ __device__ static inline bf16_t aq_f2bf(float f) {
    union { float f; uint32_t u; } v; v.f = f;
    if ((v.u & 0x7fffffffu) > 0x7f800000u) return (bf16_t)((v.u >> 16) | 0x40);
    return (bf16_t)((v.u + 0x7fffu + ((v.u >> 16) & 1u)) >> 16);
}
__host__ __device__ static inline float aq_bf2f(bf16_t h) {
    union { float f; uint32_t u; } v; v.u = ((uint32_t)h) << 16; return v.f;
}

// ---- test-time augmentation (augment.hip, stem_conv.hip) ----
// Channel c of pixel (y, x) of the network input of a scaled pass: scale_img(flip(u8 / 255)) [UPSTREAM utils/torch_utils.py scale_img] --
// the bilinear sample inside h x w, 0.447 in the padding up to hp x wp, 0 (the conv's own zero padding) outside.  img: one uint8 RGB tile
// of width W0.  Every rounding is explicit (no contraction): h0 (w0 x00 + w1 x01) + h1 (w0 x10 + w1 x11), as PyTorch's CPU kernel.
__device__ static inline float aq_aug_value(const uint8_t* img, int W0, const aq_tap* ytab, const aq_tap* xtab, int h, int w, int hp, int wp,
                                            int y, int x, int c) {
    if (y < 0 || y >= hp || x < 0 || x >= wp) return 0.0f;
    if (y >= h || x >= w) return 0.447f;
    const aq_tap ty = ytab[y], tx = xtab[x];
    const uint8_t* r0 = img + (size_t)ty.i0 * W0 * 3;
    const uint8_t* r1 = img + (size_t)ty.i1 * W0 * 3;
    const float x00 = (float)r0[tx.i0 * 3 + c] / 255.0f, x01 = (float)r0[tx.i1 * 3 + c] / 255.0f;
    const float x10 = (float)r1[tx.i0 * 3 + c] / 255.0f, x11 = (float)r1[tx.i1 * 3 + c] / 255.0f;
    const float t0 = __fadd_rn(__fmul_rn(tx.l0, x00), __fmul_rn(tx.l1, x01));
    const float t1 = __fadd_rn(__fmul_rn(tx.l0, x10), __fmul_rn(tx.l1, x11));
    return __fadd_rn(__fmul_rn(ty.l0, t0), __fmul_rn(ty.l1, t1));
}
// Launches the fill of `out` taps (aq_augment_taps's arithmetic, on the device: the engine's augmented call writes its tables into its
// workspace instead of copying them from host memory).
int aq_augment_fill_taps(aq_tap* taps_dev, int in, int out, int flip, hipStream_t stream);

// ---- conv kernel parameter block (conv_igemm.hip) ----
struct ConvParams {
    const char* in;      // input tensor base + first-channel offset (bytes)
    char* out;
    const char* res;     // nullptr: none
    const char* w;       // packed [cout_pad][kgroups_pad] x 16 B
    const float* bias;   // [cout_pad]
    const char* zero;    // >= 16 zero bytes
    int in_ld_b, out_ld_b, res_ld_b;   // pixel strides in BYTES
    int B, H, W, Ho, Wo;
    int cout;            // real cout (multiple of 8)
    int k, stride, pad, taps;
    int G;               // 16-byte groups per tap = cin * sizeof(T) / 16
    int kgroups;         // taps * G
    int kgroups_pad;     // multiple of 8
    int nchunks;         // kgroups_pad / 8
    int npix;            // B * Ho * Wo
    int act;
    int n_tiles_m, n_tiles_n;
    int bias_n;          // bias entries staged into LDS (filled by aq_launch_conv)
    int x3_off;          // AQ_F16X3: the per-channel 2^-s follow the (scaled) bias at this float offset of `bias`
    unsigned long long* debug;   // diagnostic (stamped) builds only: per-wave phase cycle sums
    int halo, xrows, nixr, xper;   // conv_halo.hip: W + 1, region rows in LDS, region rows / 8, loads per step part
    float inv_hw, inv_wo;        // reciprocals for division-free pixel decode (filled by aq_launch_conv)
    unsigned magic_G, magic_k, magic_ntm;   // floor(2^32 / d) + 1
};

// Packed weight rows (and bias entries) beyond cout, all zero: a tile of BM rows whose first row is below cout reads BM whole rows, so
// the last tile row ends at most BM - 1 rows past cout.  384 = the tallest tile of any conv kernel (conv_halo.hip; the launchers check
// their tile tables against it).  With fewer, a taller tile reads past the packed buffer of a layer with few output channels.
constexpr int kConvCoutSlack = 384;

int aq_launch_conv(const ConvParams& p, int precision, int out_f32, int cfg, hipStream_t stream);
int aq_conv_pick_config(int cout, int npix, int precision);
int aq_launch_conv_halo(const ConvParams& p, int precision, int out_f32, int hcfg, bool one_tile_per_wg, hipStream_t stream);
int aq_conv_halo_num_configs();
int aq_conv_halo_tiles(int hcfg, int* bm, int* bn);
extern "C" int aq_conv_config_tiles(int cfg, int* bm, int* bn);
// aq_conv3x3_pl with the tile chosen for a batch of pick_B images (the engine passes its tuned table's batch size)
int aq_conv3x3_pl_at(const void* in_dev, long long in_sp, long long in_ss, int cin, void* out_dev, int out_ld, int out_choff, int cout,
                     const void* res_dev, int res_ld, int res_choff, const void* packed_w_dev, const float* bias_dev, int B, int H, int W,
                     int act, int pick_B, void* stream);
extern "C" int aq_conv_num_configs(void);

// ---- launch-time device state (launch_state.hip): kept per device, under one mutex ----
// Compute units the persistent grids are sized for: the device's count, or AQ_NUM_CUS when the caller runs this process's streams on a
// subset of the CUs (hipExtStreamCreateWithCUMask: bench.py --cu-split gives each of the two batches in flight half of the chip).
// Read once per device, so set the variable before the first launch.  Results do not depend on the count, bit for bit (which workgroup
// computes a tile changes nothing): tests/test_gpu_cu_counts.py runs every launcher that calls this at 1, 2, 3 and 13 CUs against the device's own.
hipError_t aq_cus(int* cus);
// The length of a persistent grid over `units` work items: per_cu workgroups per compute unit of aq_cus (so AQ_NUM_CUS applies), or `units`
// when that is fewer (at least 1).  Its one caller is mosaic.hip, whose CU-count cases are tests/val_plots_cu_cases.py: sizing the grid here
// keeps mosaic.hip out of the inventory tests/test_cu_cases.py takes of the files that call aq_cus themselves (DESIGN.md section 29 says why).
// Not for further launchers: a new one calls aq_cus and joins that inventory.
hipError_t aq_persistent_grid(long long units, int per_cu, unsigned* grid);
// Raises fn's dynamic-LDS limit to max_dyn_lds (once per device and kernel).
hipError_t aq_kernel_lds(const void* fn, int max_dyn_lds);
// aq_kernel_lds, then the workgroups of `threads` threads and `lds` bytes of dynamic LDS that stay resident per CU (at least 1).
hipError_t aq_kernel_blocks(const void* fn, int threads, size_t lds, int max_dyn_lds, int* blocks);
// Kernel `name` of an embedded code object, loaded once per device.  optional: a kernel the object lacks gives a null *fn, not an error.
hipError_t aq_asm_fn(const void* image, const char* name, hipFunction_t* fn, bool optional);
// Launches an assembly kernel: a 1-D grid, its argument block passed as one buffer.
hipError_t aq_asm_launch(hipFunction_t fn, unsigned grid, unsigned threads, void* args, size_t bytes, hipStream_t stream);
// 256 zero bytes on the CURRENT device (allocated on first use, one per device, never freed): the LDS-DMA source for pixels
// outside the image in the standalone kernel entry points (the engine passes its own zero page to the conv kernels).
const char* aq_zero_page();
// The stamp buffer aq_debug_conv_stamp armed, when it holds bytes_needed; else null (diagnostic builds only).
unsigned long long* aq_stamp_target(size_t bytes_needed);
