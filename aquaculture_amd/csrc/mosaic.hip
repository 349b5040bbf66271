// val.py --plots: the mosaic of the first images of a batch [UPSTREAM utils/plots.py plot_images], written in one launch straight from the
// letterboxed uint8 batch.  Upstream pastes image i at (W (i / ns), H (i % ns)) of a white ns H x ns W canvas and, when that is larger than
// max_size, cv2.resize()s the canvas to ns h x ns w.  Here the canvas is never materialised: every output pixel takes its two column taps
// and two row taps from the 11-bit tables of the ns W -> ns w and ns H -> ns h resizes (dataloader._axis_coeffs, as aq_letterbox_u8), and each
// tap's canvas coordinate (sx, sy) resolves to pixel (sx - W cx, sy - H cy) of image cx ns + cy, or to white where that cell holds no
// image.  Taps at a cell edge therefore blend two images, or an image and white, exactly as the resize of the pasted canvas does.  The
// arithmetic is resize_u8.h's, shared with the letterbox.  Without a resize (scale >= 1) the tables are the identity ones and the same
// kernel is the paste.
//
// Layout, as annotate.hip: a persistent grid of CU-sized length; a workgroup takes 1024 pixels of one output row at a time, four pixels
// (12 bytes) per lane, stored as three dwords where the address allows, byte by byte otherwise.  No LDS, no atomics.
#include "aq_common.h"
#include "resize_u8.h"

namespace {

struct MosaicParams {
    const unsigned char* batch;   // n images of H x W x 3, one after the other
    unsigned char* out;           // out_h x out_w x 3
    const int4* xtab;             // out_w entries (i0, i1, w0, w1), i in [0, ns W)
    const int4* ytab;             // out_h entries, i in [0, ns H)
    int n, ns, H, W, out_h, out_w;
    int chunks;                   // 1024-pixel pieces of a row
    int n_units;                  // out_h * chunks
};

__global__ __launch_bounds__(256) void mosaic_kernel(const MosaicParams p) {
    for (int u = blockIdx.x; u < p.n_units; u += gridDim.x) {
        const int y = u / p.chunks, x0 = (u - y * p.chunks) * 1024 + 4 * (int)threadIdx.x;
        if (x0 >= p.out_w) continue;
        const int cnt = min(4, p.out_w - x0);
        const int4 yt = p.ytab[y];
        // the two row taps: cell row and row inside the image.  The launcher has refused any host table with an index outside the source
        // mosaic, and that check is what the results rely on; the clamps here and below only keep the reads inside the batch if the device
        // table is not the copy of the host table the caller promised
        const int sy0 = min(max(yt.x, 0), p.ns * p.H - 1), sy1 = min(max(yt.y, 0), p.ns * p.H - 1);
        const int cy0 = sy0 / p.H, cy1 = sy1 / p.H;
        const int ly0 = sy0 - cy0 * p.H, ly1 = sy1 - cy1 * p.H;
        unsigned char px[12];
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            if (e >= cnt) { px[3 * e] = px[3 * e + 1] = px[3 * e + 2] = 0; continue; }
            const int4 xt = p.xtab[x0 + e];
            const int sxa = min(max(xt.x, 0), p.ns * p.W - 1), sxb = min(max(xt.y, 0), p.ns * p.W - 1);
            const int cxa = sxa / p.W, cxb = sxb / p.W;
            const int lxa = sxa - cxa * p.W, lxb = sxb - cxb * p.W;
            // image of each tap (>= n: white) and the tap's first byte
            const int i00 = cxa * p.ns + cy0, i01 = cxb * p.ns + cy0, i10 = cxa * p.ns + cy1, i11 = cxb * p.ns + cy1;
            const unsigned char* t00 = p.batch + (((long long)i00 * p.H + ly0) * p.W + lxa) * 3;
            const unsigned char* t01 = p.batch + (((long long)i01 * p.H + ly0) * p.W + lxb) * 3;
            const unsigned char* t10 = p.batch + (((long long)i10 * p.H + ly1) * p.W + lxa) * 3;
            const unsigned char* t11 = p.batch + (((long long)i11 * p.H + ly1) * p.W + lxb) * 3;
#pragma unroll
            for (int c = 0; c < 3; ++c) {
                const int p00 = i00 < p.n ? t00[c] : 255, p01 = i01 < p.n ? t01[c] : 255;
                const int p10 = i10 < p.n ? t10[c] : 255, p11 = i11 < p.n ? t11[c] : 255;
                px[3 * e + c] = aq_resize_linear_u8(p00, p01, p10, p11, xt.z, xt.w, yt.z, yt.w);
            }
        }
        unsigned char* d = p.out + ((long long)y * p.out_w + x0) * 3;
        if (cnt == 4 && ((uintptr_t)d & 3) == 0) {
            uint3 v;
            v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
            v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
            v.z = px[8] | (px[9] << 8) | (px[10] << 16) | ((unsigned)px[11] << 24);
            *(uint3*)d = v;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < 3 * cnt) d[i] = px[i];
        }
    }
}

}  // namespace

// The mosaic of the first n images (H x W uint8 RGB, one after the other at batch_dev) of a batch, ns x ns cells of h x w pixels, into
// out_dev (out_h x out_w x 3, rows 3 out_w bytes apart).  xtab / ytab: out_w / out_h entries (i0, i1, w0, w1) of the ns W -> out_w and
// ns H -> out_h resizes in device memory; *_host = the same tables in host memory, checked here: an index outside the source mosaic
// is refused before anything is launched.  Nothing is written on a refusal.
extern "C" int aq_val_mosaic_u8(const uint8_t* batch_dev, long long batch_bytes, int n, int ns, int H, int W, int h, int w, uint8_t* out_dev,
                                long long out_bytes, int out_h, int out_w, const int32_t* xtab_dev, const int32_t* xtab_host,
                                const int32_t* ytab_dev, const int32_t* ytab_host, void* stream) {
    AQ_REQUIRE(batch_dev && out_dev && xtab_dev && xtab_host && ytab_dev && ytab_host, "val_mosaic: null pointer");
    AQ_REQUIRE(n >= 1 && n <= (int)sg::kMosaicMaxImages, "val_mosaic: %d images (1 to %d)", n, (int)sg::kMosaicMaxImages);
    AQ_REQUIRE(ns >= 1 && (long long)ns * ns >= n, "val_mosaic: a grid of %d x %d cells does not hold %d images", ns, ns, n);
    AQ_REQUIRE(H > 0 && W > 0 && h > 0 && w > 0 && out_h > 0 && out_w > 0, "val_mosaic: bad sizes (%d x %d images, %d x %d cells)", H, W, h, w);
    AQ_REQUIRE(sg::mosaic_fits(n, ns, H, W, h, w), "val_mosaic: mosaic too large (%d x %d cells of %d x %d from %d x %d)", ns, ns, h, w, H, W);
    AQ_REQUIRE((long long)ns * h == out_h && (long long)ns * w == out_w, "val_mosaic: the output is %d x %d, not %d x %d cells of %d x %d", out_h, out_w, ns, ns, h, w);
    AQ_REQUIRE(batch_bytes >= (long long)n * H * W * 3, "val_mosaic: the batch holds %lld bytes, %d images need %lld", batch_bytes, n, (long long)n * H * W * 3);
    AQ_REQUIRE(out_bytes >= (long long)out_h * out_w * 3, "val_mosaic: the output holds %lld bytes, the mosaic needs %lld", out_bytes, (long long)out_h * out_w * 3);
    AQ_REQUIRE(((uintptr_t)xtab_dev & 15) == 0 && ((uintptr_t)ytab_dev & 15) == 0, "val_mosaic: unaligned table");
    for (int x = 0; x < out_w; ++x)
        AQ_REQUIRE(xtab_host[4 * x] >= 0 && xtab_host[4 * x] < ns * W && xtab_host[4 * x + 1] >= 0 && xtab_host[4 * x + 1] < ns * W,
                   "val_mosaic: column %d reads columns %d and %d of a source mosaic %d wide", x, xtab_host[4 * x], xtab_host[4 * x + 1], ns * W);
    for (int y = 0; y < out_h; ++y)
        AQ_REQUIRE(ytab_host[4 * y] >= 0 && ytab_host[4 * y] < ns * H && ytab_host[4 * y + 1] >= 0 && ytab_host[4 * y + 1] < ns * H,
                   "val_mosaic: row %d reads rows %d and %d of a source mosaic %d high", y, ytab_host[4 * y], ytab_host[4 * y + 1], ns * H);
    MosaicParams p;
    p.batch = batch_dev; p.out = out_dev; p.xtab = (const int4*)xtab_dev; p.ytab = (const int4*)ytab_dev;
    p.n = n; p.ns = ns; p.H = H; p.W = W; p.out_h = out_h; p.out_w = out_w;
    p.chunks = (out_w + 1023) / 1024;
    const long long units = (long long)out_h * p.chunks;      // < 2^31 / 3 (mosaic_fits)
    p.n_units = (int)units;
    unsigned grid = 0;
    AQ_CHECK_HIP(aq_persistent_grid(units, 32, &grid));       // 32 workgroups per CU of aq_cus, as annotate.hip
    hipLaunchKernelGGL(mosaic_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
