// Annotated images: the detections' boxes and labels drawn on a copy of every image of a batch, as upstream's Annotator.box_label draws them
// in its Pillow branch [UPSTREAM utils/plots.py, pil=True]: ImageDraw.rectangle outlines, filled label rectangles, label text composited
// through 8-bit FreeType masks.  All of it is integer arithmetic; the host (postprocess.annotation_prims) reduces every detection to
// primitives of two kinds, already clipped to the image:
//   a filled rectangle [x0, x1] x [y0, y1] of one colour (an outline of width lw is four of them, as ImagingDrawRectangle's hline / line
//   calls cover them), and
//   a mask blit: out = (out (255 - m) + ink m + 128, then (t + (t >> 8)) >> 8) per channel, Pillow's BLEND8 (fill_mask_L), m read from an
//   atlas of rasterised label strings.
//
// The kernel is pixel-centric and out of place: every output pixel starts as the source pixel and applies, in order, the primitives that
// cover it, so the result does not depend on scheduling and the source stays clean for --save-crop.  The host bins the primitives per
// 16 x 16-pixel cell (CSR: cell_start / cell_prims, ascending primitive index inside a cell), so a pixel only walks the few primitives of
// its own cell.  A workgroup draws four cells side by side: 16 rows of 64 pixels, four pixels (12 bytes) per lane.
#include "aq_common.h"

namespace {

struct AnnotateParams {
    const unsigned char* src;
    unsigned char* dst;
    const aq_canvas* canvases;
    int n_canvases;
    int n_units;
    const aq_prim* prims;
    int n_prims;
    const int* cell_start;
    const int* cell_prims;
    int n_entries;
    const unsigned char* atlas;
    long long atlas_bytes;
};

__device__ __forceinline__ unsigned blend8(unsigned out, unsigned ink, unsigned m) {
    const unsigned t = out * (255u - m) + ink * m + 128u;
    return ((t >> 8) + t) >> 8;
}

__global__ __launch_bounds__(256) void annotate_kernel(const AnnotateParams p) {
    const int r = threadIdx.x >> 4, xq = threadIdx.x & 15;
    for (int u = blockIdx.x; u < p.n_units; u += gridDim.x) {
        int lo = 0, hi = p.n_canvases - 1;                    // the canvas that holds unit u: the last one that starts at or before it
        while (lo < hi) {
            const int mid = (lo + hi + 1) >> 1;
            if (p.canvases[mid].unit <= u) lo = mid; else hi = mid - 1;
        }
        const aq_canvas c = p.canvases[lo];
        const int cw = (c.w + 15) >> 4, uw = (cw + 3) >> 2, k = u - c.unit, uy = k / max(uw, 1), ux = k - uy * uw;
        const int y = 16 * uy + r, x0 = 64 * ux + 4 * xq;
        if (y >= c.h || x0 >= c.w) continue;
        const int n = min(4, c.w - x0);
        const unsigned char* s = p.src + c.src + (long long)y * c.src_pitch + 3 * x0;
        unsigned char* d = p.dst + c.dst + (long long)y * c.dst_pitch + 3 * x0;
        unsigned char px[12];
        if (n == 4 && ((uintptr_t)s & 3) == 0) {
            const uint3 v = *(const uint3*)s;
            const unsigned w3[3] = {v.x, v.y, v.z};
#pragma unroll
            for (int i = 0; i < 12; ++i) px[i] = (unsigned char)(w3[i >> 2] >> (8 * (i & 3)));
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i) px[i] = i < 3 * n ? s[i] : 0;
        }
        const int cell = c.cell + uy * cw + (x0 >> 4);
        const int e0 = max(p.cell_start[cell], 0), e1 = min(p.cell_start[cell + 1], p.n_entries);
        for (int e = e0; e < e1; ++e) {
            const int pi = p.cell_prims[e];
            if (pi < 0 || pi >= p.n_prims) continue;
            const aq_prim q = p.prims[pi];
            if (y < q.y0 || y > q.y1 || x0 + 3 < q.x0 || x0 > q.x1) continue;
            const unsigned ink[3] = {q.rgb & 255u, (q.rgb >> 8) & 255u, (q.rgb >> 16) & 255u};
            if (q.mask_w <= 0) {
#pragma unroll
                for (int i = 0; i < 4; ++i)
                    if (x0 + i >= q.x0 && x0 + i <= q.x1) { px[3 * i] = (unsigned char)ink[0]; px[3 * i + 1] = (unsigned char)ink[1]; px[3 * i + 2] = (unsigned char)ink[2]; }
            } else {
                // (a mask that leaves the atlas is skipped: the caller's table is checked on the host, this keeps every read inside)
                if (q.mask < 0 || q.mask + (long long)(q.y1 - q.y0) * q.mask_w + (q.x1 - q.x0) >= p.atlas_bytes) continue;
                const unsigned char* mrow = p.atlas + q.mask + (long long)(y - q.y0) * q.mask_w;
#pragma unroll
                for (int i = 0; i < 4; ++i) {
                    if (x0 + i < q.x0 || x0 + i > q.x1) continue;
                    const unsigned m = mrow[x0 + i - q.x0];
                    px[3 * i] = (unsigned char)blend8(px[3 * i], ink[0], m);
                    px[3 * i + 1] = (unsigned char)blend8(px[3 * i + 1], ink[1], m);
                    px[3 * i + 2] = (unsigned char)blend8(px[3 * i + 2], ink[2], m);
                }
            }
        }
        if (n == 4 && ((uintptr_t)d & 3) == 0) {
            uint3 v;
            v.x = px[0] | (px[1] << 8) | (px[2] << 16) | ((unsigned)px[3] << 24);
            v.y = px[4] | (px[5] << 8) | (px[6] << 16) | ((unsigned)px[7] << 24);
            v.z = px[8] | (px[9] << 8) | (px[10] << 16) | ((unsigned)px[11] << 24);
            *(uint3*)d = v;
        } else {
#pragma unroll
            for (int i = 0; i < 12; ++i)
                if (i < 3 * n) d[i] = px[i];
        }
    }
}

}  // namespace

// Draws a batch: canvas i is the w x h image whose pixel (x, y) is at src_dev + src + y src_pitch + 3 x; its annotated copy goes to
// dst_dev + dst + y dst_pitch + 3 x.  canvases_host = the same table in host memory, checked here (windows inside the two buffers, cells and
// units following each other from 0).  cell_start_dev: n_cells + 1 ascending offsets into cell_prims_dev (n_entries primitive indices).  Nothing is
// drawn outside a canvas whatever the primitives say; a mask read that would leave the atlas is skipped.
extern "C" int aq_annotate_u8(const uint8_t* src_dev, long long src_bytes, uint8_t* dst_dev, long long dst_bytes, const aq_canvas* canvases_dev,
                              const aq_canvas* canvases_host, int n_canvases, const aq_prim* prims_dev, int n_prims, const int32_t* cell_start_dev,
                              int n_cells, const int32_t* cell_prims_dev, int n_entries, const uint8_t* atlas_dev, long long atlas_bytes, void* stream) {
    AQ_REQUIRE(src_dev && dst_dev && canvases_dev && canvases_host && cell_start_dev, "annotate: null pointer");
    AQ_REQUIRE(n_canvases > 0 && n_prims >= 0 && n_entries >= 0 && atlas_bytes >= 0, "annotate: bad sizes");
    AQ_REQUIRE(n_prims == 0 || (prims_dev && cell_prims_dev), "annotate: primitives without their tables");
    AQ_REQUIRE(((uintptr_t)canvases_dev & 7) == 0 && ((uintptr_t)prims_dev & 7) == 0 && ((uintptr_t)cell_start_dev & 3) == 0, "annotate: unaligned table");
    long long cells = 0, units = 0;
    for (int i = 0; i < n_canvases; ++i) {
        const aq_canvas& c = canvases_host[i];
        AQ_REQUIRE(c.w > 0 && c.h > 0 && c.src >= 0 && c.dst >= 0 && c.src_pitch >= 3LL * c.w && c.dst_pitch >= 3LL * c.w &&
                   c.src + (long long)(c.h - 1) * c.src_pitch + 3LL * c.w <= src_bytes && c.dst + (long long)(c.h - 1) * c.dst_pitch + 3LL * c.w <= dst_bytes,
                   "annotate: image %d (%d x %d) is empty or leaves its buffer (source %lld bytes, destination %lld)", i, c.w, c.h, src_bytes, dst_bytes);
        AQ_REQUIRE(c.cell == cells && c.unit == units, "annotate: image %d does not start where image %d ends (cell %d, unit %d)", i, i - 1, c.cell, c.unit);
        const long long cw = (c.w + 15) / 16, ch = (c.h + 15) / 16;
        cells += cw * ch;
        units += (cw + 3) / 4 * ch;
        AQ_REQUIRE(cells < (1LL << 31), "annotate: more than 2^31 cells in one call");
    }
    AQ_REQUIRE(cells == n_cells, "annotate: the images have %lld cells, the cell table %d", cells, n_cells);
    int cus = 0;
    AQ_CHECK_HIP(aq_cus(&cus));
    AnnotateParams p;
    p.src = src_dev; p.dst = dst_dev; p.canvases = canvases_dev; p.n_canvases = n_canvases; p.n_units = (int)units; p.prims = prims_dev;
    p.n_prims = n_prims; p.cell_start = cell_start_dev; p.cell_prims = cell_prims_dev; p.n_entries = n_entries; p.atlas = atlas_dev;
    p.atlas_bytes = atlas_dev ? atlas_bytes : 0;
    const unsigned grid = (unsigned)(units < 32LL * cus ? units : 32LL * cus);
    hipLaunchKernelGGL(annotate_kernel, dim3(grid), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
