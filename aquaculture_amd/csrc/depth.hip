// --bathymetry: the water depth under every facility (reference src/utils_tonnage.py:591-665, add_facility_depth: rasterstats.zonal_stats with
// all_touched=True over the union of a facility's circle and square cages), from a window of the depth raster: float32 [nrows][ncols], row 0
// the northernmost, cell (r, c) the half-open square [x0 + c dx, x0 + (c + 1) dx) x (y0 - (r + 1) dy, y0 - r dy].  Facility f owns the cages
// entry_start[f] .. entry_start[f + 1] - 1, each an axis-parallel box (lon_min, lon_max, lat_min, lat_max) in the raster's coordinates.
//   ranges   c0 = floor((lon_min - x0) / dx), c1 = floor((lon_max - x0) / dx), r0 = floor((y0 - lat_max) / dy), r1 = floor((y0 - lat_min) / dy),
//            all fp64, kept inside [-1, ncols] / [-1, nrows] in fp64 (anything that is not >= -1, a NaN included, becomes -1) and only then
//            converted; the cage touches columns c0 .. c1 and rows r0 .. r1 intersected with the window's, so a closed box against half-open
//            cells; a cage with no such cell, or with a coordinate that is NaN, is stored as (0, -1, 0, -1).  The facility's window is the
//            bounding rectangle of its cages' ranges, (0, -1, 0, -1) without any.  One wavefront per facility: lanes stride over the cages,
//            the window is a wavefront min / max.
//   stats    one wavefront per facility.  The touched set is the union of the cages' cell rectangles, as bits of the facility's words of a
//            bitmap the caller zeroed: bit i = cell (i / W, i % W) of the window, W its width; lanes stride over the cages and set the runs
//            of every row with atomicOr (integer, so the order does not matter).  After a fence the lanes walk the window: lane l takes the
//            indices i = l, l + 64, .. in ascending order and keeps, over the touched cells whose value is neither NaN nor nodata, its partial
//            sum (from +0.0, the float32 value widened), its min, max and count.  The 64 partial sums are added in lane order from +0.0 --
//            not as a tree: bathymetry.stats_numpy adds in the same order and gives the same bytes; min, max and count do not depend on
//            order (a min or max that is a zero is +0.0).  Without a valid cell: min = +inf, max = -inf, sum = +0.0, count = 0.
// Only fp64 - and /, floor, comparisons, selections, fp64 + and integer instructions; no fp atomics, no libm.
#include "aq_common.h"

namespace {

struct DepthParams {
    const int* entry_start;        // [F + 1]
    const double* cages;           // [E][4]: lon_min, lon_max, lat_min, lat_max
    int* cage_range;               // [E][4]: c0, c1, r0, r1 (ranges: out; stats: in)
    int* window;                   // [F][4]: c0, c1, r0, r1
    const long long* word_start;   // [F + 1]: the facility's first bitmap word
    const float* raster;           // [nrows][ncols]
    unsigned* bitmap;              // [bitmap_words], zeroed
    double* stats;                 // out [F][3]: min, max, sum
    long long* count;              // out [F]
    long long F, E, bitmap_words;
    int nrows, ncols;
    double x0, y0, dx, dy, nodata;
};

// floor(t) kept inside [-1, n], as an integer: not >= -1 (NaN too) gives -1
__device__ __forceinline__ int cell_of(double t, int n) {
    const double f = floor(t);
    return !(f >= -1.0) ? -1 : f > (double)n ? n : (int)f;
}

__device__ __forceinline__ int wave_min(int v) {
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o < v ? o : v; }
    return v;
}
__device__ __forceinline__ int wave_max(int v) {
    for (int m = 32; m >= 1; m >>= 1) { const int o = __shfl_xor(v, m); v = o > v ? o : v; }
    return v;
}

// the facility's entries, kept inside [0, E] whatever the table holds
__device__ __forceinline__ void entries_of(const DepthParams& p, long long f, long long* first, long long* end) {
    long long a = p.entry_start[f], b = p.entry_start[f + 1];
    a = a < 0 ? 0 : a > p.E ? p.E : a;
    b = b < a ? a : b > p.E ? p.E : b;
    *first = a; *end = b;
}

__global__ __launch_bounds__(64) void depth_ranges_kernel(const DepthParams p) {
    const long long f = blockIdx.x;                                             // one wavefront per facility
    const int lane = threadIdx.x;
    long long first, end;
    entries_of(p, f, &first, &end);
    int wc0 = 0x7fffffff, wc1 = -1, wr0 = 0x7fffffff, wr1 = -1;
    for (long long e = first + lane; e < end; e += 64) {
        const double4 b = *(const double4*)(p.cages + 4 * e);
        int c0 = cell_of((b.x - p.x0) / p.dx, p.ncols), c1 = cell_of((b.y - p.x0) / p.dx, p.ncols);
        int r0 = cell_of((p.y0 - b.w) / p.dy, p.nrows), r1 = cell_of((p.y0 - b.z) / p.dy, p.nrows);
        c0 = c0 < 0 ? 0 : c0; c1 = c1 > p.ncols - 1 ? p.ncols - 1 : c1;
        r0 = r0 < 0 ? 0 : r0; r1 = r1 > p.nrows - 1 ? p.nrows - 1 : r1;
        const bool some = c0 <= c1 && r0 <= r1 && b.x == b.x && b.y == b.y && b.z == b.z && b.w == b.w;
        if (some) {
            wc0 = c0 < wc0 ? c0 : wc0; wc1 = c1 > wc1 ? c1 : wc1;
            wr0 = r0 < wr0 ? r0 : wr0; wr1 = r1 > wr1 ? r1 : wr1;
        }
        *(int4*)(p.cage_range + 4 * e) = some ? make_int4(c0, c1, r0, r1) : make_int4(0, -1, 0, -1);
    }
    wc0 = wave_min(wc0); wc1 = wave_max(wc1); wr0 = wave_min(wr0); wr1 = wave_max(wr1);
    if (lane == 0) *(int4*)(p.window + 4 * f) = wc1 >= 0 ? make_int4(wc0, wc1, wr0, wr1) : make_int4(0, -1, 0, -1);
}

__global__ __launch_bounds__(64) void depth_stats_kernel(const DepthParams p) {
    const long long f = blockIdx.x;                                             // one wavefront per facility: everything below is uniform in it
    const int lane = threadIdx.x;
    const double inf = __builtin_inf();
    const int4 w = *(const int4*)(p.window + 4 * f);
    // the window inside the raster and its words inside the bitmap, whatever the tables hold; one that does not fit its words counts as empty
    const int c0 = w.x < 0 ? 0 : w.x, c1 = w.y > p.ncols - 1 ? p.ncols - 1 : w.y;
    const int r0 = w.z < 0 ? 0 : w.z, r1 = w.w > p.nrows - 1 ? p.nrows - 1 : w.w;
    const long long ws = p.word_start[f], we = p.word_start[f + 1];
    const long long W = (long long)c1 - c0 + 1, H = (long long)r1 - r0 + 1;
    const long long cells = W > 0 && H > 0 ? W * H : 0;
    const bool fits = ws >= 0 && we >= ws && we <= p.bitmap_words && cells < (1LL << 31) && (cells + 31) / 32 <= we - ws;
    double sum = 0.0, mn = inf, mx = -inf;
    long long cnt = 0;
    if (cells > 0 && fits) {
        unsigned* bm = p.bitmap + ws;
        const unsigned Wu = (unsigned)W;
        long long first, end;
        entries_of(p, f, &first, &end);
        for (long long e = first + lane; e < end; e += 64) {
            const int4 g = *(const int4*)(p.cage_range + 4 * e);
            const int a0 = g.x < c0 ? c0 : g.x, a1 = g.y > c1 ? c1 : g.y, b0 = g.z < r0 ? r0 : g.z, b1 = g.w > r1 ? r1 : g.w;
            if (a0 > a1) continue;
            for (int r = b0; r <= b1; ++r) {                                    // the bits i0 .. i1 of this row, word by word
                const unsigned i0 = (unsigned)(r - r0) * Wu + (unsigned)(a0 - c0), i1 = i0 + (unsigned)(a1 - a0);
                for (unsigned k = i0 >> 5; k <= i1 >> 5; ++k) {
                    const unsigned lo = k == i0 >> 5 ? i0 & 31 : 0, hi = k == i1 >> 5 ? i1 & 31 : 31;
                    atomicOr(bm + k, (0xffffffffu >> (31 - hi)) & (0xffffffffu << lo));
                }
            }
        }
        __threadfence();                                                        // the bits are in memory before any lane reads a word
        __syncthreads();
        const unsigned n = (unsigned)cells;
        for (unsigned i = lane; i < n; i += 64) {
            // (read past the vector cache: a neighbouring facility's words can share a line another wavefront of this CU has read)
            const unsigned word = __hip_atomic_load(bm + (i >> 5), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (!((word >> (i & 31)) & 1)) continue;
            const unsigned row = i / Wu, col = i - row * Wu;
            const double v = (double)p.raster[(long long)(r0 + (int)row) * p.ncols + (c0 + (int)col)];
            if (v != v || v == p.nodata) continue;
            sum = sum + v;
            mn = v < mn ? v : mn;
            mx = v > mx ? v : mx;
            ++cnt;
        }
    }
    double total = 0.0;
    for (int l = 0; l < 64; ++l) total = total + __shfl(sum, l);                // in lane order: the restatement's order
    for (int m = 32; m >= 1; m >>= 1) {
        const double a = __shfl_xor(mn, m), b = __shfl_xor(mx, m);
        mn = a < mn ? a : mn;
        mx = b > mx ? b : mx;
        cnt += __shfl_xor(cnt, m);
    }
    if (lane == 0) {
        p.stats[3 * f] = mn + 0.0;                                              // (-0.0 + 0.0 = +0.0: a zero is +0.0 whichever cell gave it)
        p.stats[3 * f + 1] = mx + 0.0;
        p.stats[3 * f + 2] = total;
        p.count[f] = cnt;
    }
}

}  // namespace

extern "C" int aq_depth_ranges_f64(const int32_t* entry_start_dev, long long F, const double* cages_dev, long long E, double x0, double y0,
                                   double dx, double dy, int nrows, int ncols, int32_t* cage_range_dev, int32_t* window_dev, void* stream) {
    AQ_REQUIRE(F >= 0 && F < (1LL << 31), "depth: %lld facilities (at most 2^31 - 1 in one call)", F);
    AQ_REQUIRE(E >= 0 && E < (1LL << 31), "depth: %lld cages (at most 2^31 - 1 in one call)", E);
    AQ_REQUIRE(nrows >= 0 && ncols >= 0, "depth: a window of %d x %d cells", nrows, ncols);
    AQ_REQUIRE(dx > 0.0 && dx < __builtin_inf() && dy > 0.0 && dy < __builtin_inf(), "depth: cell size %g x %g (it has to be positive and finite)", dx, dy);
    AQ_REQUIRE(x0 > -__builtin_inf() && x0 < __builtin_inf() && y0 > -__builtin_inf() && y0 < __builtin_inf(), "depth: origin (%g, %g) (it has to be finite)", x0, y0);
    if (F == 0) return AQ_OK;
    AQ_REQUIRE(entry_start_dev && window_dev && (E == 0 || (cages_dev && cage_range_dev)), "depth: null pointer");
    AQ_REQUIRE(((uintptr_t)cages_dev & 31) == 0 && ((uintptr_t)cage_range_dev & 15) == 0 && ((uintptr_t)window_dev & 15) == 0 &&
               ((uintptr_t)entry_start_dev & 3) == 0, "depth: unaligned array");
    DepthParams p = {};
    p.entry_start = entry_start_dev; p.cages = cages_dev; p.cage_range = cage_range_dev; p.window = window_dev;
    p.F = F; p.E = E; p.nrows = nrows; p.ncols = ncols; p.x0 = x0; p.y0 = y0; p.dx = dx; p.dy = dy;
    hipLaunchKernelGGL(depth_ranges_kernel, dim3((unsigned)F), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_depth_stats_f64(const int32_t* entry_start_dev, long long F, const int32_t* cage_range_dev, long long E, const int32_t* window_dev,
                                  const int32_t* window_host, const long long* word_start_dev, const long long* word_start_host,
                                  const float* raster_dev, int nrows, int ncols, double nodata, uint32_t* bitmap_dev, long long bitmap_words,
                                  double* stats_dev, long long* count_dev, void* stream) {
    AQ_REQUIRE(F >= 0 && F < (1LL << 31), "depth: %lld facilities (at most 2^31 - 1 in one call)", F);
    AQ_REQUIRE(E >= 0 && E < (1LL << 31), "depth: %lld cages (at most 2^31 - 1 in one call)", E);
    AQ_REQUIRE(nrows >= 0 && ncols >= 0, "depth: a window of %d x %d cells", nrows, ncols);
    // the size guard: every bit index of a facility and every word index of the bitmap fits 32 bits
    AQ_REQUIRE(bitmap_words >= 0 && bitmap_words < (1LL << 31), "depth: a bitmap of %lld words (at most 2^31 - 1 in one call: fewer facilities at a time)", bitmap_words);
    if (F == 0) return AQ_OK;
    AQ_REQUIRE(window_host && word_start_host, "depth: null pointer");
    AQ_REQUIRE(word_start_host[0] >= 0, "depth: the bitmap words of facility 0 start at %lld", word_start_host[0]);
    for (long long f = 0; f < F; ++f) {
        const int32_t* w = window_host + 4 * f;
        const long long W = (long long)w[1] - w[0] + 1, H = (long long)w[3] - w[2] + 1;
        const long long have = word_start_host[f + 1] - word_start_host[f];
        AQ_REQUIRE(have >= 0 && word_start_host[f + 1] <= bitmap_words, "depth: the bitmap words of facility %lld end at %lld of %lld", f, word_start_host[f + 1], bitmap_words);
        if (W <= 0 || H <= 0) continue;
        AQ_REQUIRE(w[0] >= 0 && w[1] < ncols && w[2] >= 0 && w[3] < nrows, "depth: the window of facility %lld leaves the %d x %d cells", f, nrows, ncols);
        AQ_REQUIRE(W * H < (1LL << 31), "depth: the window of facility %lld has %lld x %lld cells (fewer than 2^31)", f, H, W);
        AQ_REQUIRE((W * H + 31) / 32 <= have, "depth: facility %lld has %lld bitmap words for %lld cells", f, have, W * H);
    }
    AQ_REQUIRE(entry_start_dev && window_dev && word_start_dev && stats_dev && count_dev && (E == 0 || cage_range_dev) &&
               (bitmap_words == 0 || (bitmap_dev && raster_dev)), "depth: null pointer");
    AQ_REQUIRE(((uintptr_t)cage_range_dev & 15) == 0 && ((uintptr_t)window_dev & 15) == 0 && ((uintptr_t)entry_start_dev & 3) == 0 &&
               ((uintptr_t)word_start_dev & 7) == 0 && ((uintptr_t)raster_dev & 3) == 0 && ((uintptr_t)bitmap_dev & 3) == 0 &&
               ((uintptr_t)stats_dev & 7) == 0 && ((uintptr_t)count_dev & 7) == 0, "depth: unaligned array");
    DepthParams p = {};
    p.entry_start = entry_start_dev; p.cage_range = const_cast<int32_t*>(cage_range_dev); p.window = const_cast<int32_t*>(window_dev);
    p.word_start = word_start_dev; p.raster = raster_dev; p.bitmap = bitmap_dev; p.stats = stats_dev; p.count = (long long*)count_dev;
    p.F = F; p.E = E; p.bitmap_words = bitmap_words; p.nrows = nrows; p.ncols = ncols; p.nodata = nodata;
    hipLaunchKernelGGL(depth_stats_kernel, dim3((unsigned)F), dim3(64), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
