// --land-images: which images lie wholly on land (reference src/utils.py:46-69, mark_land_images: the image's rectangle `within` the land
// polygons shrunk by 5 m, buffer(-5) in EPSG:3857, dissolved).  No polygon buffer: a rectangle R lies inside the erosion of a region L by r
// exactly when R lies in L and no point of the boundary of L is nearer to R than r.  That is the land filter's corner parity plus a minimum
// over rectangle-to-edge distances.
//
// THE RULE (land_images.land_images_numpy restates it; both evaluate these expressions in this order, built with -ffp-contract=off).  N rectangles
// (x0, y0, x1, y1), x0 <= x1 and y0 <= y1; E segments (ax, ay, bx, by) of all rings of the land, exterior and holes alike; an indent r > 0;
// all fp64 EPSG:3857 metres.  max(u, v) below is the one that keeps a NaN of either side: (u > v || u != u) ? u : v.
//   psd(p; a, b)   point to segment, squared: ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay, L = ux ux + uy uy,
//                  t = (wx ux + wy uy) / L, replaced by 0 by a selection when !(L > 0) (the 0 / 0 of a segment of no length never gets
//                  through), then t = t < 0 ? 0 : (t > 1 ? 1 : t), ex = wx - t ux, ey = wy - t uy, result ex ex + ey ey
//   prd(p; R)      point to rectangle, squared: dx = max(max(x0 - px, px - x1), 0), dy = max(max(y0 - py, py - y1), 0), result dx dx + dy dy
//   d2(R, seg)     0 if the segment meets the closed rectangle, by the land filter's bit-0 predicate as it stands (land_filter.hip); else
//                  the minimum of psd for the corners (x0, y0), (x1, y0), (x1, y1), (x0, y1), then prd(a; R), then prd(b; R): for a segment
//                  and a convex polygon that do not meet, one of these six attains the distance
// Every minimum is the selection v < m ? v : m starting from m = +inf, so a NaN (an entry that is no segment, a rectangle that is not a
// number) never enters.  Per rectangle one double and one byte:
//   dist2    the minimum of d2 over the searched segments, capped: m < cap2 ? m : cap2, cap2 = (2 r) (2 r)
//   bit 0    dist2 < r r: a coast edge is nearer than the indent, an edge that meets the rectangle included
//   bit 1    the land filter's corner parity as it stands: the even-odd rule for (x0, y0) over the run of band(y0)
// An image is on land iff the byte is 2; at distance r exactly it is on land, as `within` allows touching.
// Searched segments: those entered in the bands band(y0 - 3 r) .. band(y1 + 3 r) of the table land_bands.h describes.  A segment outside
// them has a y-gap above 3 r (1 - 1e-9), so its computed d2 exceeds cap2 and neither output depends on the band height: that is why the reach
// is 3 r and the cap 2 r, not both r.  A rectangle wholly above or below all bands gets byte 0 and dist2 = cap2, which is what the rule gives
// it; a rectangle with a coordinate that is not a number gets the same, by a test of its own before anything else.
// Launches of one call, both on the caller's stream:
//   gather   the segments' coordinates in entry order (land_bands.h)
//   images   one wavefront per rectangle, four per block; its 64 lanes stride over the one run of entries, each keeping its own minimum and
//            nothing stops early (dist2 is an output); the minimum is reduced across the wave by the same selection (no NaN is left to order,
//            and the minimum of a set does not depend on the order), the crossing count is the sum of the ballots' popcounts over the part
//            of the run that is band(y0); lane 0 stores
// No atomics at all and nothing that depends on order: two calls give the same bytes.
#include "land_bands.h"

namespace {

struct LandImagesParams {
    LandBands t;
    const double* rects;       // [N][4]
    unsigned char* flags;      // out [N]
    double* dist2;             // out [N]
    int N;
    double reach, r2, cap2;    // 3 r, r r, (2 r) (2 r)
};

__device__ __forceinline__ double max_nan(double u, double v) { return (u > v || u != u) ? u : v; }

__device__ __forceinline__ double psd(double px, double py, double ax, double ay, double bx, double by) {
    const double ux = bx - ax, uy = by - ay, wx = px - ax, wy = py - ay;
    const double L = ux * ux + uy * uy;
    double t = (wx * ux + wy * uy) / L;
    t = L > 0.0 ? t : 0.0;
    t = t < 0.0 ? 0.0 : (t > 1.0 ? 1.0 : t);
    const double ex = wx - t * ux, ey = wy - t * uy;
    return ex * ex + ey * ey;
}

__device__ __forceinline__ double prd(double px, double py, double x0, double y0, double x1, double y1) {
    const double dx = max_nan(max_nan(x0 - px, px - x1), 0.0), dy = max_nan(max_nan(y0 - py, py - y1), 0.0);
    return dx * dx + dy * dy;
}

__device__ __forceinline__ double d2_of(const double4 s, double x0, double y0, double x1, double y1, double o) {
    if ((s.x <= x1 || s.z <= x1) && (s.x >= x0 || s.z >= x0) && (s.y <= y1 || s.w <= y1) && (s.y >= y0 || s.w >= y0)) {
        const double o1 = orient(s.x, s.y, s.z, s.w, x1, y0), o2 = orient(s.x, s.y, s.z, s.w, x1, y1);
        const double o3 = orient(s.x, s.y, s.z, s.w, x0, y1);
        if (!((o > 0.0 && o1 > 0.0 && o2 > 0.0 && o3 > 0.0) || (o < 0.0 && o1 < 0.0 && o2 < 0.0 && o3 < 0.0))) return 0.0;
    }
    double m = __builtin_inf(), v;
    v = psd(x0, y0, s.x, s.y, s.z, s.w); m = v < m ? v : m;
    v = psd(x1, y0, s.x, s.y, s.z, s.w); m = v < m ? v : m;
    v = psd(x1, y1, s.x, s.y, s.z, s.w); m = v < m ? v : m;
    v = psd(x0, y1, s.x, s.y, s.z, s.w); m = v < m ? v : m;
    v = prd(s.x, s.y, x0, y0, x1, y1); m = v < m ? v : m;
    v = prd(s.z, s.w, x0, y0, x1, y1); m = v < m ? v : m;
    return m;
}

__global__ __launch_bounds__(256) void land_images_kernel(const LandImagesParams p) {
    const long long img = blockIdx.x * 4LL + (threadIdx.x >> 6);                // one wavefront per rectangle: everything below is uniform in it
    if (img >= p.N) return;
    const int lane = threadIdx.x & 63;
    const double4 b = *(const double4*)(p.rects + 4 * img);
    const double x0 = b.x, y0 = b.y, x1 = b.z, y1 = b.w;
    const double tlo = band_of(p.t, y0 - p.reach), thi = band_of(p.t, y1 + p.reach);
    if (x0 != x0 || y0 != y0 || x1 != x1 || y1 != y1 || !(thi >= 0.0) || !(tlo < (double)p.t.nbands)) {      // a coordinate that is not a number, or wholly below or above all bands
        if (lane == 0) { p.flags[img] = 0; p.dist2[img] = p.cap2; }
        return;
    }
    const int blo = tlo < 0.0 ? 0 : (int)tlo;
    const int bhi = thi < (double)p.t.nbands ? (int)thi : p.t.nbands - 1;
    const long long first = start_of(p.t, blo);
    const long long end = bhi >= blo ? start_of(p.t, bhi + 1) : first;
    const double t0 = band_of(p.t, y0);                                         // the run of band(y0), inside [first, end): the crossing count
    long long c0 = 0, c1 = 0;                                                   // (empty when y0 is outside the bands: nothing crosses its level)
    if (t0 >= 0.0 && t0 < (double)p.t.nbands) {
        c0 = start_of(p.t, (int)t0);
        c1 = start_of(p.t, (int)t0 + 1);
    }
    double m = __builtin_inf();
    int crossings = 0;
    for (long long base = first; base < end; base += 64) {
        const long long e = base + lane;
        bool c_ = false;
        if (e < end) {
            const double4 s = p.t.eseg[e];
            const double o = orient(s.x, s.y, s.z, s.w, x0, y0);
            const bool up = s.y <= y0;
            c_ = e >= c0 && e < c1 && (up != (s.w <= y0)) && (up ? o > 0.0 : o < 0.0);
            const double v = d2_of(s, x0, y0, x1, y1, o);
            m = v < m ? v : m;
        }
        crossings += __popcll(__ballot(c_));
    }
    for (int w = 32; w >= 1; w >>= 1) {
        const double v = __shfl_xor(m, w, 64);
        m = v < m ? v : m;
    }
    m = m < p.cap2 ? m : p.cap2;
    if (lane == 0) {
        p.flags[img] = (unsigned char)((m < p.r2 ? 1 : 0) | ((crossings & 1) << 1));
        p.dist2[img] = m;
    }
}

// no land: byte 0 and dist2 = cap2 for every rectangle
__global__ __launch_bounds__(256) void land_images_none_kernel(unsigned char* flags, double* dist2, int N, double cap2) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= N) return;
    flags[i] = 0;
    dist2[i] = cap2;
}

}  // namespace

// Bytes of scratch aq_land_images_f64 needs for `entries` band entries: 32 (the segment's coordinates) per entry; 0 for entries <= 0 or
// entries >= 2^31.
extern "C" size_t aq_land_images_scratch_bytes(long long entries) {
    if (entries <= 0 || entries >= (1LL << 31)) return 0;
    return (size_t)entries * 32;
}

extern "C" int aq_land_images_f64(const double* seg_dev, long long E, const int32_t* entry_seg_dev, long long entries, const int32_t* band_start_dev,
                                  int nbands, double Y0, double h, const double* rects_dev, long long N, double indent, void* scratch_dev,
                                  size_t scratch_bytes, uint8_t* flags_dev, double* dist2_dev, void* stream) {
    AQ_REQUIRE(E >= 0 && E < (1LL << 31), "land images: %lld segments (at most 2^31 - 1 in one call)", E);
    AQ_REQUIRE(N >= 0 && N < (1LL << 31), "land images: %lld rectangles (at most 2^31 - 1 in one call)", N);
    AQ_REQUIRE(entries >= 0 && entries < (1LL << 31), "land images: %lld band entries (at most 2^31 - 1 in one call)", entries);
    AQ_REQUIRE(h > 0.0 && h < __builtin_inf(), "land images: band height h = %g (it has to be positive and finite)", h);      // (NaN fails too)
    AQ_REQUIRE(Y0 > -__builtin_inf() && Y0 < __builtin_inf(), "land images: Y0 = %g (it has to be finite)", Y0);
    AQ_REQUIRE(nbands >= 1, "land images: nbands = %d (at least 1)", nbands);
    AQ_REQUIRE(indent > 0.0 && indent < __builtin_inf(), "land images: indent = %g (it has to be positive and finite)", indent);
    if (N == 0) return AQ_OK;
    hipStream_t st = (hipStream_t)stream;
    const double two_r = 2.0 * indent, cap2 = two_r * two_r;
    AQ_REQUIRE(flags_dev && dist2_dev, "land images: null pointer");
    AQ_REQUIRE(((uintptr_t)dist2_dev & 7) == 0, "land images: unaligned array");
    if (E == 0 || entries == 0) {                                               // no land: no edge is near and no corner is inside
        hipLaunchKernelGGL(land_images_none_kernel, dim3((unsigned)((N + 255) / 256)), dim3(256), 0, st, flags_dev, dist2_dev, (int)N, cap2);
        AQ_CHECK_HIP(hipGetLastError());
        return AQ_OK;
    }
    AQ_REQUIRE(seg_dev && entry_seg_dev && band_start_dev && rects_dev && scratch_dev, "land images: null pointer");
    AQ_REQUIRE(((uintptr_t)seg_dev & 31) == 0 && ((uintptr_t)rects_dev & 31) == 0 && ((uintptr_t)scratch_dev & 31) == 0 &&
               ((uintptr_t)entry_seg_dev & 3) == 0 && ((uintptr_t)band_start_dev & 3) == 0, "land images: unaligned array");
    const size_t need = aq_land_images_scratch_bytes(entries);
    AQ_REQUIRE(scratch_bytes >= need, "land images: %zu bytes of scratch, %zu needed (aq_land_images_scratch_bytes)", scratch_bytes, need);
    LandImagesParams p = {};
    p.t.seg = seg_dev; p.t.entry_seg = entry_seg_dev; p.t.band_start = band_start_dev; p.rects = rects_dev;
    p.t.eseg = (double4*)scratch_dev; p.flags = flags_dev; p.dist2 = dist2_dev;
    p.t.entries = entries; p.t.E = (int)E; p.N = (int)N; p.t.nbands = nbands; p.t.Y0 = Y0; p.t.h = h;
    p.reach = 3.0 * indent; p.r2 = indent * indent; p.cap2 = cap2;
    hipLaunchKernelGGL(land_gather_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, p.t);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(land_images_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
