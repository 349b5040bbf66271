// --tonnage-missing / --tonnage-near-sites: does a closed box meet a union of image regions?  (reference src/utils_tonnage.py:1108-1136,
// modify_cage_list_using_geometry: cage.intersects(unary_union of a pass's image polygons).)  I images in the host's order, sorted by (pass,
// name); image i has the closed rectangle rect[i] = (west, south, east, north) and, if ring_start[i + 1] > ring_start[i], is a ring image:
// its region is the closed even-odd region of the closed walk xy[ring_start[i] .. ring_start[i + 1] - 1] (first vertex repeated at the end,
// axis-parallel segments, metres in fp64 computed by the host, both ends of a vertical segment holding the same double).  Otherwise its
// region is the rectangle.  For a query (box B = (x0, y0, x1, y1), target pass tp):
//   rectangle image   meets iff x0 <= east && x1 >= west && y0 <= north && y1 >= south
//   ring image        (tested only if its rectangle meets B, which every ring lies in) meets iff some segment's closed bounding box
//                     overlaps B, or an odd number of segments have (ay <= y0) != (by <= y0) and ax > x0: the corner (x0, y0) strictly
//                     inside, which only decides when no segment meets B
//   first[q]          the smallest image number of pass tp that meets B, or -1; a box with a NaN, or a pass outside [0, P), gives -1
// land_filter.hip takes the parity over all rings together; two images over the same ground would cancel there.  Here the parity is per
// image and the images are OR-ed (a minimum over the hits).
// Search structure, the one of land_filter.hip, per pass: nbands horizontal bands, band(y) = floor((y - Y0[p]) / h[p]) clamped to
// [0, nbands); the host entered image i of pass p in every band from band(south) to band(north) with the SAME expression, which is monotone
// in y.  entry_img lists the entries pass by pass and band by band, band_start [P nbands + 1] their first entries, so the bands band(y0) ..
// band(y1) of a query are ONE run of its target pass.  Launches of one call, both on the caller's stream:
//   gather   the rectangles in entry order (the runs are read contiguously from here on)
//   first    one wavefront per query; lanes stride over the run and test the rectangle; a rectangle image that passes is a hit; the ring
//            images that pass are collected by ballot and handled one at a time, wave-uniformly: lanes stride over the ring's segments, the
//            segment hit is a ballot, the parity the sum of the ballots' popcounts.  first = the minimum over the hits, by wave reduction.
//            An image met through two bands gives the same answer twice.
// Comparisons and integer minima only; no atomics: two calls give the same bytes.  Every index is kept inside its array on the device.
#include "aq_common.h"

namespace {

struct CoverageParams {
    const double* rect;        // [I][4]
    const int* ring_start;     // [I + 1]
    const double* xy;          // [V][2]
    const int* entry_img;      // [entries]
    const int* band_start;     // [P * nbands + 1]
    const double* band;        // [P][2]: Y0, h
    const double* box;         // [Q][4]
    const int* qpass;          // [Q]
    double4* erect;            // scratch [entries]: rectangles by entry
    int* first;                // out [Q]
    long long entries, V;
    int I, P, Q, nbands;
};

__global__ __launch_bounds__(256) void coverage_gather_kernel(const CoverageParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.entries) return;
    const int s = p.entry_img[i];
    const double nan = __builtin_nan("");
    double4 v = {nan, nan, nan, nan};                                           // an entry that is no image meets nothing
    if ((unsigned)s < (unsigned)p.I) v = *(const double4*)(p.rect + 4LL * s);
    p.erect[i] = v;
}

// first entry of band slot b (pass * nbands + band), kept inside [0, entries] whatever the table holds
__device__ __forceinline__ long long start_of(const CoverageParams& p, long long b) {
    const long long v = p.band_start[b];
    return v < 0 ? 0 : v > p.entries ? p.entries : v;
}

// vertex offset kept inside [0, V]
__device__ __forceinline__ long long vertex_of(const CoverageParams& p, int i) {
    const long long v = p.ring_start[i];
    return v < 0 ? 0 : v > p.V ? p.V : v;
}

__global__ __launch_bounds__(256) void coverage_first_kernel(const CoverageParams p) {
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: everything below is uniform in it
    if (q >= p.Q) return;
    const int lane = threadIdx.x & 63;
    const double4 b = *(const double4*)(p.box + 4 * q);
    const double x0 = b.x, y0 = b.y, x1 = b.z, y1 = b.w;
    const int tp = p.qpass[q];
    if (tp < 0 || tp >= p.P || !(x0 == x0 && y0 == y0 && x1 == x1 && y1 == y1)) {  // no such pass, or a box with a NaN: it meets nothing
        if (lane == 0) p.first[q] = -1;
        return;
    }
    const double Y0 = p.band[2 * tp], h = p.band[2 * tp + 1];
    const double t0 = floor((y0 - Y0) / h), t1 = floor((y1 - Y0) / h);
    const double top = (double)p.nbands;
    const int b0 = !(t0 >= 0.0) ? 0 : t0 < top ? (int)t0 : p.nbands - 1;        // clamped, as the host clamped the images' bands
    const int b1 = !(t1 >= 0.0) ? 0 : t1 < top ? (int)t1 : p.nbands - 1;
    const long long slot = (long long)tp * p.nbands;
    const long long run0 = start_of(p, slot + b0);
    const long long run1 = b1 >= b0 ? start_of(p, slot + b1 + 1) : run0;
    int best = 0x7FFFFFFF;
    for (long long base = run0; base < run1; base += 64) {
        const long long e = base + lane;
        int img = -1;
        bool ring = false;
        if (e < run1) {
            const double4 r = p.erect[e];
            const int i = p.entry_img[e];
            if ((unsigned)i < (unsigned)p.I && x0 <= r.z && x1 >= r.x && y0 <= r.w && y1 >= r.y) {
                img = i;
                ring = vertex_of(p, i + 1) > vertex_of(p, i);
                if (!ring) best = min(best, i);                                 // a rectangle image that passes is a hit
            }
        }
        unsigned long long todo = __ballot(ring);
        while (todo) {                                                          // the ring images that passed, one at a time
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int i = __shfl(img, src);
            const long long s0 = vertex_of(p, i);
            const long long nseg = vertex_of(p, i + 1) - s0 - 1;
            bool hit = false;
            int crossings = 0;
            for (long long sb = 0; sb < nseg && !hit; sb += 64) {
                const long long s = sb + lane;
                bool h_ = false, c_ = false;
                if (s < nseg) {
                    const double2 a = *(const double2*)(p.xy + 2 * (s0 + s)), c = *(const double2*)(p.xy + 2 * (s0 + s + 1));
                    h_ = (a.x <= x1 || c.x <= x1) && (a.x >= x0 || c.x >= x0) && (a.y <= y1 || c.y <= y1) && (a.y >= y0 || c.y >= y0);
                    c_ = ((a.y <= y0) != (c.y <= y0)) && a.x > x0;
                }
                hit = __ballot(h_) != 0ULL;
                crossings += __popcll(__ballot(c_));
            }
            if (hit || (crossings & 1)) best = min(best, i);
        }
    }
    for (int d = 32; d >= 1; d >>= 1) best = min(best, __shfl_xor(best, d));
    if (lane == 0) p.first[q] = best == 0x7FFFFFFF ? -1 : best;
}

}  // namespace

extern "C" int aq_coverage_first_i32(const double* rect_dev, const int32_t* ring_start_dev, const int32_t* ring_start_host, long long I,
                                     const double* xy_dev, long long V, const int32_t* entry_img_dev, long long entries,
                                     const int32_t* band_start_dev, const int32_t* band_start_host, const double* band_dev,
                                     const double* band_host, long long P, long long nbands, const double* box_dev, const int32_t* qpass_dev,
                                     long long Q, void* scratch_dev, size_t scratch_bytes, int32_t* first_dev, void* stream) {
    AQ_REQUIRE(sg::coverage_count_fits(I) && sg::coverage_count_fits(entries) && sg::coverage_count_fits(Q) && sg::coverage_count_fits(P),
               "coverage: %lld images, %lld band entries, %lld queries, %lld passes (each 0 .. 2^31 - 1 in one call)", I, entries, Q, P);
    AQ_REQUIRE(sg::coverage_count_fits(V), "coverage: %lld ring vertices (0 .. 2^31 - 1 in one call: they are 32-bit offsets)", V);
    AQ_REQUIRE(sg::coverage_bands_fit(P, nbands), "coverage: %lld bands for each of %lld passes (at least 1, P nbands + 1 below 2^31)", nbands, P);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(first_dev && box_dev && qpass_dev, "coverage: null pointer");
    AQ_REQUIRE(((uintptr_t)box_dev & 31) == 0 && ((uintptr_t)qpass_dev & 3) == 0 && ((uintptr_t)first_dev & 3) == 0, "coverage: unaligned array");
    hipStream_t st = (hipStream_t)stream;
    CoverageParams p = {};
    p.box = box_dev; p.qpass = qpass_dev; p.first = first_dev; p.Q = (int)Q;
    if (P > 0 && I > 0 && entries > 0) {
        AQ_REQUIRE(rect_dev && ring_start_dev && ring_start_host && entry_img_dev && band_start_dev && band_start_host && band_dev && band_host &&
                   scratch_dev && (xy_dev || V == 0), "coverage: null pointer");
        AQ_REQUIRE(((uintptr_t)rect_dev & 31) == 0 && ((uintptr_t)scratch_dev & 31) == 0 && ((uintptr_t)xy_dev & 15) == 0 &&
                   ((uintptr_t)band_dev & 7) == 0 && ((uintptr_t)ring_start_dev & 3) == 0 && ((uintptr_t)entry_img_dev & 3) == 0 &&
                   ((uintptr_t)band_start_dev & 3) == 0, "coverage: unaligned array");
        AQ_REQUIRE(scratch_bytes >= (size_t)entries * 32, "coverage: %zu bytes of scratch, %zu needed (32 per band entry)", scratch_bytes,
                   (size_t)entries * 32);
        AQ_REQUIRE(ring_start_host[0] >= 0 && ring_start_host[I] <= V, "coverage: ring starts %d .. %d leave the %lld vertices",
                   ring_start_host[0], ring_start_host[I], V);
        for (long long i = 0; i < I; ++i)
            AQ_REQUIRE(ring_start_host[i] <= ring_start_host[i + 1], "coverage: ring starts are not sorted at image %lld", i);
        AQ_REQUIRE(band_start_host[0] >= 0 && band_start_host[P * nbands] <= entries, "coverage: band starts %d .. %d leave the %lld entries",
                   band_start_host[0], band_start_host[P * nbands], entries);
        for (long long k = 0; k < P * nbands; ++k)
            AQ_REQUIRE(band_start_host[k] <= band_start_host[k + 1], "coverage: band starts are not sorted at pass %lld, band %lld", k / nbands,
                       k % nbands);
        for (long long k = 0; k < P; ++k) {
            const double Y0 = band_host[2 * k], h = band_host[2 * k + 1];
            AQ_REQUIRE(h > 0.0 && h < __builtin_inf() && Y0 > -__builtin_inf() && Y0 < __builtin_inf(),
                       "coverage: pass %lld has Y0 = %g, band height h = %g (finite, h positive)", k, Y0, h);         // (NaN fails too)
        }
        p.rect = rect_dev; p.ring_start = ring_start_dev; p.xy = xy_dev; p.entry_img = entry_img_dev; p.band_start = band_start_dev;
        p.band = band_dev; p.erect = (double4*)scratch_dev;
        p.entries = entries; p.V = V; p.I = (int)I; p.P = (int)P; p.nbands = (int)nbands;
        hipLaunchKernelGGL(coverage_gather_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, p);
        AQ_CHECK_HIP(hipGetLastError());
    }                                                                           // else p.P = 0: no image anywhere, every query gets -1
    hipLaunchKernelGGL(coverage_first_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
