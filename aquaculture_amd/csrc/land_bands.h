// The band table of the land kernels (land_filter.hip, land_images.hip) and what both do with it: the segments' coordinates gathered in
// entry order, a band's first entry, the band of a y, and the orientation determinant.  The table is the caller's (engine.land_band_table):
// nbands horizontal bands of height h from Y0, band(y) = floor((y - Y0) / h); every segment entered in each band from band(min y) to
// band(max y) with that same expression, which is monotone in y under fp64 rounding; entry_seg lists the segments band by band and
// band_start the bands' first entries, so the bands b0 .. b1 are ONE run of entries.  Everything here has internal linkage: each file that
// includes it gets its own copy of the gather kernel.
#pragma once
#include "aq_common.h"

namespace {

struct LandBands {
    const double* seg;         // [E][4]
    const int* entry_seg;      // [entries]: segment of every entry, band by band
    const int* band_start;     // [nbands + 1]
    double4* eseg;             // scratch [entries]: coordinates by entry
    long long entries;
    int E, nbands;
    double Y0, h;
};

__device__ __forceinline__ double orient(double ax, double ay, double bx, double by, double cx, double cy) {
    return (bx - ax) * (cy - ay) - (by - ay) * (cx - ax);
}

// the segments' coordinates in entry order (the runs are read contiguously from here on)
__global__ __launch_bounds__(256) void land_gather_kernel(const LandBands t) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= t.entries) return;
    const int s = t.entry_seg[i];
    const double nan = __builtin_nan("");
    double4 v = {nan, nan, nan, nan};                                           // an entry that is no segment meets nothing and crosses nothing
    if ((unsigned)s < (unsigned)t.E) v = *(const double4*)(t.seg + 4LL * s);
    t.eseg[i] = v;
}

// first entry of band b, kept inside [0, entries] whatever the table holds
__device__ __forceinline__ long long start_of(const LandBands& t, int b) {
    const long long v = t.band_start[b];
    return v < 0 ? 0 : v > t.entries ? t.entries : v;
}

// band(y) as a double, unclamped: the expression the caller built the table with
__device__ __forceinline__ double band_of(const LandBands& t, double y) {
    return floor((y - t.Y0) / t.h);
}

}  // namespace
