// --land-filter: which detection boxes lie on land (reference src/process_yolo/geocode_results.py:200-218, remove_land_detections:
// detections.sjoin(land, how='inner') with the predicate `intersects`), for N boxes (x0, y0, x1, y1), x0 <= x1 and y0 <= y1, against the E
// segments (ax, ay, bx, by) of all rings of the land polygons, exterior and holes alike, all in fp64 EPSG:3857 metres.  One byte per box:
//   bit 0    some segment meets the closed box: the two bounding boxes overlap (closed comparisons) and the four corners of the box are not
//            all strictly on one side of the segment's line, by the sign of orient(a, b, c) = (bx - ax) (cy - ay) - (by - ay) (cx - ax),
//            evaluated in fp64 in exactly that form (built with -ffp-contract=off: y is about 5e6 m, a box a few metres).  A segment of no
//            length has orient = 0 everywhere and is a point-in-box test, with no special case.
//   bit 1    the corner (x0, y0) is inside the land under the even-odd rule over all rings: the parity of the segments with
//            (ay <= y0) != (by <= y0) (half-open in y) that have the corner strictly on their left if they go up, strictly on their right
//            if they go down, again by the sign of orient.
// A box that no ring edge meets lies wholly inside or wholly outside the land, so byte != 0 is `intersects`, touching included.
// Search structure, one-dimensional: nbands horizontal bands of height h from Y0, band(y) = floor((y - Y0) / h) clamped to [0, nbands); the
// caller entered every segment in each band from band(min y) to band(max y), with the SAME expression, which is monotone in y under fp64
// rounding: a segment whose y-range overlaps a box's shares a band with it.  entry_seg lists the segments band by band and band_start the
// bands' first entries, so the bands band(y0) .. band(y1) of a box are ONE run of entries, and the segments that can cross the ray from
// (x0, y0) towards +x are all in the run of band(y0), each once.  Launches of one call, both on the caller's stream:
//   gather   the segments' coordinates in entry order (the runs are read contiguously from here on)
//   flags    one wavefront per box; its 64 lanes stride over the run; the hit bit is a ballot (no more hit tests once it is set), the
//            crossing count the sum of the ballots' popcounts over the run of band(y0)
// No atomics at all and nothing that depends on order: two calls give the same bytes.
#include "land_bands.h"                                                         // the table, the gather launch, start_of, orient: shared with land_images.hip

namespace {

struct LandParams {
    LandBands t;
    const double* boxes;       // [N][4]
    unsigned char* flags;      // out [N]
    int N;
};

__global__ __launch_bounds__(256) void land_flags_kernel(const LandParams p) {
    const long long box = blockIdx.x * 4LL + (threadIdx.x >> 6);                // one wavefront per box: everything below is uniform in it
    if (box >= p.N) return;
    const int lane = threadIdx.x & 63;
    const double4 b = *(const double4*)(p.boxes + 4 * box);
    const double x0 = b.x, y0 = b.y, x1 = b.z, y1 = b.w;
    const double t0 = band_of(p.t, y0), t1 = band_of(p.t, y1);
    if (!(t1 >= 0.0) || !(t0 < (double)p.t.nbands)) {                           // wholly below or above all bands (or not a number): at sea
        if (lane == 0) p.flags[box] = 0;
        return;
    }
    const int b0 = t0 < 0.0 ? 0 : (int)t0;
    const int b1 = t1 < (double)p.t.nbands ? (int)t1 : p.t.nbands - 1;
    const long long first = start_of(p.t, b0);
    const long long end0 = start_of(p.t, b0 + 1);                               // the run of band(y0): the crossing count
    const long long end = b1 >= b0 ? start_of(p.t, b1 + 1) : end0;
    bool hit = false;
    int crossings = 0;
    for (long long base = first; base < end0; base += 64) {
        const long long e = base + lane;
        bool h_ = false, c_ = false;
        if (e < end0) {
            const double4 s = p.t.eseg[e];
            const double o = orient(s.x, s.y, s.z, s.w, x0, y0);
            const bool up = s.y <= y0;
            c_ = (up != (s.w <= y0)) && (up ? o > 0.0 : o < 0.0);
            if (!hit && (s.x <= x1 || s.z <= x1) && (s.x >= x0 || s.z >= x0) && (s.y <= y1 || s.w <= y1) && (s.y >= y0 || s.w >= y0)) {
                const double o1 = orient(s.x, s.y, s.z, s.w, x1, y0), o2 = orient(s.x, s.y, s.z, s.w, x1, y1);
                const double o3 = orient(s.x, s.y, s.z, s.w, x0, y1);
                h_ = !((o > 0.0 && o1 > 0.0 && o2 > 0.0 && o3 > 0.0) || (o < 0.0 && o1 < 0.0 && o2 < 0.0 && o3 < 0.0));
            }
        }
        crossings += __popcll(__ballot(c_));
        hit = hit || __ballot(h_) != 0ULL;
    }
    for (long long base = end0; base < end && !hit; base += 64) {               // the other bands of the box: the hit bit only
        const long long e = base + lane;
        bool h_ = false;
        if (e < end) {
            const double4 s = p.t.eseg[e];
            if ((s.x <= x1 || s.z <= x1) && (s.x >= x0 || s.z >= x0) && (s.y <= y1 || s.w <= y1) && (s.y >= y0 || s.w >= y0)) {
                const double o = orient(s.x, s.y, s.z, s.w, x0, y0), o1 = orient(s.x, s.y, s.z, s.w, x1, y0);
                const double o2 = orient(s.x, s.y, s.z, s.w, x1, y1), o3 = orient(s.x, s.y, s.z, s.w, x0, y1);
                h_ = !((o > 0.0 && o1 > 0.0 && o2 > 0.0 && o3 > 0.0) || (o < 0.0 && o1 < 0.0 && o2 < 0.0 && o3 < 0.0));
            }
        }
        hit = __ballot(h_) != 0ULL;
    }
    if (lane == 0) p.flags[box] = (unsigned char)((hit ? 1 : 0) | ((crossings & 1) << 1));
}

}  // namespace

// Bytes of scratch aq_land_filter_f64 needs for `entries` band entries: 32 (the segment's coordinates) per entry; 0 for entries <= 0 or
// entries >= 2^31.
extern "C" size_t aq_land_scratch_bytes(long long entries) {
    if (entries <= 0 || entries >= (1LL << 31)) return 0;
    return (size_t)entries * 32;
}

extern "C" int aq_land_filter_f64(const double* seg_dev, long long E, const int32_t* entry_seg_dev, long long entries, const int32_t* band_start_dev,
                                  int nbands, double Y0, double h, const double* boxes_dev, long long N, void* scratch_dev, size_t scratch_bytes,
                                  uint8_t* flags_dev, void* stream) {
    AQ_REQUIRE(E >= 0 && E < (1LL << 31), "land filter: %lld segments (at most 2^31 - 1 in one call)", E);
    AQ_REQUIRE(N >= 0 && N < (1LL << 31), "land filter: %lld boxes (at most 2^31 - 1 in one call)", N);
    AQ_REQUIRE(entries >= 0 && entries < (1LL << 31), "land filter: %lld band entries (at most 2^31 - 1 in one call)", entries);
    AQ_REQUIRE(h > 0.0 && h < __builtin_inf(), "land filter: band height h = %g (it has to be positive and finite)", h);      // (NaN fails too)
    AQ_REQUIRE(Y0 > -__builtin_inf() && Y0 < __builtin_inf(), "land filter: Y0 = %g (it has to be finite)", Y0);
    AQ_REQUIRE(nbands >= 1, "land filter: nbands = %d (at least 1)", nbands);
    if (N == 0) return AQ_OK;
    hipStream_t st = (hipStream_t)stream;
    if (E == 0 || entries == 0) {                                               // no land: every box is at sea
        AQ_REQUIRE(flags_dev, "land filter: null pointer");
        AQ_CHECK_HIP(hipMemsetAsync(flags_dev, 0, (size_t)N, st));
        return AQ_OK;
    }
    AQ_REQUIRE(seg_dev && entry_seg_dev && band_start_dev && boxes_dev && scratch_dev && flags_dev, "land filter: null pointer");
    AQ_REQUIRE(((uintptr_t)seg_dev & 31) == 0 && ((uintptr_t)boxes_dev & 31) == 0 && ((uintptr_t)scratch_dev & 31) == 0 &&
               ((uintptr_t)entry_seg_dev & 3) == 0 && ((uintptr_t)band_start_dev & 3) == 0, "land filter: unaligned array");
    const size_t need = aq_land_scratch_bytes(entries);
    AQ_REQUIRE(scratch_bytes >= need, "land filter: %zu bytes of scratch, %zu needed (aq_land_scratch_bytes)", scratch_bytes, need);
    LandParams p = {};
    p.t.seg = seg_dev; p.t.entry_seg = entry_seg_dev; p.t.band_start = band_start_dev; p.boxes = boxes_dev;
    p.t.eseg = (double4*)scratch_dev; p.flags = flags_dev;
    p.t.entries = entries; p.t.E = (int)E; p.N = (int)N; p.t.nbands = nbands; p.t.Y0 = Y0; p.t.h = h;
    hipLaunchKernelGGL(land_gather_kernel, dim3((unsigned)((entries + 255) / 256)), dim3(256), 0, st, p.t);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(land_flags_kernel, dim3((unsigned)((N + 3) / 4)), dim3(256), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
