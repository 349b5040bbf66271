// --dedup-overlaps: every cage once where the download boxes overlap (reference src/utils.py:241-322, deduplicate_download_boxes and
// deduplicate_gdf_with_bboxes).  n closed axis-parallel boxes R_i = (x0, y0, x1, y1) in file order, fp64 EPSG:3857; a box yields to every
// box before it.  The rule (aquaculture_amd/overlaps.py), comparisons only:
//   C_i          the earlier boxes j < i whose open interiors meet R_i's: x0_j < x1_i && x1_j > x0_i, likewise in y
//   grid of i    xs = the distinct x0_i, x1_i and x0_j, x1_j of the boxes taking part, clamped into [x0_i, x1_i]; ys likewise; a cell is
//                covered iff one of those boxes contains it
//   detection D  of box i, on the grid built from P(D) = the boxes of C_i that meet the closed D:
//                0 dropped   no uncovered cell meets the closed D            1 whole      uncovered cells, and no covered one, meet D's open interior
//                2 clipped   an uncovered and a covered cell meet it         3 touching   an uncovered cell meets the closed D only
//                clip_bounds = min / max over the pieces cell ^ D of the uncovered cells that meet the closed D; clip_area = their areas
//                (min(x1) - max(x0)) * (min(y1) - max(y0)), added per row of the grid to a row sum from 0, the row sums added bottom to top
//                (built with -ffp-contract=off); state 0: NaN bounds, area 0
//   has_region   of box i: the detection D = R_i is not dropped
// aq_overlap_partners_f64: the lists C_i.  Search structure, the one of land_filter.hip / coverage.hip: nbands horizontal bands,
// band(y) = floor((y - Y0) / h) clamped to [0, nbands); the host entered box j in every band from band(y0_j) to band(y1_j) with the SAME
// expression, ascending j inside a band.  One wavefront per box i over the runs of band(y0_i) .. band(y1_i); a box met in several bands
// counts in the first of them, max(band(y0_j), band(y0_i)).  Count pass (start[i] = |C_i|), an exclusive scan in place (one workgroup), then,
// in a second call once the host has sized the list, the fill pass: a partner's place is the number of partners with a smaller j (ballots
// and shuffles over the same runs), so every list is ascending whatever the bands.
// aq_overlap_clip_f64: one wavefront per detection.  Lanes hold the partners of the box (64 at a time; the first 64 stay in registers,
// longer lists are read again from memory on every pass, so no count is too large), keep those that meet the closed D, and the wavefront
// walks D's grid in the written order: the next edge after v is the minimum over the lanes of the clamped partner edges above v (a wave
// reduction), a cell's `covered` a ballot.  Without a partner that meets D the grid is the one cell R_i and the walk is two steps.  The
// grid is never stored, so none is too large.
// No atomics, no LDS, plain vector stores; every index read from memory is kept inside its array.  Two calls give the same bytes.
#include "aq_common.h"

namespace {

struct PartnerParams {
    const double* boxes;       // [n][4]
    const int* entry_box;      // [entries]
    const int* band_start;     // [nbands + 1]
    long long* start;          // [n + 1]: counts, then (scan) first list entries
    int* partner;              // [cap] (fill)
    long long entries, cap;
    int n, nbands;
    double Y0, h;
};

__device__ __forceinline__ long long start_of(const PartnerParams& p, int b) {
    const long long v = p.band_start[b];
    return v < 0 ? 0 : v > p.entries ? p.entries : v;
}

__device__ __forceinline__ int band_of(const PartnerParams& p, double y) {
    const double t = floor((y - p.Y0) / p.h);
    return !(t >= 0.0) ? 0 : t < (double)p.nbands ? (int)t : p.nbands - 1;
}

// the partner at entry k of band b for box i (r; first band b0), or -1
__device__ __forceinline__ int partner_at(const PartnerParams& p, long long k, long long end, int b, int b0, int i, const double4& r) {
    if (k >= end) return -1;
    const int j = p.entry_box[k];
    if ((unsigned)j >= (unsigned)i) return -1;
    const double4 q = *(const double4*)(p.boxes + 4LL * j);
    if (!(q.x < r.z && q.z > r.x && q.y < r.w && q.w > r.y)) return -1;
    const int lo = band_of(p, q.y);
    return b == (lo > b0 ? lo : b0) ? j : -1;
}

template <bool FILL>
__global__ __launch_bounds__(256) void overlap_partners_kernel(const PartnerParams p) {
    const long long i = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per box: everything below is uniform in it
    if (i >= p.n) return;
    const int lane = threadIdx.x & 63;
    const double4 r = *(const double4*)(p.boxes + 4 * i);
    const int b0 = band_of(p, r.y), b1 = band_of(p, r.w);
    long long first = 0, mine = 0;
    if (FILL) {
        first = p.start[i];
        mine = p.start[i + 1] - first;
        if (first < 0 || mine <= 0 || first + mine > p.cap) return;             // (a table that is not this call's scan: nothing is written)
    }
    long long count = 0;
    for (int b = b0; b <= b1; ++b) {
        const long long s = start_of(p, b), e = start_of(p, b + 1);
        for (long long base = s; base < e; base += 64) {
            const int j = partner_at(p, base + lane, e, b, b0, (int)i, r);
            const unsigned long long found = __ballot(j >= 0);
            count += __popcll(found);
            if (!FILL || found == 0ULL) continue;
            long long rank = 0;                                                 // partners below j, over the same runs
            for (int b2 = b0; b2 <= b1; ++b2) {
                const long long s2 = start_of(p, b2), e2 = start_of(p, b2 + 1);
                for (long long base2 = s2; base2 < e2; base2 += 64) {
                    const int j2 = partner_at(p, base2 + lane, e2, b2, b0, (int)i, r);
                    unsigned long long todo = __ballot(j2 >= 0);
                    while (todo) {
                        const int src = __ffsll((long long)todo) - 1;
                        todo &= todo - 1;
                        rank += __shfl(j2, src) < j ? 1 : 0;
                    }
                }
            }
            if (j >= 0 && rank < mine) p.partner[first + rank] = j;
        }
    }
    if (!FILL && lane == 0) p.start[i] = count;
}

// exclusive scan of start[0 .. n) in place, start[n] = the total: one workgroup
__global__ __launch_bounds__(256) void overlap_scan_kernel(long long* start, int n) {
    __shared__ long long wsum[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    long long carry = 0;
    for (long long base = 0; base < n; base += 256) {
        const long long i = base + threadIdx.x;
        const long long v = i < n ? start[i] : 0;
        long long inc = v;
        for (int d = 1; d < 64; d <<= 1) {
            const long long t = __shfl_up(inc, d);
            if (lane >= d) inc += t;
        }
        if (lane == 63) wsum[w] = inc;
        __syncthreads();
        long long off = 0;
        for (int k = 0; k < w; ++k) off += wsum[k];
        const long long total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
        if (i < n) start[i] = carry + off + inc - v;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) start[n] = carry;
}

struct ClipParams {
    const double* boxes;       // [n][4]
    const long long* start;    // [n + 1]
    const int* partner;        // [T]
    const int* det_row;        // [m]; null: the boxes themselves (has_region)
    const double* dets;        // [m][4]
    unsigned char* state;      // out [m]
    double* bounds;            // out [m][4]
    double* area;              // out [m]
    unsigned char* has_region; // out [n]
    long long T;
    int n, m;
};

struct Partners {              // of one box, seen from one lane
    const ClipParams* p;
    long long first, count;    // the list partner[first .. first + count)
    double4 D;
    double4 q0;                // this lane's partner of the first 64 (NaN: none, or it does not meet the closed D)
    int chunks;                // 64 partners each; 0: nobody meets D

    __device__ __forceinline__ double4 fetch(int c) const {
        const double nan = __builtin_nan("");
        double4 q = {nan, nan, nan, nan};
        const long long k = c * 64LL + (threadIdx.x & 63);
        if (k < count) {
            const int j = p->partner[first + k];
            if ((unsigned)j < (unsigned)p->n) {
                const double4 v = *(const double4*)(p->boxes + 4LL * j);
                if (v.x <= D.z && D.x <= v.z && v.y <= D.w && D.y <= v.w) q = v;
            }
        }
        return q;
    }
    __device__ __forceinline__ double4 at(int c) const { return c == 0 ? q0 : fetch(c); }

    // the smallest of hi and the partners' edges along one axis, clamped into [lo, hi], above cur
    template <bool Y>
    __device__ __forceinline__ double next_edge(double cur, double lo, double hi) const {
        if (chunks == 0) return hi;
        double best = hi;
        for (int c = 0; c < chunks; ++c) {
            const double4 q = at(c);
            double e0 = Y ? q.y : q.x, e1 = Y ? q.w : q.z;
            e0 = e0 < lo ? lo : e0 > hi ? hi : e0;
            e1 = e1 < lo ? lo : e1 > hi ? hi : e1;
            if (e0 > cur && e0 < best) best = e0;
            if (e1 > cur && e1 < best) best = e1;
        }
        for (int d = 32; d >= 1; d >>= 1) {
            const double o = __shfl_xor(best, d);
            best = o < best ? o : best;
        }
        return best;
    }

    __device__ __forceinline__ bool covered(double xa, double ya, double xb, double yb) const {
        for (int c = 0; c < chunks; ++c) {
            const double4 q = at(c);
            if (__ballot(q.x <= xa && xb <= q.z && q.y <= ya && yb <= q.w) != 0ULL) return true;
        }
        return false;
    }
};

__global__ __launch_bounds__(256) void overlap_clip_kernel(const ClipParams p, const int boxes_only) {
    const int lane = threadIdx.x & 63;
    const long long items = boxes_only ? p.n : p.m;
    for (long long k = blockIdx.x * 4LL + (threadIdx.x >> 6); k < items; k += gridDim.x * 4LL) {   // one wavefront per item: uniform below
        const double nan = __builtin_nan("");
        const long long i = boxes_only ? k : (long long)p.det_row[k];
        int state = 0;
        double bx0 = nan, by0 = nan, bx1 = nan, by1 = nan, area = 0.0;
        if (i >= 0 && i < p.n) {
            const double4 R = *(const double4*)(p.boxes + 4 * i);
            const double4 D = boxes_only ? R : *(const double4*)(p.dets + 4 * k);
            Partners P;
            P.p = &p;
            P.D = D;
            long long s = p.start[i], e = p.start[i + 1];
            s = s < 0 ? 0 : s > p.T ? p.T : s;
            e = e < s ? s : e > p.T ? p.T : e;
            P.first = s;
            P.count = e - s;
            P.chunks = (int)((P.count + 63) / 64);                              // (count < 2^31: the list of one box holds earlier boxes once)
            P.q0 = P.fetch(0);
            bool any = false;
            for (int c = 0; c < P.chunks && !any; ++c) {
                const double4 q = P.at(c);
                any = __ballot(q.x == q.x) != 0ULL;
            }
            if (!any) P.chunks = 0;
            bool u_closed = false, u_open = false, c_open = false;
            const double inf = __builtin_inf();
            double mx0 = inf, my0 = inf, mx1 = -inf, my1 = -inf;
            const long long steps = 2 * P.count + 2;                            // more edges than a grid has: the walk ends whatever the data
            double ya = R.y;
            for (long long ny = 0; ya < R.w && ny < steps; ++ny) {
                const double yb = P.next_edge<true>(ya, R.y, R.w);
                if (ya <= D.w && D.y <= yb) {
                    double row = 0.0;
                    double xa = R.x;
                    for (long long nx = 0; xa < R.z && nx < steps; ++nx) {
                        const double xb = P.next_edge<false>(xa, R.x, R.z);
                        if (xa <= D.z && D.x <= xb) {
                            const bool cov = P.covered(xa, ya, xb, yb);
                            const double px0 = xa > D.x ? xa : D.x, px1 = xb < D.z ? xb : D.z;
                            const double py0 = ya > D.y ? ya : D.y, py1 = yb < D.w ? yb : D.w;
                            const bool opens = px0 < px1 && py0 < py1;
                            if (cov) {
                                c_open = c_open || opens;
                            } else {
                                u_closed = true;
                                u_open = u_open || opens;
                                mx0 = px0 < mx0 ? px0 : mx0;
                                my0 = py0 < my0 ? py0 : my0;
                                mx1 = px1 > mx1 ? px1 : mx1;
                                my1 = py1 > my1 ? py1 : my1;
                                row = row + (px1 - px0) * (py1 - py0);
                            }
                        }
                        xa = xb;
                    }
                    area = area + row;
                }
                ya = yb;
            }
            if (u_closed) {
                state = u_open && c_open ? 2 : u_open ? 1 : 3;
                bx0 = mx0; by0 = my0; bx1 = mx1; by1 = my1;
            } else {
                area = 0.0;
            }
        }
        if (lane == 0) {
            if (boxes_only) {
                p.has_region[k] = state != 0;
            } else {
                p.state[k] = (unsigned char)state;
                p.bounds[4 * k + 0] = bx0;
                p.bounds[4 * k + 1] = by0;
                p.bounds[4 * k + 2] = bx1;
                p.bounds[4 * k + 3] = by1;
                p.area[k] = area;
            }
        }
    }
}

// workgroups of a grid-stride launch over `waves` wavefronts of work, four to a workgroup: at most 8 resident workgroups' worth per CU
hipError_t grid_for(long long waves, unsigned* grid) {
    int cus = 0;
    const hipError_t e = aq_cus(&cus);
    if (e != hipSuccess) return e;
    const long long want = sg::cdiv(waves, 4), cap = 8LL * (cus > 0 ? cus : 1);
    *grid = (unsigned)(want < cap ? want : cap);
    return hipSuccess;
}

}  // namespace

extern "C" int aq_overlap_partners_f64(const double* boxes_dev, long long n, const int32_t* entry_box_dev, long long entries,
                                       const int32_t* band_start_dev, long long nbands, double Y0, double h, long long* start_dev,
                                       int32_t* partner_dev, long long partner_cap, void* stream) {
    AQ_REQUIRE(sg::overlap_count_fits(n) && sg::overlap_count_fits(entries) && sg::overlap_count_fits(partner_cap),
               "overlaps: %lld boxes, %lld band entries, room for %lld partners (each 0 .. 2^31 - 1 in one call)", n, entries, partner_cap);
    AQ_REQUIRE(sg::overlap_bands_fit(nbands), "overlaps: nbands = %lld (1 .. 2^31 - 2)", nbands);
    AQ_REQUIRE(h > 0.0 && h < __builtin_inf(), "overlaps: band height h = %g (it has to be positive and finite)", h);           // (NaN fails too)
    AQ_REQUIRE(Y0 > -__builtin_inf() && Y0 < __builtin_inf(), "overlaps: Y0 = %g (it has to be finite)", Y0);
    AQ_REQUIRE(start_dev && ((uintptr_t)start_dev & 7) == 0, "overlaps: start is null or unaligned");
    hipStream_t st = (hipStream_t)stream;
    const bool fill = partner_dev != nullptr;
    if (fill && (n == 0 || partner_cap == 0)) return AQ_OK;
    PartnerParams p = {};
    p.start = start_dev; p.partner = partner_dev; p.cap = partner_cap; p.n = (int)n;
    if (n > 0) {
        AQ_REQUIRE(boxes_dev && band_start_dev && (entry_box_dev || entries == 0), "overlaps: null pointer");
        AQ_REQUIRE(((uintptr_t)boxes_dev & 31) == 0 && ((uintptr_t)entry_box_dev & 3) == 0 && ((uintptr_t)band_start_dev & 3) == 0 &&
                   ((uintptr_t)partner_dev & 3) == 0, "overlaps: unaligned array");
        p.boxes = boxes_dev; p.entry_box = entry_box_dev; p.band_start = band_start_dev;
        p.entries = entries; p.nbands = (int)nbands; p.Y0 = Y0; p.h = h;
        const dim3 grid((unsigned)sg::cdiv(n, 4));
        if (fill) hipLaunchKernelGGL(overlap_partners_kernel<true>, grid, dim3(256), 0, st, p);
        else hipLaunchKernelGGL(overlap_partners_kernel<false>, grid, dim3(256), 0, st, p);
        AQ_CHECK_HIP(hipGetLastError());
    }
    if (!fill) {
        hipLaunchKernelGGL(overlap_scan_kernel, dim3(1), dim3(256), 0, st, start_dev, (int)n);
        AQ_CHECK_HIP(hipGetLastError());
    }
    return AQ_OK;
}

extern "C" int aq_overlap_clip_f64(const double* boxes_dev, long long n, const long long* start_dev, const int32_t* partner_dev, long long T,
                                   const int32_t* det_row_dev, const double* dets_dev, long long m, uint8_t* state_dev, double* bounds_dev,
                                   double* area_dev, uint8_t* has_region_dev, void* stream) {
    AQ_REQUIRE(sg::overlap_count_fits(n) && sg::overlap_count_fits(T) && sg::overlap_count_fits(m),
               "overlaps: %lld boxes, %lld partners, %lld detections (each 0 .. 2^31 - 1 in one call)", n, T, m);
    if (n == 0 && m == 0) return AQ_OK;
    hipStream_t st = (hipStream_t)stream;
    ClipParams p = {};
    p.n = (int)n; p.m = (int)m; p.T = T;
    if (n > 0) {
        AQ_REQUIRE(boxes_dev && start_dev && has_region_dev && (partner_dev || T == 0), "overlaps: null pointer");
        AQ_REQUIRE(((uintptr_t)boxes_dev & 31) == 0 && ((uintptr_t)start_dev & 7) == 0 && ((uintptr_t)partner_dev & 3) == 0, "overlaps: unaligned array");
        p.boxes = boxes_dev; p.start = start_dev; p.partner = partner_dev; p.has_region = has_region_dev;
        unsigned grid = 0;
        AQ_CHECK_HIP(grid_for(n, &grid));
        hipLaunchKernelGGL(overlap_clip_kernel, dim3(grid), dim3(256), 0, st, p, 1);
        AQ_CHECK_HIP(hipGetLastError());
    }
    if (m > 0) {
        AQ_REQUIRE(det_row_dev && dets_dev && state_dev && bounds_dev && area_dev, "overlaps: null pointer");
        AQ_REQUIRE(((uintptr_t)dets_dev & 31) == 0 && ((uintptr_t)det_row_dev & 3) == 0 && ((uintptr_t)bounds_dev & 7) == 0 &&
                   ((uintptr_t)area_dev & 7) == 0, "overlaps: unaligned array");
        p.det_row = det_row_dev; p.dets = dets_dev; p.state = state_dev; p.bounds = bounds_dev; p.area = area_dev;
        unsigned grid = 0;
        AQ_CHECK_HIP(grid_for(m, &grid));
        hipLaunchKernelGGL(overlap_clip_kernel, dim3(grid), dim3(256), 0, st, p, 0);   // (n = 0: every row is outside the table: dropped)
        AQ_CHECK_HIP(hipGetLastError());
    }
    return AQ_OK;
}
