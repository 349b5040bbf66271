// The neighbour search that facilities.hip (--facilities) and evaluate.hip (--evaluate) share: n points (x, y) in metres (fp64) of dense groups
// that never interact, sorted by the caller by a key that packs (group, cell row, cell column) of a grid whose cell edge is a little above eps
// (engine.facility_sort_keys), so that every neighbour of a point lies in the 3 x 3 cells around its own, and the three cells cx - 1 .. cx + 1
// of one cell row are ONE run of the sorted keys: two binary searches per row, no hash table, no O(n^2) memory.  One thread per point, in
// sorted order, so that the threads of a wave read the same runs.  The distance test is dx dx + dy dy <= eps eps in fp64 and in exactly that
// form: every file that includes this is built with -ffp-contract=off.
#pragma once
#include "aq_common.h"

namespace {

struct FacRuns {
    const long long* keys;     // [n] ascending
    const int* perm;           // [n] sorted position -> original index
    const double* xy;          // [n][2], original order
    const int* group;          // [n], original order
    int n;
    double eps2;
    double2* sxy;              // scratch [n]: coordinates by sorted position
    int2* runs;                // scratch [n][3]: [first, end) sorted positions of the cell rows cy - 1, cy, cy + 1
};

// first position in [0, n) whose key is >= k (upper = false) or > k (upper = true); n if none
__device__ __forceinline__ int fac_bound(const long long* keys, int n, long long k, bool upper) {
    int lo = 0, hi = n;
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        const long long v = keys[mid];
        if (upper ? v <= k : v < k) lo = mid + 1; else hi = mid;
    }
    return lo;
}

// original index of the point at sorted position k, or -1 for an entry that is no index (a permutation the caller did not check)
__device__ __forceinline__ int fac_orig(const FacRuns& p, int k) {
    const int o = p.perm[k];
    return (unsigned)o < (unsigned)p.n ? o : -1;
}

// The gather of sorted position i < n: its coordinates into sxy, its three runs into runs -> its original index, or -1
__device__ __forceinline__ int fac_gather(const FacRuns& p, long long i) {
    const int o = fac_orig(p, (int)i);
    double2 v = {0.0, 0.0};
    if (o >= 0) v = *(const double2*)(p.xy + 2LL * o);
    p.sxy[i] = v;
    const long long key = p.keys[i];
    const long long cx = key & AQ_FACILITY_CELL_MASK, cy = (key >> AQ_FACILITY_CELL_BITS) & AQ_FACILITY_CELL_MASK;
    const long long g = o >= 0 ? (long long)p.group[o] : 0;
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        int2 run = {0, 0};                                                      // a cell at the grid's edge (the caller leaves a free ring) or a bad entry: no run
        if (o >= 0 && g >= 0 && g <= AQ_FACILITY_CELL_MASK && cx >= 1 && cx < AQ_FACILITY_CELL_MASK && cy + r >= 1 && cy + r - 1 <= AQ_FACILITY_CELL_MASK) {
            const long long row = (g << (2 * AQ_FACILITY_CELL_BITS)) | ((cy + r - 1) << AQ_FACILITY_CELL_BITS);
            run.x = fac_bound(p.keys, p.n, row | (cx - 1), false);
            run.y = fac_bound(p.keys, p.n, row | (cx + 1), true);
        }
        p.runs[3 * i + r] = run;
    }
    return o;
}

// f(k) for the sorted positions k of the points within eps in the runs of sorted position i, the point itself included
template <typename F>
__device__ __forceinline__ void fac_neighbours(const FacRuns& p, long long i, F f) {
    const double2 a = p.sxy[i];
#pragma unroll
    for (int r = 0; r < 3; ++r) {
        const int2 run = p.runs[3 * i + r];
        for (int k = run.x; k < run.y; ++k) {
            const double2 b = p.sxy[k];
            const double dx = b.x - a.x, dy = b.y - a.y;
            if (dx * dx + dy * dy <= p.eps2) f(k);
        }
    }
}

}  // namespace
