// The pieces the three box joins share (box_match_kernel of evaluate.hip, box_match_subsets_kernel of eval_subsets.hip and
// model_error_match_kernel of model_errors.hip): Q query boxes against N key boxes sorted by (group, x0), one wavefront (64 lanes) per query.
// A fix to the run bound, the predicate or a wave reduction is made here once.  Only comparisons and selections: every file that includes
// this is built with -ffp-contract=off, and each join stays bit-identical to its numpy restatement.
#pragma once
#include "aq_common.h"

namespace {

// whether the closed boxes (x0, y0, x1, y1) a and b intersect: touching edges and corners count, as shapely's `intersects`; false with a NaN.
// (The condition sits in an `if`, as it did in each kernel: returned as a value it compiles to a two-level branch in model_error_match_kernel.)
__device__ __forceinline__ bool boxes_meet(const double4& a, const double4& b) {
    if (a.x <= b.z && b.x <= a.z && a.y <= b.w && b.y <= a.w) return true;
    return false;
}

struct KeyRun { int first, end; };     // sorted key positions [first, end)

// The keys a query of group g with right edge x1 can meet: its group's run of group_start [G + 1], cut at the first key with x0 > x1 (a binary
// search, the same in every lane).  A group outside [0, G) and a NaN x1 give an empty run.
__device__ __forceinline__ KeyRun box_join_run(const int* group_start, int G, int N, const double4* kbox, int g, double x1) {
    KeyRun r = {0, 0};
    if ((unsigned)g < (unsigned)G) {                                            // (a table the caller got wrong stays inside [0, N])
        r.first = min(max(group_start[g], 0), N);
        r.end = min(max(group_start[g + 1], r.first), N);
    }
    int lo = r.first, hi = r.end;                                               // the first key of the run with x0 > query.x1; NaN: an empty run
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (kbox[mid].x <= x1) lo = mid + 1; else hi = mid;
    }
    r.end = lo;
    return r;
}

// the maximum of v over the 64 lanes, in every lane (a NaN never wins over a number); every lane of the wave has to take part
__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double w = __shfl_xor(v, s, 64);
        v = w > v ? w : v;
    }
    return v;
}

// the OR of v over the 64 lanes, in every lane
__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v |= (unsigned)__shfl_xor((int)v, s, 64);
    return v;
}

// out[m] = the maximum of payload[k][m], m < K <= KMAX, over the keys k of the run with match(k); -inf without one.  The lanes stride over the
// run, then one wave_max per column (K is uniform: every lane takes part) and lane 0 stores.  payload is never read when K = 0.  -> whether
// this lane met a matching key.
template <int KMAX, typename F>
__device__ __forceinline__ bool box_join_max(KeyRun run, int lane, const double* payload, int K, double* out, F match) {
    double mx[KMAX];
#pragma unroll
    for (int m = 0; m < KMAX; ++m) mx[m] = -__builtin_inf();
    bool any = false;
    for (int k = run.first + lane; k < run.end; k += 64) {
        if (match(k)) {
            any = true;
            const double* t = payload + (long long)k * K;
#pragma unroll
            for (int m = 0; m < KMAX; ++m)
                if (m < K) { const double v = t[m]; mx[m] = v > mx[m] ? v : mx[m]; }
        }
    }
#pragma unroll
    for (int m = 0; m < KMAX; ++m) {
        if (m < K) {
            const double v = wave_max(mx[m]);
            if (lane == 0) out[m] = v;
        }
    }
    return any;
}

}  // namespace
