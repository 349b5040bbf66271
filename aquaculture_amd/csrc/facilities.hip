// --facilities: DBSCAN of the detections' centroids (reference src/cluster_facilities.py: sklearn.cluster.DBSCAN(eps = 10 m, min_samples = 5)
// per year or image pass), for n points (x, y) in metres (fp64) of dense groups that never interact.
//   core     a point with at least min_samples points of its group (itself included) at dx dx + dy dy <= eps eps, in fp64 and in exactly
//            that form (built with -ffp-contract=off: EPSG:3035 coordinates are about 4e6 m, so fp32 or the expanded ||a||^2 - 2 a.b + ||b||^2
//            decides pairs near eps wrongly)
//   cluster  a connected component of core points under that relation; its root is the smallest original index among its core points
//   border   a point that is not core takes the smallest root among its core neighbours (sklearn grows clusters in label order, so that
//            cluster reaches the point first); without a core neighbour it is noise: root -1
// The neighbour search (the caller's sort by grid cell, the three key runs of every point, one thread per point in sorted order) is
// facility_runs.h, which evaluate.hip shares.  Launches of one call, all on the caller's stream:
//   gather   the points' coordinates in sorted order (the runs are read contiguously from here on), the three runs of every point
//   count    neighbours in the runs -> core (also by sorted position); root = the point itself for a core point, else -1
//   unite    every core-core pair once (from its later point): find, then atomicMin on the larger root until both agree, in the forest that
//            `root` is, indexed by original index; a parent is never larger than its child, so a root is the set's smallest index
//   flatten  root = find(root) for core points
//   border   the minimum root among the core neighbours of every point that is not core
// Only integer min atomics, whose result does not depend on their order: two calls give the same bytes.  Unbounded loops: find (parents
// decrease strictly) and unite (the larger of the two roots decreases strictly).
#include "facility_runs.h"
#include <limits.h>

namespace {

struct FacParams : FacRuns {   // (the sorted keys, the points and the scratch of the gather: facility_runs.h)
    int min_samples;
    unsigned char* score;      // scratch [n]: core, by sorted position
    unsigned char* core;       // out [n]
    int* root;                 // out [n]; the forest meanwhile
};

__device__ __forceinline__ int ld(const int* p) { return __hip_atomic_load(p, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT); }

// (q < 0 happens only for a perm_dev that names a point twice, once as core and once not: the walk ends there instead of leaving the array)
__device__ __forceinline__ int find(const int* parent, int a) {
    for (int q; (q = ld(parent + a)) != a && q >= 0;) a = q;
    return a;
}

__device__ void unite(int* parent, int a, int b) {
    a = find(parent, a);
    b = find(parent, b);
    while (a != b) {
        if (a < b) { const int t = a; a = b; b = t; }
        const int old = atomicMin(parent + a, b);          // a was a root: it hangs under b now; else what it hung under has to meet b
        if (old == a) break;
        a = old;
    }
}

__global__ __launch_bounds__(256) void fac_gather_kernel(const FacParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < p.n) fac_gather(p, i);
}

__global__ __launch_bounds__(256) void fac_count_kernel(const FacParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n) return;
    const int o = fac_orig(p, (int)i);
    int cnt = 0;
    fac_neighbours(p, i, [&](int) { ++cnt; });
    const bool c = o >= 0 && cnt >= p.min_samples;
    p.score[i] = c ? 1 : 0;
    if (o >= 0) {
        p.core[o] = c ? 1 : 0;
        p.root[o] = c ? o : -1;
    }
}

__global__ __launch_bounds__(256) void fac_unite_kernel(const FacParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n || !p.score[i]) return;
    const int o = fac_orig(p, (int)i);
    fac_neighbours(p, i, [&](int k) {
        if (k < i && p.score[k]) unite(p.root, o, fac_orig(p, k));                  // (core entries have an index: count made sure)
    });
}

__global__ __launch_bounds__(256) void fac_flatten_kernel(const FacParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n || !p.score[i]) return;
    const int o = fac_orig(p, (int)i);
    __hip_atomic_store(p.root + o, find(p.root, o), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);     // (still an ancestor for whoever reads it meanwhile)
}

__global__ __launch_bounds__(256) void fac_border_kernel(const FacParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n || p.score[i]) return;
    const int o = fac_orig(p, (int)i);
    if (o < 0) return;
    int best = INT_MAX;
    fac_neighbours(p, i, [&](int k) {
        if (p.score[k]) best = min(best, p.root[fac_orig(p, k)]);                   // flat: a core point's root is its cluster's
    });
    if (best != INT_MAX) p.root[o] = best;                                      // (nobody reads the root of a point that is not core)
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

}  // namespace

// Bytes of scratch aq_facility_dbscan_f64 needs for n points: 16 (coordinates) + 24 (runs) + 1 (core flag) per point, each array rounded up to
// 16 bytes; 0 for n <= 0 or n >= 2^31.
extern "C" size_t aq_facility_scratch_bytes(long long n) {
    if (n <= 0 || n >= (1LL << 31)) return 0;
    return align16((size_t)n * 16) + align16((size_t)n * 24) + align16((size_t)n);
}

extern "C" int aq_facility_dbscan_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev,
                                      long long n, double eps, int min_samples, void* scratch_dev, size_t scratch_bytes, uint8_t* core_dev,
                                      int32_t* root_dev, void* stream) {
    AQ_REQUIRE(n >= 0 && n < (1LL << 31), "facilities: %lld points (at most 2^31 - 1 in one call)", n);
    AQ_REQUIRE(eps > 0.0 && eps * eps < __builtin_inf(), "facilities: eps = %g (it has to be positive and finite)", eps);      // (NaN fails too)
    AQ_REQUIRE(min_samples >= 1, "facilities: min_samples = %d (at least 1)", min_samples);
    if (n == 0) return AQ_OK;
    AQ_REQUIRE(keys_sorted_dev && perm_dev && xy_dev && group_dev && scratch_dev && core_dev && root_dev, "facilities: null pointer");
    AQ_REQUIRE(((uintptr_t)keys_sorted_dev & 7) == 0 && ((uintptr_t)perm_dev & 3) == 0 && ((uintptr_t)xy_dev & 15) == 0 &&
               ((uintptr_t)group_dev & 3) == 0 && ((uintptr_t)scratch_dev & 15) == 0 && ((uintptr_t)root_dev & 3) == 0, "facilities: unaligned array");
    const size_t need = aq_facility_scratch_bytes(n);
    AQ_REQUIRE(scratch_bytes >= need, "facilities: %zu bytes of scratch, %zu needed (aq_facility_scratch_bytes)", scratch_bytes, need);
    FacParams p = {};
    p.keys = keys_sorted_dev; p.perm = perm_dev; p.xy = xy_dev; p.group = group_dev;
    p.n = (int)n; p.min_samples = min_samples; p.eps2 = eps * eps;
    char* s = (char*)scratch_dev;
    p.sxy = (double2*)s;
    p.runs = (int2*)(s + align16((size_t)n * 16));
    p.score = (unsigned char*)(s + align16((size_t)n * 16) + align16((size_t)n * 24));
    p.core = core_dev; p.root = root_dev;
    const dim3 grid((unsigned)((n + 255) / 256)), block(256);
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fac_gather_kernel, grid, block, 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fac_count_kernel, grid, block, 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fac_unite_kernel, grid, block, 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fac_flatten_kernel, grid, block, 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    hipLaunchKernelGGL(fac_border_kernel, grid, block, 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
