// --facility-sites: the three device steps behind "known vs additional facilities" (reference src/Results/FacilitiesMaps.py:64-188:
// get_true_facilities, classify_our_facilities, count_unique_locations).  Closed boxes (x0, y0, x1, y1), fp64, EPSG:3857; `meet` is
// box_join.h's boxes_meet (touching counts, a NaN meets nothing).  Only comparisons, selections, integer adds and minima: every output is
// bit-identical to its numpy restatement in aquaculture_amd/facility_sites.py.  One wavefront per facility or query, four to a workgroup; no
// atomics, plain vector stores, nothing allocated, the caller's stream.
//
// aq_facility_bounds_f64.  Facility f owns the entries entry_start[f] .. entry_start[f + 1] - 1 (the CSR layout of aq_depth_ranges_f64) of
// entry_box [E][4]; those with entry_use[e] != 0 take part.  Lane l walks the entries a + l, a + l + 64, ... in ascending order keeping
//   x0 = v < x0 ? v : x0 (from +inf), likewise y0;   x1 = v > x1 ? v : x1 (from -inf), likewise y1     -- a NaN is never selected
// and the 64 partials fold by halves: m[i] = m[i + 32] < m[i] ? m[i + 32] : m[i], then + 16, ... + 1 (lane 0's view of the xor exchange).
// bounds[f] = the four selections; four canonical NaNs when one of them is not finite (no entry that takes part, or none with a number).
//
// aq_box_join_count_i32.  Q queries against N keys sorted by (group, x0) as aq_box_match_f64 takes them; kid [N] = the keys' original rows.
// count[q] = the keys of the query's group that meet it, first[q] = the smallest kid among them, -1 without one.
//
// aq_box_join_list_i32.  The same join; the kid of every meeting key, in ascending position of the sorted run, goes to
// list[offset[q] .. offset[q + 1]).  Per chunk of 64 keys: a ballot of the lanes that meet, lane l's slot = the running base + the
// popcount of the ballot's bits below l, base += the popcount of the ballot (uniform over the wave).  A slot outside the query's own slice
// (clamped into [0, total]) is not written: offsets the caller got wrong lose entries but write nowhere else.
#include "box_join.h"

namespace {

// the minimum of v over the 64 lanes, read in lane 0 (a NaN is never selected); every lane of the wave has to take part
__device__ __forceinline__ double wave_min_f64(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double w = __shfl_xor(v, s, 64);
        v = w < v ? w : v;
    }
    return v;
}

// the minimum and the sum of v over the 64 lanes, in every lane
__device__ __forceinline__ int wave_min_i32(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const int w = __shfl_xor(v, s, 64);
        v = w < v ? w : v;
    }
    return v;
}
__device__ __forceinline__ int wave_sum_i32(int v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v += __shfl_xor(v, s, 64);
    return v;
}

struct BoundsParams {
    const int* entry_start;    // [F + 1]
    const double4* entry_box;  // [E]
    const uint8_t* entry_use;  // [E]
    int F, E;
    double4* bounds;           // out [F]
};

__global__ __launch_bounds__(256) void facility_bounds_kernel(const BoundsParams p) {
    const int lane = threadIdx.x & 63;
    const long long f = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per facility: uniform from here on
    if (f >= p.F) return;
    const int a = min(max(p.entry_start[f], 0), p.E);                           // (a table the caller got wrong stays inside [0, E])
    const int b = min(max(p.entry_start[f + 1], a), p.E);
    const double inf = __builtin_inf();
    double x0 = inf, y0 = inf, x1 = -inf, y1 = -inf;
    for (int e = a + lane; e < b; e += 64) {
        if (p.entry_use[e]) {
            const double4 c = p.entry_box[e];
            x0 = c.x < x0 ? c.x : x0;
            y0 = c.y < y0 ? c.y : y0;
            x1 = c.z > x1 ? c.z : x1;
            y1 = c.w > y1 ? c.w : y1;
        }
    }
    x0 = wave_min_f64(x0);
    y0 = wave_min_f64(y0);
    x1 = wave_max(x1);
    y1 = wave_max(y1);
    if (lane == 0) {
        const bool finite = x0 > -inf && x0 < inf && y0 > -inf && y0 < inf && x1 > -inf && x1 < inf && y1 > -inf && y1 < inf;
        const double nan = __builtin_nan("");
        p.bounds[f] = finite ? make_double4(x0, y0, x1, y1) : make_double4(nan, nan, nan, nan);
    }
}

struct JoinParams {
    const double4* qbox;       // [Q]
    const int* qgroup;         // [Q]
    const double4* kbox;       // [N], sorted by (group, x0)
    const int* kid;            // [N] original row of each sorted key
    const int* group_start;    // [G + 1]
    int Q, N, G;
    int* count;                // out [Q]        (the count join)
    int* first;                // out [Q]
    const long long* offset;   // [Q + 1]        (the list join)
    int* list;                 // out [total]
    long long total;
};

__global__ __launch_bounds__(256) void box_join_count_kernel(const JoinParams p) {
    const int lane = threadIdx.x & 63;
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: uniform from here on
    if (q >= p.Q) return;
    const double4 b = p.qbox[q];
    const KeyRun run = box_join_run(p.group_start, p.G, p.N, p.kbox, p.qgroup[q], b.z);
    int cnt = 0, lowest = 0x7fffffff;
    for (int k = run.first + lane; k < run.end; k += 64) {
        if (boxes_meet(p.kbox[k], b)) {
            const int id = p.kid[k];
            cnt += 1;
            lowest = id < lowest ? id : lowest;
        }
    }
    cnt = wave_sum_i32(cnt);
    lowest = wave_min_i32(lowest);
    if (lane == 0) {
        p.count[q] = cnt;
        p.first[q] = cnt > 0 ? lowest : -1;
    }
}

__global__ __launch_bounds__(256) void box_join_list_kernel(const JoinParams p) {
    const int lane = threadIdx.x & 63;
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: uniform from here on
    if (q >= p.Q) return;
    const double4 b = p.qbox[q];
    const KeyRun run = box_join_run(p.group_start, p.G, p.N, p.kbox, p.qgroup[q], b.z);
    long long base = min(max(p.offset[q], 0LL), p.total);                       // the query's own slice, kept inside [0, total]
    const long long end = min(max(p.offset[q + 1], base), p.total);
    const unsigned long long below = (1ULL << lane) - 1ULL;                     // the lanes before this one
    for (int k0 = run.first; k0 < run.end; k0 += 64) {                          // uniform trip count: every lane votes in every chunk
        const int k = k0 + lane;
        bool m = false;
        if (k < run.end) m = boxes_meet(p.kbox[k], b);
        const unsigned long long mask = __ballot(m);
        const long long at = base + __popcll(mask & below);
        if (m && at < end) p.list[at] = p.kid[k];
        base += __popcll(mask);
    }
}

int join_arguments(const char* what, const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev,
                   const int32_t* kid_dev, const int32_t* group_start_dev, const int32_t* group_start_host, long long N, long long G) {
    AQ_REQUIRE(sg::facility_sites_count_fits(Q) && sg::facility_sites_count_fits(N) && sg::facility_sites_count_fits(G),
               "%s: %lld queries, %lld keys, %lld groups (each from 0 to 2^31 - 1 in one call)", what, Q, N, G);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(group_start_host, "%s: null pointer (the host copy of the group starts)", what);
    for (long long g = 0; g <= G; ++g)
        AQ_REQUIRE(group_start_host[g] >= 0 && group_start_host[g] <= N && (g == 0 || group_start_host[g] >= group_start_host[g - 1]),
                   "%s: group start %lld is %d (sorted, inside [0, %lld])", what, g, group_start_host[g], N);
    AQ_REQUIRE(qbox_dev && qgroup_dev && group_start_dev && (N == 0 || (kbox_dev && kid_dev)), "%s: null pointer", what);
    AQ_REQUIRE(((uintptr_t)qbox_dev & 31) == 0 && ((uintptr_t)kbox_dev & 31) == 0 && ((uintptr_t)qgroup_dev & 3) == 0 &&
               ((uintptr_t)kid_dev & 3) == 0 && ((uintptr_t)group_start_dev & 3) == 0, "%s: unaligned array", what);
    return AQ_OK;
}

}  // namespace

extern "C" int aq_facility_bounds_f64(const int32_t* entry_start_dev, const int32_t* entry_start_host, long long F, const double* entry_box_dev,
                                      const uint8_t* entry_use_dev, long long E, double* bounds_dev, void* stream) {
    AQ_REQUIRE(sg::facility_sites_count_fits(F) && sg::facility_sites_count_fits(E),
               "facility bounds: %lld facilities, %lld entries (each from 0 to 2^31 - 1 in one call)", F, E);
    if (F == 0) return AQ_OK;
    AQ_REQUIRE(entry_start_host, "facility bounds: null pointer (the host copy of the entry starts)");
    for (long long f = 0; f <= F; ++f)
        AQ_REQUIRE(entry_start_host[f] >= 0 && entry_start_host[f] <= E && (f == 0 || entry_start_host[f] >= entry_start_host[f - 1]),
                   "facility bounds: entry start %lld is %d (sorted, inside [0, %lld])", f, entry_start_host[f], E);
    AQ_REQUIRE(entry_start_dev && bounds_dev && (E == 0 || (entry_box_dev && entry_use_dev)), "facility bounds: null pointer");
    AQ_REQUIRE(((uintptr_t)entry_start_dev & 3) == 0 && ((uintptr_t)entry_box_dev & 31) == 0 && ((uintptr_t)bounds_dev & 31) == 0,
               "facility bounds: unaligned array");
    BoundsParams p = {};
    p.entry_start = entry_start_dev; p.entry_box = (const double4*)entry_box_dev; p.entry_use = entry_use_dev;
    p.F = (int)F; p.E = (int)E;
    p.bounds = (double4*)bounds_dev;
    hipLaunchKernelGGL(facility_bounds_kernel, dim3((unsigned)((F + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_box_join_count_i32(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, const int32_t* kid_dev,
                                     const int32_t* group_start_dev, const int32_t* group_start_host, long long N, long long G,
                                     int32_t* count_dev, int32_t* first_dev, void* stream) {
    const int rc = join_arguments("box join count", qbox_dev, qgroup_dev, Q, kbox_dev, kid_dev, group_start_dev, group_start_host, N, G);
    if (rc != AQ_OK || Q == 0) return rc;
    AQ_REQUIRE(count_dev && first_dev, "box join count: null pointer");
    AQ_REQUIRE(((uintptr_t)count_dev & 3) == 0 && ((uintptr_t)first_dev & 3) == 0, "box join count: unaligned array");
    JoinParams p = {};
    p.qbox = (const double4*)qbox_dev; p.qgroup = qgroup_dev; p.kbox = (const double4*)kbox_dev; p.kid = kid_dev; p.group_start = group_start_dev;
    p.Q = (int)Q; p.N = (int)N; p.G = (int)G;
    p.count = count_dev; p.first = first_dev;
    hipLaunchKernelGGL(box_join_count_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_box_join_list_i32(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, const int32_t* kid_dev,
                                    const int32_t* group_start_dev, const int32_t* group_start_host, long long N, long long G,
                                    const long long* offset_dev, const long long* offset_host, int32_t* list_dev, long long total, void* stream) {
    const int rc = join_arguments("box join list", qbox_dev, qgroup_dev, Q, kbox_dev, kid_dev, group_start_dev, group_start_host, N, G);
    if (rc != AQ_OK) return rc;
    AQ_REQUIRE(sg::facility_sites_count_fits(total), "box join list: %lld list entries (from 0 to 2^31 - 1 in one call)", total);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(offset_host, "box join list: null pointer (the host copy of the offsets)");
    for (long long q = 0; q <= Q; ++q)
        AQ_REQUIRE(offset_host[q] >= 0 && offset_host[q] <= total && (q == 0 || offset_host[q] >= offset_host[q - 1]),
                   "box join list: offset %lld is %lld (sorted, inside [0, %lld])", q, offset_host[q], total);
    AQ_REQUIRE(offset_dev && (total == 0 || list_dev), "box join list: null pointer");
    AQ_REQUIRE(((uintptr_t)offset_dev & 7) == 0 && ((uintptr_t)list_dev & 3) == 0, "box join list: unaligned array");
    JoinParams p = {};
    p.qbox = (const double4*)qbox_dev; p.qgroup = qgroup_dev; p.kbox = (const double4*)kbox_dev; p.kid = kid_dev; p.group_start = group_start_dev;
    p.Q = (int)Q; p.N = (int)N; p.G = (int)G;
    p.offset = offset_dev; p.list = list_dev; p.total = total;
    hipLaunchKernelGGL(box_join_list_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
