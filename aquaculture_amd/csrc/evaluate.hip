// --evaluate: the two device steps of the cage-level precision / recall grid (reference src/get_kfold_cluster_performance.py: every
// combination of a confidence threshold c, a DBSCAN eps and a min_samples m, each one DBSCAN run per year plus two spatial joins).
//
// aq_eval_member_conf_f64.  Whether a detection belongs to ANY cluster at (c, m) needs no clustering.  With c_i the confidence of point i
// and N[i] its closed eps-neighbourhood in its group (dx dx + dy dy <= eps eps, i included; the search of facility_runs.h):
//   core     i is a core point at (c, m) iff c_i >= c and at least m points of N[i] have confidence >= c, that is
//            c <= T(i, m) = min(c_i, m-th largest confidence in N[i]); -inf when N[i] has fewer than m points
//   member   sklearn labels i >= 0 at (c, m) iff c_i >= c and some j of N[i] is core, that is
//            c <= M(i, m) = min(c_i, max over j in N[i] of T(j, m))
// for every m = 1 .. K at once.  Launches of one call, all on the caller's stream:
//   gather   coordinates and confidences in sorted order, the three key runs of every point
//   topk     the K largest confidences of N[i], kept sorted in registers (one compare-exchange per slot and neighbour) -> T, by sorted position
//   member   the maximum of T over N[i], per m, and the min with c_i -> M, in the caller's order
// Every T and M is one of the input confidences, bit for bit (only comparisons and selections), or -inf; no atomics: two calls give the
// same bytes.  A NaN confidence never enters a selection.
//
// aq_box_match_f64.  Q query boxes against N key boxes sorted by (group, x0): a query matches a key of its own group when the closed boxes
// intersect (touching edges and corners count, as shapely's `intersects`).  One wavefront (64 lanes) per query: a binary search bounds the
// group's run by key.x0 <= query.x1, the lanes stride over what is left, then a wave reduction: hit = any match; with a payload [N][K], the
// elementwise maximum over the matching keys (-inf when none).
#include "facility_runs.h"

namespace {

constexpr int EVAL_MAX_K = 16;

struct EvalParams : FacRuns {
    const double* conf;        // [n], original order
    int K;
    double* sconf;             // scratch [n]: confidences by sorted position; -inf for an entry of perm that is no index
    double* T;                 // scratch [n][K], by sorted position
    double* M;                 // out [n][K], original order
};

__global__ __launch_bounds__(256) void eval_gather_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n) return;
    const int o = fac_gather(p, i);
    p.sconf[i] = o >= 0 ? p.conf[o] : -__builtin_inf();
}

template <int KC>
__global__ __launch_bounds__(256) void eval_topk_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n) return;
    double top[KC];                                                             // descending; static indices only, so it stays in registers
#pragma unroll
    for (int m = 0; m < KC; ++m) top[m] = -__builtin_inf();
    fac_neighbours(p, i, [&](int k) {
        double v = p.sconf[k];
#pragma unroll
        for (int m = 0; m < KC; ++m) {                                          // v sinks to its place, what it displaces sinks on
            const double t = top[m];
            const bool gt = v > t;
            top[m] = gt ? v : t;
            v = gt ? t : v;
        }
    });
    const double c = p.sconf[i];
    double* out = p.T + i * p.K;
#pragma unroll
    for (int m = 0; m < KC; ++m)
        if (m < p.K) out[m] = top[m] < c ? top[m] : c;
}

template <int KC>
__global__ __launch_bounds__(256) void eval_member_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n) return;
    const int o = fac_orig(p, (int)i);
    if (o < 0) return;
    double mx[KC];
#pragma unroll
    for (int m = 0; m < KC; ++m) mx[m] = -__builtin_inf();
    fac_neighbours(p, i, [&](int k) {
        const double* t = p.T + (long long)k * p.K;
#pragma unroll
        for (int m = 0; m < KC; ++m)
            if (m < p.K) { const double v = t[m]; mx[m] = v > mx[m] ? v : mx[m]; }
    });
    const double c = p.sconf[i];
    double* out = p.M + (long long)o * p.K;
#pragma unroll
    for (int m = 0; m < KC; ++m)
        if (m < p.K) out[m] = mx[m] < c ? mx[m] : c;
}

struct MatchParams {
    const double4* qbox;       // [Q] (x0, y0, x1, y1)
    const int* qgroup;         // [Q]
    const double4* kbox;       // [N], sorted by (group, x0)
    const int* group_start;    // [G + 1]
    const double* payload;     // [N][K] or null
    int Q, N, G, K;            // K = 0 without a payload
    unsigned char* hit;        // out [Q]
    double* out;               // out [Q][K] or null
};

__global__ __launch_bounds__(256) void box_match_kernel(const MatchParams p) {
    const int lane = threadIdx.x & 63;
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: uniform from here on
    if (q >= p.Q) return;
    const double4 b = p.qbox[q];
    const int g = p.qgroup[q];
    int first = 0, end = 0;
    if ((unsigned)g < (unsigned)p.G) {                                          // (a table the caller got wrong stays inside [0, N])
        first = min(max(p.group_start[g], 0), p.N);
        end = min(max(p.group_start[g + 1], first), p.N);
    }
    int lo = first, hi = end;                                                   // the first key of the run with x0 > query.x1; NaN: an empty run
    while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (p.kbox[mid].x <= b.z) lo = mid + 1; else hi = mid;
    }
    end = lo;
    double mx[EVAL_MAX_K];
#pragma unroll
    for (int m = 0; m < EVAL_MAX_K; ++m) mx[m] = -__builtin_inf();
    bool any = false;
    for (int k = first + lane; k < end; k += 64) {
        const double4 a = p.kbox[k];
        if (a.x <= b.z && b.x <= a.z && a.y <= b.w && b.y <= a.w) {
            any = true;
            const double* t = p.payload + (long long)k * p.K;                   // (never read when K = 0)
#pragma unroll
            for (int m = 0; m < EVAL_MAX_K; ++m)
                if (m < p.K) { const double v = t[m]; mx[m] = v > mx[m] ? v : mx[m]; }
        }
    }
    const bool hit = __any(any) != 0;
    if (lane == 0) p.hit[q] = hit ? 1 : 0;
#pragma unroll
    for (int m = 0; m < EVAL_MAX_K; ++m) {
        if (m < p.K) {                                                          // uniform: every lane of the wave takes part in the exchange
            double v = mx[m];
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                const double w = __shfl_xor(v, s, 64);
                v = w > v ? w : v;
            }
            if (lane == 0) p.out[q * p.K + m] = v;
        }
    }
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

template <int KC>
void launch_member(const EvalParams& p, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL(eval_topk_kernel<KC>, grid, dim3(256), 0, st, p);
    hipLaunchKernelGGL(eval_member_kernel<KC>, grid, dim3(256), 0, st, p);
}

}  // namespace

// Bytes of scratch aq_eval_member_conf_f64 needs for n points and K sizes: 16 (coordinates) + 24 (runs) + 8 (confidence) + 8 K (T) per point,
// each array rounded up to 16 bytes; 0 for n <= 0, n >= 2^31 or K outside 1 .. 16.
extern "C" size_t aq_eval_scratch_bytes(long long n, int K) {
    if (n <= 0 || n >= (1LL << 31) || K < 1 || K > EVAL_MAX_K) return 0;
    return align16((size_t)n * 16) + align16((size_t)n * 24) + align16((size_t)n * 8) + align16((size_t)n * 8 * (size_t)K);
}

extern "C" int aq_eval_member_conf_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev,
                                       const double* conf_dev, long long n, double eps, int K, void* scratch_dev, size_t scratch_bytes,
                                       double* member_conf_dev, void* stream) {
    AQ_REQUIRE(n >= 0 && n < (1LL << 31), "evaluate: %lld points (at most 2^31 - 1 in one call)", n);
    AQ_REQUIRE(eps > 0.0 && eps * eps < __builtin_inf(), "evaluate: eps = %g (it has to be positive and finite)", eps);        // (NaN fails too)
    AQ_REQUIRE(K >= 1 && K <= EVAL_MAX_K, "evaluate: K = %d cluster sizes (1 to %d)", K, EVAL_MAX_K);
    if (n == 0) return AQ_OK;
    AQ_REQUIRE(keys_sorted_dev && perm_dev && xy_dev && group_dev && conf_dev && scratch_dev && member_conf_dev, "evaluate: null pointer");
    AQ_REQUIRE(((uintptr_t)keys_sorted_dev & 7) == 0 && ((uintptr_t)perm_dev & 3) == 0 && ((uintptr_t)xy_dev & 15) == 0 &&
               ((uintptr_t)group_dev & 3) == 0 && ((uintptr_t)conf_dev & 7) == 0 && ((uintptr_t)scratch_dev & 15) == 0 &&
               ((uintptr_t)member_conf_dev & 7) == 0, "evaluate: unaligned array");
    const size_t need = aq_eval_scratch_bytes(n, K);
    AQ_REQUIRE(scratch_bytes >= need, "evaluate: %zu bytes of scratch, %zu needed (aq_eval_scratch_bytes)", scratch_bytes, need);
    EvalParams p = {};
    p.keys = keys_sorted_dev; p.perm = perm_dev; p.xy = xy_dev; p.group = group_dev;
    p.n = (int)n; p.eps2 = eps * eps;
    p.conf = conf_dev; p.K = K;
    char* s = (char*)scratch_dev;
    p.sxy = (double2*)s;
    s += align16((size_t)n * 16);
    p.runs = (int2*)s;
    s += align16((size_t)n * 24);
    p.sconf = (double*)s;
    s += align16((size_t)n * 8);
    p.T = (double*)s;
    p.M = member_conf_dev;
    const dim3 grid((unsigned)((n + 255) / 256));
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(eval_gather_kernel, grid, dim3(256), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    if (K == 1) launch_member<1>(p, grid, st);
    else if (K <= 4) launch_member<4>(p, grid, st);
    else if (K <= 8) launch_member<8>(p, grid, st);
    else launch_member<EVAL_MAX_K>(p, grid, st);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_box_match_f64(const double* qbox_dev, const int32_t* qgroup_dev, long long Q, const double* kbox_dev, long long N,
                                const int32_t* group_start_dev, int G, const double* payload_dev, int K, uint8_t* hit_dev, double* out_dev,
                                void* stream) {
    AQ_REQUIRE(Q >= 0 && Q < (1LL << 31) && N >= 0 && N < (1LL << 31), "box match: %lld queries, %lld keys (at most 2^31 - 1 of each in one call)", Q, N);
    AQ_REQUIRE(G >= 0, "box match: %d groups", G);
    AQ_REQUIRE(K >= 0 && K <= EVAL_MAX_K, "box match: K = %d payload columns (0: no payload, to %d)", K, EVAL_MAX_K);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(qbox_dev && qgroup_dev && group_start_dev && hit_dev && (N == 0 || kbox_dev) && (K == 0 || (out_dev && (N == 0 || payload_dev))), "box match: null pointer");
    AQ_REQUIRE(((uintptr_t)qbox_dev & 31) == 0 && ((uintptr_t)kbox_dev & 31) == 0 && ((uintptr_t)qgroup_dev & 3) == 0 &&
               ((uintptr_t)group_start_dev & 3) == 0 && ((uintptr_t)payload_dev & 7) == 0 && ((uintptr_t)out_dev & 7) == 0, "box match: unaligned array");
    MatchParams p = {};
    p.qbox = (const double4*)qbox_dev; p.qgroup = qgroup_dev; p.kbox = (const double4*)kbox_dev; p.group_start = group_start_dev;
    p.payload = payload_dev; p.Q = (int)Q; p.N = (int)N; p.G = G; p.K = K;
    p.hit = hit_dev; p.out = out_dev;
    hipLaunchKernelGGL(box_match_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
