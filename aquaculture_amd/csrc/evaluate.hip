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
//
// The three member-confidence kernels are eval_member.h's with SUBSETS = false (eval_subsets.hip runs the same source with masks); the join
// is built from box_join.h, which eval_subsets.hip's and model_errors.hip's joins share.
#include "eval_member.h"
#include "box_join.h"

namespace {

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
    const KeyRun run = box_join_run(p.group_start, p.G, p.N, p.kbox, p.qgroup[q], b.z);
    const bool any = box_join_max<EVAL_MAX_K>(run, lane, p.payload, p.K, p.out + q * p.K,      // one pass: the hit and the payload maxima together
                                              [&](int k) { const double4 a = p.kbox[k]; return boxes_meet(a, b); });
    const bool hit = __any(any) != 0;
    if (lane == 0) p.hit[q] = hit ? 1 : 0;
}

}  // namespace

// Bytes of scratch aq_eval_member_conf_f64 needs for n points and K sizes: 16 (coordinates) + 24 (runs) + 8 (confidence) + 8 K (T) per point,
// each array rounded up to 16 bytes; 0 for n <= 0, n >= 2^31 or K outside 1 .. 16.
extern "C" size_t aq_eval_scratch_bytes(long long n, int K) {
    if (n <= 0 || n >= (1LL << 31) || K < 1 || K > EVAL_MAX_K) return 0;
    EvalParams p = {};
    return eval_scratch_layout<false>(p, nullptr, (size_t)n, (size_t)K, 1);
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
    p.conf = conf_dev; p.K = K; p.S = 1;
    eval_scratch_layout<false>(p, scratch_dev, (size_t)n, (size_t)K, 1);
    p.M = member_conf_dev;
    return eval_member_launch<false>(p, (hipStream_t)stream);
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
