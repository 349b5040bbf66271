// --evaluate-kfold: the two device steps of evaluate.hip for up to 32 subsets of one point set at once.  The folds of a cross-validation
// (reference src/get_kfold_cluster_performance.py: StratifiedKFold over the images, the 82 x 8 x 10 grid on every fold's train images, the
// winners on its test images) are subsets of the same detections and labels; a subset is one bit of a uint32 word per point.  One sort, one
// gather and one set of key runs per distance serve all of them (facility_runs.h, unchanged): only the neighbourhoods and the joins are cut
// down to the subset, by one bit test per candidate.
//
// aq_eval_member_conf_subsets_f64.  For point i of subset s, with N[i] the closed eps-neighbourhood of evaluate.hip:
//   T_s(i, m) = min(c_i, m-th largest confidence in N[i] ∩ s)          (-inf when there are fewer than m)
//   M_s(i, m) = min(c_i, max over j in N[i] ∩ s of T_s(j, m))
// which is evaluate.hip's M of the points of s alone.  Rows of points outside s are -inf.  Launches of one call, all on the caller's stream:
//   gather   as evaluate.hip's, and the mask words by sorted position (bits at and above S cleared)
//   topk     one lane per (sorted point, subset): blockIdx.y is the subset, the 64 lanes of a wave are 64 neighbouring sorted points, as in
//            evaluate.hip, so the lanes of a wave walk nearly the same key runs and their loads of coordinates, confidences and mask words
//            fall into the same cache lines; the K largest confidences stay in registers (static indices only) -> T [S][n][K]
//   member   the same mapping: the maximum of T_s over N[i] ∩ s, min with c_i -> M [S][n][K], in the caller's order
// Only comparisons and selections, no atomics: two calls give the same bytes; every value is an input confidence or -inf.
//
// aq_box_match_subsets_f64.  evaluate.hip's join, one wavefront per query, with a mask word per query and per key:
//   hitmask[q] = qmask[q] & OR of kmask over the matching keys
//   out[s][q][m] = max of payload[s][k][m] over the matching keys k that have bit s; -inf when there is none or q is not in s
// A first pass over the run ORs the matching keys' words (wave reduction); the loop over the set bits of the result -- the same word in every
// lane -- then takes one more pass per subset that has a match, every lane in every exchange.  Subsets without a match are filled with -inf.
//
// The three member-confidence kernels are eval_member.h's with SUBSETS = true: evaluate.hip's source, not a copy of it.  The join's run bound,
// predicate, reductions and per-subset pass are box_join.h's.
#include "eval_member.h"
#include "box_join.h"

namespace {

struct SubsetMatchParams {
    const double4* qbox;       // [Q] (x0, y0, x1, y1)
    const int* qgroup;         // [Q]
    const unsigned* qmask;     // [Q]
    const double4* kbox;       // [N], sorted by (group, x0)
    const unsigned* kmask;     // [N], key order
    const int* group_start;    // [G + 1]
    const double* payload;     // [S][N][K] or null
    int Q, N, G, K, S;         // K = 0 without a payload
    unsigned* hitmask;         // out [Q]
    double* out;               // out [S][Q][K] or null
};

__global__ __launch_bounds__(256) void box_match_subsets_kernel(const SubsetMatchParams p) {
    const int lane = threadIdx.x & 63;
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: uniform from here on
    if (q >= p.Q) return;
    const double4 b = p.qbox[q];
    const unsigned qm = p.qmask[q] & low_bits(p.S);
    const KeyRun run = box_join_run(p.group_start, p.G, p.N, p.kbox, p.qgroup[q], b.z);
    unsigned km = 0;
    for (int k = run.first + lane; k < run.end; k += 64)
        if (boxes_meet(p.kbox[k], b)) km |= p.kmask[k];
    const unsigned live = (unsigned)__builtin_amdgcn_readfirstlane((int)(wave_or(km) & qm));    // the same in every lane: the loops below are uniform
    if (lane == 0) p.hitmask[q] = live;
    if (p.K == 0) return;
    for (int s = 0; s < p.S; ++s) {
        double* out = p.out + ((long long)s * p.Q + q) * p.K;
        if (!((live >> s) & 1u)) {
            if (lane < p.K) out[lane] = -__builtin_inf();
            continue;
        }
        box_join_max<EVAL_MAX_K>(run, lane, p.payload + (long long)s * p.N * p.K, p.K, out,
                                 [&](int k) { return ((p.kmask[k] >> s) & 1u) && boxes_meet(p.kbox[k], b); });
    }
}

bool shape_ok(int K, int S, bool payload_optional) {
    return S >= 1 && S <= EVAL_MAX_S && K >= (payload_optional ? 0 : 1) && K <= EVAL_MAX_K;
}

}  // namespace

// Bytes of scratch aq_eval_member_conf_subsets_f64 needs for n points, K sizes and S subsets: 16 (coordinates) + 24 (runs) + 8 (confidence) +
// 4 (mask word) + 8 K S (T) per point, each array rounded up to 16 bytes; 0 for n <= 0, K outside 1 .. 16, S outside 1 .. 32 or a size
// sg::eval_subsets_fit refuses.
extern "C" size_t aq_eval_subsets_scratch_bytes(long long n, int K, int S) {
    if (n <= 0 || !shape_ok(K, S, false) || !sg::eval_subsets_fit(n, K, S)) return 0;
    EvalParams p = {};
    return eval_scratch_layout<true>(p, nullptr, (size_t)n, (size_t)K, (size_t)S);
}

// Bytes of scratch aq_box_match_subsets_f64 needs: none today (0); the query is there so that a caller sizes through it and the size guard
// is asked before anything is allocated: (size_t)-1 for sizes the launcher refuses.
extern "C" size_t aq_box_match_subsets_scratch_bytes(long long Q, long long N, int K, int S) {
    if (!shape_ok(K, S, true) || !sg::eval_subsets_fit(Q, K, S) || !sg::eval_subsets_fit(N, K, S)) return (size_t)-1;
    return 0;
}

extern "C" int aq_eval_member_conf_subsets_f64(const long long* keys_sorted_dev, const int32_t* perm_dev, const double* xy_dev, const int32_t* group_dev,
                                               const double* conf_dev, const uint32_t* mask_dev, long long n, double eps, int K, int S,
                                               void* scratch_dev, size_t scratch_bytes, double* member_conf_dev, void* stream) {
    AQ_REQUIRE(S >= 1 && S <= EVAL_MAX_S, "evaluate subsets: S = %d subsets (1 to %d)", S, EVAL_MAX_S);
    AQ_REQUIRE(K >= 1 && K <= EVAL_MAX_K, "evaluate subsets: K = %d cluster sizes (1 to %d)", K, EVAL_MAX_K);
    AQ_REQUIRE(sg::eval_subsets_fit(n, K, S), "evaluate subsets: %lld points (at most 2^31 - 1 in one call, and S n K below 2^36)", n);
    AQ_REQUIRE(eps > 0.0 && eps * eps < __builtin_inf(), "evaluate subsets: eps = %g (it has to be positive and finite)", eps);        // (NaN fails too)
    if (n == 0) return AQ_OK;
    AQ_REQUIRE(keys_sorted_dev && perm_dev && xy_dev && group_dev && conf_dev && mask_dev && scratch_dev && member_conf_dev, "evaluate subsets: null pointer");
    AQ_REQUIRE(((uintptr_t)keys_sorted_dev & 7) == 0 && ((uintptr_t)perm_dev & 3) == 0 && ((uintptr_t)xy_dev & 15) == 0 &&
               ((uintptr_t)group_dev & 3) == 0 && ((uintptr_t)conf_dev & 7) == 0 && ((uintptr_t)mask_dev & 3) == 0 &&
               ((uintptr_t)scratch_dev & 15) == 0 && ((uintptr_t)member_conf_dev & 7) == 0, "evaluate subsets: unaligned array");
    const size_t need = aq_eval_subsets_scratch_bytes(n, K, S);
    AQ_REQUIRE(scratch_bytes >= need, "evaluate subsets: %zu bytes of scratch, %zu needed (aq_eval_subsets_scratch_bytes)", scratch_bytes, need);
    EvalParams p = {};
    p.keys = keys_sorted_dev; p.perm = perm_dev; p.xy = xy_dev; p.group = group_dev;
    p.n = (int)n; p.eps2 = eps * eps;
    p.conf = conf_dev; p.mask = mask_dev; p.K = K; p.S = S;
    eval_scratch_layout<true>(p, scratch_dev, (size_t)n, (size_t)K, (size_t)S);
    p.M = member_conf_dev;
    return eval_member_launch<true>(p, (hipStream_t)stream);
}

extern "C" int aq_box_match_subsets_f64(const double* qbox_dev, const int32_t* qgroup_dev, const uint32_t* qmask_dev, long long Q,
                                        const double* kbox_dev, const uint32_t* kmask_dev, long long N, const int32_t* group_start_dev, int G,
                                        const double* payload_dev, int K, int S, uint32_t* hitmask_dev, double* out_dev, void* stream) {
    AQ_REQUIRE(S >= 1 && S <= EVAL_MAX_S, "box match subsets: S = %d subsets (1 to %d)", S, EVAL_MAX_S);
    AQ_REQUIRE(K >= 0 && K <= EVAL_MAX_K, "box match subsets: K = %d payload columns (0: no payload, to %d)", K, EVAL_MAX_K);
    AQ_REQUIRE(sg::eval_subsets_fit(Q, K, S) && sg::eval_subsets_fit(N, K, S),
               "box match subsets: %lld queries, %lld keys (at most 2^31 - 1 of each in one call, and S n K below 2^36)", Q, N);
    AQ_REQUIRE(G >= 0, "box match subsets: %d groups", G);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(qbox_dev && qgroup_dev && qmask_dev && group_start_dev && hitmask_dev && (N == 0 || (kbox_dev && kmask_dev)) &&
               (K == 0 || (out_dev && (N == 0 || payload_dev))), "box match subsets: null pointer");
    AQ_REQUIRE(((uintptr_t)qbox_dev & 31) == 0 && ((uintptr_t)kbox_dev & 31) == 0 && ((uintptr_t)qgroup_dev & 3) == 0 && ((uintptr_t)qmask_dev & 3) == 0 &&
               ((uintptr_t)kmask_dev & 3) == 0 && ((uintptr_t)group_start_dev & 3) == 0 && ((uintptr_t)payload_dev & 7) == 0 &&
               ((uintptr_t)hitmask_dev & 3) == 0 && ((uintptr_t)out_dev & 7) == 0, "box match subsets: unaligned array");
    SubsetMatchParams p = {};
    p.qbox = (const double4*)qbox_dev; p.qgroup = qgroup_dev; p.qmask = qmask_dev; p.kbox = (const double4*)kbox_dev; p.kmask = kmask_dev;
    p.group_start = group_start_dev; p.payload = payload_dev; p.Q = (int)Q; p.N = (int)N; p.G = G; p.K = K; p.S = S;
    p.hitmask = hitmask_dev; p.out = out_dev;
    hipLaunchKernelGGL(box_match_subsets_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
