// --model-errors: the two device steps of the cage-area error distributions (reference src/utils_tonnage.py:130-203,
// define_model_error_distributions, with :284-327, get_cage_area_errors_from_labels: every detection keeps the label of its year and type that
// it overlaps most, error = label area - detection area, one normal fit per (image pass, cage type)).
//
// aq_model_error_match_f64.  Q query boxes against N key boxes sorted by (group, x0), as aq_box_match_f64 takes them.  Key k is a candidate of
// query q when the groups agree and the closed boxes intersect (box_match_kernel's predicate); with
//   inter(q, k) = (min(q.x1, k.x1) - max(q.x0, k.x0)) * (min(q.y1, k.y1) - max(q.y0, k.y0))       two subtractions and one product, as written
// the match is the candidate with the largest inter; among equal inter the smallest original row (krow) wins; a NaN inter never wins over a
// number (among NaNs the smallest row).  One wavefront per query: box_join.h's run bound, box_match_kernel's, cuts the group's run at
// key.x0 <= query.x1, the lanes stride over what is left, each keeping its best (inter, row, position), then six exchange steps under the
// same rule -- a total order, since rows are distinct, so every lane ends with the same winner.  Lane 0 writes
//   match    the winner's original row, -1 without a candidate
//   overlap  100 * inter / ((q.x1 - q.x0) * (q.y1 - q.y0)) as computed (inf for a query without area), NaN without a candidate
//   error    karea[winner] - qarea[q], NaN without a candidate
// Every NaN written is the canonical quiet NaN (0x7FF8000000000000), whatever the operation that made it.
//
// aq_model_error_moments_f64.  n, mean and population sd of the errors per moment group, in one written order of the sums.  Query q is a
// member of group g when match[q] >= 0, mgroup[q] == g and error[q] is finite.  One wavefront per group, two passes over [Q]:
//   lane l adds the values of the rows q = l, l + 64, l + 128, ... in increasing q, +0.0 for a non-member (exact);
//   the 64 partials fold as v[i] + v[i + 32], then + 16, ... + 1 (the xor exchange: lane i + s computes the same sum, + is commutative);
//   pass 1: S = sum of error, the count in integers, mean = S / n;   pass 2: D = sum of (error - mean)^2, sd = sqrt(D / n).
// n = 0: mean and sd are NaN.  fp64 in + - x / sqrt only, each rounded as written (this file is built with -ffp-contract=off).
#include "box_join.h"

namespace {

struct ErrMatchParams {
    const double4* qbox;       // [Q] (x0, y0, x1, y1)
    const int* qgroup;         // [Q]
    const double* qarea;       // [Q]
    const double4* kbox;       // [N], sorted by (group, x0)
    const int* krow;           // [N] original row of each sorted key
    const double* karea;       // [N], sorted as kbox
    const int* group_start;    // [G + 1]
    int Q, N, G;
    int* match;                // out [Q]
    double* overlap;           // out [Q]
    double* error;             // out [Q]
};

__device__ inline double canonical(double v) { return v != v ? __builtin_nan("") : v; }

// whether candidate (ci, cr) comes before the best so far (bi, br); a row of -1: none
__device__ inline bool err_better(double ci, int cr, double bi, int br) {
    if (cr < 0) return false;
    if (br < 0) return true;
    const bool cn = ci != ci, bn = bi != bi;
    if (cn != bn) return bn;
    if (!cn && ci != bi) return ci > bi;
    return cr < br;
}

__global__ __launch_bounds__(256) void model_error_match_kernel(const ErrMatchParams p) {
    const int lane = threadIdx.x & 63;
    const long long q = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per query: uniform from here on
    if (q >= p.Q) return;
    const double4 b = p.qbox[q];
    const KeyRun run = box_join_run(p.group_start, p.G, p.N, p.kbox, p.qgroup[q], b.z);
    double bi = 0.0;
    int br = -1, bk = -1;
    for (int k = run.first + lane; k < run.end; k += 64) {
        const double4 a = p.kbox[k];
        if (boxes_meet(a, b)) {
            const double w = (b.z < a.z ? b.z : a.z) - (b.x > a.x ? b.x : a.x);
            const double h = (b.w < a.w ? b.w : a.w) - (b.y > a.y ? b.y : a.y);
            const double ci = w * h;
            const int cr = p.krow[k];
            if (cr >= 0 && err_better(ci, cr, bi, br)) { bi = ci; br = cr; bk = k; }
        }
    }
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) {
        const double oi = __shfl_xor(bi, s, 64);
        const int orow = __shfl_xor(br, s, 64), ok = __shfl_xor(bk, s, 64);
        if (err_better(oi, orow, bi, br)) { bi = oi; br = orow; bk = ok; }
    }
    if (lane == 0) {
        p.match[q] = br;
        if (br >= 0) {
            p.overlap[q] = canonical(100.0 * bi / ((b.z - b.x) * (b.w - b.y)));
            p.error[q] = canonical(p.karea[bk] - p.qarea[q]);
        } else {
            p.overlap[q] = __builtin_nan("");
            p.error[q] = __builtin_nan("");
        }
    }
}

struct ErrMomentParams {
    const double* error;       // [Q]
    const int* match;          // [Q]
    const int* mgroup;         // [Q]
    int Q, G;
    long long* n;              // out [G]
    double* mean;              // out [G]
    double* sd;                // out [G]
};

__device__ inline double fold64(double v) {
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, 64);
    return v;
}

__global__ __launch_bounds__(256) void model_error_moments_kernel(const ErrMomentParams p) {
    const int lane = threadIdx.x & 63;
    const long long g = blockIdx.x * 4LL + (threadIdx.x >> 6);                  // one wavefront per moment group
    if (g >= p.G) return;
    const double inf = __builtin_inf();
    double s = 0.0;
    int cnt = 0;
    for (int q = lane; q < p.Q; q += 64) {
        const double e = p.error[q];
        const bool member = p.match[q] >= 0 && p.mgroup[q] == (int)g && e > -inf && e < inf;
        s = s + (member ? e : 0.0);
        cnt += member ? 1 : 0;
    }
    long long n = cnt;
#pragma unroll
    for (int sft = 32; sft >= 1; sft >>= 1) n += __shfl_xor(n, sft, 64);
    const double S = fold64(s);
    if (n == 0) {
        if (lane == 0) { p.n[g] = 0; p.mean[g] = __builtin_nan(""); p.sd[g] = __builtin_nan(""); }
        return;
    }
    const double mean = S / (double)n;
    double d2 = 0.0;
    for (int q = lane; q < p.Q; q += 64) {
        const double e = p.error[q];
        const bool member = p.match[q] >= 0 && p.mgroup[q] == (int)g && e > -inf && e < inf;
        const double d = e - mean;
        d2 = d2 + (member ? d * d : 0.0);
    }
    const double D = fold64(d2);
    if (lane == 0) {
        p.n[g] = n;
        p.mean[g] = canonical(mean);
        p.sd[g] = canonical(__builtin_sqrt(D / (double)n));
    }
}

}  // namespace

extern "C" int aq_model_error_match_f64(const double* qbox_dev, const int32_t* qgroup_dev, const double* qarea_dev, long long Q,
                                        const double* kbox_dev, const int32_t* krow_dev, const double* karea_dev, long long N,
                                        const int32_t* group_start_dev, int G, int32_t* match_dev, double* overlap_dev, double* error_dev,
                                        void* stream) {
    AQ_REQUIRE(sg::model_error_count_fits(Q) && sg::model_error_count_fits(N),
               "model errors: %lld queries, %lld keys (at most 2^31 - 1 of each in one call)", Q, N);
    AQ_REQUIRE(G >= 0, "model errors: %d groups", G);
    if (Q == 0) return AQ_OK;
    AQ_REQUIRE(qbox_dev && qgroup_dev && qarea_dev && group_start_dev && match_dev && overlap_dev && error_dev &&
               (N == 0 || (kbox_dev && krow_dev && karea_dev)), "model errors: null pointer");
    AQ_REQUIRE(((uintptr_t)qbox_dev & 31) == 0 && ((uintptr_t)kbox_dev & 31) == 0 && ((uintptr_t)qgroup_dev & 3) == 0 &&
               ((uintptr_t)qarea_dev & 7) == 0 && ((uintptr_t)krow_dev & 3) == 0 && ((uintptr_t)karea_dev & 7) == 0 &&
               ((uintptr_t)group_start_dev & 3) == 0 && ((uintptr_t)match_dev & 3) == 0 && ((uintptr_t)overlap_dev & 7) == 0 &&
               ((uintptr_t)error_dev & 7) == 0, "model errors: unaligned array");
    ErrMatchParams p = {};
    p.qbox = (const double4*)qbox_dev; p.qgroup = qgroup_dev; p.qarea = qarea_dev;
    p.kbox = (const double4*)kbox_dev; p.krow = krow_dev; p.karea = karea_dev; p.group_start = group_start_dev;
    p.Q = (int)Q; p.N = (int)N; p.G = G;
    p.match = match_dev; p.overlap = overlap_dev; p.error = error_dev;
    hipLaunchKernelGGL(model_error_match_kernel, dim3((unsigned)((Q + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_model_error_moments_f64(const double* error_dev, const int32_t* match_dev, const int32_t* mgroup_dev, long long Q, long long G,
                                          long long* n_dev, double* mean_dev, double* sd_dev, void* stream) {
    AQ_REQUIRE(sg::model_error_count_fits(Q) && sg::model_error_count_fits(G),
               "model errors: %lld queries, %lld moment groups (at most 2^31 - 1 of each in one call)", Q, G);
    if (G == 0) return AQ_OK;
    AQ_REQUIRE(n_dev && mean_dev && sd_dev && (Q == 0 || (error_dev && match_dev && mgroup_dev)), "model errors: null pointer");
    AQ_REQUIRE(((uintptr_t)error_dev & 7) == 0 && ((uintptr_t)match_dev & 3) == 0 && ((uintptr_t)mgroup_dev & 3) == 0 &&
               ((uintptr_t)n_dev & 7) == 0 && ((uintptr_t)mean_dev & 7) == 0 && ((uintptr_t)sd_dev & 7) == 0, "model errors: unaligned array");
    ErrMomentParams p = {};
    p.error = error_dev; p.match = match_dev; p.mgroup = mgroup_dev;
    p.Q = (int)Q; p.G = (int)G;
    p.n = n_dev; p.mean = mean_dev; p.sd = sd_dev;
    hipLaunchKernelGGL(model_error_moments_kernel, dim3((unsigned)((G + 3) / 4)), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
