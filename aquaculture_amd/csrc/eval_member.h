// The member-confidence kernels of evaluate.hip (--evaluate) and eval_subsets.hip (--evaluate-kfold), written once: gather, topk and member
// over the neighbour search of facility_runs.h, as the header comments of those two files state them.  SUBSETS = false is evaluate.hip's
// form: one lane per sorted point.  SUBSETS = true is eval_subsets.hip's: one lane per (sorted point, subset) with blockIdx.y the subset, a
// point or a neighbour outside the subset skipped by one bit test of its mask word, and the subset's [n][K] slab of T and M.  Every mask load,
// bit test and subset offset is behind `if constexpr`: the SUBSETS = false kernels carry none of them.  The scratch layout, the K dispatch and
// the limits are here too, once for both launchers.
#pragma once
#include "facility_runs.h"

namespace {

constexpr int EVAL_MAX_K = 16;
constexpr int EVAL_MAX_S = 32;

struct EvalParams : FacRuns {
    const double* conf;        // [n], original order
    const unsigned* mask;      // [n], original order (SUBSETS only)
    int K, S;                  // S = 1 without subsets
    double* sconf;             // scratch [n]: confidences by sorted position; -inf for an entry of perm that is no index
    unsigned* smask;           // scratch [n] (SUBSETS only): mask words by sorted position, bits >= S cleared; 0 for an entry of perm that is no index
    double* T;                 // scratch [S][n][K], by sorted position; rows of points outside the subset are never written nor read
    double* M;                 // out [S][n][K], original order
};

__device__ __forceinline__ unsigned low_bits(int S) { return S >= 32 ? 0xFFFFFFFFu : ((1u << S) - 1u); }

// whether the point at sorted position k is in subset s; every point without subsets
template <bool SUBSETS>
__device__ __forceinline__ bool eval_in_subset(const EvalParams& p, long long k, unsigned s) {
    if constexpr (SUBSETS) return (p.smask[k] >> s) & 1u;
    else return true;
}

// row i of subset s in an array [S][n][K] (T or M); of [n][K] without subsets
template <bool SUBSETS>
__device__ __forceinline__ double* eval_row(const EvalParams& p, double* a, long long i, unsigned s) {
    if constexpr (SUBSETS) i += (long long)s * p.n;
    return a + i * p.K;
}

template <bool SUBSETS>
__global__ __launch_bounds__(256) void eval_gather_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i >= p.n) return;
    const int o = fac_gather(p, i);
    p.sconf[i] = o >= 0 ? p.conf[o] : -__builtin_inf();
    if constexpr (SUBSETS) p.smask[i] = o >= 0 ? (p.mask[o] & low_bits(p.S)) : 0u;
}

template <int KC, bool SUBSETS>
__global__ __launch_bounds__(256) void eval_topk_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    const unsigned s = SUBSETS ? blockIdx.y : 0u;                               // < S <= 32
    if (i >= p.n) return;
    if (!eval_in_subset<SUBSETS>(p, i, s)) return;
    double top[KC];                                                             // descending; static indices only, so it stays in registers
#pragma unroll
    for (int m = 0; m < KC; ++m) top[m] = -__builtin_inf();
    fac_neighbours(p, i, [&](int k) {
        if (!eval_in_subset<SUBSETS>(p, k, s)) return;
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
    double* out = eval_row<SUBSETS>(p, p.T, i, s);
#pragma unroll
    for (int m = 0; m < KC; ++m)
        if (m < p.K) out[m] = top[m] < c ? top[m] : c;
}

template <int KC, bool SUBSETS>
__global__ __launch_bounds__(256) void eval_member_kernel(const EvalParams p) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    const unsigned s = SUBSETS ? blockIdx.y : 0u;
    if (i >= p.n) return;
    const int o = fac_orig(p, (int)i);
    if (o < 0) return;
    if (!eval_in_subset<SUBSETS>(p, i, s)) {
        double* out = eval_row<SUBSETS>(p, p.M, o, s);
#pragma unroll
        for (int m = 0; m < KC; ++m)
            if (m < p.K) out[m] = -__builtin_inf();
        return;
    }
    double mx[KC];
#pragma unroll
    for (int m = 0; m < KC; ++m) mx[m] = -__builtin_inf();
    const double* Ts = eval_row<SUBSETS>(p, p.T, 0, s);
    fac_neighbours(p, i, [&](int k) {
        if (!eval_in_subset<SUBSETS>(p, k, s)) return;
        const double* t = Ts + (long long)k * p.K;
#pragma unroll
        for (int m = 0; m < KC; ++m)
            if (m < p.K) { const double v = t[m]; mx[m] = v > mx[m] ? v : mx[m]; }
    });
    const double c = p.sconf[i];
    double* out = eval_row<SUBSETS>(p, p.M, o, s);
#pragma unroll
    for (int m = 0; m < KC; ++m)
        if (m < p.K) out[m] = mx[m] < c ? mx[m] : c;
}

size_t align16(size_t v) { return (v + 15) & ~(size_t)15; }

// The scratch of one call, from `base` on: coordinates, runs, confidences, (SUBSETS) mask words and T of n points, each array rounded up to
// 16 bytes.  Sets p's scratch pointers and returns the bytes: the *_scratch_bytes queries (base = null) and the launchers walk one layout.
template <bool SUBSETS>
size_t eval_scratch_layout(EvalParams& p, void* base, size_t n, size_t K, size_t S) {
    uintptr_t at = (uintptr_t)base;
    auto take = [&](size_t bytes) { void* a = (void*)at; at += align16(bytes); return a; };
    p.sxy = (double2*)take(n * 16);
    p.runs = (int2*)take(n * 24);
    p.sconf = (double*)take(n * 8);
    if (SUBSETS) p.smask = (unsigned*)take(n * 4);
    p.T = (double*)take(n * 8 * K * S);
    return at - (uintptr_t)base;
}

template <int KC, bool SUBSETS>
void eval_launch_kc(const EvalParams& p, dim3 grid, hipStream_t st) {
    hipLaunchKernelGGL((eval_topk_kernel<KC, SUBSETS>), grid, dim3(256), 0, st, p);
    hipLaunchKernelGGL((eval_member_kernel<KC, SUBSETS>), grid, dim3(256), 0, st, p);
}

// gather, then topk and member at the smallest list size KC >= K, on `st`; p.n >= 1
template <bool SUBSETS>
int eval_member_launch(const EvalParams& p, hipStream_t st) {
    const unsigned blocks = (unsigned)((p.n + 255LL) / 256);
    hipLaunchKernelGGL(eval_gather_kernel<SUBSETS>, dim3(blocks), dim3(256), 0, st, p);
    AQ_CHECK_HIP(hipGetLastError());
    const dim3 grid(blocks, SUBSETS ? (unsigned)p.S : 1u);
    if (p.K == 1) eval_launch_kc<1, SUBSETS>(p, grid, st);
    else if (p.K <= 4) eval_launch_kc<4, SUBSETS>(p, grid, st);
    else if (p.K <= 8) eval_launch_kc<8, SUBSETS>(p, grid, st);
    else eval_launch_kc<EVAL_MAX_K, SUBSETS>(p, grid, st);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

}  // namespace
