// --performance: the Monte-Carlo behind the upper bound on the cage population (reference src/Results/upper_bound_calculation.R): K samples of
// S Bernoulli draws, counted at up to 16 rates.  include/aq_engine.h states the draw; performance.counts_numpy restates it.
//
//   draw      simulation k, sample j: Philox4x32-10 (philox.h), key = the seed's two halves, counter (k, j >> 1, 16, 0) -> (w0, w1, w2, w3);
//             an even j takes (w1 : w0), an odd j (w3 : w2), each through philox.h's 53-bit uniform; slot 16 lies outside tonnage.hip's 0 .. 6
//   count     count[k][i] = #{j < S : u(k, j) < rates[i]}, the fp64 comparison as written; every rate sees the same uniforms
//
// One wavefront per simulation: the lanes stride over the ceil(S / 2) Philox calls with their counters in registers, the wave adds them up
// with integer shuffles and lane 0 stores the row.  Integers and comparisons only: the order of the additions cannot show, so the bytes are
// those of the restatement.  Built with -ffp-contract=off like its neighbours (the uniform's one product and one sum are rounded as written).
#include "aq_common.h"
#include "philox.h"

namespace {

constexpr int POP_MAX_RATES = 16;
constexpr uint32_t POP_SLOT = 16;

// RN = the rate count rounded up to a multiple of 4: the counters beyond R compare against 0 and stay 0.
template <int RN>
__global__ __launch_bounds__(256) void bernoulli_counts_kernel(uint32_t key0, uint32_t key1, long long k0, long long K, int S, const double* rates,
                                                               int R, int32_t* counts) {
    const int lane = threadIdx.x & 63;
    const int calls = (int)(((long long)S + 1) >> 1);
    double rate[RN];
#pragma unroll
    for (int i = 0; i < RN; ++i) rate[i] = i < R ? rates[i] : 0.0;
    for (long long kr = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + blockIdx.x * 4LL; kr < K; kr += gridDim.x * 4LL) {
        const uint32_t k = (uint32_t)(k0 + kr);
        int cnt[RN];
#pragma unroll
        for (int i = 0; i < RN; ++i) cnt[i] = 0;
        for (int c = lane; c < calls; c += 64) {
            const PhiloxWords w = philox4x32(key0, key1, k, (uint32_t)c, POP_SLOT, 0u);
            const double u0 = philox_words_uniform(w.w0, w.w1), u1 = philox_words_uniform(w.w2, w.w3);
            const bool odd = 2LL * c + 1 < S;                // the draw of j = 2 c + 1 exists
#pragma unroll
            for (int i = 0; i < RN; ++i) cnt[i] += (int)(u0 < rate[i]) + (int)(odd && u1 < rate[i]);
        }
#pragma unroll
        for (int i = 0; i < RN; ++i) {
#pragma unroll
            for (int d = 32; d >= 1; d >>= 1) cnt[i] += __shfl_xor(cnt[i], d, 64);
        }
        if (lane == 0) {
            int32_t* row = counts + kr * R;
#pragma unroll
            for (int i = 0; i < RN; ++i)
                if (i < R) row[i] = cnt[i];
        }
    }
}

}  // namespace

extern "C" int aq_bernoulli_counts_i32(unsigned long long seed, long long k0, long long K, long long S, const double* rates_dev,
                                       const double* rates_host, int R, int32_t* counts_dev, void* stream) {
    AQ_REQUIRE(R >= 1 && R <= POP_MAX_RATES, "population: %d rates (1 to %d)", R, POP_MAX_RATES);
    AQ_REQUIRE(S >= 1 && S < (1LL << 31), "population: samples of %lld draws (1 to 2^31 - 1)", S);
    AQ_REQUIRE(K >= 0 && k0 >= 0 && k0 <= (1LL << 32) && K <= (1LL << 32) - k0,
               "population: %lld simulations from %lld (the counter's word holds 0 .. 2^32 - 1)", K, k0);
    AQ_REQUIRE(rates_host, "population: null pointer");
    for (int i = 0; i < R; ++i)
        AQ_REQUIRE(rates_host[i] >= 0.0 && rates_host[i] <= 1.0, "population: rate %d = %g (a probability)", i, rates_host[i]);    // (NaN fails too)
    if (K == 0) return AQ_OK;
    AQ_REQUIRE(rates_dev && counts_dev, "population: null pointer");
    AQ_REQUIRE(((uintptr_t)rates_dev & 7) == 0 && ((uintptr_t)counts_dev & 3) == 0, "population: unaligned array");
    const long long blocks = (K + 3) / 4;
    const dim3 grid((unsigned)(blocks < (1LL << 20) ? blocks : (1LL << 20)));
    hipStream_t st = (hipStream_t)stream;
    const uint32_t key0 = (uint32_t)seed, key1 = (uint32_t)(seed >> 32);
    if (R <= 4)
        hipLaunchKernelGGL(bernoulli_counts_kernel<4>, grid, dim3(256), 0, st, key0, key1, k0, K, (int)S, rates_dev, R, counts_dev);
    else if (R <= 8)
        hipLaunchKernelGGL(bernoulli_counts_kernel<8>, grid, dim3(256), 0, st, key0, key1, k0, K, (int)S, rates_dev, R, counts_dev);
    else if (R <= 12)
        hipLaunchKernelGGL(bernoulli_counts_kernel<12>, grid, dim3(256), 0, st, key0, key1, k0, K, (int)S, rates_dev, R, counts_dev);
    else
        hipLaunchKernelGGL(bernoulli_counts_kernel<16>, grid, dim3(256), 0, st, key0, key1, k0, K, (int)S, rates_dev, R, counts_dev);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
