// --tonnage: the bootstrap of the facilities' live-weight production (reference src/utils_tonnage.py:28-127, compute_facility_tonnage_estimates,
// and :330-458, sample_model_errors), one wavefront lane per (simulation k, facility f).  include/aq_engine.h states every formula and order.
//
// Everything is fp64 and this file is built with -ffp-contract=off: the only floating-point operations are + - x / sqrt (correctly rounded
// here and in numpy), comparisons and selections, so tonnage.simulate_numpy gives the same bytes.  No libm call, no fma, no float atomics.
//
// Operation order, written once (the host restatement follows it literally):
//   philox    Philox4x32-10, counter (c0, c1, c2, c3) = (k, entity, slot, attempt), key (seed low word, seed high word); per round
//             (hi0, lo0) = M0 c0, (hi1, lo1) = M1 c2, c <- (hi1 ^ c1 ^ k0, lo1, hi0 ^ c3 ^ k1, lo0); the key grows by (W0, W1) between rounds
//   uniform   x = (w1 : w0) >> 11 (53 bits); u = ((double)x + 0.5) * 2^-53; u = u < 1 ? u : 1 - 2^-53
//   alog(x)   x = m 2^e, 0.5 <= m < 1; if m < 0.7071067811865476: m = m 2, e = e - 1; s = (m - 1) / (m + 1); s2 = s s;
//             acc = 1/27; for j = 25, 23 .. 1: acc = acc s2 + 1/j; result = e LN2 + (2 s) acc
//   ndtri(p)  Cephes: p outside [0, 1] or NaN -> NaN, 0 -> -inf, 1 -> +inf; y = p, or 1 - p when p > 1 - e^-2 (then no sign change);
//             y > e^-2: y = y - 0.5, y2 = y y, (y + y ((y2 P0(y2)) / Q0(y2))) s2pi;
//             else x = sqrt(-2 alog(y)), x0 = x - alog(x) / x, z = 1 / x, x1 = (z P(z)) / Q(z) with (P1, Q1) for x < 8, else (P2, Q2);
//             x0 - x1, negated unless y was mirrored.  Polynomials by Horner from the first coefficient.
#include "aq_common.h"
#include "philox.h"    // philox_uniform: the generator and the 53-bit uniform of the head comment, shared with population.hip

namespace {

constexpr int TON_MAX_ATTEMPTS = 64;
enum { SLOT_ERROR = 0, SLOT_AREA = 1, SLOT_BERNOULLI = 2, SLOT_DEPTH_A = 3, SLOT_DEPTH_B = 4, SLOT_STOCKING = 5, SLOT_HARVEST = 6 };

// x positive and finite (every caller's is)
__device__ inline double alog(double x) {
    int sub = 0;
    if (x < 0x1p-1022) { x = x * 0x1p54; sub = 54; }                           // a subnormal: exact
    const uint64_t b = (uint64_t)__double_as_longlong(x);
    int e = (int)((b >> 52) & 0x7ff) - 1022 - sub;
    double m = __longlong_as_double((long long)((b & 0x800fffffffffffffULL) | 0x3fe0000000000000ULL));
    const bool lo = m < 0.7071067811865476;
    m = lo ? m * 2.0 : m;
    e = lo ? e - 1 : e;
    const double s = (m - 1.0) / (m + 1.0);
    const double s2 = s * s;
    double acc = 1.0 / 27.0;
#pragma unroll
    for (int j = 25; j >= 1; j -= 2) acc = acc * s2 + 1.0 / (double)j;
    return (double)e * 0.6931471805599453 + (2.0 * s) * acc;
}

template <int N>
__device__ inline double horner(double x, const double (&c)[N]) {
    double r = c[0];
#pragma unroll
    for (int i = 1; i < N; ++i) r = r * x + c[i];
    return r;
}

// The coefficient tables of the Cephes Math Library's ndtri (Stephen L. Moshier; 3-clause BSD).
__device__ inline double ndtri(double p) {
    constexpr double P0[5] = {-5.99633501014107895267E1, 9.80010754185999661536E1, -5.66762857469070293439E1, 1.39312609387279679503E1,
                              -1.23916583867381258016E0};
    constexpr double Q0[9] = {1.00000000000000000000E0, 1.95448858338141759834E0, 4.67627912898881538453E0, 8.63602421390890590575E1,
                              -2.25462687854119370527E2, 2.00260212380060660359E2, -8.20372256168333339912E1, 1.59056225126211695515E1,
                              -1.18331621121330003142E0};
    constexpr double P1[9] = {4.05544892305962419923E0, 3.15251094599893866154E1, 5.71628192246421288162E1, 4.40805073893200834700E1,
                              1.46849561928858024014E1, 2.18663306850790267539E0, -1.40256079171354495875E-1, -3.50424626827848203418E-2,
                              -8.57456785154685413611E-4};
    constexpr double Q1[9] = {1.00000000000000000000E0, 1.57799883256466749731E1, 4.53907635128879210584E1, 4.13172038254672030440E1,
                              1.50425385692907503408E1, 2.50464946208309415979E0, -1.42182922854787788574E-1, -3.80806407691578277194E-2,
                              -9.33259480895457427372E-4};
    constexpr double P2[9] = {3.23774891776946035970E0, 6.91522889068984211695E0, 3.93881025292474443415E0, 1.33303460815807542389E0,
                              2.01485389549179081538E-1, 1.23716634817820021358E-2, 3.01581553508235416007E-4, 2.65806974686737550832E-6,
                              6.23974539184983293730E-9};
    constexpr double Q2[9] = {1.00000000000000000000E0, 6.02427039364742014255E0, 3.67983563856160859403E0, 1.37702099489081330271E0,
                              2.16236993594496635890E-1, 1.34204006088543189037E-2, 3.28014464682127739104E-4, 2.89247864745380683936E-6,
                              6.79019408009981274425E-9};
    constexpr double EXPM2 = 0.13533528323661269189, S2PI = 2.50662827463100050242E0;
    if (!(p >= 0.0 && p <= 1.0)) return __builtin_nan("");
    if (p == 0.0) return -__builtin_inf();
    if (p == 1.0) return __builtin_inf();
    const bool mirrored = p > 1.0 - EXPM2;
    double y = mirrored ? 1.0 - p : p;
    if (y > EXPM2) {
        y = y - 0.5;
        const double y2 = y * y;
        return (y + y * ((y2 * horner(y2, P0)) / horner(y2, Q0))) * S2PI;
    }
    const double x = __builtin_sqrt(-2.0 * alog(y));
    const double x0 = x - alog(x) / x;
    const double z = 1.0 / x;
    const double x1 = x < 8.0 ? (z * horner(z, P1)) / horner(z, Q1) : (z * horner(z, P2)) / horner(z, Q2);
    const double r = x0 - x1;
    return mirrored ? r : -r;
}

struct TonParams {
    uint32_t key0, key1;
    long long k0, K, F;
    const int32_t* entry_start;    // [F + 1]
    const double* area;            // [E]
    const double2* err;            // [E] (mean, sd)
    const uint8_t* flags;          // [E]
    int E, P;
    const double* depth;           // [F]
    const int32_t* pass;           // [F]
    const double* pp;              // [P][6]: s_mean, s_sd, pS0, pS1, h_mean, h_sd
    double mix, min_depth, pA0, pA1, pB0, pB1;
    double* ton;                   // [K][F]
};

// One wavefront per (facility, 64 consecutive simulations): the entry loop has the same length in every lane and the entries' loads are
// wave-uniform; a lane leaves the common path only to draw a cage's error again.
__global__ __launch_bounds__(256) void tonnage_simulate_kernel(const TonParams p) {
    const long long kblocks = (p.K + 63) >> 6, items = kblocks * p.F;
    const int lane = threadIdx.x & 63;
    for (long long w = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)) + blockIdx.x * 4LL; w < items; w += gridDim.x * 4LL) {
        const long long f = w / kblocks, kr = (w - f * kblocks) * 64 + lane;
        if (kr >= p.K) continue;
        const uint32_t k = (uint32_t)(p.k0 + kr);
        const int first = min(max(p.entry_start[f], 0), p.E), end = min(max(p.entry_start[f + 1], first), p.E);
        double lo = 0.0, hi = 0.0;
        for (int e = first; e < end; ++e) {
            const double a0 = p.area[e];
            const double2 er = p.err[e];
            const int fl = p.flags[e];
            double a = a0;
            int attempt = 0;
            for (; attempt < TON_MAX_ATTEMPTS; ++attempt) {
                a = a0 + (er.x + er.y * ndtri(philox_uniform(p.key0, p.key1, k, (uint32_t)e, SLOT_ERROR, (uint32_t)attempt)));
                if (!(a <= 0.0)) break;
            }
            a = attempt == TON_MAX_ATTEMPTS ? a0 : a;
            const int kind = fl & 3;
            const double mn = kind == 1 ? (4.0 * a) / (2.0 + 3.141592653589793) : kind == 2 ? (2.0 * a) / 3.0 : a;
            const double mx = kind == 1 ? ((2.0 * 3.141592653589793) * a) / (2.0 + 3.141592653589793) : kind == 2 ? (4.0 * a) / 3.0 : a;
            lo = (fl & 4) ? lo + mn : lo;
            hi = (fl & 8) ? hi + mx : hi;
        }
        const uint32_t fe = (uint32_t)f;
        const double sim_area = lo + (hi - lo) * philox_uniform(p.key0, p.key1, k, fe, SLOT_AREA, 0);
        const double d = p.depth[f], m = p.min_depth;
        double depth = m;
        if (d > m) {
            if (philox_uniform(p.key0, p.key1, k, fe, SLOT_BERNOULLI, 0) < p.mix)
                depth = d + ((d - m) / 1.96) * ndtri(p.pA0 + philox_uniform(p.key0, p.key1, k, fe, SLOT_DEPTH_A, 0) * (p.pA1 - p.pA0));
            else
                depth = d + (d / 1.96) * ndtri(p.pB0 + philox_uniform(p.key0, p.key1, k, fe, SLOT_DEPTH_B, 0) * (p.pB1 - p.pB0));
        }
        const double* q = p.pp + 6LL * min(max(p.pass[f], 0), p.P - 1);
        const double stocking = q[0] + q[1] * ndtri(q[2] + philox_uniform(p.key0, p.key1, k, fe, SLOT_STOCKING, 0) * (q[3] - q[2]));
        const double harvest = q[4] + q[5] * ndtri(philox_uniform(p.key0, p.key1, k, fe, SLOT_HARVEST, 0));
        p.ton[kr * p.F + f] = ((sim_area * depth) * stocking) * (harvest * (1.0 / 1000.0));
    }
}

// T[k][p]: one thread per (k, p), the facilities in ascending f.
__global__ __launch_bounds__(256) void tonnage_pass_kernel(const double* ton, long long K, long long F, const int32_t* pass, int P, double* T) {
    const long long total = K * P;
    for (long long i = blockIdx.x * 256LL + threadIdx.x; i < total; i += gridDim.x * 256LL) {
        const long long k = i / P;
        const int pi = (int)(i - k * P);
        const double* row = ton + k * F;
        double acc = 0.0;
        for (long long f = 0; f < F; ++f) acc = pass[f] == pi ? acc + row[f] : acc;
        T[i] = acc;
    }
}

// moments[f] += (sum, sum of squares) over the chunk's simulations in ascending k: one thread per facility, coalesced over f.
__global__ __launch_bounds__(64) void tonnage_moment_kernel(const double* ton, long long K, long long F, double2* moments) {
    const long long f = blockIdx.x * 64LL + threadIdx.x;
    if (f >= F) return;
    double2 m = moments[f];
#pragma unroll 8
    for (long long k = 0; k < K; ++k) {
        const double t = ton[k * F + f];
        m.x = m.x + t;
        m.y = m.y + t * t;
    }
    moments[f] = m;
}

__global__ __launch_bounds__(256) void tonnage_ndtri_kernel(const double* p, long long n, double* out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < n) out[i] = ndtri(p[i]);
}

__global__ __launch_bounds__(256) void tonnage_uniform_kernel(uint32_t key0, uint32_t key1, const uint32_t* c, long long n, double* out) {
    const long long i = blockIdx.x * 256LL + threadIdx.x;
    if (i < n) out[i] = philox_uniform(key0, key1, c[4 * i], c[4 * i + 1], c[4 * i + 2], c[4 * i + 3]);
}

bool is_finite(double v) { return v - v == 0.0; }

}  // namespace

extern "C" int aq_tonnage_simulate_f64(unsigned long long seed, long long k0, long long K_chunk, const int32_t* entry_start_dev,
                                       const int32_t* entry_start_host, long long F, const double* entry_area_dev, const double* entry_err_dev,
                                       const uint8_t* entry_flags_dev, long long E, const double* depth_dev, const int32_t* pass_dev,
                                       const double* pass_params_dev, const double* pass_params_host, int P, double mix, double min_depth,
                                       const double* depth_probs, double* ton_dev, void* stream) {
    AQ_REQUIRE(K_chunk >= 0 && K_chunk < (1LL << 31) && F >= 0 && F < (1LL << 31) && E >= 0 && E < (1LL << 31) && P >= 0,
               "tonnage: %lld simulations, %lld facilities, %lld entries, %d passes (at most 2^31 - 1 of each in one call)", K_chunk, F, E, P);
    AQ_REQUIRE(K_chunk == 0 || F == 0 || K_chunk < (1LL << 62) / F, "tonnage: %lld x %lld values (fewer than 2^62)", K_chunk, F);
    AQ_REQUIRE(k0 >= 0 && k0 <= (1LL << 32) - K_chunk, "tonnage: %lld simulations from %lld (the counter's word holds 0 .. 2^32 - 1)", K_chunk, k0);
    AQ_REQUIRE(mix >= 0.0 && mix <= 1.0, "tonnage: mix = %g (a probability)", mix);                                  // (NaN fails too)
    AQ_REQUIRE(is_finite(min_depth), "tonnage: min_depth = %g", min_depth);
    if (F == 0 || K_chunk == 0) return AQ_OK;
    AQ_REQUIRE(entry_start_dev && entry_start_host && depth_dev && pass_dev && pass_params_dev && pass_params_host && depth_probs && ton_dev &&
               (E == 0 || (entry_area_dev && entry_err_dev && entry_flags_dev)), "tonnage: null pointer");
    AQ_REQUIRE(P >= 1, "tonnage: %lld facilities and no pass", F);
    AQ_REQUIRE(((uintptr_t)entry_start_dev & 3) == 0 && ((uintptr_t)entry_area_dev & 7) == 0 && ((uintptr_t)entry_err_dev & 15) == 0 &&
               ((uintptr_t)depth_dev & 7) == 0 && ((uintptr_t)pass_dev & 3) == 0 && ((uintptr_t)pass_params_dev & 7) == 0 &&
               ((uintptr_t)ton_dev & 7) == 0, "tonnage: unaligned array");
    for (int i = 0; i < 4; ++i) AQ_REQUIRE(is_finite(depth_probs[i]), "tonnage: depth probability %d = %g", i, depth_probs[i]);
    for (int i = 0; i < P; ++i) {
        const double* q = pass_params_host + 6LL * i;
        for (int j = 0; j < 6; ++j) AQ_REQUIRE(is_finite(q[j]), "tonnage: pass %d, parameter %d = %g", i, j, q[j]);
        AQ_REQUIRE(q[1] > 0.0, "tonnage: pass %d, s_sd = %g (it has to be positive)", i, q[1]);
    }
    AQ_REQUIRE(entry_start_host[0] >= 0 && entry_start_host[F] <= E, "tonnage: entry offsets %d .. %d leave the %lld entries", entry_start_host[0],
               entry_start_host[F], E);
    for (long long f = 0; f < F; ++f)
        AQ_REQUIRE(entry_start_host[f] <= entry_start_host[f + 1], "tonnage: entry offsets decrease at facility %lld", f);
    TonParams p = {};
    p.key0 = (uint32_t)seed; p.key1 = (uint32_t)(seed >> 32);
    p.k0 = k0; p.K = K_chunk; p.F = F;
    p.entry_start = entry_start_dev; p.area = entry_area_dev; p.err = (const double2*)entry_err_dev; p.flags = entry_flags_dev;
    p.E = (int)E; p.P = P;
    p.depth = depth_dev; p.pass = pass_dev; p.pp = pass_params_dev;
    p.mix = mix; p.min_depth = min_depth;
    p.pA0 = depth_probs[0]; p.pA1 = depth_probs[1]; p.pB0 = depth_probs[2]; p.pB1 = depth_probs[3];
    p.ton = ton_dev;
    const long long items = ((K_chunk + 63) >> 6) * F, blocks = (items + 3) / 4;
    hipLaunchKernelGGL(tonnage_simulate_kernel, dim3((unsigned)(blocks < (1LL << 20) ? blocks : (1LL << 20))), dim3(256), 0, (hipStream_t)stream, p);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_tonnage_reduce_f64(const double* ton_dev, long long K_chunk, long long F, const int32_t* pass_dev, int P, double* T_dev,
                                     double* moments_dev, void* stream) {
    AQ_REQUIRE(K_chunk >= 0 && K_chunk < (1LL << 31) && F >= 0 && F < (1LL << 31) && P >= 0,
               "tonnage: %lld simulations, %lld facilities, %d passes (at most 2^31 - 1 of each in one call)", K_chunk, F, P);
    AQ_REQUIRE(K_chunk == 0 || F == 0 || K_chunk < (1LL << 62) / F, "tonnage: %lld x %lld values (fewer than 2^62)", K_chunk, F);
    if (K_chunk == 0) return AQ_OK;
    AQ_REQUIRE((P == 0 || T_dev) && (F == 0 || (ton_dev && pass_dev && moments_dev)), "tonnage: null pointer");
    AQ_REQUIRE(((uintptr_t)ton_dev & 7) == 0 && ((uintptr_t)pass_dev & 3) == 0 && ((uintptr_t)T_dev & 7) == 0 && ((uintptr_t)moments_dev & 15) == 0,
               "tonnage: unaligned array");
    hipStream_t st = (hipStream_t)stream;
    if (P > 0) {
        const long long blocks = (K_chunk * P + 255) / 256;
        hipLaunchKernelGGL(tonnage_pass_kernel, dim3((unsigned)(blocks < (1LL << 20) ? blocks : (1LL << 20))), dim3(256), 0, st, ton_dev, K_chunk, F,
                           pass_dev, P, T_dev);
        AQ_CHECK_HIP(hipGetLastError());
    }
    if (F > 0) {
        hipLaunchKernelGGL(tonnage_moment_kernel, dim3((unsigned)((F + 63) / 64)), dim3(64), 0, st, ton_dev, K_chunk, F, (double2*)moments_dev);
        AQ_CHECK_HIP(hipGetLastError());
    }
    return AQ_OK;
}

extern "C" int aq_tonnage_ndtri_f64(const double* p_dev, long long n, double* out_dev, void* stream) {
    AQ_REQUIRE(n >= 0 && n < (1LL << 31), "tonnage: %lld probabilities (at most 2^31 - 1 in one call)", n);
    if (n == 0) return AQ_OK;
    AQ_REQUIRE(p_dev && out_dev, "tonnage: null pointer");
    AQ_REQUIRE(((uintptr_t)p_dev & 7) == 0 && ((uintptr_t)out_dev & 7) == 0, "tonnage: unaligned array");
    hipLaunchKernelGGL(tonnage_ndtri_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, p_dev, n, out_dev);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}

extern "C" int aq_tonnage_uniform_f64(unsigned long long seed, const uint32_t* counters_dev, long long n, double* out_dev, void* stream) {
    AQ_REQUIRE(n >= 0 && n < (1LL << 31), "tonnage: %lld counters (at most 2^31 - 1 in one call)", n);
    if (n == 0) return AQ_OK;
    AQ_REQUIRE(counters_dev && out_dev, "tonnage: null pointer");
    AQ_REQUIRE(((uintptr_t)counters_dev & 3) == 0 && ((uintptr_t)out_dev & 7) == 0, "tonnage: unaligned array");
    hipLaunchKernelGGL(tonnage_uniform_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, (uint32_t)seed,
                       (uint32_t)(seed >> 32), counters_dev, n, out_dev);
    AQ_CHECK_HIP(hipGetLastError());
    return AQ_OK;
}
