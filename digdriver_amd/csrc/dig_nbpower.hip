// dig_nbpower.hip -- the power of the element route's burden test: per pair (r, e) of a [rows, n] plane the CRITICAL COUNT of the
// upper mid-p test at the row's level, and the probability of reaching it under a fold of selection (include/dig_hip.h: the rule).
//
// One lane owns one pair; a workgroup of kPowerBlock lanes owns kPowerBlock neighbouring elements of ONE row, so the row's level
// and scale are wave-uniform loads.  The grid is rows * chunks workgroups, not capped (refused from 2^31 on).  The three planes are
// read once and the outputs written once, by their owner: no atomics, no workspace.
//
// The search for K = min{k in [0, k_max] : M(k) <= level}, M(k) = nb_midp_upper(k, alpha, p) strictly falling in k:
//   gallop   hi = floor(mean) (the mean alpha theta' pi: M is about a half there), then hi + 1, + 2, + 4, ... until M(hi) <= level
//            (or hi = k_max with M still above: K = -1).  lo = the last count found ABOVE the level (-1 at the start: M(-1) = 1).
//            The statistic is evaluated by the project's own nb_midp_upper at ONE call site inside the loop, so the lanes of a wave
//            run their evaluations side by side; K - mean doubles its way in, log2 evaluations.
//   walk     down from hi with M(k - 1) = M(k) + (pmf(k) + pmf(k - 1)) / 2, pmf(k - 1) = pmf(k) k / ((alpha + k - 1)(1 - p)): only
//            additions of positive terms (stepping up would subtract and cancel), one pmf evaluation, at most hi - lo - 1 steps
//            because lo is known to lie above the level; hi - lo <= K - mean, so the search is O(K) steps in all.
//   bisect   where pmf(hi) is below 1e-290 (levels far under the 1e-250 of the tolerance contract) the walk's terms would be
//            subnormal, and a walk may be longer than kPowerWalkMax steps only for a level next to 1 under a mean of that size:
//            what is then left of (lo, hi] is bisected on nb_midp_upper, so a lane's work is bounded whatever its inputs.
// A wave lasts as long as its longest lane (the lanes of a wave are neighbouring elements, whose parameters are unrelated).  At a
// K of 4 (the median of the fixture's ranges) a lane's gallop is 3 - 4 evaluations of at most 8 recurrence steps and its walk 0 - 3
// steps; at the K of 23 - 32 of the flagship workload (DESIGN, Power of the element route) 5 - 6 evaluations and up to 15 steps.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"

namespace dig {

constexpr int kPowerBlock = 256;                         // lanes of a workgroup = elements of a chunk (nb_tables_init needs > kSmallK)
static_assert(kPowerBlock > kSmallK, "nb_tables_init fills 1 / k! with one lane per entry");
constexpr int kPowerWalkMax = 1 << 16;                   // steps of a walk; what is left of (lo, hi] after them is bisected

struct PowerArgs {
    const double *alpha, *theta, *pi;                    // [rows, n]
    const double *scale, *level;                         // [rows]; scale may be NULL
    const double* folds;                                 // [n_folds]
    int64_t rows, n;
    uint32_t chunks;                                     // per row
    int n_folds;
    int32_t k_max;
    int32_t* k_crit;                                     // [rows, n]
    double* power;                                       // [n_folds, rows, n]
};

// p(f) = 1 / ((theta' pi) f + 1), t = theta' pi: every product and the sum rounded once
__device__ __forceinline__ double power_success_prob(double t, double f)
{
#pragma clang fp contract(off)
    const double tf = t * f;
    const double d = tf + 1.0;
    return 1.0 / d;
}

// K for a level inside (0, 1); -1: no count up to k_max reaches it; -2: the statistic is NaN
__device__ __forceinline__ int nb_critical_count(double alpha, double p, double mean, double level, int k_max)
{
    int64_t lo = -1, hi = (int64_t)fmin(fmax(floor(mean), 0.0), (double)k_max), step = 1;
    double Mh;
    for (;;) {
        Mh = nb_midp_upper((double)hi, alpha, p);
        if (!(Mh > level)) break;                        // (a NaN leaves here too)
        if (hi == k_max) return -1;
        lo = hi;
        hi = hi + step < k_max ? hi + step : k_max;
        step += step;
    }
    if (isnan(Mh)) return -2;
    if (hi - lo == 1) return (int)hi;
    double pm = nbinom_pmf((double)hi, alpha, p);
    if (pm >= 1e-290) {
        const double x = 1.0 - p;                        // (p < 1 here: at p = 1 the gallop ends with hi - lo = 1)
        double M = Mh, kd = (double)hi;
        for (int s = 0; hi - lo > 1 && s < kPowerWalkMax; ++s) {
            const double pm1 = pm * (kd * recip_nr((alpha + (kd - 1.0)) * x));
            const double M1 = M + 0.5 * (pm + pm1);
            if (M1 > level) { lo = hi - 1; break; }
            hi -= 1, kd -= 1.0, M = M1, pm = pm1;
        }
    }
    while (hi - lo > 1) {                                // (entered only by a walk that was not taken or not finished)
        const int64_t mid = lo + (hi - lo) / 2;
        if (nb_midp_upper((double)mid, alpha, p) > level) lo = mid; else hi = mid;
    }
    return (int)hi;
}

__global__ __launch_bounds__(kPowerBlock) void nb_power_kernel(PowerArgs a)
{
    nb_tables_init();                                    // (every lane of the block arrives)
    const uint32_t w = blockIdx.x, r = w / a.chunks, c = w - r * a.chunks;
    const int64_t e = (int64_t)c * kPowerBlock + threadIdx.x;
    if (e >= a.n) return;
    const int64_t i = (int64_t)r * a.n + e;
    const double level = a.level[r];
    const double alpha = a.alpha[i];
    const double theta = a.scale ? mul_rn(a.theta[i], a.scale[r]) : a.theta[i];
    const double t = mul_rn(theta, a.pi[i]);
    int K = -2;
    if (level > 0.0 && level < 1.0) K = nb_critical_count(alpha, power_success_prob(t, 1.0), mul_rn(alpha, t), level, a.k_max);
    a.k_crit[i] = K < 0 ? -1 : K;
    const int64_t plane = a.rows * a.n;
#pragma unroll 1
    for (int j = 0; j < a.n_folds; ++j) {
        double g = K == -1 ? 0.0 : dnan();
        if (K >= 0) g = nb_greater((double)K, alpha, power_success_prob(t, a.folds[j]));
        a.power[j * plane + i] = g;
    }
}

// what the entry point and its host twin check before anything is read: nothing of it looks at an array
int nb_power_sizes(const char* fn, int64_t rows, int64_t n, const double* folds, int n_folds, int32_t k_max, const double* power,
                   int64_t* chunks)
{
    DIG_REQUIRE_IN(fn, rows >= 0 && n >= 0, "rows, n >= 0");
    DIG_REQUIRE_IN(fn, n_folds >= 0 && n_folds <= DIG_NB_POWER_MAX_FOLDS, "0 <= n_folds <= 8");
    DIG_REQUIRE_IN(fn, k_max >= 0 && k_max <= (1 << 30), "0 <= k_max <= 2^30");
    DIG_REQUIRE_IN(fn, n_folds == 0 || folds, "non-null folds for n_folds > 0");
    DIG_REQUIRE_IN(fn, (n_folds > 0) == (power != nullptr), "power non-null with n_folds > 0, NULL with n_folds = 0");
    DIG_REQUIRE_IN(fn, n < ((int64_t)1 << 31), "fewer than 2^31 elements per row");
    const int64_t ch = (n + kPowerBlock - 1) / kPowerBlock;
    DIG_REQUIRE_IN(fn, rows < ((int64_t)1 << 31) && rows * ch < ((int64_t)1 << 31),
                   "rows * chunks below 2^31 (a chunk per workgroup): fewer rows per call");
    *chunks = ch;
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_nb_power(const double* alpha, const double* theta, const double* pi, const double* scale, const double* level, int64_t rows,
                 int64_t n, const double* folds, int n_folds, int32_t k_max, int32_t* k_crit, double* power, void* stream)
{
    int64_t chunks = 0;
    if (int rc = nb_power_sizes(__func__, rows, n, folds, n_folds, k_max, power, &chunks)) return rc;
    if (rows * n == 0) return DIG_OK;
    DIG_REQUIRE(alpha && theta && pi && level && k_crit, "non-null alpha, theta, pi, level, k_crit");
    PowerArgs a{};
    a.alpha = alpha, a.theta = theta, a.pi = pi, a.scale = scale, a.level = level, a.folds = folds;
    a.rows = rows, a.n = n, a.chunks = (uint32_t)chunks, a.n_folds = n_folds, a.k_max = k_max, a.k_crit = k_crit, a.power = power;
    hipLaunchKernelGGL(nb_power_kernel, dim3((unsigned)(rows * chunks)), dim3(kPowerBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
