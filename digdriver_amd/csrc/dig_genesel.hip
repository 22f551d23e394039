// dig_genesel.hip -- the gene route's dN/dS correction and selection tests as ONE launch.
//
// Reference (DIGDriver/driver_model/transfer_tools.py), per gene and cohort, six mutation classes
// SYN, MIS, NONS, SPL, TRUNC = NONS + SPL, NONSYN = MIS + TRUNC:
//   gene_expected_muts_dnds  :363-392   EXP_c = ALPHA * THETA * Pi_c;  T_SYN = _mle_t(OBS_SYN, 1, ALPHA, THETA * Pi_SYN);
//                                       MRFOLD = max(1e-10, T_SYN / EXP_SYN);  EXP_c_ML = EXP_c * MRFOLD        (:1264-1277)
//   gene_pvalue_burden_dnds  :617-655   PVAL_c_BURDEN_DNDS = nb_pvalue_greater_midp(OBS_c, ALPHA, 1 / (EXP_c_ML / ALPHA + 1))
//   gene_pvalue_sel_nb       :657-676   likelihood-ratio tests of _llr_test_nb (:1172-1213): SYN, MIS, TRUNC (df 1), MIS + TRUNC (df 2)
//   gene_pvalue_sel_gamma    :749-765   the same under the Gamma-Poisson model, _llr_test_gamma_poiss (:1215-1252): SYN, MIS, NONS, MIS + NONS
//   selection_coefficient    :1280-1292 SEL_c = (OBS_c + 1e-16) / (EXP_c + 1e-16) and its df 1 likelihood-ratio p-value
// The reference walks the frame row by row (iterrows) and makes ~50 scipy calls per gene; its own driver has the calls
// commented out (:833-853).  Here one thread takes one (gene, cohort) pair through all 34 outputs.
//
// The likelihood ratios.  Two likelihoods of a test differ in the terms of the replaced classes only, and in those only in
// what holds theta: with p = 1 / (1 + theta) as the reference rounds it,
//     ll(theta0) - ll(theta1) = alpha (log p0 - log p1) + k (log1p(-p0) - log1p(-p1))        (the k term is 0 at k = 0)
// -- no lgamma, nothing of the size of k log k to cancel.  (log p = -log1p(theta) and log1p(-p) = log theta - log1p theta; the
// logs are taken of the rounded p because the reference's own value hangs on that rounding when theta ~ 1e-12.)  What the
// reference's full sums do beyond that is kept by hand: a class that is NOT replaced but has probability 0 with a count above 0
// puts -inf on both sides (NaN); so does a Gamma density term that is not finite in the Gamma-Poisson tests.
// Python's max(a, b) returns a unless b > a: a NaN T_SYN / EXP_SYN gives MRFOLD = 1e-10, not NaN (pymax below, never fmax).
#include "dig_common.hpp"
#include "dig_math.hpp"

#pragma clang fp contract(off)   // every product and sum below is one numpy operation of the reference, rounded as it rounds

namespace dig {

struct GeneSelArgs {
    const double *alpha, *theta;   // [G, C]; theta already scaled by the cohort factor (the frame's THETA)
    const double* pi;              // [G, n_pi, C]
    const int32_t* obs;            // [G, 5, C]: SYN, MIS, NONS, SPL, INDEL (unused)
    double* out;                   // [34, G, C]
    int64_t G, C;
    int n_pi;
};

constexpr int kGeneSelBlock = 256;

__device__ __forceinline__ double pymax(double a, double b) { return (b > a) ? b : a; }

__device__ __forceinline__ bool finite_nonneg(double v) { return v >= 0.0 && v < __longlong_as_double(0x7ff0000000000000LL); }

// nbinom.logpmf(k, alpha, 1 / (1 + th0)) - nbinom.logpmf(k, alpha, 1 / (1 + th1)); NaN where scipy's argument check fails
__device__ __noinline__ double nb_llr(double k, double alpha, double th0, double th1)
{
    if (!(alpha > 0.0 && finite_nonneg(alpha) && finite_nonneg(th0) && finite_nonneg(th1))) return dnan();
    const double p0 = 1.0 / (1.0 + th0), p1 = 1.0 / (1.0 + th1);
    double d = alpha * (log(p0) - log(p1));
    if (k != 0.0) d = d + k * (log1p(-p0) - log1p(-p1));
    return d;
}

// poisson.logpmf(k, lam) - poisson.logpmf(k, k)
__device__ inline double pois_llr(double k, double lam)
{
    if (!finite_nonneg(lam)) return dnan();
    const double kt = (k == 0.0) ? 0.0 : k * (log(lam) - log(k));
    return kt - lam + k;
}

// The four tests of one model from the three class terms d[] (ll0 - ll1 of the class on its own) and zero[] (the class
// has probability 0 under the null and a count above 0: its term of ll0 is -inf): tests 0..2 replace class 0..2, test 3
// replaces classes 1 and 2.
__device__ __forceinline__ void llr_tests(const double d[3], const bool zero[3], bool common_ok, double pv[4])
{
    const bool any_nan = isnan(d[0]) || isnan(d[1]) || isnan(d[2]) || !common_ok;
    pv[0] = (any_nan || zero[1] || zero[2]) ? dnan() : chi2_sf1(-2.0 * d[0]);
    pv[1] = (any_nan || zero[0] || zero[2]) ? dnan() : chi2_sf1(-2.0 * d[1]);
    pv[2] = (any_nan || zero[0] || zero[1]) ? dnan() : chi2_sf1(-2.0 * d[2]);
    pv[3] = (any_nan || zero[0]) ? dnan() : chi2_sf2(-2.0 * (d[1] + d[2]));
}

__global__ __launch_bounds__(kGeneSelBlock) void gene_selection_kernel(GeneSelArgs a)
{
    nb_tables_init();
    const double inf = __longlong_as_double(0x7ff0000000000000LL);
    const int64_t n = a.G * a.C;
    const int64_t stride = (int64_t)gridDim.x * kGeneSelBlock;
    for (int64_t i = (int64_t)blockIdx.x * kGeneSelBlock + threadIdx.x; i < n; i += stride) {
        const int64_t g = i / a.C, c = i - g * a.C;
        const double alpha = a.alpha[i], theta = a.theta[i];
        double pi[6], k[6];
        for (int q = 0; q < a.n_pi; ++q) pi[q] = a.pi[(g * a.n_pi + q) * a.C + c];
        if (a.n_pi == 4) {                         // as dig_gene_stats forms them
            pi[4] = pi[2] + pi[3];
            pi[5] = pi[1] + pi[4];
        }
        int ki[6];
        for (int q = 0; q < 4; ++q) ki[q] = a.obs[(g * 5 + q) * a.C + c];
        ki[4] = ki[2] + ki[3];
        ki[5] = ki[1] + ki[4];
        for (int q = 0; q < 6; ++q) k[q] = (double)ki[q];

        // gene_expected_muts_dnds :367-390, _mle_t :1264-1272, _mrfold_factor :1274-1277
        const double rate = alpha * theta;
        const double exp_syn = rate * pi[0];
        const double tps = theta * pi[0];
        double t_syn = ((k[0] + alpha) - 1.0) / (1.0 + 1.0 / tps);
        if (alpha <= 1.0) t_syn = pymax(alpha * tps, t_syn);
        const double mrfold = pymax(1e-10, t_syn / exp_syn);
        a.out[0 * n + i] = t_syn;
        a.out[1 * n + i] = mrfold;

#pragma unroll 1
        for (int q = 0; q < 6; ++q) {
            const double ex = rate * pi[q], ex_ml = ex * mrfold;
            const double tp = theta * pi[q];
            // gene_pvalue_burden_dnds :623-646
            const double p = 1.0 / (ex_ml / alpha + 1.0);
            double r1 = 0.0, dummy = 0.0;
            const unsigned done = nb_midp_upper_fast2<1>(k[q], 0.0, 1u, alpha, p, r1, dummy);
            if (!(done & 1u)) r1 = nb_midp_upper_unresolved(k[q], alpha, p);
            // selection_coefficient :1285-1292
            const double sel = (k[q] + 1e-16) / (ex + 1e-16);
            a.out[(2 + q) * n + i] = ex_ml;
            a.out[(8 + q) * n + i] = r1;
            a.out[(22 + q) * n + i] = sel;
            a.out[(28 + q) * n + i] = chi2_sf1(-2.0 * nb_llr(k[q], alpha, tp, tp * sel));
        }
        // the class terms of _llr_test_nb :1174-1204 (SYN, MIS, TRUNC) and _llr_test_gamma_poiss :1217-1244 (SYN, MIS, NONS)
        double d_nb[3], d_pg[3];
        bool z_nb[3], z_pg[3];
#pragma unroll 1
        for (int s = 0; s < 3; ++s) {
            const int q = s == 2 ? 4 : s;
            const double th0 = (theta * pi[q]) * mrfold;
            d_nb[s] = nb_llr(k[q], alpha, th0, k[q] / alpha);
            z_nb[s] = k[q] > 0.0 && th0 == 0.0;
            const double lam = (rate * pi[s]) * mrfold;     // ALPHA * THETA * Pi_c * MRFOLD: the operations of EXP_c_ML
            d_pg[s] = pois_llr(k[s], lam);
            z_pg[s] = k[s] > 0.0 && lam == 0.0;
        }
        double pv[4];
        llr_tests(d_nb, z_nb, true, pv);
        for (int j = 0; j < 4; ++j) a.out[(14 + j) * n + i] = pv[j];
        // gamma.logpdf(T_SYN, ALPHA, scale = THETA * Pi_SYN * MRFOLD), in all five likelihoods: it cancels where it is finite
        const double scale = tps * mrfold;
        const bool gamma_ok = alpha > 0.0 && alpha < inf && scale > 0.0 && scale < inf &&
                              ((t_syn > 0.0 && t_syn < inf) || (t_syn == 0.0 && alpha == 1.0));
        llr_tests(d_pg, z_pg, gamma_ok, pv);
        for (int j = 0; j < 4; ++j) a.out[(18 + j) * n + i] = pv[j];
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_gene_selection(const double* alpha, const double* theta, const double* pi, int n_pi, const int32_t* obs, double* out,
                       int64_t G, int64_t C, void* stream)
{
    DIG_REQUIRE(G >= 0 && C >= 0, "G, C >= 0");
    DIG_REQUIRE(n_pi == 4 || n_pi == 6, "n_pi: 4 (SYN, MIS, NONS, SPL: TRUNC and NONSYN are formed here) or 6");
    if (G == 0 || C == 0) return DIG_OK;
    DIG_REQUIRE(alpha && theta && pi && obs && out, "non-null pointers");
    const GeneSelArgs a{alpha, theta, pi, obs, out, G, C, n_pi};
    hipLaunchKernelGGL(gene_selection_kernel, dim3(grid_for(G * C, kGeneSelBlock, 8)), dim3(kGeneSelBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
