// dig_mapreport.hip -- how good a mutation-rate map is: its bins merged into larger windows with the region burden test per window
// (dig_map_windows), and the per-cohort scores of a merged plane (dig_map_scores).  include/dig_hip.h: the rules.
//
// dig_map_windows.  A merged window is a run of bins run_ptr[m] .. run_ptr[m + 1] - 1 of one cohort's row; its two float sums are
// SEQUENTIAL double additions in ascending bin order from +0.0 (a gated-out bin adds +0.0, which changes no bit of a sum that began
// at +0.0), std * std rounded before it is added.  A chain of dependent additions cannot be split over lanes without changing its
// bits, so what is shared out is the MEMORY side:
//   a workgroup of kMapBlock lanes owns `wpb` neighbouring windows of one cohort (wpb <= kMapBlock, chosen on the host from the mean
//   run length N / M so that a group's bins are about kMapGroupBins) and streams their bins -- one contiguous stretch of the
//   cohort's row -- through LDS in tiles of kMapTile bins: every lane loads (coalesced, 8 B a lane), gates, squares and stores; then
//   lane w adds the part of ITS window that lies in the tile, first bin to last, from LDS.
//     s = 1     wpb = 256: a tile is the workgroup's 256 bins, every lane adds one value and runs one test -- a stream plus tests;
//     s = 100   wpb = 40: four tiles, ten windows a tile; a lane-per-window walk of global memory would have strided the wave by 800 B;
//     a run of a whole chromosome   wpb = 1: all 256 lanes load the run's tiles, lane 0 walks them from LDS -- the serial part is
//               the add chain alone (about 12 000 x two dependent additions), never a lane's serial walk of global memory, and the
//               (cohort, chromosome) chains run side by side, one workgroup each.
//   A workgroup takes `gpw` such groups one after the other (the 1 / k! and log tables of dig_math.hpp are filled once per workgroup).
// Every output element is written once, by its owner: no atomics, no workspace.  run_ptr is read on the device; a value outside
// [0, N] or below its left neighbour is clamped there, so a bad run_ptr reads nothing outside the tables (the host twin refuses it).
//
// dig_map_scores.  Floating sums in an order fixed by (M, C) alone:
//   the M windows of a cohort are cut into chunks of kScoreChunk = 1024 (the last one shorter); a workgroup of 256 lanes owns one
//   chunk: lane t adds the terms of windows t, t + 256, t + 512, t + 768 of the chunk in that order from +0.0 (a window with
//   N_BINS = 0, or past M, adds +0.0), the 256 lane sums are folded by halves (lane t += lane t + 128, then + 64, ... + 1), and the
//   chunk sums are added first chunk to last from +0.0.
//   pass 1: EXP_TOTAL = sum of Y_PRED, and the integer scores (any order: they are integers);
//   the means  mx = (double)OBS_TOTAL / (double)N_WINDOWS,  my = EXP_TOTAL / (double)N_WINDOWS  from pass 1's chunk sums, first
//   to last, once per cohort (a kernel of its own: every workgroup of pass 2 summing them for itself cost more than pass 2);
//   pass 2: with dx = (double)Y_TRUE - mx, dy = Y_PRED - my:  Sxx = sum dx * dx, Syy = sum dy * dy, Sxy = sum dx * dy, each product
//   rounded before it is added (no fused multiply-add);
//   a last kernel adds the chunk sums of both passes per cohort.  Workspace: 11 eight-byte slots per (cohort, chunk), then the two
//   means per cohort.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"

namespace dig {

constexpr int kMapBlock = 256;                           // lanes of a workgroup (nb_tables_init needs > kSmallK)
static_assert(kMapBlock > kSmallK, "nb_tables_init fills 1 / k! with one lane per entry");
constexpr int kMapTile = 1024;                           // bins of an LDS tile
constexpr int kMapGroupBins = 4096;                      // the bins a group of windows aims at: four tiles (one tile: 1.1 - 2.1 x the time, DESIGN)
constexpr int kMapMaxGroupsPerBlock = 8;

struct MapWindowArgs {
    const double *mu, *sd;                               // [C, N]
    const int32_t* y;                                    // [C, N]
    const uint8_t* flag;                                 // [C, N] or NULL
    const int64_t* run_ptr;                              // [M + 1]
    int64_t N, M;
    int64_t groups;                                      // per cohort: ceil(M / wpb)
    uint32_t blocks;                                     // per cohort: ceil(groups / gpw)
    int wpb, gpw, drop_flagged, tail;
    int32_t* n_bins;                                     // [C, M]
    int64_t* y_true;
    double *y_pred, *sd_out, *pval;
};

__device__ __forceinline__ int64_t map_clamp(int64_t v, int64_t lo, int64_t hi) { return v < lo ? lo : (v > hi ? hi : v); }

__global__ __launch_bounds__(kMapBlock) void map_windows_kernel(MapWindowArgs a)
{
    __shared__ double s_mu[kMapTile], s_var[kMapTile];
    __shared__ int32_t s_y[kMapTile];
    __shared__ uint8_t s_g[kMapTile];
    nb_tables_init();                                    // (every lane of the block arrives)
    const uint32_t c = blockIdx.x / a.blocks, b = blockIdx.x - c * a.blocks;
    const int tid = threadIdx.x;
    const int64_t row = (int64_t)c * a.N;
#pragma unroll 1
    for (int gi = 0; gi < a.gpw; ++gi) {
        const int64_t grp = (int64_t)b * a.gpw + gi;     // (uniform: every lane of the block leaves together)
        if (grp >= a.groups) break;
        const int64_t m0 = grp * a.wpb;
        const int nwin = (int)(a.M - m0 < a.wpb ? a.M - m0 : a.wpb);
        const int64_t r0 = map_clamp(a.run_ptr[m0], 0, a.N), r1 = map_clamp(a.run_ptr[m0 + nwin], r0, a.N);
        const bool mine = tid < nwin;
        int64_t lo = 0, hi = 0;
        if (mine) {
            lo = map_clamp(a.run_ptr[m0 + tid], r0, r1);
            hi = map_clamp(a.run_ptr[m0 + tid + 1], lo, r1);
        }
        double sum_mu = 0.0, sum_var = 0.0;
        int64_t sum_y = 0;
        int32_t sum_n = 0;
        for (int64_t t0 = r0; t0 < r1; t0 += kMapTile) {
            const int nt = (int)(r1 - t0 < kMapTile ? r1 - t0 : kMapTile);
#pragma unroll 4
            for (int i = tid; i < nt; i += kMapBlock) {
                const int64_t o = row + t0 + i;
                const bool g = !(a.drop_flagged && a.flag[o]);
                const double m = a.mu[o], s = a.sd[o];
                const int32_t yy = a.y[o];
                s_mu[i] = g ? m : 0.0;
                s_var[i] = g ? mul_rn(s, s) : 0.0;
                s_y[i] = g ? yy : 0;
                s_g[i] = g;
            }
            __syncthreads();
            if (mine) {
                const int i0 = (int)((lo > t0 ? lo : t0) - t0), i1 = (int)((hi < t0 + nt ? hi : t0 + nt) - t0);
#pragma unroll 8
                for (int i = i0; i < i1; ++i) {          // (i1 <= i0: the window has nothing in this tile)
                    sum_mu += s_mu[i];
                    sum_var += s_var[i];
                    sum_y += s_y[i];
                    sum_n += s_g[i];
                }
            }
            __syncthreads();
        }
        if (mine) {
            const int64_t o = (int64_t)c * a.M + m0 + tid;
            const double sd = sqrt(sum_var);
            double pv = dnan();
            if (sum_n > 0) {
                const GammaParams gp = normal_params_to_gamma(sum_mu, sd);
                const double p = nb_success_prob(gp.theta, 1.0);
                pv = a.tail ? nb_midp_twosided((double)sum_y, gp.alpha, p) : nb_midp_upper((double)sum_y, gp.alpha, p);
            }
            a.n_bins[o] = sum_n;
            a.y_true[o] = sum_y;
            a.y_pred[o] = sum_mu;
            a.sd_out[o] = sd;
            a.pval[o] = pv;
        }
    }
}

// ---- scores ---------------------------------------------------------------------------------------------------------------------
constexpr int kScoreBlock = 256;
constexpr int kScoreChunk = 1024;                        // windows of a chunk: four per lane
constexpr int kScoreInts = 7;                            // N_WINDOWS, N_TESTED, OBS_TOTAL, N_BELOW[4]
constexpr int kScoreSlots = kScoreInts + 1 + 3;          // + EXP_TOTAL (pass 1) + Sxx, Syy, Sxy (pass 2): 8-byte slots per (cohort, chunk)

__device__ __forceinline__ double score_fold(double* red, double v)          // lane sums -> the chunk sum, by halves (on lane 0)
{
    const int t = threadIdx.x;
    __syncthreads();                                     // (the last fold has been read)
    red[t] = v;
    __syncthreads();
    for (int w = kScoreBlock / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

__device__ __forceinline__ int64_t score_fold_int(int64_t* red, int64_t v)
{
    const int t = threadIdx.x;
    __syncthreads();
    red[t] = v;
    __syncthreads();
    for (int w = kScoreBlock / 2; w > 0; w >>= 1) {
        if (t < w) red[t] += red[t + w];
        __syncthreads();
    }
    return red[0];
}

__global__ __launch_bounds__(kScoreBlock) void map_scores_pass1(const int32_t* __restrict__ n_bins, const int64_t* __restrict__ y_true,
                                                                const double* __restrict__ y_pred, const double* __restrict__ pval,
                                                                int64_t M, uint32_t chunks, int64_t* __restrict__ part)
{
    __shared__ int64_t red[kScoreBlock];
    const uint32_t c = blockIdx.x / chunks, j = blockIdx.x - c * chunks;
    const int64_t base = (int64_t)c * M, w0 = (int64_t)j * kScoreChunk;
    int64_t cnt[kScoreInts] = {0, 0, 0, 0, 0, 0, 0};
    double e = 0.0;
#pragma unroll
    for (int q = 0; q < kScoreChunk / kScoreBlock; ++q) {
        const int64_t w = w0 + q * kScoreBlock + threadIdx.x;
        if (w < M && n_bins[base + w] > 0) {
            const double p = pval[base + w];
            cnt[0] += 1;
            cnt[1] += !isnan(p);
            cnt[2] += y_true[base + w];
            cnt[3] += p < 0.05;
            cnt[4] += p < 0.01;
            cnt[5] += p < 0.001;
            cnt[6] += p < 0.0001;
            e += y_pred[base + w];
        }
    }
    int64_t* out = part + ((int64_t)c * chunks + j) * kScoreSlots;
#pragma unroll
    for (int i = 0; i < kScoreInts; ++i) {
        const int64_t v = score_fold_int(red, cnt[i]);
        if (threadIdx.x == 0) out[i] = v;
    }
    const double es = score_fold((double*)red, e);
    if (threadIdx.x == 0) ((double*)out)[kScoreInts] = es;
}

// per cohort: the two means from pass 1's chunk sums, first chunk to last
__global__ __launch_bounds__(64) void map_scores_means(const int64_t* __restrict__ part, uint32_t chunks, double* __restrict__ mean)
{
    if (threadIdx.x != 0) return;
    const uint32_t c = blockIdx.x;
    const int64_t* p = part + (int64_t)c * chunks * kScoreSlots;
    int64_t n = 0, obs = 0;
    double e = 0.0;
    for (uint32_t k = 0; k < chunks; ++k, p += kScoreSlots) n += p[0], obs += p[2], e += ((const double*)p)[kScoreInts];
    mean[2 * c] = (double)obs / (double)n;
    mean[2 * c + 1] = e / (double)n;
}

__global__ __launch_bounds__(kScoreBlock) void map_scores_pass2(const int32_t* __restrict__ n_bins, const int64_t* __restrict__ y_true,
                                                                const double* __restrict__ y_pred, int64_t M, uint32_t chunks,
                                                                const double* __restrict__ mean, int64_t* __restrict__ part)
{
#pragma clang fp contract(off)
    __shared__ double red[kScoreBlock];
    const uint32_t c = blockIdx.x / chunks, j = blockIdx.x - c * chunks;
    const double mx = mean[2 * c], my = mean[2 * c + 1];
    const int64_t base = (int64_t)c * M, w0 = (int64_t)j * kScoreChunk;
    double sxx = 0.0, syy = 0.0, sxy = 0.0;
#pragma unroll
    for (int q = 0; q < kScoreChunk / kScoreBlock; ++q) {
        const int64_t w = w0 + q * kScoreBlock + threadIdx.x;
        if (w < M && n_bins[base + w] > 0) {
            const double dx = (double)y_true[base + w] - mx, dy = y_pred[base + w] - my;
            const double xx = dx * dx, yy = dy * dy, xy = dx * dy;
            sxx += xx, syy += yy, sxy += xy;
        }
    }
    double* out = (double*)(part + ((int64_t)c * chunks + j) * kScoreSlots) + kScoreInts + 1;
    const double a = score_fold(red, sxx), b = score_fold(red, syy), d = score_fold(red, sxy);
    if (threadIdx.x == 0) out[0] = a, out[1] = b, out[2] = d;
}

// per cohort: the chunk sums first to last (lane i < 7: an integer score; lanes 7 .. 10: EXP_TOTAL, Sxx, Syy, Sxy)
__global__ __launch_bounds__(64) void map_scores_finish(const int64_t* __restrict__ part, uint32_t chunks, int64_t* __restrict__ counts,
                                                        double* __restrict__ sums)
{
    const uint32_t c = blockIdx.x;
    const int i = threadIdx.x;
    if (i >= kScoreSlots) return;
    const int64_t* p = part + (int64_t)c * chunks * kScoreSlots + i;
    if (i < kScoreInts) {
        int64_t s = 0;
        for (uint32_t k = 0; k < chunks; ++k) s += p[(int64_t)k * kScoreSlots];
        counts[(int64_t)c * kScoreInts + i] = s;
    } else {
        double s = 0.0;
        for (uint32_t k = 0; k < chunks; ++k) s += ((const double*)p)[(int64_t)k * kScoreSlots];
        sums[(int64_t)c * 4 + (i - kScoreInts)] = s;
    }
}

// what dig_map_windows and its host twin check before anything is read: nothing of it looks at an array
int map_windows_sizes(const char* fn, int64_t C, int64_t N, int64_t M, int drop_flagged, int tail, const void* flag_cm, MapWindowPlan* plan)
{
    DIG_REQUIRE_IN(fn, C >= 0 && N >= 0 && M >= 0, "C, N, M >= 0");
    DIG_REQUIRE_IN(fn, tail == 0 || tail == 1, "tail = 0 (upper) or 1 (two-sided)");
    DIG_REQUIRE_IN(fn, drop_flagged == 0 || drop_flagged == 1, "drop_flagged = 0 or 1");
    DIG_REQUIRE_IN(fn, !drop_flagged || flag_cm || C * N == 0, "non-null flag_cm with drop_flagged");
    DIG_REQUIRE_IN(fn, C < ((int64_t)1 << 31) && N < ((int64_t)1 << 40) && M < ((int64_t)1 << 40), "C < 2^31, N and M < 2^40");
    int64_t wpb = kMapBlock;                             // windows per group: about kMapGroupBins bins at the mean run length
    if (M > 0 && N / M > 0) wpb = kMapGroupBins / (N / M);
    wpb = wpb < 1 ? 1 : (wpb > kMapBlock ? kMapBlock : wpb);
    const int64_t groups = (M + wpb - 1) / wpb;
    DIG_REQUIRE_IN(fn, C * groups < ((int64_t)1 << 31), "C * window groups below 2^31 (a workgroup takes at most eight): fewer cohorts per call");
    plan->wpb = (int)wpb, plan->groups = groups;
    return DIG_OK;
}

// the chunks (one per workgroup) of a cohort
int map_scores_sizes(const char* fn, int64_t C, int64_t M, int64_t* chunks)
{
    DIG_REQUIRE_IN(fn, C >= 0 && M >= 0, "C, M >= 0");
    const int64_t ch = (M + kScoreChunk - 1) / kScoreChunk;
    DIG_REQUIRE_IN(fn, C < ((int64_t)1 << 31) && ch < ((int64_t)1 << 31) && C * ch < ((int64_t)1 << 31),
                   "C * chunks below 2^31 (a chunk of 1024 windows per workgroup): fewer cohorts per call");
    *chunks = ch;
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_map_windows(const double* mu_cm, const double* std_cm, const int32_t* y_cm, const uint8_t* flag_cm, int64_t C, int64_t N,
                    const int64_t* run_ptr, int64_t M, int drop_flagged, int tail, int32_t* n_bins, int64_t* y_true, double* y_pred,
                    double* std, double* pval, void* stream)
{
    MapWindowPlan plan{};
    if (int rc = map_windows_sizes(__func__, C, N, M, drop_flagged, tail, flag_cm, &plan)) return rc;
    if (C * M == 0) return DIG_OK;
    DIG_REQUIRE(run_ptr && n_bins && y_true && y_pred && std && pval, "non-null run_ptr, n_bins, y_true, y_pred, std, pval");
    DIG_REQUIRE(N == 0 || (mu_cm && std_cm && y_cm), "non-null mu_cm, std_cm, y_cm");
    // groups per workgroup: enough workgroups to fill the card several times over, the tables filled once for up to eight groups
    const int64_t want = (C * plan.groups) / ((int64_t)cu_count() * 16);
    const int gpw = (int)(want < 1 ? 1 : (want > kMapMaxGroupsPerBlock ? kMapMaxGroupsPerBlock : want));
    const int64_t blocks = (plan.groups + gpw - 1) / gpw;
    MapWindowArgs a{};
    a.mu = mu_cm, a.sd = std_cm, a.y = y_cm, a.flag = flag_cm, a.run_ptr = run_ptr, a.N = N, a.M = M;
    a.groups = plan.groups, a.blocks = (uint32_t)blocks, a.wpb = plan.wpb, a.gpw = gpw, a.drop_flagged = drop_flagged, a.tail = tail;
    a.n_bins = n_bins, a.y_true = y_true, a.y_pred = y_pred, a.sd_out = std, a.pval = pval;
    hipLaunchKernelGGL(map_windows_kernel, dim3((unsigned)(C * blocks)), dim3(kMapBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int64_t dig_map_scores_workspace(int64_t C, int64_t M)
{
    if (C <= 0 || M <= 0) return 0;
    return C * (((M + kScoreChunk - 1) / kScoreChunk) * kScoreSlots + 2) * (int64_t)sizeof(int64_t);
}

int dig_map_scores(const int32_t* n_bins, const int64_t* y_true, const double* y_pred, const double* pval, int64_t C, int64_t M,
                   int64_t* counts, double* sums, void* workspace, int64_t workspace_bytes, void* stream)
{
    int64_t chunks = 0;
    if (int rc = map_scores_sizes(__func__, C, M, &chunks)) return rc;
    if (C == 0) return DIG_OK;
    DIG_REQUIRE(counts && sums, "non-null counts, sums");
    hipStream_t s = (hipStream_t)stream;
    if (M == 0) {                                        // no window: every score is 0
        DIG_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)C * kScoreInts * sizeof(int64_t), s));
        DIG_HIP_TRY(hipMemsetAsync(sums, 0, (size_t)C * 4 * sizeof(double), s));
        return DIG_OK;
    }
    DIG_REQUIRE(n_bins && y_true && y_pred && pval && workspace, "non-null n_bins, y_true, y_pred, pval, workspace");
    DIG_REQUIRE(workspace_bytes >= dig_map_scores_workspace(C, M), "workspace smaller than dig_map_scores_workspace(C, M)");
    DIG_REQUIRE(((uintptr_t)workspace & 7u) == 0, "workspace 8-byte aligned");
    int64_t* part = (int64_t*)workspace;
    const unsigned grid = (unsigned)(C * chunks);
    hipLaunchKernelGGL(map_scores_pass1, dim3(grid), dim3(kScoreBlock), 0, s, n_bins, y_true, y_pred, pval, M, (uint32_t)chunks, part);
    DIG_HIP_TRY(hipGetLastError());
    double* mean = (double*)(part + C * chunks * kScoreSlots);
    hipLaunchKernelGGL(map_scores_means, dim3((unsigned)C), dim3(64), 0, s, (const int64_t*)part, (uint32_t)chunks, mean);
    DIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(map_scores_pass2, dim3(grid), dim3(kScoreBlock), 0, s, n_bins, y_true, y_pred, M, (uint32_t)chunks, (const double*)mean, part);
    DIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(map_scores_finish, dim3((unsigned)C), dim3(64), 0, s, (const int64_t*)part, (uint32_t)chunks, counts, sums);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
