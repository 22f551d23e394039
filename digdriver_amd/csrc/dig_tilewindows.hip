// dig_tilewindows.hip -- sliding windows in the per-base route: the NB test of every run of `width` consecutive tiles of a region,
// from the base planes pt, k [C, R, T] that dig_base_tile_probs* and dig_tile_mut_counts (or dig_tile_sample_counts) leave.
//
// The tiles of the per-base route start at a region's first position, so a cluster of mutations that straddles a tile border is
// split over two tiles.  A window of m tiles has pt_w = sum pt and k_w = sum k over its tiles and the region's (mu, sigma); the test is
// that of dig_tiled_nb_test (dig_nb.hip), through the same device functions: equal inputs give equal bits.  With nv = min(n_valid[r], T):
//   n_windows[r]    = 0 when nv <= 0, else max(nv - m + 1, 1): full windows only, or ONE window over all tiles of a region that has
//                     fewer than m
//   window t        covers the tiles t .. min(t + m, nv) - 1
//   pt_w[c, r, t]   = ((pt[t] + pt[t + 1]) + pt[t + 2]) + ...: the window's terms added left to right in float64, the first term taken
//                     as it is.  The order is part of the contract (a prefix-sum difference would not give these bits).
//   k_w[c, r, t]    = the integer sum
//   pval_w, exp_w   = nb_exact(k_w, alpha, 1 / (pt_w theta + 1)), pt_w mu
//   t >= n_windows  pt_w NaN (the NaN of the base planes), k_w 0, and pval_w, exp_w what the test makes of those: NaN
//
// tile_window_kernel: a row (c, r) is T consecutive elements and the rows lie one behind the other, so a workgroup takes a run of
// consecutive elements of the flat planes:
//   T <= 1024  min(1024 / T, 64) whole rows (a window never leaves its row: no halo);
//   T >  1024  1024 outputs of one row and the width - 1 tiles behind them (the halo), cut at the row's end.
// The run is staged in LDS (8 + 4 bytes per tile; every load of a pass is issued before its first LDS write), the rows' Gamma
// parameters and window counts are formed once per row by one thread each, and lane i then walks s[i], s[i + 1], ...: at every step
// consecutive lanes read consecutive LDS addresses (no bank conflict for 8-byte and 4-byte elements).  `width` LDS reads of either
// plane per output; 12 bytes read and 28 written per (tile, cohort) in memory.  One workgroup per run, the grid is not capped: there is
// no grid-stride pass.  Scalar loads and stores only: every pointer needs its element's alignment and no more.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"

namespace dig {

constexpr int kWinBlock = 256;
constexpr int kWinItems = 4;
constexpr int kWinChunk = kWinBlock * kWinItems;       // outputs of a workgroup
constexpr int kWinRowsMax = 64;                        // rows of a workgroup (T <= kWinChunk)
// LDS: (kWinChunk + width - 1) staged tiles of 12 bytes, 36 852 bytes at the largest width, beside 5 KB of tables
static_assert((kWinChunk + DIG_TILE_WINDOW_MAX_WIDTH - 1) * 12 + 8192 <= 65536, "the staged run must fit 64 KB of LDS");

struct TileWindowArgs {
    const double* pt;                                  // [C, R, T]
    const int32_t* k;                                  // [C, R, T]
    const double *mu, *sigma;                          // [C, R]
    const int32_t* n_valid;                            // [R]
    int64_t rows, R, T;                                // rows = C R
    int width;
    int rows_per_group;                                // T <= kWinChunk: whole rows of a workgroup; else 0
    int64_t chunks_per_row;                            // T > kWinChunk
    int stage_max;                                     // the most tiles a workgroup stages
    double* pt_w;                                      // [C, R, T] each, or NULL
    int32_t* k_w;
    double *exp_w, *pval_w;
    int32_t* n_windows;                                // [R] or NULL
};

__global__ __launch_bounds__(kWinBlock) void tile_window_kernel(TileWindowArgs a)
{
    extern __shared__ __attribute__((aligned(8))) unsigned char s_staged[];
    __shared__ double s_alpha[kWinRowsMax], s_theta[kWinRowsMax], s_mu[kWinRowsMax];
    __shared__ int s_nv[kWinRowsMax], s_nw[kWinRowsMax];
    double* s_pt = reinterpret_cast<double*>(s_staged);
    int32_t* s_k = reinterpret_cast<int32_t*>(s_pt + a.stage_max);
    nb_tables_init();
    const int tid = threadIdx.x;
    const int T = (int)a.T;
    // the workgroup's run: n_out outputs from tile t0 of row row0 on, n_stage >= n_out tiles staged, n_rows rows touched
    int64_t row0;
    int t0 = 0, n_rows = 1, n_out, n_stage;
    if (a.rows_per_group > 0) {
        row0 = (int64_t)blockIdx.x * a.rows_per_group;
        n_rows = (int)(a.rows - row0 < a.rows_per_group ? a.rows - row0 : a.rows_per_group);
        n_out = n_stage = n_rows * T;
    } else {
        row0 = (int64_t)blockIdx.x / a.chunks_per_row;
        t0 = (int)((int64_t)blockIdx.x - row0 * a.chunks_per_row) * kWinChunk;
        n_out = T - t0 < kWinChunk ? T - t0 : kWinChunk;
        const int64_t want = (int64_t)n_out + a.width - 1;
        n_stage = (int)(want < T - t0 ? want : T - t0);
    }
    const int64_t e0 = row0 * a.T + t0;
    if (tid < n_rows) {
        const int64_t row = row0 + tid, r = row % a.R;
        int nv = a.n_valid[r];
        nv = nv < 0 ? 0 : (nv > T ? T : nv);
        const int nw = nv == 0 ? 0 : (nv - a.width + 1 > 1 ? nv - a.width + 1 : 1);
        s_nv[tid] = nv;
        s_nw[tid] = nw;
        const double m = a.mu[row];
        const GammaParams g = normal_params_to_gamma(m, a.sigma[row]);
        s_alpha[tid] = g.alpha;
        s_theta[tid] = g.theta;
        s_mu[tid] = m;
        if (a.n_windows && row < a.R && t0 == 0) a.n_windows[r] = nw;      // (cohort 0's rows write the region table)
    }
    for (int i0 = 0; i0 < n_stage; i0 += kWinChunk) {
        double p[kWinItems];
        int kk[kWinItems];
#pragma unroll
        for (int u = 0; u < kWinItems; ++u) {
            const int i = i0 + u * kWinBlock + tid;
            p[u] = i < n_stage ? __builtin_nontemporal_load(&a.pt[e0 + i]) : 0.0;
            kk[u] = i < n_stage ? __builtin_nontemporal_load(&a.k[e0 + i]) : 0;
        }
#pragma unroll
        for (int u = 0; u < kWinItems; ++u) {
            const int i = i0 + u * kWinBlock + tid;
            if (i < n_stage) s_pt[i] = p[u], s_k[i] = kk[u];
        }
    }
    __syncthreads();
#pragma unroll 1
    for (int u = 0; u < kWinItems; ++u) {
        const int i = u * kWinBlock + tid;
        if (i >= n_out) break;
        int rs = 0, t = t0 + i;
        if (a.rows_per_group > 0) {
            rs = (int)((unsigned)i / (unsigned)T);
            t = i - rs * T;
        }
        double ptw = dnan();
        int kw = 0;
        if (t < s_nw[rs]) {
            const int left = s_nv[rs] - t, len = left < a.width ? left : a.width;      // >= 1, and i + len <= n_stage
            ptw = s_pt[i];
            kw = s_k[i];
            for (int j = 1; j < len; ++j) {
                ptw += s_pt[i + j];
                kw += s_k[i + j];
            }
        }
        const int64_t e = e0 + i;
        // (written once: non-temporal, as dig_tiled_nb_test writes its planes)
        if (a.pt_w) __builtin_nontemporal_store(ptw, &a.pt_w[e]);
        if (a.k_w) __builtin_nontemporal_store(kw, &a.k_w[e]);
        if (a.pval_w) {
            const double p = nb_success_prob(ptw, s_theta[rs]);                          // 1 / (pt * theta + 1), nb_model.py:151
            __builtin_nontemporal_store(nb_exact((double)kw, s_alpha[rs], p), &a.pval_w[e]);      // :152
        }
        if (a.exp_w) __builtin_nontemporal_store(mul_rn(ptw, s_mu[rs]), &a.exp_w[e]);   // :157
    }
}

// what the entry point and its host twin require of the sizes: nothing is read before it
int tile_window_sizes(const char* fn, int64_t C, int64_t R, int64_t T, int32_t width)
{
    DIG_REQUIRE_IN(fn, width >= 1 && width <= DIG_TILE_WINDOW_MAX_WIDTH, "1 <= width <= DIG_TILE_WINDOW_MAX_WIDTH (2048)");
    return tile_select_sizes(fn, C, R, T);
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_tile_window_test(const double* pt, const int32_t* k, const double* mu, const double* sigma, const int32_t* n_valid, int64_t C,
                         int64_t R, int64_t T, int32_t width, double* pt_w, int32_t* k_w, double* exp_w, double* pval_w,
                         int32_t* n_windows, void* stream)
{
    if (int rc = tile_window_sizes(__func__, C, R, T, width)) return rc;
    const int64_t rows = C * R;
    if (rows == 0 || T == 0) return DIG_OK;
    if (!pt_w && !k_w && !exp_w && !pval_w && !n_windows) return DIG_OK;
    DIG_REQUIRE(pt && k && mu && sigma && n_valid, "non-null pt, k, mu, sigma, n_valid");
    TileWindowArgs a{};
    a.pt = pt, a.k = k, a.mu = mu, a.sigma = sigma, a.n_valid = n_valid, a.rows = rows, a.R = R, a.T = T, a.width = width;
    a.pt_w = pt_w, a.k_w = k_w, a.exp_w = exp_w, a.pval_w = pval_w, a.n_windows = n_windows;
    int64_t groups;
    if (T <= kWinChunk) {
        a.rows_per_group = (int)(kWinChunk / T < kWinRowsMax ? kWinChunk / T : kWinRowsMax);
        a.stage_max = a.rows_per_group * (int)T;
        groups = (rows + a.rows_per_group - 1) / a.rows_per_group;
    } else {
        a.chunks_per_row = (T + kWinChunk - 1) / kWinChunk;
        const int64_t want = (int64_t)kWinChunk + width - 1;
        a.stage_max = (int)(want < T ? want : T);
        groups = rows * a.chunks_per_row;
    }
    DIG_REQUIRE(groups < ((int64_t)1 << 31), "fewer than 2^31 workgroups (C R ceil(T / 1024)): fewer cohorts or regions per call");
    hipLaunchKernelGGL(tile_window_kernel, dim3((unsigned)groups), dim3(kWinBlock), (size_t)a.stage_max * 12, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
