// dig_tilesparsewindows.hip -- sliding windows over the MUTATED tiles only (DESIGN.md "Sparse sliding windows"): what stands behind
// nb_model.nb_model_window_hits_sparse and tileDriver --sparse --sparse-windows.
//
// dig_tile_window_test (dig_tilewindows.hip) tests every window of m consecutive tiles from the dense planes [C, R, T].  A window that
// holds no mutation row has the closed-form p-value (1 + theta pt_w)^(-alpha), which the host bounds from the region denominators
// (zero_tile_floor at binsize m); only the windows that hold a row need a test, and their number follows the rows.  With the sorted
// keys (cohort R + region) T + tile of dig_sparse_tile_keys (a run of equal keys: a mutated tile), nv = min(n_valid[r], T) and the
// windows of dig_tile_window_test (n_windows[r] = 0 when nv <= 0, else max(nv - m + 1, 1); window w covers the tiles
// w .. min(w + m, nv) - 1), a MUTATED WINDOW of row (c, r) is a window w < n_windows[r] that covers a mutated tile of the row:
//   k_w    the keys of the row with tile in [w, min(w + m, nv))
//   pt_w   (the sum of S[c][context] over the window's positions in ascending order, valid contexts only, started at 0.0) / denom[c, r]:
//          ONE division, the arithmetic of sparse_tile_test_kernel on the window's positions.  At width 1 this is dig_sparse_tile_test
//          bit for bit, and an aligned full window at (binsize, m) has the pt bits of the sparse tile at binsize m.  The dense window
//          route adds the tiles' quotients instead: against it pt_w agrees to rounding (1e-12 relative), not in bits.
//   exp_w, pval_w   pt_w mu, nb_exact(k_w, alpha, 1 / (pt_w theta + 1)): the device functions of dig_tiled_nb_test.
// Every mutated window is named once, through its FIRST mutated tile: with t_prev the mutated tile in front of t in the row (-1: none),
// tile t is the first mutated tile of exactly the windows [lo, hi), lo = max(t_prev + 1, t - m + 1, 0), hi = min(t + 1, n_windows[r])
// (the interval argument of dig_tilewindowsamples.hip with "mutated tile" in the place of "tile of a sample").
//   tile_window_census_kernel   one workgroup per region, one pass per 64 cohorts over its tiles (the walk and the cohort masks of
//                               tile_census_kernel).  Per chunk of 256 tiles the four ballot words of cohort bit b go to LDS; lane b
//                               folds them, with count-trailing-zeros steps, into its running run of tiles without a positive
//                               position and its count of windows that lie inside such a run: n_positive_w[c, r] = n_windows[r] -
//                               sum over the maximal runs of Z such tiles of max(Z - m + 1, 0) (nv >= m; below m: one window, counted
//                               when any tile is positive).  LDS does not depend on T; integers only, no atomics.  With the census'
//                               n_positive, a (region, pass) whose cohorts all have n_positive 0 or nv is answered without the walk.
//   sparse_window_count_kernel  one lane per sorted key: a run's head writes max(hi - lo, 0), every other lane 0.
//   -- the caller turns the counts into exclusive offsets (i64 [n + 1]: the total may exceed 2^31) --
//   sparse_window_test_kernel   one lane per candidate window j of a chunk [w_begin, w_begin + w_count) of the flat list: the owner head
//                               is the last i with offsets[i] <= j (binary search), w = lo(i) + j - offsets[i], k_w = (the first index
//                               at or behind the head whose key is >= row T + min(w + m, nv)) - i (one more binary search: the keys
//                               ascend and t is the window's first mutated tile), then the walk and the test of
//                               sparse_tile_test_kernel.  Neighbouring lanes walk overlapping positions (the plain form).
// The walkers read the 4-bit genome through its view (TileGenome, sparse_region, WindowWalk: dig_tiles.hpp), every word index clamped
// into the array; a key or an offset that names nothing is passed over before anything is dereferenced.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"
#include "dig_tiles.hpp"

namespace dig {

// the tiles and the windows of a region: nv = min(n_valid, T) (<= 0: none)
__device__ __forceinline__ int window_count(int64_t nv, int width) { return nv <= 0 ? 0 : (int)(nv - width + 1 > 1 ? nv - width + 1 : 1); }

// ---- the windows with a positive tile ----
struct WindowCensusArgs {
    TileGenome g;
    int64_t C;
    int binsize;
    int64_t n_tiles;
    int width;
    const uint64_t* mask;                            // [passes][K]
    const int32_t* n_positive;                       // [C, R] or NULL
    int32_t* n_windows;                              // [R]
    int32_t* n_positive_w;                           // [C, R]
};

// The next `n` tiles of a cohort (bit i of x: tile i has a positive position; the bits at and above n are 0) behind a run of `run`
// tiles without one: the runs that end here add their windows to `zero_w`.
__device__ __forceinline__ void fold_tiles(uint64_t x, int n, int width, int64_t& run, int64_t& zero_w)
{
    while (n > 0) {
        if (x == 0) {
            run += n;
            return;
        }
        const int z = __builtin_ctzll(x);            // < n: the bit lies below n
        run += z;
        if (run >= width) zero_w += run - width + 1;
        run = 0;
        x >>= z;
        const int ones = ~x == 0 ? 64 : __builtin_ctzll(~x);
        x = ones == 64 ? 0 : x >> ones;
        n -= z + ones;
    }
}

template <int U>
__global__ __launch_bounds__(kSparseBlock) void tile_window_census_kernel(WindowCensusArgs a)
{
    constexpr int K = WindowWalk<U>::K;
    __shared__ uint64_t s_mask[K];
    __shared__ uint64_t s_ballot[kSparseBlock / 64][64];      // [wave][cohort bit]: the wave's 64 tiles of the chunk
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x, R = a.g.R;
    bool too_long;
    const TileRegion reg = sparse_region<U>(a.g, r, &too_long);
    const int64_t tiles_valid = (reg.n_pos + a.binsize - 1) / a.binsize;
    const int64_t nv = too_long ? -1 : (tiles_valid < a.n_tiles ? tiles_valid : a.n_tiles);
    const int nw = window_count(nv, a.width);
    if (tid == 0) a.n_windows[r] = nw;
    const int64_t passes = (a.C + 63) / 64;
    for (int64_t pass = 0; pass < passes; ++pass) {
        const int cc = (int)(a.C - 64 * pass < 64 ? a.C - 64 * pass : 64);
        const int64_t at = (64 * pass + tid) * R + r;                        // (tid < cc)
        // nothing to walk: no window, or every cohort of the pass has none or all of its tiles positive
        int np = 0;
        bool known = nw == 0;
        if (!known && a.n_positive && tid < cc) {
            np = a.n_positive[at];
            known = np == 0 || np == nv;
        }
        // (the threads behind the pass's cohorts have no say where the others read the census; without it only nw == 0 is known)
        if (__syncthreads_and(known || (tid >= cc && a.n_positive != nullptr))) {
            if (tid < cc) a.n_positive_w[at] = np == 0 ? 0 : nw;
            continue;
        }
        for (int i = tid; i < K; i += kSparseBlock) s_mask[i] = a.mask[pass * K + i];
        __syncthreads();
        int64_t run = 0, zero_w = 0, positive = 0;                           // lane b of wave 0: cohort bit b
        for (int64_t t0 = 0; t0 < nv; t0 += kSparseBlock) {
            const int64_t t = t0 + tid;
            uint64_t m = 0;
            if (t < nv) {
                const int64_t p0 = t * a.binsize, p1 = p0 + a.binsize < reg.n_pos ? p0 + a.binsize : reg.n_pos;
                WindowWalk<U> win(a.g.words, a.g.n_words);
                win.start(reg.g0 + p0);
                for (int64_t p = p0; p < p1; ++p)
                    if (win.step(reg.g0 + p)) m |= s_mask[win.ref];
            }
            uint64_t mine = 0;                                               // lane b: the wave's tiles with bit b
            if (__ballot(m != 0)) {
                for (int b = 0; b < cc; ++b) {
                    const uint64_t w = __ballot((m >> b) & 1ull);
                    if (lane == b) mine = w;
                }
            }
            s_ballot[wave][lane] = mine;
            __syncthreads();
            if (tid < cc) {
#pragma unroll
                for (int v = 0; v < kSparseBlock / 64; ++v) {
                    const int64_t left = nv - t0 - 64 * v;                   // tiles of the region from this word on
                    if (left <= 0) break;
                    const uint64_t x = s_ballot[v][tid];
                    positive += __popcll(x);
                    fold_tiles(x, left < 64 ? (int)left : 64, a.width, run, zero_w);
                }
            }
            __syncthreads();
        }
        if (tid < cc) {
            if (run >= a.width) zero_w += run - a.width + 1;                 // (the run that reaches the region's end)
            a.n_positive_w[at] = nv < a.width ? (positive > 0 ? 1 : 0) : (int32_t)(nw - zero_w);
        }
    }
}

// ---- the mutated windows, counted and tested ----
// Head i of a run of equal keys (keys ascending; key = keys[i], a key of the planes: 0 <= key < C R T): the windows [lo, hi) whose
// first mutated tile it is, lo >= hi for none.  nv: the tiles of its region.
struct OwnedWindows {
    int64_t row;
    int t, lo, hi;
};
__device__ __forceinline__ OwnedWindows owned_windows(const int64_t* keys, int64_t i, int64_t key, int64_t T, int64_t nv, int width)
{
    OwnedWindows o;
    o.row = key / T;
    o.t = (int)(key - o.row * T);
    o.lo = o.hi = 0;
    if (o.t >= nv) return o;                                                 // (nv >= 1 from here on)
    const int64_t prev = i > 0 ? keys[i - 1] : -1;
    if (prev == key) return o;                                               // not the head of its run
    const int t_prev = prev >= 0 && prev / T == o.row ? (int)(prev - o.row * T) : -1;
    int lo = o.t - width + 1;
    lo = lo < t_prev + 1 ? t_prev + 1 : lo;
    o.lo = lo < 0 ? 0 : lo;
    const int nw = window_count(nv, width);
    o.hi = o.t + 1 < nw ? o.t + 1 : nw;
    return o;
}

__global__ __launch_bounds__(kSparseBlock) void sparse_window_count_kernel(const int64_t* __restrict__ keys, int64_t n,
                                                                           const int32_t* __restrict__ n_valid, int64_t slots, int64_t R,
                                                                           int64_t T, int width, int64_t* __restrict__ counts)
{
    const int64_t i = (int64_t)blockIdx.x * kSparseBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t key = keys[i];
    int64_t count = 0;
    if (key >= 0 && key < slots) {                                           // (negative, INT64_MAX or past the last row: passed over)
        const int64_t nv = n_valid[(key / T) % R];
        const OwnedWindows o = owned_windows(keys, i, key, T, nv < T ? nv : T, width);
        count = o.hi > o.lo ? o.hi - o.lo : 0;
    }
    counts[i] = count;
}

struct SparseWindowArgs {
    TileGenome g;
    const double* s_prob;
    int64_t C;
    int binsize;
    int64_t n_tiles;
    const double *denom, *mu, *sigma;                // [C, R]
    const int64_t* keys;                             // [n] ascending
    int64_t n, slots;
    const int64_t* offsets;                          // [n + 1]
    int width;
    int64_t w_begin, w_count;
    int32_t *out_cohort, *out_region, *out_window, *out_k;    // [w_count]
    double *out_pt, *out_exp, *out_pval;                      // [w_count]
};

template <int U>
__global__ __launch_bounds__(kSparseBlock) void sparse_window_test_kernel(SparseWindowArgs a)
{
    constexpr int K = WindowWalk<U>::K;
    nb_tables_init();
    const int64_t e = (int64_t)blockIdx.x * kSparseBlock + threadIdx.x;
    if (e >= a.w_count) return;
    const int64_t j = a.w_begin + e;
    int32_t c = -1, r = -1, w = -1, k = 0;
    double pt = dnan(), ex = dnan(), pv = dnan();
    // the owner: the last head i with offsets[i] <= j (the heads without a window share their successor's offset)
    int64_t lo = 0, hi = a.n + 1;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.offsets[mid] > j) hi = mid;
        else lo = mid + 1;
    }
    const int64_t i = lo - 1;
    const int64_t key = i >= 0 && i < a.n ? a.keys[i] : -1;
    if (key >= 0 && key < a.slots) {
        const int64_t cr = key / a.n_tiles, cc = cr / a.g.R, rr = cr - cc * a.g.R;
        bool too_long;
        const TileRegion reg = sparse_region<U>(a.g, rr, &too_long);
        const int64_t tiles_valid = (reg.n_pos + a.binsize - 1) / a.binsize;
        const int64_t nv = too_long ? -1 : (tiles_valid < a.n_tiles ? tiles_valid : a.n_tiles);
        const OwnedWindows o = owned_windows(a.keys, i, key, a.n_tiles, nv, a.width);
        const int64_t ww = o.lo + (j - a.offsets[i]);
        if (ww >= o.lo && ww < o.hi) {                                       // (offsets of another key list name nothing)
            const int64_t end = ww + a.width < nv ? ww + a.width : nv;       // one past the window's last tile
            const int64_t stop = cr * a.n_tiles + end;                       // the first key behind the window
            int64_t b0 = i, b1 = a.n;
            while (b0 < b1) {
                const int64_t mid = b0 + ((b1 - b0) >> 1);
                if (a.keys[mid] >= stop) b1 = mid;
                else b0 = mid + 1;
            }
            const int64_t p0 = ww * a.binsize;
            const int64_t p1 = end * a.binsize < reg.n_pos ? end * a.binsize : reg.n_pos;
            const double* S = a.s_prob + cc * K;
            double sum = 0.0;
            WindowWalk<U> win(a.g.words, a.g.n_words);
            win.start(reg.g0 + p0);
            for (int64_t p = p0; p < p1; ++p)
                if (win.step(reg.g0 + p)) sum += S[win.ref];
            const int64_t at = cc * a.g.R + rr;
            const double m = a.mu[at];
            const GammaParams g = normal_params_to_gamma(m, a.sigma[at]);
            c = (int32_t)cc, r = (int32_t)rr, w = (int32_t)ww, k = (int32_t)(b0 - i);
            pt = sum / a.denom[at];
            pv = nb_exact((double)k, g.alpha, nb_success_prob(pt, g.theta));
            ex = mul_rn(pt, m);
        }
    }
    a.out_cohort[e] = c;
    a.out_region[e] = r;
    a.out_window[e] = w;
    a.out_k[e] = k;
    a.out_pt[e] = pt;
    a.out_exp[e] = ex;
    a.out_pval[e] = pv;
}

// what the three entry points and their host twins require of the sizes: nothing is read before it
int sparse_window_sizes(const char* fn, int64_t C, int64_t R, int64_t T, int32_t width, int64_t* slots)
{
    if (int rc = tile_window_sizes(fn, C, R, T, width)) return rc;
    return sparse_tile_slots(fn, C, R, T, slots);
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_tile_window_census(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                           const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, const double* s_prob,
                           int64_t C, int n_up, int binsize, int64_t n_tiles, int32_t width, const int32_t* n_positive, int32_t* n_windows,
                           int32_t* n_positive_w, void* workspace, int64_t workspace_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const TileArgs t{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, s};
    if (int rc = check_tile_args(__func__, t, false)) return rc;
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, n_tiles, width, &slots)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(n_windows, "non-null n_windows");
    DIG_REQUIRE(C == 0 || (s_prob && n_positive_w), "non-null s_prob, n_positive_w");
    const int64_t need = tile_census_workspace_bytes(C, n_up);
    DIG_REQUIRE(workspace && workspace_bytes >= need, "workspace of dig_tile_census_workspace(C, n_up) bytes");
    DIG_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace aligned to 8 bytes");
    uint64_t* mask = static_cast<uint64_t*>(workspace);
    if (C > 0) launch_tile_census_mask(s_prob, C, n_up, mask, s);
    const WindowCensusArgs a{t.g, C, binsize, n_tiles, width, mask, n_positive, n_windows, n_positive_w};
    if (n_up == 1) hipLaunchKernelGGL(tile_window_census_kernel<1>, dim3((unsigned)R), dim3(kSparseBlock), 0, s, a);
    else hipLaunchKernelGGL(tile_window_census_kernel<2>, dim3((unsigned)R), dim3(kSparseBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_sparse_window_count(const int64_t* keys_sorted, int64_t n, const int32_t* n_valid, int64_t C, int64_t R, int64_t T, int32_t width,
                            int64_t* counts, void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, T, width, &slots)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted && counts, "non-null keys, counts");
    DIG_REQUIRE(slots == 0 || n_valid, "non-null n_valid");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kSparseBlock, &blocks)) return rc;
    hipLaunchKernelGGL(sparse_window_count_kernel, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, keys_sorted, n, n_valid, slots,
                       R, T, width, counts);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_sparse_window_test(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                           const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, const double* s_prob,
                           int64_t C, int n_up, int binsize, int64_t n_tiles, const double* denom, const double* mu, const double* sigma,
                           const int64_t* keys_sorted, int64_t n, const int64_t* offsets, int32_t width, int64_t w_begin, int64_t w_count,
                           int32_t* out_cohort, int32_t* out_region, int32_t* out_window, int32_t* out_k, double* out_pt, double* out_exp,
                           double* out_pval, void* stream)
{
    const TileArgs t{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, (hipStream_t)stream};
    if (int rc = check_tile_args(__func__, t, false)) return rc;
    int64_t slots = 0;
    if (int rc = sparse_window_sizes(__func__, C, R, n_tiles, width, &slots)) return rc;
    DIG_REQUIRE(n >= 0 && w_begin >= 0 && w_count >= 0 && w_count <= INT32_MAX, "n, w_begin >= 0, 0 <= w_count < 2^31");
    if (w_count == 0) return DIG_OK;
    DIG_REQUIRE(offsets && out_cohort && out_region && out_window && out_k && out_pt && out_exp && out_pval, "non-null offsets and outputs");
    DIG_REQUIRE(n == 0 || keys_sorted, "non-null keys");
    DIG_REQUIRE(slots == 0 || n == 0 || (s_prob && denom && mu && sigma), "non-null s_prob, denom, mu, sigma");
    const SparseWindowArgs a{t.g, s_prob, C, binsize, n_tiles, denom, mu, sigma, keys_sorted, n, slots, offsets, width, w_begin, w_count,
                             out_cohort, out_region, out_window, out_k, out_pt, out_exp, out_pval};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, w_count, kSparseBlock, &blocks)) return rc;
    if (n_up == 1) hipLaunchKernelGGL(sparse_window_test_kernel<1>, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sparse_window_test_kernel<2>, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
