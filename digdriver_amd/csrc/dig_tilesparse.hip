// dig_tilesparse.hip -- the per-base route for the MUTATED tiles only (DESIGN.md "Sparse per-base scan"): what stands behind
// nb_model.nb_model_hits_sparse and tileDriver --sparse.
//
// The dense route (dig_base_tile_probs_ctx -> dig_tile_mut_counts -> dig_tiled_nb_test) keeps four [C, R, T] planes.  A tile
// without a row has the closed-form p-value (1 + pt theta)^(-alpha); the host bounds it from the region denominators alone, so
// only the tiles that hold a row need a test.  Nothing here is [C, R, T]: the work and the memory follow the rows and C R.
//   tile_census_mask_kernel   per context the bit mask of the cohorts whose table entry is positive ([ceil(C / 64)][4^W] words,
//                             the call's workspace: built once, read by every region's workgroup out of L2).
//   tile_census_kernel        one workgroup per region, one streaming pass over its bases per 64 cohorts.  A thread walks a tile's
//                             positions with a sliding window; the region's exact integer context counts collect in LDS (integer
//                             atomics), a tile's cohort mask is the OR of its windows' masks, and the tiles with bit b set are
//                             counted with one ballot per cohort and 64 tiles.  first_pos, n_valid as dig_base_tile_probs_ctx;
//                             denom[c, r] = sum over the contexts of count * S[c][context] in ONE order: lane l of a wave adds the
//                             contexts l, l + 64, ... ascending with fma, then the 64 partial sums fold by halves (32, 16, ..., 1).
//                             No floating-point atomics: the bits depend on the region and the table alone.
//   sparse_tile_keys_kernel   one thread per (mutation, region) pair of the interval join: key = tile_mut_counts_kernel's slot
//                             (tile_slot, dig_tiles.hpp), (cohort R + region) T + tile; INT64_MAX for a pair that counts nowhere.
//   -- the caller sorts the keys --
//   sparse_tile_test_kernel   one thread per sorted key.  A run of equal keys is one mutated tile with k = its length; the run's
//                             head (left neighbour in global memory differs) finds the length (run_length, dig_keyruns.hpp),
//                             walks the tile's positions in order, pt = sum / denom, and runs
//                             the arithmetic of tiled_nb_generic_kernel through the same device functions.  Every other entry is
//                             written as "no tile" (k = 0).  Neighbouring lanes hold neighbouring tiles of one cohort: neighbouring
//                             genome words and one table.
// Both genome walkers read the tile kernels' 4-bit layout through its view (TileGenome, sparse_region, WindowWalk: dig_tiles.hpp),
// every word index clamped into the array; dig_tilesparsewindows.hip walks the same way.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"
#include "dig_tiles.hpp"

namespace dig {

// the sizes of the key (cohort R + region) T + tile: each below 2^31, the product within 62 bits
int sparse_tile_slots(const char* fn, int64_t C, int64_t R, int64_t T, int64_t* slots)
{
    DIG_REQUIRE_IN(fn, C >= 0 && R >= 0 && T >= 0, "C, R, n_tiles >= 0");
    const int64_t lim = (int64_t)1 << 31;
    DIG_REQUIRE_IN(fn, C < lim && R < lim && T < lim, "C, R and n_tiles below 2^31");
    const int64_t rows = C * R;                      // < 2^62
    DIG_REQUIRE_IN(fn, T == 0 || rows <= (((int64_t)1 << 62) - 1) / T,
                   "the key (cohort, region, tile) does not fit 62 bits: fewer cohorts or regions per call");
    *slots = rows * T;
    return DIG_OK;
}

int64_t tile_census_workspace_bytes(int64_t C, int n_up)
{
    if (C < 0 || (n_up != 1 && n_up != 2)) return 0;
    const int64_t K = tile_contexts(n_up), passes = (C + 63) / 64;
    return (passes > 0 ? passes : 1) * K * (int64_t)sizeof(uint64_t);
}

// ---- census ----
__global__ __launch_bounds__(kSparseBlock) void tile_census_mask_kernel(const double* __restrict__ s_prob, int64_t C, int K,
                                                                        uint64_t* __restrict__ mask, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * kSparseBlock + threadIdx.x;      // pass * K + context
    if (i >= n) return;
    const int64_t pass = i / K, ctx = i % K;
    uint64_t m = 0;
    for (int b = 0; b < 64; ++b) {
        const int64_t c = pass * 64 + b;
        if (c < C && s_prob[c * K + ctx] > 0.0) m |= 1ull << b;
    }
    mask[i] = m;
}

void launch_tile_census_mask(const double* s_prob, int64_t C, int n_up, uint64_t* mask, hipStream_t stream)
{
    const int K = tile_contexts(n_up);
    const int64_t n_mask = tile_census_workspace_bytes(C, n_up) / (int64_t)sizeof(uint64_t);
    hipLaunchKernelGGL(tile_census_mask_kernel, dim3((unsigned)((n_mask + kSparseBlock - 1) / kSparseBlock)), dim3(kSparseBlock), 0, stream,
                       s_prob, C, K, mask, n_mask);
}

struct CensusArgs {
    TileGenome g;
    const double* s_prob;
    int64_t C;
    int binsize;
    int64_t n_tiles;
    const uint64_t* mask;                            // [passes][K]
    int64_t* first_pos;
    int32_t* n_valid;
    double* denom;                                   // [C, R]
    int32_t* n_positive;                             // [C, R]
};

template <int U>
__global__ __launch_bounds__(kSparseBlock) void tile_census_kernel(CensusArgs a)
{
    constexpr int K = WindowWalk<U>::K;
    __shared__ uint64_t s_mask[K];
    __shared__ unsigned s_hist[K];
    __shared__ int s_cnt[64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int64_t r = blockIdx.x, R = a.g.R;
    bool too_long;
    const TileRegion reg = sparse_region<U>(a.g, r, &too_long);
    const int64_t tiles_valid = (reg.n_pos + a.binsize - 1) / a.binsize;
    const int64_t nv = too_long ? -1 : (tiles_valid < a.n_tiles ? tiles_valid : a.n_tiles);
    if (tid == 0) {
        a.first_pos[r] = reg.first;
        a.n_valid[r] = (int32_t)nv;
    }
    const int64_t passes = (a.C + 63) / 64;
    for (int64_t pass = 0; pass < (passes > 0 ? passes : 1); ++pass) {
        const int cc = (int)(a.C - 64 * pass < 64 ? (a.C > 64 * pass ? a.C - 64 * pass : 0) : 64);
        __syncthreads();
        for (int i = tid; i < K; i += kSparseBlock) {
            s_mask[i] = cc ? a.mask[pass * K + i] : 0ull;
            if (pass == 0) s_hist[i] = 0u;
        }
        if (tid < 64) s_cnt[tid] = 0;
        __syncthreads();
        // pass 0 walks every position (the denominator covers the region, also behind n_tiles), a later one the counted tiles
        const int64_t walk = pass == 0 ? tiles_valid : (nv > 0 ? nv : 0);
        int mine = 0;                                // lane b: the tiles of this wave with bit b
        for (int64_t t0 = 0; t0 < walk; t0 += kSparseBlock) {
            const int64_t t = t0 + tid;
            uint64_t m = 0;
            if (t < walk) {
                const int64_t p0 = t * a.binsize, p1 = p0 + a.binsize < reg.n_pos ? p0 + a.binsize : reg.n_pos;
                WindowWalk<U> win(a.g.words, a.g.n_words);
                win.start(reg.g0 + p0);
                for (int64_t p = p0; p < p1; ++p)
                    if (win.step(reg.g0 + p)) {
                        if (pass == 0) atomicAdd(&s_hist[win.ref], 1u);
                        m |= s_mask[win.ref];
                    }
                if (t >= nv) m = 0;
            }
            if (__ballot(m != 0)) {
                for (int b = 0; b < cc; ++b) {
                    const int n = __popcll(__ballot((m >> b) & 1ull));
                    if (lane == b) mine += n;
                }
            }
        }
        if (mine) atomicAdd(&s_cnt[lane], mine);
        __syncthreads();
        if (tid < cc) a.n_positive[(64 * pass + tid) * R + r] = s_cnt[tid];
    }
    // (the last barrier above stands behind pass 0's walk: the counts are complete)
    for (int64_t c = wave; c < a.C; c += kSparseBlock / 64) {
        const double* S = a.s_prob + c * K;
        double acc = 0.0;
        for (int j = lane; j < K; j += 64) acc = fma((double)s_hist[j], S[j], acc);
#pragma unroll
        for (int d = 32; d >= 1; d >>= 1) acc += __shfl_xor(acc, d, 64);
        if (lane == 0) a.denom[c * R + r] = acc;
    }
}

// ---- keys ----
struct SparseKeyArgs {
    const int32_t *pair_mut, *pair_reg;              // [n_pairs]
    int64_t n_pairs;
    const int64_t* mut_start;                        // [n_mut]
    const int32_t* mut_cohort;                       // [n_mut]
    int64_t n_mut;
    const int64_t* first_pos;                        // [R]
    const int32_t* n_valid;                          // [R]
    int binsize;
    int64_t n_tiles, R, C;
    int64_t* keys;                                   // [n_pairs]
};

__global__ __launch_bounds__(kSparseBlock) void sparse_tile_keys_kernel(SparseKeyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kSparseBlock + threadIdx.x;
    if (i >= a.n_pairs) return;
    const int64_t m = a.pair_mut[i], r = a.pair_reg[i];
    int64_t key = kSparseNoKey;
    if ((uint64_t)m < (uint64_t)a.n_mut && (uint64_t)r < (uint64_t)a.R) {        // (a pair outside the tables reads nothing)
        const int64_t slot = tile_slot(a.mut_start[m], a.mut_cohort[m], a.first_pos[r], a.n_valid[r], a.binsize, a.n_tiles, a.R, a.C, r);
        if (slot >= 0) key = slot;
    }
    a.keys[i] = key;
}

// ---- test ----
struct SparseTestArgs {
    TileGenome g;
    const double* s_prob;
    int64_t C;
    int binsize;
    int64_t n_tiles;
    const double *denom, *mu, *sigma;                // [C, R]
    const int64_t* keys;                             // [n] ascending
    int64_t n, slots;
    int32_t *out_cohort, *out_region, *out_tile, *out_k;      // [n]
    double *out_pt, *out_exp, *out_pval;                      // [n]
};

template <int U>
__global__ __launch_bounds__(kSparseBlock) void sparse_tile_test_kernel(SparseTestArgs a)
{
    constexpr int K = WindowWalk<U>::K;
    nb_tables_init();
    const int64_t i = (int64_t)blockIdx.x * kSparseBlock + threadIdx.x;
    int64_t key = -1;
    bool row = false, head = false;                  // row: a key of a tile
    if (i < a.n) {
        key = a.keys[i];
        row = key >= 0 && key < a.slots;             // (negative, INT64_MAX or past the last tile: passed over, never dereferenced)
        head = row && (i == 0 || a.keys[i - 1] != key);
    }
    const int64_t len = run_length(a.keys, a.n, i, key, head, row);
    int32_t c = -1, r = -1, t = -1, k = 0;
    double pt = dnan(), ex = dnan(), pv = dnan();
    if (head) {
        const int64_t cr = key / a.n_tiles, tt = key - cr * a.n_tiles;
        const int64_t cc = cr / a.g.R, rr = cr - cc * a.g.R;
        bool too_long;
        const TileRegion reg = sparse_region<U>(a.g, rr, &too_long);
        const int64_t p0 = tt * a.binsize;
        if (!too_long && p0 < reg.n_pos) {           // (a key the key kernel makes always names an existing tile)
            const int64_t p1 = p0 + a.binsize < reg.n_pos ? p0 + a.binsize : reg.n_pos;
            const double* S = a.s_prob + cc * K;
            double sum = 0.0;
            WindowWalk<U> win(a.g.words, a.g.n_words);
            win.start(reg.g0 + p0);
            for (int64_t p = p0; p < p1; ++p)
                if (win.step(reg.g0 + p)) sum += S[win.ref];
            const int64_t at = cc * a.g.R + rr;
            const double m = a.mu[at];
            const GammaParams g = normal_params_to_gamma(m, a.sigma[at]);
            c = (int32_t)cc, r = (int32_t)rr, t = (int32_t)tt, k = (int32_t)len;
            pt = sum / a.denom[at];
            pv = nb_exact((double)len, g.alpha, nb_success_prob(pt, g.theta));
            ex = mul_rn(pt, m);
        }
    }
    if (i < a.n) {
        a.out_cohort[i] = c;
        a.out_region[i] = r;
        a.out_tile[i] = t;
        a.out_k[i] = k;
        a.out_pt[i] = pt;
        a.out_exp[i] = ex;
        a.out_pval[i] = pv;
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int64_t dig_tile_census_workspace(int64_t C, int n_up) { return tile_census_workspace_bytes(C, n_up); }

int dig_tile_census(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                    const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, const double* s_prob,
                    int64_t C, int n_up, int binsize, int64_t n_tiles, int64_t* first_pos, int32_t* n_valid, double* denom,
                    int32_t* n_positive, void* workspace, int64_t workspace_bytes, void* stream)
{
    hipStream_t s = (hipStream_t)stream;
    const TileArgs t{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, first_pos, n_valid, s};
    if (int rc = check_tile_args(__func__, t, false)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(first_pos && n_valid, "non-null first_pos, n_valid");
    DIG_REQUIRE(C == 0 || (s_prob && denom && n_positive), "non-null s_prob, denom, n_positive");
    const int64_t need = tile_census_workspace_bytes(C, n_up);
    DIG_REQUIRE(workspace && workspace_bytes >= need, "workspace of dig_tile_census_workspace(C, n_up) bytes");
    DIG_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace aligned to 8 bytes");
    uint64_t* mask = static_cast<uint64_t*>(workspace);
    launch_tile_census_mask(s_prob, C, n_up, mask, s);
    const CensusArgs a{t.g, s_prob, C, binsize, n_tiles, mask, first_pos, n_valid, denom, n_positive};
    if (n_up == 1) hipLaunchKernelGGL(tile_census_kernel<1>, dim3((unsigned)R), dim3(kSparseBlock), 0, s, a);
    else hipLaunchKernelGGL(tile_census_kernel<2>, dim3((unsigned)R), dim3(kSparseBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_sparse_tile_keys(const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, const int64_t* mut_start, int64_t n_mut,
                         const int32_t* mut_cohort, const int64_t* first_pos, const int32_t* n_valid, int binsize, int64_t n_tiles,
                         int64_t R, int64_t C, int64_t* keys, void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && n_mut >= 0 && binsize >= 1, "n_pairs, n_mut >= 0, binsize >= 1");
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(__func__, C, R, n_tiles, &slots)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(pair_mut && pair_reg && keys, "non-null pair arrays, keys");
    DIG_REQUIRE(n_mut == 0 || (mut_start && mut_cohort), "non-null mutation arrays");
    DIG_REQUIRE(R == 0 || (first_pos && n_valid), "non-null region tables");
    const SparseKeyArgs a{pair_mut, pair_reg, n_pairs, mut_start, mut_cohort, n_mut, first_pos, n_valid, binsize, n_tiles, R, C, keys};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_pairs, kSparseBlock, &blocks)) return rc;
    hipLaunchKernelGGL(sparse_tile_keys_kernel, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_sparse_tile_test(const uint32_t* genome_words, int64_t n_words, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                         const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, int64_t R, const double* s_prob,
                         int64_t C, int n_up, int binsize, int64_t n_tiles, const double* denom, const double* mu, const double* sigma,
                         const int64_t* keys_sorted, int64_t n, int32_t* out_cohort, int32_t* out_region, int32_t* out_tile,
                         int32_t* out_k, double* out_pt, double* out_exp, double* out_pval, void* stream)
{
    const TileArgs t{{genome_words, n_words, chrom_off, chrom_len, n_chrom, reg_chrom, reg_start, reg_end, R}, s_prob, C, n_up, binsize,
                     n_tiles, nullptr, nullptr, nullptr, (hipStream_t)stream};
    if (int rc = check_tile_args(__func__, t, false)) return rc;
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(__func__, C, R, n_tiles, &slots)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted && out_cohort && out_region && out_tile && out_k && out_pt && out_exp && out_pval, "non-null keys and outputs");
    DIG_REQUIRE(slots == 0 || (s_prob && denom && mu && sigma), "non-null s_prob, denom, mu, sigma");
    const SparseTestArgs a{t.g, s_prob, C, binsize, n_tiles, denom, mu, sigma, keys_sorted, n, slots,
                           out_cohort, out_region, out_tile, out_k, out_pt, out_exp, out_pval};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kSparseBlock, &blocks)) return rc;
    if (n_up == 1) hipLaunchKernelGGL(sparse_tile_test_kernel<1>, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, a);
    else hipLaunchKernelGGL(sparse_tile_test_kernel<2>, dim3(blocks), dim3(kSparseBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
