// dig_pairs.hip -- co-occurrence and exclusivity of called elements: the element x sample incidence of a cohort as bit rows
// (dig_pair_bits), and per pair of rows the size of their intersection and the two one-sided Fisher exact p-values
// (dig_pair_fisher).  include/dig_hip.h states the rule; this is how it is evaluated.
//
// dig_pair_bits     one thread per (row, sample) key, one 32-bit atomicOr into the row's word (bit s of u64 word s / 64 is bit s % 32
//                   of u32 word s / 32: little-endian).  A key with a row or a sample outside the matrix sets nothing.
// dig_pair_fisher   three launches on the stream:
//   pair_lnfact_kernel   the table ln(x!) = lgamma(x + 1), x = 0 .. n_max, one thread per entry: at most 512 KiB, read through L2
//   pair_rowcount_kernel N_ROW: one wave per row, a popcount per word, a shuffle sum
//   pair_fisher_kernel   one workgroup of kPairBlock = 256 lanes per 64 x 64 TILE (cohort, block i <= block j) of a cohort's pair
//       matrix.  The two 64-row panels go through LDS kPairChunk = 32 words (2 048 samples) at a time, loaded 16 bytes a lane; a
//       row's pitch is 33 words, so the 32 lanes of a half wave that read 32 different rows of one word index fall on the 64 banks
//       two by two ((a / 4) % 64 = (66 row + 2 w) % 64 = 2 (row + w) % 64: all different), and the reads of the i rows, which are
//       the same row for a whole wave, are broadcasts.  Lane t owns column j = t % 64 of the tile and the 16 rows i = t / 64 + 4 m:
//       16 counters in registers, one AND + popcount per word and pair.  Only the words that hold the cohort's n samples are walked.
//       Then the tail rule per pair, the 16 pairs of a lane one after the other through ONE copy of the code.  The lanes of a wave
//       differ in tail length (the sum runs until a term is below 2^-56 of it: about 8 standard deviations of the table, 15 - 20
//       steps at the sizes of the element route, a division each); a wave lasts as long as its longest lane.
//       A wave's stores are 64 neighbouring slots of one row i of the upper triangle.
// No atomics other than the atomicOr, no workspace beyond the table; every output slot is written once by the lane that owns it.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"

namespace dig {

constexpr int kPairTile = DIG_PAIR_TILE;                 // rows of a panel
constexpr int kPairBlock = 256;
constexpr int kPairChunk = 32;                           // words of a row per LDS chunk (DIG_PAIR_CHUNK_BITS / 64)
constexpr int kPairPitch = kPairChunk + 1;               // words between two rows of a panel in LDS
constexpr int kPairPer = kPairTile * kPairTile / kPairBlock;      // pairs of a lane
static_assert(kPairChunk * 64 == DIG_PAIR_CHUNK_BITS && kPairTile == 64 && kPairPer == 16, "the lane layout below");

typedef unsigned long long PairWords2 __attribute__((ext_vector_type(2)));

struct PairArgs {
    const uint64_t* bits;                                // [H_total, W]
    const int64_t* row_ptr;                              // [C + 1]
    const int32_t* n_samples;                            // [C]
    const int64_t* pair_ptr;                             // [C + 1]
    const int32_t* tiles;                                // [n_tiles, 3]: cohort, block i, block j
    const double* lnfact;                                // [n_max + 1]
    const int32_t* n_row;                                // [H_total]
    int64_t H_total, W, C, n_pairs;
    int32_t n_max, h_max;
    int32_t* n_both;                                     // [n_pairs]
    double *p_co, *p_ex;                                 // [n_pairs]
};

__global__ __launch_bounds__(kPairBlock) void pair_bits_kernel(const int32_t* __restrict__ row, const int32_t* __restrict__ sample,
                                                               int64_t n_keys, int64_t H_total, int64_t W, uint32_t* bits)
{
    const int64_t i = (int64_t)blockIdx.x * kPairBlock + threadIdx.x;
    if (i >= n_keys) return;
    const int64_t r = row[i], s = sample[i];
    if (r < 0 || r >= H_total || s < 0 || s >= W * 64) return;
    atomicOr(bits + r * (W * 2) + (s >> 5), 1u << (s & 31));
}

__global__ __launch_bounds__(kPairBlock) void pair_lnfact_kernel(double* lnfact, int n_max)
{
    const int x = blockIdx.x * kPairBlock + threadIdx.x;
    if (x <= n_max) lnfact[x] = x < 2 ? 0.0 : lgamma((double)x + 1.0);
}

__global__ __launch_bounds__(kPairBlock) void pair_rowcount_kernel(const uint64_t* __restrict__ bits, int64_t H_total, int64_t W,
                                                                   int32_t* n_row)
{
    const int lane = threadIdx.x & 63;
    const int64_t r = (int64_t)blockIdx.x * (kPairBlock / 64) + (threadIdx.x >> 6);
    if (r >= H_total) return;                            // (a whole wave leaves)
    int s = 0;
    for (int64_t w = lane; w < W; w += 64) s += __popcll(bits[r * W + w]);
#pragma unroll
    for (int d = 32; d >= 1; d >>= 1) s += __shfl_xor(s, d, 64);
    if (lane == 0) n_row[r] = s;
}

// The two tails of the table (n, r, k, a): the one on the side of a away from the mode is summed outward from pmf(a) by the ratio
// recurrence, the other is 1 - that + pmf(a); both are capped at 1.  A table that cannot be one (bits set behind the cohort's n
// samples) gives NaN.
__device__ __forceinline__ void pair_tails(const double* __restrict__ lf, int n, int r, int k, int a, double& p_co, double& p_ex)
{
    const int lo = r + k - n > 0 ? r + k - n : 0, hi = r < k ? r : k;
    if (r > n || k > n || a < lo) {
        p_co = p_ex = dnan();
        return;
    }
    if (r == 0 || k == 0 || r == n || k == n) {
        p_co = p_ex = 1.0;
        return;
    }
    const int mode = (int)(((int64_t)(r + 1) * (k + 1)) / (n + 2));
    const int d = n - k - r + a;                         // samples in neither row
    const double logp = ((lf[k] - lf[a] - lf[k - a]) + (lf[n - k] - lf[r - a] - lf[d])) - (lf[n] - lf[r] - lf[n - r]);
    const double pa = exp(logp);
    double t = pa, s = pa;
    const bool up = a >= mode;
    if (up) {
        for (int x = a; x < hi; ++x) {
            t *= ((double)(k - x) * (double)(r - x)) / ((double)(x + 1) * (double)(d + (x - a) + 1));
            s += t;
            if (!(t > s * 0x1p-56)) break;
        }
    } else {
        for (int x = a; x > lo; --x) {
            t *= ((double)x * (double)(d - (a - x))) / ((double)(k - x + 1) * (double)(r - x + 1));
            s += t;
            if (!(t > s * 0x1p-56)) break;
        }
    }
    const double small = fmin(1.0, s), large = fmin(1.0, (1.0 - s) + pa);
    p_co = up ? small : large;
    p_ex = up ? large : small;
}

template <bool TAILS>
__global__ __launch_bounds__(kPairBlock) void pair_fisher_kernel(PairArgs g)
{
    __shared__ uint64_t panel[2][kPairTile * kPairPitch];
    const int t = threadIdx.x, tj = t & 63, ti0 = t >> 6;
    const int32_t* tile = g.tiles + (int64_t)blockIdx.x * 3;
    const int c = tile[0], bi = tile[1], bj = tile[2];
    if (c < 0 || c >= g.C || bi < 0 || bj < bi) return;  // (uniform: the whole workgroup leaves)
    const int64_t r0 = g.row_ptr[c];
    int64_t H = g.row_ptr[c + 1] - r0;
    if (r0 < 0 || r0 > g.H_total) return;
    H = H < g.H_total - r0 ? H : g.H_total - r0;
    H = H < g.h_max ? H : g.h_max;
    if ((int64_t)bj * kPairTile >= H) return;
    int n = g.n_samples[c];
    n = n < 0 ? 0 : n < g.n_max ? n : g.n_max;
    const int64_t W = g.W;
    const int64_t words = ((int64_t)n + 63) / 64 < W ? ((int64_t)n + 63) / 64 : W;
    const int64_t base[2] = {(int64_t)bi * kPairTile, (int64_t)bj * kPairTile};

    int cnt[kPairPer];
#pragma unroll
    for (int m = 0; m < kPairPer; ++m) cnt[m] = 0;
    for (int64_t w0 = 0; w0 < words; w0 += kPairChunk) {
        // both panels, 2 x 64 rows x 32 words, 16 bytes a lane and step (W is even and bits lies at 0 (mod 16))
#pragma unroll
        for (int q = 0; q < 2 * kPairTile * kPairChunk / 2 / kPairBlock; ++q) {
            const int flat = q * kPairBlock + t, p = flat >> 10, rr = (flat >> 4) & 63, w2 = (flat & 15) * 2;
            const int64_t row = base[p] + rr;
            PairWords2 v = {0ull, 0ull};
            if (row < H && w0 + w2 < W) v = *reinterpret_cast<const PairWords2*>(g.bits + (r0 + row) * W + w0 + w2);
            panel[p][rr * kPairPitch + w2] = v.x, panel[p][rr * kPairPitch + w2 + 1] = v.y;
        }
        __syncthreads();
        const int cw = words - w0 < kPairChunk ? (int)(words - w0) : kPairChunk;
        for (int w = 0; w < cw; ++w) {
            const uint64_t b = panel[1][tj * kPairPitch + w];
#pragma unroll
            for (int m = 0; m < kPairPer; ++m) cnt[m] += __popcll(panel[0][(ti0 + 4 * m) * kPairPitch + w] & b);
        }
        __syncthreads();
    }

    const int64_t gj = base[1] + tj;
    const int k = gj < H ? g.n_row[r0 + gj] : 0;
    const int64_t p0 = g.pair_ptr[c];
    // the 16 pairs one after the other through one copy of the tail code: pair m's count is taken from slot 0 and the others move
    // down a slot, all with compile-time indices, which keeps them in registers
#pragma unroll 1
    for (int m = 0; m < kPairPer; ++m) {
        const int a = cnt[0];
#pragma unroll
        for (int i = 0; i + 1 < kPairPer; ++i) cnt[i] = cnt[i + 1];
        const int64_t gi = base[0] + ti0 + 4 * m;
        if (gi >= H || gj >= H || gi >= gj) continue;
        const int64_t slot = p0 + gi * (2 * H - gi - 1) / 2 + (gj - gi - 1);
        if (slot < 0 || slot >= g.n_pairs) continue;
        g.n_both[slot] = a;
        if (TAILS) {
            double p_co, p_ex;
            pair_tails(g.lnfact, n, g.n_row[r0 + gi], k, a, p_co, p_ex);
            g.p_co[slot] = p_co, g.p_ex[slot] = p_ex;
        }
    }
}

int pair_bits_sizes(const char* fn, int64_t n_keys, int64_t H_total, int64_t W, const void* bits, unsigned* blocks)
{
    DIG_REQUIRE_IN(fn, n_keys >= 0 && H_total >= 0, "n_keys, H_total >= 0");
    DIG_REQUIRE_IN(fn, W >= 2 && W % 2 == 0 && W <= DIG_PAIR_MAX_SAMPLES / 64, "W even, 2 <= W <= 1024 (16-byte rows of at most 65 536 samples)");
    DIG_REQUIRE_IN(fn, H_total < ((int64_t)1 << 31), "fewer than 2^31 rows");
    DIG_REQUIRE_IN(fn, H_total == 0 || (bits && ((uintptr_t)bits & 15) == 0), "bits non-null and 16-byte aligned");
    return row_blocks(fn, n_keys, kPairBlock, blocks);
}

int pair_fisher_sizes(const char* fn, const void* bits, int64_t H_total, int64_t W, int64_t C, int64_t n_tiles, int64_t n_pairs,
                      int32_t n_max, int32_t h_max)
{
    DIG_REQUIRE_IN(fn, H_total >= 0 && C >= 0 && n_tiles >= 0 && n_pairs >= 0 && n_max >= 0 && h_max >= 0,
                   "H_total, C, n_tiles, n_pairs, n_max, h_max >= 0");
    DIG_REQUIRE_IN(fn, n_max <= DIG_PAIR_MAX_SAMPLES, "n_max <= 65 536 samples per cohort");
    DIG_REQUIRE_IN(fn, h_max <= DIG_PAIR_MAX_ROWS, "h_max <= 8 192 rows per cohort: a higher min_samples or a stricter cut");
    DIG_REQUIRE_IN(fn, n_pairs < ((int64_t)1 << 31), "fewer than 2^31 pairs per call: fewer cohorts per call");
    DIG_REQUIRE_IN(fn, n_tiles < ((int64_t)1 << 31) && C < ((int64_t)1 << 31) && H_total < ((int64_t)1 << 31),
                   "fewer than 2^31 tiles (a tile per workgroup), cohorts and rows");
    DIG_REQUIRE_IN(fn, W >= 2 && W % 2 == 0 && W <= DIG_PAIR_MAX_SAMPLES / 64 && W * 64 >= n_max,
                   "W even, 2 <= W <= 1024, W * 64 >= n_max (16-byte rows that hold n_max samples)");
    DIG_REQUIRE_IN(fn, H_total == 0 || (bits && ((uintptr_t)bits & 15) == 0), "bits non-null and 16-byte aligned");
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_pair_bits(const int32_t* row, const int32_t* sample, int64_t n_keys, int64_t H_total, int64_t W, uint64_t* bits, void* stream)
{
    unsigned blocks = 0;
    if (int rc = pair_bits_sizes(__func__, n_keys, H_total, W, bits, &blocks)) return rc;
    if (H_total == 0) return DIG_OK;
    DIG_REQUIRE(n_keys == 0 || (row && sample), "non-null row, sample");
    DIG_HIP_TRY(hipMemsetAsync(bits, 0, (size_t)H_total * W * sizeof(uint64_t), (hipStream_t)stream));
    if (n_keys == 0) return DIG_OK;
    hipLaunchKernelGGL(pair_bits_kernel, dim3(blocks), dim3(kPairBlock), 0, (hipStream_t)stream, row, sample, n_keys, H_total, W,
                       reinterpret_cast<uint32_t*>(bits));
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

static int pair_fisher_launch(const char* fn, bool tails, const uint64_t* bits, int64_t H_total, int64_t W, const int64_t* row_ptr,
                              const int32_t* n_samples, const int64_t* pair_ptr, int64_t C, const int32_t* tiles, int64_t n_tiles,
                              int64_t n_pairs, int32_t n_max, int32_t h_max, double* lnfact, int32_t* n_row, int32_t* n_both,
                              double* pval_cooccur, double* pval_exclusive, void* stream)
{
    if (int rc = pair_fisher_sizes(fn, bits, H_total, W, C, n_tiles, n_pairs, n_max, h_max)) return rc;
    DIG_REQUIRE_IN(fn, !tails || lnfact, "non-null lnfact");
    DIG_REQUIRE_IN(fn, H_total == 0 || n_row, "non-null n_row");
    DIG_REQUIRE_IN(fn, n_pairs == 0 || (n_both && (!tails || (pval_cooccur && pval_exclusive))),
                   "non-null n_both, pval_cooccur, pval_exclusive");
    DIG_REQUIRE_IN(fn, n_tiles == 0 || (row_ptr && n_samples && pair_ptr && tiles), "non-null row_ptr, n_samples, pair_ptr, tiles");
    if (tails)
        hipLaunchKernelGGL(pair_lnfact_kernel, dim3((unsigned)(n_max / kPairBlock + 1)), dim3(kPairBlock), 0, (hipStream_t)stream,
                           lnfact, (int)n_max);
    if (H_total)
        hipLaunchKernelGGL(pair_rowcount_kernel, dim3((unsigned)((H_total + 3) / 4)), dim3(kPairBlock), 0, (hipStream_t)stream, bits,
                           H_total, W, n_row);
    if (n_tiles && n_pairs) {
        PairArgs g{};
        g.bits = bits, g.row_ptr = row_ptr, g.n_samples = n_samples, g.pair_ptr = pair_ptr, g.tiles = tiles, g.lnfact = lnfact;
        g.n_row = n_row, g.H_total = H_total, g.W = W, g.C = C, g.n_pairs = n_pairs, g.n_max = n_max, g.h_max = h_max;
        g.n_both = n_both, g.p_co = pval_cooccur, g.p_ex = pval_exclusive;
        if (tails)
            hipLaunchKernelGGL(pair_fisher_kernel<true>, dim3((unsigned)n_tiles), dim3(kPairBlock), 0, (hipStream_t)stream, g);
        else
            hipLaunchKernelGGL(pair_fisher_kernel<false>, dim3((unsigned)n_tiles), dim3(kPairBlock), 0, (hipStream_t)stream, g);
    }
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_pair_fisher(const uint64_t* bits, int64_t H_total, int64_t W, const int64_t* row_ptr, const int32_t* n_samples,
                    const int64_t* pair_ptr, int64_t C, const int32_t* tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                    int32_t h_max, double* lnfact, int32_t* n_row, int32_t* n_both, double* pval_cooccur, double* pval_exclusive,
                    void* stream)
{
    return pair_fisher_launch(__func__, true, bits, H_total, W, row_ptr, n_samples, pair_ptr, C, tiles, n_tiles, n_pairs, n_max, h_max,
                              lnfact, n_row, n_both, pval_cooccur, pval_exclusive, stream);
}

int dig_pair_counts(const uint64_t* bits, int64_t H_total, int64_t W, const int64_t* row_ptr, const int32_t* n_samples,
                    const int64_t* pair_ptr, int64_t C, const int32_t* tiles, int64_t n_tiles, int64_t n_pairs, int32_t n_max,
                    int32_t h_max, int32_t* n_row, int32_t* n_both, void* stream)
{
    return pair_fisher_launch(__func__, false, bits, H_total, W, row_ptr, n_samples, pair_ptr, C, tiles, n_tiles, n_pairs, n_max, h_max,
                              nullptr, n_row, n_both, nullptr, nullptr, stream);
}

}  // extern "C"
