// dig_cnvwindows.hip -- the copy-number training labels of the region model for MANY cohorts: per window of the data container's
// `idx` the mean over the window's W positions of three per-base tracks (duplications, copy-neutral / LOH, deletions) built from a
// cohort's copy-number segments.
//
// Reference, per cohort and per window (scripts/DataExtractor.py:100-154 fetch_cnv_region_avg, :535-539): a tabix fetch of the
// segments that overlap [s, s + W), a per-base difference track, its cumulative sum and np.mean over the W positions.  In closed form
//   label[window, class] = double(S) / double(W),   S = sum over the overlapping segments of weight * (min(end, s + W) - max(start, s))
// with class / weight from cp_num alone: 2 -> LOH / 1, below 2 -> deletion / 2 - cp_num, above 2 -> duplication / cp_num - 2.
// Segments are megabases long and windows 10 kb, so (segment, window) pairs are never formed.  The distinct window starts lie sorted
// per chromosome, and the windows a segment [a, b) meets are one run of them:
//   p0 = first start > a - W     f0 = first start >= a     f1 = first start > b - W     p1 = first start >= b
//   [f0, f1)  the windows it covers whole (when f0 < f1): +weight W at f0, -weight W at f1 of a DIFFERENCE array
//   [p0, f0) and [max(f0, f1), p1)  the windows it covers in part -- one at either end for windows that tile, more only where windows
//             overlap each other or the segment is shorter than W: the exact overlap v as +v at n and -v at n + 1
//   cnv_segment_deltas_kernel   one thread per segment: the chromosome's row, four binary searches, 64-bit integer atomics into
//                               deltas i64 [C, 3, N + 1] (element N: where the last window's -v goes)
//   cnv_chunk_sums_kernel       the sum of every chunk of kCnvChunk = 2 048 windows of every row            |  an inclusive prefix
//   cnv_chunk_carries_kernel    per row the exclusive prefix of its chunk sums, one wave per row             |  sum of each of the
//   cnv_window_means_kernel     one workgroup per (cohort, chunk): the three rows scanned, label = S / W     |  3 C rows
// What a chromosome adds it takes away again by its last window + 1, so one scan over all chromosomes of a row is the scan of each.
// Integer atomics only: the result does not depend on their order; the division is IEEE, the sums are exact below 2^53.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kCnvBlock = 256;
constexpr int kCnvPerLane = 8;                                   // windows per lane of the scan: a wave scans 512, a workgroup kCnvChunk
constexpr int kCnvWaves = kCnvBlock / 64;
constexpr int64_t kCnvChunk = DIG_CNV_SCAN_CHUNK;
constexpr int64_t kCnvCoordMax = (int64_t)1 << 40;
static_assert(kCnvChunk == (int64_t)kCnvBlock * kCnvPerLane, "a workgroup scans one chunk");

int cnv_sizes(const char* fn, int64_t C, int64_t N, int64_t W, CnvSizes* sz)
{
    DIG_REQUIRE_IN(fn, C >= 1 && C < ((int64_t)1 << 20), "C within [1, 2^20)");
    DIG_REQUIRE_IN(fn, N >= 0 && N < ((int64_t)1 << 31), "N within [0, 2^31)");
    DIG_REQUIRE_IN(fn, W >= 1 && W < ((int64_t)1 << 31), "W within [1, 2^31)");
    sz->rows = 3 * C;
    sz->chunks = (N + kCnvChunk - 1) / kCnvChunk;
    DIG_REQUIRE_IN(fn, sz->rows * (N + 1) < ((int64_t)1 << 40), "3 C (N + 1) below 2^40");
    DIG_REQUIRE_IN(fn, sz->rows * (sz->chunks > 0 ? sz->chunks : 1) < ((int64_t)1 << 31), "fewer than 2^31 (row, chunk) workgroups");
    sz->delta_bytes = sz->rows * (N + 1) * (int64_t)sizeof(int64_t);
    sz->carry_bytes = sz->rows * sz->chunks * (int64_t)sizeof(int64_t);
    return DIG_OK;
}

struct CnvSegmentArgs {
    const int64_t* win_start;       // [N] ascending within a chromosome's run
    const int64_t* chrom_id;        // [n_chrom] ascending
    const int64_t* chrom_off;       // [n_chrom + 1]
    int64_t n_chrom, N, W;
    const int64_t *seg_chrom, *seg_start, *seg_end;     // [n_seg]
    const uint8_t* seg_class;
    const int32_t *seg_weight, *seg_cohort;
    int64_t n_seg, C;
    int64_t* deltas;                // [C, 3, N + 1]
};

__device__ __forceinline__ void cnv_add(int64_t* p, int64_t v)
{
    atomicAdd(reinterpret_cast<unsigned long long*>(p), (unsigned long long)v);
}

// first index in [lo, hi) with starts[index] >= v (strict: > v); hi when there is none
template <bool kStrict>
__device__ __forceinline__ int64_t cnv_bound(const int64_t* starts, int64_t lo, int64_t hi, int64_t v)
{
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t s = starts[mid];
        if (kStrict ? s > v : s >= v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

__global__ __launch_bounds__(kCnvBlock) void cnv_segment_deltas_kernel(CnvSegmentArgs g)
{
    const int64_t i = (int64_t)blockIdx.x * kCnvBlock + threadIdx.x;
    if (i >= g.n_seg) return;
    const int64_t a = g.seg_start[i], b = g.seg_end[i], ch = g.seg_chrom[i], c = g.seg_cohort[i];
    const int k = g.seg_class[i];
    // (a segment outside the tables adds nothing; the host twin refuses it)
    if (k > 2 || c < 0 || c >= g.C || a < 0 || b <= a || b > kCnvCoordMax) return;
    const int64_t r = cnv_bound<false>(g.chrom_id, 0, g.n_chrom, ch);
    if (r >= g.n_chrom || g.chrom_id[r] != ch) return;              // a chromosome without a window
    int64_t lo = g.chrom_off[r], hi = g.chrom_off[r + 1];
    lo = lo < 0 ? 0 : (lo > g.N ? g.N : lo);                        // (whatever the table holds, every index below stays within [0, N])
    hi = hi < lo ? lo : (hi > g.N ? g.N : hi);
    if (lo == hi) return;
    const int64_t W = g.W, wt = g.seg_weight[i];
    const int64_t* s = g.win_start;
    const int64_t p0 = cnv_bound<true>(s, lo, hi, a - W);
    const int64_t p1 = cnv_bound<false>(s, p0, hi, b);
    if (p0 >= p1) return;
    const int64_t f0 = cnv_bound<false>(s, p0, p1, a);
    int64_t f1 = cnv_bound<true>(s, p0, p1, b - W);
    if (f1 < f0) f1 = f0;
    int64_t* row = g.deltas + (c * 3 + k) * (g.N + 1);
    if (f0 < f1) {
        cnv_add(row + f0, wt * W);
        cnv_add(row + f1, -wt * W);
    }
    for (int64_t n = p0; n < p1; ++n) {
        if (n == f0) n = f1;                                        // (past the windows covered whole)
        if (n >= p1) break;
        const int64_t ws = s[n];
        const int64_t v = wt * ((b < ws + W ? b : ws + W) - (a > ws ? a : ws));
        cnv_add(row + n, v);
        cnv_add(row + n + 1, -v);
    }
}

__device__ __forceinline__ int64_t cnv_wave_inclusive(int64_t v, int lane)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int64_t o = __shfl_up((long long)v, d, 64);
        if (lane >= d) v += o;
    }
    return v;
}

// sums [rows, chunks]: the sum of deltas[row, chunk kCnvChunk .. + kCnvChunk) below N
__global__ __launch_bounds__(kCnvBlock) void cnv_chunk_sums_kernel(const int64_t* deltas, int64_t N, int64_t chunks, int64_t* sums)
{
    __shared__ int64_t s_part[kCnvWaves];
    const int64_t row = blockIdx.x / chunks, chunk = blockIdx.x - row * chunks;
    const int64_t* src = deltas + row * (N + 1);
    const int64_t n0 = chunk * kCnvChunk + threadIdx.x;
    int64_t v = 0;
#pragma unroll
    for (int j = 0; j < kCnvPerLane; ++j) {
        const int64_t n = n0 + (int64_t)j * kCnvBlock;
        if (n < N) v += src[n];
    }
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    v = cnv_wave_inclusive(v, lane);
    if (lane == 63) s_part[wave] = v;
    __syncthreads();
    if (threadIdx.x == 0) {
        int64_t t = 0;
        for (int w = 0; w < kCnvWaves; ++w) t += s_part[w];
        sums[blockIdx.x] = t;
    }
}

// in place, per row: sums[row, chunk] <- the sum of the row's chunks before it.  One wave per row.
__global__ __launch_bounds__(64) void cnv_chunk_carries_kernel(int64_t* sums, int64_t chunks)
{
    int64_t* row = sums + (int64_t)blockIdx.x * chunks;
    const int lane = threadIdx.x;
    int64_t carry = 0;
    for (int64_t base = 0; base < chunks; base += 64) {
        const int64_t i = base + lane;
        const int64_t v = i < chunks ? row[i] : 0;
        const int64_t incl = cnv_wave_inclusive(v, lane);
        if (i < chunks) row[i] = carry + incl - v;
        carry += __shfl((long long)incl, 63, 64);
    }
}

// labels [C, N, 3]: a workgroup takes one chunk of one cohort, a wave 512 consecutive windows of it, a lane the windows
// base + 64 j + lane: loads of a row are contiguous per wave, and the three classes of a window are stored side by side.
__global__ __launch_bounds__(kCnvBlock) void cnv_window_means_kernel(const int64_t* deltas, const int64_t* carries, int64_t N, int64_t chunks,
                                                                     int64_t W, double* labels)
{
    __shared__ int64_t s_tot[kCnvWaves][3];
    const int64_t c = blockIdx.x / chunks, chunk = blockIdx.x - c * chunks;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int64_t n0 = chunk * kCnvChunk + (int64_t)wave * (64 * kCnvPerLane) + lane;
    int64_t v[3][kCnvPerLane];
    int64_t run[3];
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        const int64_t* src = deltas + (c * 3 + k) * (N + 1);
#pragma unroll
        for (int j = 0; j < kCnvPerLane; ++j) {
            const int64_t n = n0 + 64 * j;
            v[k][j] = n < N ? src[n] : 0;
        }
        int64_t acc = 0;                                            // the wave's windows before step j
#pragma unroll
        for (int j = 0; j < kCnvPerLane; ++j) {
            const int64_t incl = cnv_wave_inclusive(v[k][j], lane);
            v[k][j] = acc + incl;
            acc += __shfl((long long)incl, 63, 64);
        }
        if (lane == 0) s_tot[wave][k] = acc;
    }
    __syncthreads();
    const double w = (double)W;
#pragma unroll
    for (int k = 0; k < 3; ++k) {
        int64_t before = carries[(c * 3 + k) * chunks + chunk];
        for (int q = 0; q < wave; ++q) before += s_tot[q][k];
        run[k] = before;
    }
    double* dst = labels + c * N * 3;
#pragma unroll
    for (int j = 0; j < kCnvPerLane; ++j) {
        const int64_t n = n0 + 64 * j;
        if (n < N) {
#pragma unroll
            for (int k = 0; k < 3; ++k) dst[n * 3 + k] = (double)(run[k] + v[k][j]) / w;
        }
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int64_t dig_cnv_segment_deltas_size(int64_t C, int64_t N)
{
    CnvSizes sz;
    return cnv_sizes(__func__, C, N, 1, &sz) ? -1 : sz.delta_bytes;
}

int64_t dig_cnv_window_means_size(int64_t C, int64_t N)
{
    CnvSizes sz;
    return cnv_sizes(__func__, C, N, 1, &sz) ? -1 : sz.carry_bytes;
}

int dig_cnv_segment_deltas(const int64_t* win_start, const int64_t* chrom_id, const int64_t* chrom_off, int64_t n_chrom, int64_t N, int64_t W,
                           const int64_t* seg_chrom, const int64_t* seg_start, const int64_t* seg_end, const uint8_t* seg_class,
                           const int32_t* seg_weight, const int32_t* seg_cohort, int64_t n_seg, int64_t C, int64_t* deltas, void* stream)
{
    DIG_REQUIRE(n_chrom >= 0 && n_chrom <= N && n_seg >= 0, "0 <= n_chrom <= N, n_seg >= 0");
    CnvSizes sz;
    if (int rc = cnv_sizes(__func__, C, N, W, &sz)) return rc;
    DIG_REQUIRE(deltas, "non-null deltas");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(deltas, 0, (size_t)sz.delta_bytes, s));
    if (n_seg == 0 || N == 0) return DIG_OK;
    DIG_REQUIRE(win_start && chrom_id && chrom_off && seg_chrom && seg_start && seg_end && seg_class && seg_weight && seg_cohort,
                "non-null pointers");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_seg, kCnvBlock, &blocks)) return rc;
    const CnvSegmentArgs a{win_start, chrom_id, chrom_off, n_chrom, N, W, seg_chrom, seg_start, seg_end, seg_class, seg_weight, seg_cohort,
                           n_seg, C, deltas};
    hipLaunchKernelGGL(cnv_segment_deltas_kernel, dim3(blocks), dim3(kCnvBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_cnv_window_means(const int64_t* deltas, int64_t N, int64_t C, int64_t W, double* labels, int64_t* carries, void* stream)
{
    CnvSizes sz;
    if (int rc = cnv_sizes(__func__, C, N, W, &sz)) return rc;
    if (N == 0) return DIG_OK;
    DIG_REQUIRE(deltas && labels && carries, "non-null pointers");
    hipStream_t s = (hipStream_t)stream;
    hipLaunchKernelGGL(cnv_chunk_sums_kernel, dim3((unsigned)(sz.rows * sz.chunks)), dim3(kCnvBlock), 0, s, deltas, N, sz.chunks, carries);
    DIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cnv_chunk_carries_kernel, dim3((unsigned)sz.rows), dim3(64), 0, s, carries, sz.chunks);
    DIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(cnv_window_means_kernel, dim3((unsigned)(C * sz.chunks)), dim3(kCnvBlock), 0, s, deltas, carries, N, sz.chunks, W, labels);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
