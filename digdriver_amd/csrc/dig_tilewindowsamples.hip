// dig_tilewindowsamples.hip -- the DISTINCT SAMPLES of every sliding window of the per-base route: what stands behind
// `tileDriver --window-tiles M --window-samples` (OBS_SAMPLES / PVAL_SAMPLE of a window).
//
// dig_tile_window_test (dig_tilewindows.hip) sums the planes of a window's tiles.  The samples of a window are no such sum: one
// sample with a burst of ten mutations at bin size 1 sits in ten tiles, and every one of them counts it.  With n(c, r, t, s) the rows
// of global sample s that dig_tile_sample_keys counts in tile (c, r, t), nv = min(n_valid[r], T), and the windows of
// dig_tile_window_test (n_windows[r] = 0 when nv <= 0, else max(nv - m + 1, 1); window t covers the tiles t .. min(t + m, nv) - 1):
//   s_w[c, r, t] = the kept samples with a counted row in one of the window's tiles      for t < n_windows[r], else 0.
// Three kernels around one key sort:
//   tile_window_rekey_kernel   one lane per key of dig_tile_sample_keys, ((row T + tile) << sb) | sample with row = cohort R + region:
//                              -> ((row << sb) | sample) T + tile.  Sorted ascending, the tiles of one sample in one row then lie
//                              next to each other, ascending.  Keys that count nowhere stay INT64_MAX.
//   -- the caller sorts the keys --
//   tile_window_diff_kernel    one lane per sorted key.  The lane whose left neighbour -- read from global memory: it may lie in the
//                              previous wave or workgroup -- holds another key is the head of its run of equal keys, and that
//                              neighbour is also its predecessor: the same (row, sample) iff prev / T == key / T.  Tile t of a sample
//                              whose previous tile in the row is t_prev (-1: none) is the FIRST tile of that sample in exactly the
//                              windows that start at w in [lo, hi), lo = max(t_prev + 1, t - m + 1, 0), hi = min(t + 1, n_windows):
//                              every window that holds a tile of the sample is counted once, through its first such tile.  The head
//                              adds +1 at s_w[row, lo] and -1 at s_w[row, hi] (hi < T): two integer atomics per (tile, sample),
//                              however many rows it has.  A tile hit by S samples costs S atomics on one address (the sample-major
//                              order keeps them apart in a wave); S is bounded by the cohort's samples, not by its rows.
//   tile_window_scan_kernel    the in-place inclusive prefix sum of every row: one wave per row, each lane four consecutive tiles,
//                              the row walked in chunks of 256 tiles with a running carry (T = 200: one step; T = 10 000: 40).  The
//                              lanes' sums are scanned with six shuffle steps; no LDS.  Every interval ends at or before n_windows,
//                              so the entries behind the last window come out 0 by construction.  Two compiled forms: 16-byte loads
//                              and stores when the plane is aligned to 16 bytes and T is a multiple of 4, else 4-byte ones (every
//                              pointer needs its element's alignment and no more).
// Integer atomics only: the result is exact and does not depend on their order.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kWinSampleBlock = 256;
constexpr int kWinScanItems = 4;                                   // consecutive tiles of a lane
constexpr int kWinScanChunk = 64 * kWinScanItems;                  // tiles of one step of a wave
constexpr int kWinScanRows = kWinSampleBlock / 64;                 // rows (waves) of a workgroup
constexpr int64_t kWinSampleNoKey = INT64_MAX;                     // the all-ones 63-bit key of dig_tile_sample_keys

__global__ __launch_bounds__(kWinSampleBlock) void tile_window_rekey_kernel(const int64_t* keys, int64_t n, int64_t slots, int64_t T,
                                                                            int sample_bits, int64_t* keys_out)
{
    const int64_t i = (int64_t)blockIdx.x * kWinSampleBlock + threadIdx.x;
    if (i >= n) return;
    const int64_t key = keys[i];
    int64_t out = kWinSampleNoKey;
    // (a key of a tile outside the planes counts nowhere either: below `slots` the new key fits the old one's 63 bits)
    if (key >= 0 && key != kWinSampleNoKey && (key >> sample_bits) < slots) {
        const int64_t slot = key >> sample_bits, sample = key - (slot << sample_bits);
        const int64_t row = slot / T, tile = slot - row * T;
        out = ((row << sample_bits) | sample) * T + tile;
    }
    keys_out[i] = out;
}

struct TileWindowSampleArgs {
    const int64_t* keys;                             // [n] sample-major, ascending
    int64_t n;
    const int32_t* n_valid;                          // [R]
    int64_t rows, R, T;                              // rows = C R
    int sample_bits, width;
    int32_t* s_w;                                    // [C, R, T], zeroed
};

__global__ __launch_bounds__(kWinSampleBlock) void tile_window_diff_kernel(TileWindowSampleArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kWinSampleBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t key = a.keys[i], prev = i > 0 ? a.keys[i - 1] : -1;
    if (key < 0 || key == kWinSampleNoKey || prev == key) return;      // counts nowhere, or not the head of its run
    const int64_t q = key / a.T, row = q >> a.sample_bits;             // q = (row << sb) | sample
    if (row >= a.rows) return;
    const int t = (int)(key - q * a.T);
    int nv = a.n_valid[row % a.R];
    nv = nv > a.T ? (int)a.T : nv;
    if (t >= nv) return;                                               // (nv >= 1 from here on)
    const int nw = nv - a.width + 1 > 1 ? nv - a.width + 1 : 1;
    // the sample's previous tile in this row: the left neighbour, when it is of the same (row, sample)
    const int t_prev = prev >= 0 && prev / a.T == q ? (int)(prev - q * a.T) : -1;
    int lo = t - a.width + 1;
    lo = lo < t_prev + 1 ? t_prev + 1 : lo;
    lo = lo < 0 ? 0 : lo;
    const int hi = t + 1 < nw ? t + 1 : nw;
    if (lo >= hi) return;                                              // 0 <= lo < hi <= nv <= T
    int32_t* s = a.s_w + row * a.T;
    atomicAdd(&s[lo], 1);
    if (hi < a.T) atomicAdd(&s[hi], -1);
}

template <bool kVec>
__global__ __launch_bounds__(kWinSampleBlock) void tile_window_scan_kernel(int32_t* s_w, int64_t rows, int64_t T)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * kWinScanRows + (threadIdx.x >> 6);
    if (row >= rows) return;                                           // (a whole wave)
    int32_t* s = s_w + row * T;
    int carry = 0;
    for (int64_t t0 = 0; t0 < T; t0 += kWinScanChunk) {
        const int64_t t = t0 + lane * kWinScanItems;
        int v[kWinScanItems] = {0, 0, 0, 0};
        if (kVec) {
            if (t < T) {                                               // (T is a multiple of 4: the four tiles exist together)
                const int4 x = *reinterpret_cast<const int4*>(s + t);
                v[0] = x.x, v[1] = x.y, v[2] = x.z, v[3] = x.w;
            }
        } else {
#pragma unroll
            for (int u = 0; u < kWinScanItems; ++u)
                if (t + u < T) v[u] = s[t + u];
        }
        v[1] += v[0], v[2] += v[1], v[3] += v[2];
        int incl = v[3];                                               // -> the sum of the lanes 0 .. lane
#pragma unroll
        for (int d = 1; d < 64; d <<= 1) {
            const int other = __shfl_up(incl, d, 64);
            if (lane >= d) incl += other;
        }
        const int before = carry + incl - v[3];
        if (kVec) {
            if (t < T) *reinterpret_cast<int4*>(s + t) = make_int4(v[0] + before, v[1] + before, v[2] + before, v[3] + before);
        } else {
#pragma unroll
            for (int u = 0; u < kWinScanItems; ++u)
                if (t + u < T) s[t + u] = v[u] + before;
        }
        carry += __shfl(incl, 63, 64);
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_tile_window_sample_keys(const int64_t* keys, int64_t n, int64_t C, int64_t R, int64_t T, int64_t n_samples, int64_t* keys_out,
                                void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, T, n_samples, &sb)) return rc;
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys && keys_out, "non-null keys, keys_out");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kWinSampleBlock, &blocks)) return rc;
    hipLaunchKernelGGL(tile_window_rekey_kernel, dim3(blocks), dim3(kWinSampleBlock), 0, (hipStream_t)stream, keys, n, C * R * T, T, sb,
                       keys_out);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_tile_window_samples(const int64_t* keys_sorted, int64_t n, const int32_t* n_valid, int64_t C, int64_t R, int64_t T,
                            int64_t n_samples, int32_t width, int32_t* s_w, void* stream)
{
    if (int rc = tile_window_sizes(__func__, C, R, T, width)) return rc;
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, T, n_samples, &sb)) return rc;
    const int64_t rows = C * R;
    if (rows == 0 || T == 0) return DIG_OK;
    DIG_REQUIRE(s_w, "non-null s_w");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kWinSampleBlock, &blocks)) return rc;
    const int64_t groups = (rows + kWinScanRows - 1) / kWinScanRows;
    DIG_REQUIRE(groups < ((int64_t)1 << 31), "fewer than 2^31 workgroups (C R / 4)");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(s_w, 0, (size_t)rows * T * sizeof(int32_t), s));
    if (n == 0) return DIG_OK;                                         // (no key: every count is 0)
    DIG_REQUIRE(keys_sorted && n_valid, "non-null keys, n_valid");
    const TileWindowSampleArgs a{keys_sorted, n, n_valid, rows, R, T, sb, width, s_w};
    hipLaunchKernelGGL(tile_window_diff_kernel, dim3(blocks), dim3(kWinSampleBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    if (T % kWinScanItems == 0 && reinterpret_cast<uintptr_t>(s_w) % 16 == 0)
        hipLaunchKernelGGL(tile_window_scan_kernel<true>, dim3((unsigned)groups), dim3(kWinSampleBlock), 0, s, s_w, rows, T);
    else
        hipLaunchKernelGGL(tile_window_scan_kernel<false>, dim3((unsigned)groups), dim3(kWinSampleBlock), 0, s, s_w, rows, T);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
