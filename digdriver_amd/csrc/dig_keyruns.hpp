// dig_keyruns.hpp -- what the counting routes (dig_genecounts.hip, dig_objectives.hip, dig_panelcounts.hip, dig_seqcounts.hip, dig_sitematch.hip, dig_tilehits.hip, dig_rowhits.hip, dig_tilesamples.hip, dig_tilesparse.hip, dig_tilesparsewindows.hip, dig_tilewindows.hip, dig_tilewindowsamples.hip, dig_cnvwindows.hip) and their host twins share:
// rows encoded as 63-bit keys, sorted by the caller, counted as runs with one integer atomic per wave segment.
#pragma once
#include "dig_common.hpp"

namespace dig {

// bits that hold the values 0 .. n - 1 (at least one)
inline int key_bits_for(int64_t n)
{
    int b = 1;
    while (b < 62 && ((int64_t)1 << b) < n) ++b;
    return b;
}

// dig_genecounts.hip: the bits of the global-sample field of a gene-count key; DIG_EINVAL (in the name of entry point `fn`) when
// (cohort (G + 2) + gene, global sample, class) does not fit 63 bits
int gene_key_layout(const char* fn, int64_t G, int64_t C, int64_t n_samples, int* sample_bits);

// dig_sitematch.hip: the bits of the global-sample field of a site-match key, (cohort E + element) << bits | global sample; DIG_EINVAL
// (in the name of entry point `fn`) when the two fields do not fit 63 bits
int site_key_layout(const char* fn, int64_t E, int64_t C, int64_t n_samples, int* sample_bits);

// dig_objectives.hip: the fields of a window-count key,
//   global sample << (window_bits + 1 + uid_bits) | window << (1 + uid_bits) | indel << uid_bits | mutation id;
// DIG_EINVAL (in the name of entry point `fn`) when they do not fit 63 bits
struct WindowKeyLayout {
    int uid_bits, window_bits;
};
int window_key_layout(const char* fn, int64_t n_samples, int64_t N, int64_t n_uid, WindowKeyLayout* lay);

// dig_panelcounts.hip: the bits of the label field of a panel-count key, global sample << bits | label; DIG_EINVAL (in the name of
// entry point `fn`) when the two fields do not fit 63 bits
int panel_key_layout(const char* fn, int64_t L, int64_t P, int64_t C, int64_t n_samples, int* label_bits);

// dig_tilehits.hip: the sizes of a score plane [C, R, T]; DIG_EINVAL (in the name of entry point `fn`) unless C R < 2^31 and T < 2^31
int tile_select_sizes(const char* fn, int64_t C, int64_t R, int64_t T);

// dig_rowhits.hip: the elements of a chunk of a score plane [rows, n] (dig_row_select_chunk), the size checks of its entry points
// and the chunks per row, ceil(n / kRowSelectChunk); DIG_EINVAL (in the name of entry point `fn`) unless rows, n >= 0, n < 2^31 and
// rows * chunks < 2^31
constexpr int kRowSelectChunk = 2048;
int row_select_sizes(const char* fn, int64_t rows, int64_t n, int64_t* chunks);

// dig_groupfisher.hip: the size checks of dig_group_fisher / dig_group_sums over planes [R, C, E] and M groups, and the chunks (one
// per workgroup) of a row; DIG_EINVAL (in the name of entry point `fn`) unless R, C, E, M >= 0, C <= 64, M <= 32, E < 2^31 and
// R * chunks < 2^31
int group_sizes(const char* fn, int64_t R, int64_t C, int64_t E, int64_t M, int64_t* chunks);

// dig_nbpower.hip: what dig_nb_power and its host twin check without looking at an array (include/dig_hip.h lists it), and the chunks
// (one per workgroup) of a row
int nb_power_sizes(const char* fn, int64_t rows, int64_t n, const double* folds, int n_folds, int32_t k_max, const double* power,
                   int64_t* chunks);

// dig_pairs.hip: what dig_pair_bits, dig_pair_fisher / dig_pair_counts and their host twins check without looking at an array
// (include/dig_hip.h lists it); the workgroups of dig_pair_bits
int pair_bits_sizes(const char* fn, int64_t n_keys, int64_t H_total, int64_t W, const void* bits, unsigned* blocks);
int pair_fisher_sizes(const char* fn, const void* bits, int64_t H_total, int64_t W, int64_t C, int64_t n_tiles, int64_t n_pairs,
                      int32_t n_max, int32_t h_max);

// dig_mapreport.hip: what dig_map_windows / dig_map_scores and their host twins check without looking at an array (include/dig_hip.h
// lists it); the windows of a group (one group of neighbouring windows of a cohort at a time per workgroup) and the groups of a
// cohort; the chunks (one per workgroup) of a cohort's windows
struct MapWindowPlan {
    int wpb;
    int64_t groups;
};
int map_windows_sizes(const char* fn, int64_t C, int64_t N, int64_t M, int drop_flagged, int tail, const void* flag_cm, MapWindowPlan* plan);
int map_scores_sizes(const char* fn, int64_t C, int64_t M, int64_t* chunks);

// dig_tilewindows.hip: tile_select_sizes and 1 <= width <= DIG_TILE_WINDOW_MAX_WIDTH, for dig_tile_window_test and its host twin
int tile_window_sizes(const char* fn, int64_t C, int64_t R, int64_t T, int32_t width);

// dig_tilesamples.hip: the bits of the global-sample field of a tile-sample key, ((cohort R + region) T + tile) << bits | global sample
// (bits for n_samples + 1 values: the all-ones key is no real one); DIG_EINVAL (in the name of entry point `fn`) when the tile field
// is refused by sparse_tile_slots or the two fields do not fit 63 bits
int tile_sample_key_layout(const char* fn, int64_t C, int64_t R, int64_t T, int64_t n_samples, int* sample_bits);

// dig_tilesparse.hip: the slots C R T of a sparse-scan key, (cohort R + region) T + tile; DIG_EINVAL (in the name of entry point `fn`)
// unless C, R, T < 2^31 and the product fits 62 bits.  tile_census_workspace_bytes: what dig_tile_census_workspace returns
int sparse_tile_slots(const char* fn, int64_t C, int64_t R, int64_t T, int64_t* slots);
int64_t tile_census_workspace_bytes(int64_t C, int n_up);

// dig_tilesparsewindows.hip: tile_window_sizes and sparse_tile_slots, for the three sparse-window entry points and their host twins
int sparse_window_sizes(const char* fn, int64_t C, int64_t R, int64_t T, int32_t width, int64_t* slots);

// dig_cnvwindows.hip: the rows (3 C) and chunks (of DIG_CNV_SCAN_CHUNK windows) of the copy-number difference array i64 [C, 3, N + 1], its
// bytes (dig_cnv_segment_deltas_size) and those of the chunk carries i64 [3 C, chunks] (dig_cnv_window_means_size); DIG_EINVAL (in the
// name of entry point `fn`) unless 1 <= C < 2^20, 0 <= N < 2^31, 1 <= W < 2^31 and 3 C (N + 1) < 2^40
struct CnvSizes {
    int64_t rows, chunks, delta_bytes, carry_bytes;
};
int cnv_sizes(const char* fn, int64_t C, int64_t N, int64_t W, CnvSizes* sz);

// dig_seqcounts.hip: the most table rows K a call takes -- a workgroup's LDS counters, 12 KB: the penta-nucleotide table
constexpr int kSeqMaxK = 3072;

// the grid of a kernel with one thread per row: a grid dimension stays below 2^31
inline int row_blocks(const char* fn, int64_t n, int block, unsigned* blocks)
{
    const int64_t b = (n + block - 1) / block;
    DIG_REQUIRE_IN(fn, b < ((int64_t)1 << 31), "fewer than 2^39 rows or pairs");
    *blocks = (unsigned)b;
    return DIG_OK;
}

// One past the last lane (64 at most) of the segment that lane `lane` begins, from two ballots of the wave: `firsts`, the lanes
// that begin a segment, and `rows`, the lanes that belong to one.  It ends at the next first lane or at the next lane outside `rows`,
// whichever comes first.  No ballot of its own: the caller's ballots are what every lane of the wave must reach.
__device__ __forceinline__ int segment_end(unsigned long long firsts, unsigned long long rows, int lane)
{
    const unsigned long long above = lane == 63 ? 0ull : ~0ull << (lane + 1);
    const unsigned long long stop = (firsts | ~rows) & above;
    return stop ? __ffsll((long long)stop) - 1 : 64;
}

// The lanes of a wave form segments: maximal runs of consecutive lanes with the same seg >= 0 (seg < 0: a lane without a
// destination).  On the first lane of a segment: the number of lanes of the segment with `flag`; on every other lane 0.
// Every lane of the wave must call it.
__device__ __forceinline__ int segment_count(int64_t seg, bool flag)
{
    const int lane = threadIdx.x & 63;
    const int64_t left = __shfl_up((long long)seg, 1, 64);
    const bool first = seg >= 0 && (lane == 0 || left != seg);
    const unsigned long long firsts = __ballot(first), rows = __ballot(seg >= 0), flags = __ballot(flag && seg >= 0);
    if (!first) return 0;
    const int end = segment_end(firsts, rows, lane);
    const unsigned long long mine = (end == 64 ? ~0ull : ((1ull << end) - 1)) & ~((1ull << lane) - 1);      // the lanes [lane, end)
    return __popcll(flags & mine);
}

// segment_count with a value per lane: on the first lane of a segment the sum of `value` over the segment's lanes; on every other
// lane 0.  A suffix sum in six shuffle steps that never crosses a segment's end.  Every lane of the wave must call it.
__device__ __forceinline__ int segment_sum(int64_t seg, int value)
{
    const int lane = threadIdx.x & 63;
    const int64_t left = __shfl_up((long long)seg, 1, 64);
    const bool first = seg >= 0 && (lane == 0 || left != seg);
    const int end = segment_end(__ballot(first), __ballot(seg >= 0), lane);
    int v = seg >= 0 ? value : 0;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        const int other = __shfl_down(v, d, 64);      // after the step v covers the lanes [lane, min(lane + 2 d, end))
        if (lane + d < end) v += other;
    }
    return first ? v : 0;
}

// first index in [lo, n) whose key is above v (keys ascending, keys[lo - 1] == v)
__device__ __forceinline__ int64_t keys_upper_bound(const int64_t* keys, int64_t lo, int64_t n, int64_t v)
{
    int64_t hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (keys[mid] > v)
            hi = mid;
        else
            lo = mid + 1;
    }
    return lo;
}

// One thread per sorted key (key = keys[i]; row: the key counts; head: it counts and keys[i - 1] -- read from global memory: it may lie
// in the previous wave or workgroup -- is another key).  On a head: the length of its run of equal keys; on every other lane 0.  The
// run ends inside the wave at the next head or the next lane without a row; only one that reaches the wave's last lane looks further:
// one load tells whether it goes on at all, then keys_upper_bound.  Every lane of the wave must call it.
__device__ __forceinline__ int64_t run_length(const int64_t* keys, int64_t n, int64_t i, int64_t key, bool head, bool row)
{
    const int lane = threadIdx.x & 63;
    const unsigned long long heads = __ballot(head), rows = __ballot(row);
    if (!head) return 0;
    const int end = segment_end(heads, rows, lane);
    int64_t len = end - lane;
    if (end == 64 && i + len < n && keys[i + len] == key) len = keys_upper_bound(keys, i + len + 1, n, key) - i;
    return len;
}

}  // namespace dig
