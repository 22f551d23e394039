// dig_objectives.hip -- the training labels of the region model for MANY cohorts: mutation counts per window of the data
// container's `idx`, the integer bookkeeping behind the interval join (dig_overlap_join_*) of all cohorts' rows with the windows.
//
// Reference, per cohort (scripts/DataExtractor.py:525-572 add_objectives without --cnv):
//   tabulate_muts_per_sample_per_element(bed12=False, drop_duplicates=True)   mutation_tools.py:191-230   joined rows, unique on
//                                      (chrom, start, end, ref, alt, sample, window), counted per (window, sample) as SNV / INDEL
//   filter_samples_by_stdev            :306-316   a sample's load is its number of (window, sample) ROWS = distinct windows it hits
//   filter_hypermut_samples            :293-304   the same load against a plain limit
//   pivot / merge                      DataExtractor.py:559-562   label[window] = sum of OBS_SNV over the samples that stay
// Here a joined pair is one 63-bit key, (global sample, window, indel bit, mutation id) from the high end -- the global sample
// holds the cohort: sample_off [C + 1] -- and the chain is three kernels around one key sort by the caller:
//   window_pair_keys_kernel      one thread per pair: the key, -1 for a pair outside the tables
//   window_sample_hits_kernel    one thread per sorted key; a key whose left neighbour has another (sample, window) opens a window
//                                of its sample: hits[sample] += 1.  Equal keys lie together, so duplicates add nothing.
//   -- the caller forms the keep bytes from hits (pandas' Series.std() per cohort: the threshold's bits stay the reference's) --
//   window_objectives_kernel     one thread per sorted key; a key counts when its indel bit is clear, its left neighbour is another
//                                key (the de-duplication) and its sample is kept: labels[window, cohort] += 1
//   window_labels_f64_kernel     int32 -> float64, the dtype the reference stores
// Both counting kernels sum their flags over the consecutive lanes of a wave that share the destination (segment_count of
// dig_keyruns.hpp: three ballots and a population count) and issue one integer atomic per segment.  A run is never walked or searched:
// a run of 700 keys is eleven wave segments, each lane does O(1) work wherever the run starts or ends, and a run that spans
// waves or workgroups simply adds once per wave.  Integer atomics only: the result does not depend on the order.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kObjBlock = 256;

// the key's four fields must fit 63 bits
int window_key_layout(const char* fn, int64_t n_samples, int64_t N, int64_t n_uid, WindowKeyLayout* lay)
{
    DIG_REQUIRE_IN(fn, n_samples >= 0 && N >= 0 && n_uid >= 0, "n_samples, N, n_uid >= 0");
    DIG_REQUIRE_IN(fn, n_samples < ((int64_t)1 << 31) && N < ((int64_t)1 << 31) && n_uid < ((int64_t)1 << 31),
                   "the sample, window and mutation-id counts below 2^31");
    lay->uid_bits = key_bits_for(n_uid);
    lay->window_bits = key_bits_for(N);
    DIG_REQUIRE_IN(fn, key_bits_for(n_samples) + lay->window_bits + 1 + lay->uid_bits <= 63,
                   "the key (global sample, window, indel bit, mutation id) does not fit 63 bits: fewer cohorts per call");
    return DIG_OK;
}

struct WindowKeyArgs {
    const int32_t *pair_row, *pair_blk;     // [P]
    const int32_t* blk_window;              // [n_blk], or null: the block row is the window
    const int32_t *row_sample, *row_uid;    // [n_rows]: global sample, mutation id
    const uint8_t* row_indel;               // [n_rows]
    int64_t P, n_rows, n_blk, n_samples, N, n_uid;
    WindowKeyLayout lay;
    int64_t* keys;                          // [P]
};

__global__ __launch_bounds__(kObjBlock) void window_pair_keys_kernel(WindowKeyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kObjBlock + threadIdx.x;
    if (i >= a.P) return;
    const int64_t r = a.pair_row[i], b = a.pair_blk[i];
    int64_t key = -1;                       // (a negative key: the counting kernels pass over it)
    if (r >= 0 && r < a.n_rows && b >= 0 && b < a.n_blk) {
        const int64_t w = a.blk_window ? a.blk_window[b] : b, s = a.row_sample[r], u = a.row_uid[r];
        if (w >= 0 && w < a.N && s >= 0 && s < a.n_samples && u >= 0 && u < a.n_uid)
            key = (((s << a.lay.window_bits) | w) << (1 + a.lay.uid_bits)) | ((int64_t)(a.row_indel[r] != 0) << a.lay.uid_bits) | u;
    }
    a.keys[i] = key;
}

struct WindowCountArgs {
    const int64_t* keys;            // [P] ascending
    int64_t P, n_samples, N, C;
    WindowKeyLayout lay;
    const uint8_t* keep;            // [n_samples]      (objectives)
    const int64_t* sample_off;      // [C + 1]          (objectives)
    int32_t* out;                   // hits [n_samples] | labels [N, C]
};

__global__ __launch_bounds__(kObjBlock) void window_sample_hits_kernel(WindowCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kObjBlock + threadIdx.x;
    const int pair_shift = 1 + a.lay.uid_bits;
    int64_t s = -1;
    bool opens = false;
    if (i < a.P) {
        const int64_t key = a.keys[i];
        if (key >= 0) {
            const int64_t pair = key >> pair_shift;
            s = pair >> a.lay.window_bits;
            if (s >= a.n_samples) s = -1;                                   // (keys that dig_window_pair_keys did not make)
            opens = i == 0 || (a.keys[i - 1] >> pair_shift) != pair;        // (a negative left neighbour shifts to a negative value)
        }
    }
    const int n = segment_count(s, opens);
    if (n) atomicAdd(&a.out[s], n);
}

__global__ __launch_bounds__(kObjBlock) void window_objectives_kernel(WindowCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kObjBlock + threadIdx.x;
    const int pair_shift = 1 + a.lay.uid_bits;
    int64_t pair = -1;
    bool counts = false;
    if (i < a.P) {
        const int64_t key = a.keys[i];
        if (key >= 0) {
            pair = key >> pair_shift;
            const int64_t s = pair >> a.lay.window_bits, w = pair & (((int64_t)1 << a.lay.window_bits) - 1);
            if (s >= a.n_samples || w >= a.N)
                pair = -1;
            else
                counts = !((key >> a.lay.uid_bits) & 1) && (i == 0 || a.keys[i - 1] != key) && a.keep[s] != 0;
        }
    }
    const int n = segment_count(pair, counts);
    if (!n) return;
    const int64_t s = pair >> a.lay.window_bits, w = pair & (((int64_t)1 << a.lay.window_bits) - 1);
    // the sample's cohort: the last c with sample_off[c] <= s
    int64_t lo = 0, hi = a.C;
    while (hi - lo > 1) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.sample_off[mid] <= s)
            lo = mid;
        else
            hi = mid;
    }
    atomicAdd(&a.out[w * a.C + lo], n);
}

__global__ __launch_bounds__(kObjBlock) void window_labels_f64_kernel(const int32_t* counts, double* labels, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * kObjBlock;
    for (int64_t i = (int64_t)blockIdx.x * kObjBlock + threadIdx.x; i < n; i += stride) labels[i] = (double)counts[i];
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_window_pair_keys(const int32_t* pair_row, const int32_t* pair_blk, int64_t n_pairs, const int32_t* blk_window, int64_t n_blk,
                         const int32_t* row_sample, const int32_t* row_uid, const uint8_t* row_indel, int64_t n_rows,
                         int64_t n_samples, int64_t N, int64_t n_uid, int64_t* keys, void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && n_blk >= 0 && n_rows >= 0, "n_pairs, n_blk, n_rows >= 0");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(pair_row && pair_blk && row_sample && row_uid && row_indel && keys, "non-null pointers");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_pairs, kObjBlock, &blocks)) return rc;
    const WindowKeyArgs a{pair_row, pair_blk, blk_window, row_sample, row_uid, row_indel, n_pairs, n_rows, n_blk, n_samples, N, n_uid,
                          lay, keys};
    hipLaunchKernelGGL(window_pair_keys_kernel, dim3(blocks), dim3(kObjBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_window_sample_hits(const int64_t* keys_sorted, int64_t n_pairs, int64_t n_samples, int64_t N, int64_t n_uid, int32_t* hits,
                           void* stream)
{
    DIG_REQUIRE(n_pairs >= 0, "n_pairs >= 0");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    DIG_REQUIRE(n_samples == 0 || hits, "non-null hits");
    hipStream_t s = (hipStream_t)stream;
    if (n_samples) DIG_HIP_TRY(hipMemsetAsync(hits, 0, (size_t)n_samples * sizeof(int32_t), s));
    if (n_pairs == 0 || n_samples == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted, "non-null keys");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_pairs, kObjBlock, &blocks)) return rc;
    const WindowCountArgs a{keys_sorted, n_pairs, n_samples, N, 1, lay, nullptr, nullptr, hits};
    hipLaunchKernelGGL(window_sample_hits_kernel, dim3(blocks), dim3(kObjBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_window_objectives(const int64_t* keys_sorted, int64_t n_pairs, const uint8_t* keep, const int64_t* sample_off, int64_t n_samples,
                          int64_t N, int64_t C, int64_t n_uid, double* labels, int32_t* scratch, void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && C >= 1, "n_pairs >= 0, C >= 1");
    WindowKeyLayout lay;
    if (int rc = window_key_layout(__func__, n_samples, N, n_uid, &lay)) return rc;
    DIG_REQUIRE(N < ((int64_t)1 << 62) / C, "N C below 2^62");
    const int64_t NC = N * C;
    if (NC == 0) return DIG_OK;
    DIG_REQUIRE(labels && scratch && sample_off && (n_samples == 0 || keep), "non-null pointers");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(scratch, 0, (size_t)NC * sizeof(int32_t), s));
    if (n_pairs && n_samples) {
        DIG_REQUIRE(keys_sorted, "non-null keys");
        unsigned blocks = 0;
        if (int rc = row_blocks(__func__, n_pairs, kObjBlock, &blocks)) return rc;
        const WindowCountArgs a{keys_sorted, n_pairs, n_samples, N, C, lay, keep, sample_off, scratch};
        hipLaunchKernelGGL(window_objectives_kernel, dim3(blocks), dim3(kObjBlock), 0, s, a);
        DIG_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(window_labels_f64_kernel, dim3(grid_for(NC, kObjBlock, 8)), dim3(kObjBlock), 0, s, scratch, labels, NC);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
