// dig_tilesamples.hip -- the per-base route's counts BY SAMPLE for many cohorts: what stands behind --max-muts-per-sample,
// --max-muts-per-tile-per-sample and --by-sample of tileDriver.
//
// dig_tile_mut_counts (dig_tiles.hip) counts rows: OBS of a tile is the number of rows whose START falls in it, whoever they belong
// to, so one sample with a cluster of mutations makes a tile a hit by itself.  The reference has no per-base form of its sample
// guards; the definitions here are the project's, modelled on filter_hypermut_samples, cap_muts_per_element_per_sample
// (mutation_tools.py:293-327) and element_pvalue_burden_nb_by_sample (transfer_tools.py:594-615).  With n(c, r, t, s) the rows of
// sample s that dig_tile_mut_counts counts in tile (c, r, t):
//   k_cap[c, r, t]     = sum over the kept samples of min(n, cap)            (cap <= 0: no cap, the sum of n)
//   k_samples[c, r, t] = the kept samples with n > 0
// Two kernels around one key sort:
//   tile_sample_keys_kernel    one thread per (mutation, region) pair of the interval join.  The tile is tile_mut_counts_kernel's
//                              (tile_slot, dig_tiles.hpp), then the sample (outside [0, n_samples), or keep[sample] == 0).  A pair
//                              that counts gets key = (((cohort R + region) T + tile) << sb) | global sample; every other pair the
//                              all-ones 63-bit key, which sorts behind every real one.
//   -- the caller sorts the keys --
//   tile_sample_counts_kernel  one thread per sorted key.  A run of equal keys is one (tile, sample) with n = its length.  The thread
//                              whose left neighbour -- read from global memory: it may lie in the previous wave or workgroup -- has
//                              another key is the run's head; it alone carries min(n, cap) and the 1 of its sample (n: run_length,
//                              dig_keyruns.hpp).  The heads' values are
//                              added up per tile inside the wave (segment_sum, segment_count) and leave as one integer atomic per
//                              plane, wave segment and tile: a tile that one sample hits with thousands of rows costs one atomic.
// Integer atomics only: the result does not depend on the order.
#include "dig_keyruns.hpp"
#include "dig_tiles.hpp"

namespace dig {

constexpr int kTileSampleBlock = 256;
constexpr int64_t kTileSampleNoKey = INT64_MAX;      // the all-ones 63-bit key: a pair that counts nowhere

// the key's two fields must fit 63 bits; the sample field has room for n_samples + 1 values, so that no real key is all ones
int tile_sample_key_layout(const char* fn, int64_t C, int64_t R, int64_t T, int64_t n_samples, int* sample_bits)
{
    DIG_REQUIRE_IN(fn, C >= 0 && R >= 0 && T >= 0 && n_samples >= 0, "C, R, n_tiles, n_samples >= 0");
    const int64_t lim = (int64_t)1 << 31;
    DIG_REQUIRE_IN(fn, C < lim && R < lim && T < lim && n_samples < lim, "C, R, n_tiles and the sample count below 2^31");
    int64_t slots = 0;
    if (int rc = sparse_tile_slots(fn, C, R, T, &slots)) return rc;
    *sample_bits = key_bits_for(n_samples + 1);
    DIG_REQUIRE_IN(fn, key_bits_for(slots) + *sample_bits <= 63,
                   "the key (cohort, region, tile, global sample) does not fit 63 bits: fewer cohorts or regions per call");
    return DIG_OK;
}

struct TileSampleKeyArgs {
    const int32_t *pair_mut, *pair_reg;              // [n_pairs]
    int64_t n_pairs;
    const int64_t* mut_start;                        // [n_mut]
    const int32_t *mut_cohort, *mut_sample;          // [n_mut]: cohort, GLOBAL sample
    int64_t n_mut;
    const uint8_t* keep;                             // [n_samples] or NULL: every sample stays
    const int64_t* first_pos;                        // [R]
    const int32_t* n_valid;                          // [R]
    int binsize;
    int64_t n_tiles, R, C, n_samples;
    int sample_bits;
    int64_t* keys;                                   // [n_pairs]
};

__global__ __launch_bounds__(kTileSampleBlock) void tile_sample_keys_kernel(TileSampleKeyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kTileSampleBlock + threadIdx.x;
    if (i >= a.n_pairs) return;
    const int64_t m = a.pair_mut[i], r = a.pair_reg[i];
    int64_t key = kTileSampleNoKey;
    if ((uint64_t)m < (uint64_t)a.n_mut && (uint64_t)r < (uint64_t)a.R) {        // (a pair outside the tables reads nothing)
        const int64_t slot = tile_slot(a.mut_start[m], a.mut_cohort[m], a.first_pos[r], a.n_valid[r], a.binsize, a.n_tiles, a.R, a.C, r);
        if (slot >= 0) {
            const int64_t s = a.mut_sample[m];
            if ((uint64_t)s < (uint64_t)a.n_samples && !(a.keep && a.keep[s] == 0)) key = (slot << a.sample_bits) | s;
        }
    }
    a.keys[i] = key;
}

struct TileSampleCountArgs {
    const int64_t* keys;                             // [n] ascending
    int64_t n, slots;                                // slots = C R T
    int sample_bits;
    int64_t cap;                                     // <= 0: no cap
    int32_t *k_cap, *k_samples;                      // [C, R, T] each, or NULL
};

__global__ __launch_bounds__(kTileSampleBlock) void tile_sample_counts_kernel(TileSampleCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kTileSampleBlock + threadIdx.x;
    int64_t slot = -1, key = -1;                     // slot: the tile, (cohort R + region) T + tile; -1: no key here, or one that counts nowhere
    bool head = false;
    if (i < a.n) {
        key = a.keys[i];
        if (key >= 0 && key != kTileSampleNoKey && (key >> a.sample_bits) < a.slots) {
            slot = key >> a.sample_bits;
            head = i == 0 || a.keys[i - 1] != key;
        }
    }
    const int64_t len = run_length(a.keys, a.n, i, key, head, slot >= 0);
    const int value = (int)(a.cap > 0 && len > a.cap ? a.cap : len);
    const int samples = segment_count(slot, head), capped = segment_sum(slot, value);
    if (!samples) return;                            // (a segment without a head: the tail of a run that another wave counts)
    if (a.k_cap) atomicAdd(&a.k_cap[slot], capped);
    if (a.k_samples) atomicAdd(&a.k_samples[slot], samples);
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_tile_sample_keys(const int32_t* pair_mut, const int32_t* pair_reg, int64_t n_pairs, const int64_t* mut_start, int64_t n_mut,
                         const int32_t* mut_cohort, const int32_t* mut_sample, const uint8_t* keep, const int64_t* first_pos,
                         const int32_t* n_valid, int binsize, int64_t n_tiles, int64_t R, int64_t C, int64_t n_samples, int64_t* keys,
                         void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && n_mut >= 0 && binsize >= 1, "n_pairs, n_mut >= 0, binsize >= 1");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, n_tiles, n_samples, &sb)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(pair_mut && pair_reg && keys, "non-null pair arrays, keys");
    DIG_REQUIRE(n_mut == 0 || (mut_start && mut_cohort && mut_sample), "non-null mutation arrays");
    DIG_REQUIRE(R == 0 || (first_pos && n_valid), "non-null region tables");
    const TileSampleKeyArgs a{pair_mut, pair_reg, n_pairs, mut_start, mut_cohort, mut_sample, n_mut, keep, first_pos, n_valid, binsize,
                              n_tiles, R, C, n_samples, sb, keys};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_pairs, kTileSampleBlock, &blocks)) return rc;
    hipLaunchKernelGGL(tile_sample_keys_kernel, dim3(blocks), dim3(kTileSampleBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_tile_sample_counts(const int64_t* keys_sorted, int64_t n, int64_t C, int64_t R, int64_t n_tiles, int64_t n_samples, int64_t cap,
                           int32_t* k_cap, int32_t* k_samples, void* stream)
{
    DIG_REQUIRE(n >= 0 && n <= INT32_MAX, "0 <= n < 2^31 (the counts are 32-bit)");
    int sb = 0;
    if (int rc = tile_sample_key_layout(__func__, C, R, n_tiles, n_samples, &sb)) return rc;
    const int64_t slots = C * R * n_tiles;
    if (slots == 0) return DIG_OK;
    hipStream_t s = (hipStream_t)stream;
    if (k_cap) DIG_HIP_TRY(hipMemsetAsync(k_cap, 0, (size_t)slots * sizeof(int32_t), s));
    if (k_samples) DIG_HIP_TRY(hipMemsetAsync(k_samples, 0, (size_t)slots * sizeof(int32_t), s));
    if (n == 0 || (!k_cap && !k_samples)) return DIG_OK;
    DIG_REQUIRE(keys_sorted, "non-null keys");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kTileSampleBlock, &blocks)) return rc;
    const TileSampleCountArgs a{keys_sorted, n, slots, sb, cap, k_cap, k_samples};
    hipLaunchKernelGGL(tile_sample_counts_kernel, dim3(blocks), dim3(kTileSampleBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
