// dig_panelcounts.hip -- the target route's panel bookkeeping for MANY cohorts: what stands behind the scale factor of targetDriver
// and the N_MUT_<panel> / N_MUT_SAMPLE_<panel> / N_SAMPLE_<panel> / N_MUT_CDS attributes of DigPretrain.py countMutations.
//
// Reference, per cohort and per panel, on the rows of read_mutation_file(drop_duplicates=True):
//   CohortRun.panel_scale     transfer_tools.py:905-935   rows (or distinct samples) of the samples that are not blacklisted whose ANNOT
//                                                         is none of Noncoding, Synonymous, Essential_Splice and whose GENE is in the panel
//   count_training_mutations  DigPretrain.py:103-177      the same rows without a blacklist: their number, their distinct (GENE, SAMPLE)
//                                                         pairs, their distinct samples; and the rows whose ANNOT is not Noncoding
// as an isin / groupby chain per panel per cohort.  Here a row is (label, sample, class, cohort), encoded on the host
// (tabulate_gpu.encode_panel_rows): label = the place of the row's GENE in a table of L genes (the union of the P <= 32 panels asked
// for; L = in no panel), label_mask u32 [L] has bit p set when the gene is in panel p, and the classes are those of the gene route
// with Noncoding apart: 0 SYN, 1 MIS, 2 NONS, 3 SPL, 4 INDEL, 5 any other label, 6 Noncoding.  Two kernels around one key sort:
//   panel_row_keys_kernel  one thread per row.  A row of a skipped (blacklisted) sample counts nowhere.  Of the others a row of class
//                          != 6 counts for n_cds (one add per run of consecutive lanes with one cohort), and a row of class 1, 2, 4
//                          or 5 whose label has a panel gets key = global sample << lb | label; every other row key -1.
//   -- the caller sorts the keys --
//   panel_counts_kernel    one thread per sorted key; the thread whose left neighbour has another key is the head of its (sample, label)
//                          run: the run's end is an upper-bound search (a run may span any number of workgroups; only its head looks at
//                          it) and the head adds the length to n_mut and 1 to n_pairs of every panel of its label.  DISTINCT SAMPLES: a
//                          sample's labels form many runs, one behind the other, and the sample counts once per panel in the OR of
//                          their masks -- the head of the sample's FIRST run walks the sample's label runs (one search each), ORs the
//                          masks and adds 1 to n_sample per bit.  No scratch and no second kernel; the walk is as long as the sample has
//                          distinct panel genes (at most L).
// Integer atomics only: the result does not depend on the order.  The masks are unsigned throughout (bit 31 is a panel like any other).
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kPanelBlock = 256;

__host__ __device__ __forceinline__ uint32_t panel_bits(int64_t P) { return P >= 32 ? 0xFFFFFFFFu : ((1u << (unsigned)P) - 1u); }

struct PanelKeyArgs {
    const int32_t *label, *sample, *cohort;
    const uint8_t* annot;
    const int64_t* sample_off;     // [C + 1]
    const uint8_t* skip;           // [n_samples] or NULL
    const uint32_t* label_mask;    // [L]
    int64_t n, L, C;
    uint32_t panels;               // the bits of the P panels
    int label_bits;
    int64_t* keys;                 // [n]
    unsigned long long* n_cds;     // [C]
};

__global__ __launch_bounds__(kPanelBlock) void panel_row_keys_kernel(PanelKeyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kPanelBlock + threadIdx.x;
    int64_t seg = -1;                              // the row's cohort; -1: no row here, a row outside the tables or of a skipped sample
    bool cds = false;
    if (i < a.n) {
        const int64_t c = a.cohort[i], lab = a.label[i], s = a.sample[i];
        const unsigned cls = a.annot[i];
        int64_t key = -1;                          // (a negative key: panel_counts_kernel passes over it)
        if (c >= 0 && c < a.C && lab >= 0 && lab <= a.L && cls <= 6u && s >= 0 && a.sample_off[c] + s < a.sample_off[c + 1]) {
            const int64_t gs = a.sample_off[c] + s;
            if (!(a.skip && a.skip[gs])) {
                seg = c;
                cds = cls != 6u;
                const bool counted = cls == 1u || cls == 2u || cls == 4u || cls == 5u;
                if (counted && lab < a.L && (a.label_mask[lab] & a.panels)) key = (gs << a.label_bits) | lab;
            }
        }
        a.keys[i] = key;
    }
    // one add per run of consecutive lanes with the same cohort
    const int rows = segment_count(seg, cds);
    if (rows) atomicAdd(&a.n_cds[seg], (unsigned long long)rows);
}

struct PanelCountArgs {
    const int64_t* keys;           // [n] ascending
    int64_t n;
    const uint32_t* label_mask;    // [L]
    const int64_t* sample_off;     // [C + 1]
    int64_t L, P, C, n_samples;
    uint32_t panels;
    int label_bits;
    unsigned long long *n_mut, *n_pairs, *n_sample;    // [C, P] each
};

__global__ __launch_bounds__(kPanelBlock) void panel_counts_kernel(PanelCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kPanelBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t key = a.keys[i];
    if (key < 0) return;
    const int64_t left = i > 0 ? a.keys[i - 1] : -1;
    if (left == key) return;                                          // not the head of its (sample, label) run
    const int64_t low = ((int64_t)1 << a.label_bits) - 1;
    const int64_t lab = key & low, gs = key >> a.label_bits;
    if (lab >= a.L || gs >= a.n_samples) return;                      // (keys that dig_panel_row_keys did not make)
    // the sample's cohort: the last c with sample_off[c] <= gs (cohorts without samples repeat an offset)
    int64_t lo = 0, hi = a.C;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a.sample_off[mid + 1] > gs)
            hi = mid;
        else
            lo = mid + 1;
    }
    if (lo >= a.C) return;
    const int64_t row = lo * a.P;
    const int64_t end = keys_upper_bound(a.keys, i + 1, a.n, key);
    const uint32_t mask = a.label_mask[lab] & a.panels;
    for (uint32_t m = mask; m; m &= m - 1u) {
        const int p = __ffs(m) - 1;
        atomicAdd(&a.n_mut[row + p], (unsigned long long)(end - i));
        atomicAdd(&a.n_pairs[row + p], 1ull);
    }
    if (left >= 0 && (left >> a.label_bits) == gs) return;            // not the sample's first run
    uint32_t seen = mask;
    int64_t pos = end;
    while (pos < a.n) {
        const int64_t k = a.keys[pos];
        if ((k >> a.label_bits) != gs) break;
        const int64_t l2 = k & low;
        if (l2 < a.L) seen |= a.label_mask[l2] & a.panels;
        pos = keys_upper_bound(a.keys, pos + 1, a.n, k);
    }
    for (uint32_t m = seen; m; m &= m - 1u) atomicAdd(&a.n_sample[row + (__ffs(m) - 1)], 1ull);
}

// the key's two fields must fit 63 bits
int panel_key_layout(const char* fn, int64_t L, int64_t P, int64_t C, int64_t n_samples, int* label_bits)
{
    DIG_REQUIRE_IN(fn, L >= 1 && L < ((int64_t)1 << 31), "L within [1, 2^31)");
    DIG_REQUIRE_IN(fn, P >= 1 && P <= 32, "P within [1, 32] (a panel is a bit of a 32-bit mask)");
    DIG_REQUIRE_IN(fn, C >= 1 && C < ((int64_t)1 << 31) && n_samples >= 0, "C within [1, 2^31), n_samples >= 0");
    *label_bits = key_bits_for(L);
    DIG_REQUIRE_IN(fn, n_samples < ((int64_t)1 << 62) && *label_bits + key_bits_for(n_samples) <= 63,
                   "the key (global sample, label) does not fit 63 bits: fewer cohorts per call");
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_panel_row_keys(const int32_t* label, const int32_t* sample, const uint8_t* annot, const int32_t* cohort, const int64_t* sample_off,
                       const uint8_t* skip, const uint32_t* label_mask, int64_t n, int64_t L, int64_t P, int64_t C, int64_t n_samples,
                       int64_t* keys, int64_t* n_cds, void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int lb = 0;
    if (int rc = panel_key_layout(__func__, L, P, C, n_samples, &lb)) return rc;
    DIG_REQUIRE(sample_off && label_mask && n_cds, "non-null sample_off, label_mask, n_cds");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(n_cds, 0, (size_t)C * sizeof(int64_t), s));
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(label && sample && annot && cohort && keys, "non-null pointers");
    const PanelKeyArgs a{label, sample, cohort, annot, sample_off, skip, label_mask, n, L, C, panel_bits(P), lb, keys,
                         reinterpret_cast<unsigned long long*>(n_cds)};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kPanelBlock, &blocks)) return rc;
    hipLaunchKernelGGL(panel_row_keys_kernel, dim3(blocks), dim3(kPanelBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_panel_counts(const int64_t* keys_sorted, int64_t n, const uint32_t* label_mask, const int64_t* sample_off, int64_t L, int64_t P,
                     int64_t C, int64_t n_samples, int64_t* n_mut, int64_t* n_pairs, int64_t* n_sample, void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int lb = 0;
    if (int rc = panel_key_layout(__func__, L, P, C, n_samples, &lb)) return rc;
    DIG_REQUIRE(sample_off && label_mask && n_mut && n_pairs && n_sample, "non-null pointers");
    hipStream_t s = (hipStream_t)stream;
    const size_t bytes = (size_t)C * P * sizeof(int64_t);
    DIG_HIP_TRY(hipMemsetAsync(n_mut, 0, bytes, s));
    DIG_HIP_TRY(hipMemsetAsync(n_pairs, 0, bytes, s));
    DIG_HIP_TRY(hipMemsetAsync(n_sample, 0, bytes, s));
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted, "non-null keys");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kPanelBlock, &blocks)) return rc;
    const PanelCountArgs a{keys_sorted, n, label_mask, sample_off, L, P, C, n_samples, panel_bits(P), lb,
                           reinterpret_cast<unsigned long long*>(n_mut), reinterpret_cast<unsigned long long*>(n_pairs),
                           reinterpret_cast<unsigned long long*>(n_sample)};
    hipLaunchKernelGGL(panel_counts_kernel, dim3(blocks), dim3(kPanelBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
