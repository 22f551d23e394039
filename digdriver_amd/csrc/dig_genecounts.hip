// dig_genecounts.hip -- the gene route's observed counts for MANY cohorts: the integer bookkeeping in front of dig_gene_stats.
//
// Reference, per cohort, on the coding rows (GENE != '.') of the mutation file:
//   filter_hypermut_samples  mutation_tools.py:293-304   drop every row of a sample with more than max_muts_per_sample rows
//   mutations_per_gene       mutation_tools.py:329-361   rows per (GENE, SAMPLE, ANNOT), clipped to max_muts_per_gene_per_sample,
//                                                        summed per (GENE, ANNOT) -> OBS_SYN, MIS, NONS, SPL, INDEL
//   transfer_gene_model      transfer_tools.py:196-270   N_SAMP_c: distinct (GENE, SAMPLE) pairs with a row of class c
//   the synonymous scale     transfer_tools.py:809-823   the number of Synonymous rows outside TP53 (genes outside the model count)
// as a group-by / pivot / merge chain in pandas.  Here a row is (gene id, sample id, annotation class, cohort), encoded on the host
// (tabulate_gpu.encode_gene_rows), and the chain is two kernels around one key sort:
//   gene_row_keys_kernel     one thread per row: key = (cohort (G + 2) + gene) << (sb + 3) | global sample << 3 | class, and + 1 on
//                            the sample's row total (consecutive lanes with one sample add once: files list a sample's rows together)
//   -- the caller sorts the keys (torch.sort on the device, the host twin's caller on the host: dig_bh_qvalues_sorted's precedent) --
//   gene_counts_kernel       one thread per sorted key; the thread whose left neighbour has another (slot, sample) is the head of
//                            that run.  A head whose sample is over the limit emits nothing; otherwise it walks the at most six
//                            class sub-runs -- each end is an upper-bound binary search in the sorted keys, O(log n) however long
//                            the run, and a run may span any number of workgroups: only its head looks at it -- and adds to the
//                            integer planes.  Integer atomics only: the result does not depend on the order.
//   gene_counts_finish_kernel  the per-(gene, sample) cap.  The reference clips the group size to the FLOAT cap, sums, and casts to
//                            int: a clipped sub-run is counted in a scratch plane instead of added, and here
//                            obs = (int)(sum of the unclipped sizes + clipped * cap) -- the reference's sum for an integer cap, and
//                            for a fractional one up to the rounding of its running float sum.  Also the blacklist bytes.
// Gene ids: 0 .. G - 1 the model's rows, G any gene outside the model, G + 1 TP53 when the model has no TP53 row (so that it can be
// left out of the synonymous count).  Classes: 0 SYN, 1 MIS, 2 NONS, 3 SPL, 4 INDEL, 5 anything else.  Rows of genes outside the
// model and of class 5 count for the sample totals (and class 0 ones for n_syn); the observed-count planes never see them.
#include <algorithm>

#include "dig_keyruns.hpp"

namespace dig {

constexpr int kGeneCountBlock = 256;

struct GeneKeyArgs {
    const int32_t *gene, *sample, *cohort;
    const uint8_t* annot;
    const int64_t* sample_off;     // [C + 1]
    int64_t n, G, C;
    int sample_bits;
    int64_t* keys;                 // [n]
    int32_t* sample_total;         // [n_samples]
};

__global__ __launch_bounds__(kGeneCountBlock) void gene_row_keys_kernel(GeneKeyArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kGeneCountBlock + threadIdx.x;
    int gs = -1;                                   // the row's global sample; -1: no row here, or a row outside the tables
    if (i < a.n) {
        const int64_t c = a.cohort[i], g = a.gene[i], s = a.sample[i];
        const unsigned cls = a.annot[i];
        int64_t key = -1;                          // (a negative key: gene_counts_kernel passes over it)
        if (c >= 0 && c < a.C && g >= 0 && g <= a.G + 1 && cls <= 5u && s >= 0 && a.sample_off[c] + s < a.sample_off[c + 1]) {
            gs = (int)(a.sample_off[c] + s);
            key = ((c * (a.G + 2) + g) << (a.sample_bits + 3)) | ((int64_t)gs << 3) | (int64_t)cls;
        }
        a.keys[i] = key;
    }
    // one add per run of consecutive lanes with the same sample
    const int rows = segment_count(gs, gs >= 0);
    if (rows) atomicAdd(&a.sample_total[gs], rows);
}

struct GeneCountArgs {
    const int64_t* keys;           // [n] ascending
    int64_t n;
    const int32_t* sample_total;   // [n_samples]
    int64_t n_samples;
    double max_per_sample, cap;
    int64_t G, C, tp53;
    int sample_bits;
    int32_t *obs, *n_samp, *extra, *capped;    // [G, 5, C], [G, 6, C], [G, 2, C], [G, 5, C]
    unsigned long long* n_syn;     // [C]
};

__global__ __launch_bounds__(kGeneCountBlock) void gene_counts_kernel(GeneCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kGeneCountBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t key = a.keys[i];
    if (key < 0) return;
    const int64_t pair = key >> 3;
    if (i > 0 && (a.keys[i - 1] >> 3) == pair) return;               // not the head of its (slot, sample) run
    const int64_t gs = pair & (((int64_t)1 << a.sample_bits) - 1), slot = pair >> a.sample_bits;
    const int64_t c = slot / (a.G + 2), g = slot - c * (a.G + 2);
    if (c >= a.C || gs >= a.n_samples) return;                        // (keys that dig_gene_row_keys did not make)
    if ((double)a.sample_total[gs] > a.max_per_sample) return;        // filter_hypermut_samples: `>`
    unsigned has = 0;
    int64_t pos = i;
    for (int step = 0; step < 6 && pos < a.n; ++step) {
        const int64_t k = a.keys[pos];
        if ((k >> 3) != pair) break;
        const int cls = (int)(k & 7);
        const int64_t end = keys_upper_bound(a.keys, pos + 1, a.n, k), len = end - pos;
        has |= 1u << cls;
        if (g < a.G && cls < 5) {
            const int64_t at = (g * 5 + cls) * a.C + c;
            if ((double)len > a.cap)
                atomicAdd(&a.capped[at], 1);
            else
                atomicAdd(&a.obs[at], (int)len);
        }
        if (cls == 0 && g != a.tp53) atomicAdd(&a.n_syn[c], (unsigned long long)len);
        pos = end;
    }
    if (g >= a.G) return;
    // distinct (GENE, SAMPLE) pairs per class: SYN, MIS, NONS, SPL, TRUNC = {NONS, SPL}, NONSYN = {MIS, NONS, SPL}; INDEL; any
    const unsigned cls6 = (has & 15u) | ((has & 12u) ? 16u : 0u) | ((has & 14u) ? 32u : 0u);
    for (int q = 0; q < 6; ++q)
        if (cls6 & (1u << q)) atomicAdd(&a.n_samp[(g * 6 + q) * a.C + c], 1);
    if (has & 16u) atomicAdd(&a.extra[(g * 2 + 0) * a.C + c], 1);
    atomicAdd(&a.extra[(g * 2 + 1) * a.C + c], 1);
}

__global__ __launch_bounds__(kGeneCountBlock) void gene_counts_finish_kernel(int32_t* obs, const int32_t* capped, int64_t n_obs, double cap,
                                                                             const int32_t* sample_total, uint8_t* blacklisted,
                                                                             int64_t n_samples, double max_per_sample)
{
    const int64_t stride = (int64_t)gridDim.x * kGeneCountBlock;
    for (int64_t i = (int64_t)blockIdx.x * kGeneCountBlock + threadIdx.x; i < n_obs || i < n_samples; i += stride) {
        if (i < n_obs && capped[i]) obs[i] = (int32_t)((double)obs[i] + (double)capped[i] * cap);
        if (i < n_samples) blacklisted[i] = (double)sample_total[i] > max_per_sample;
    }
}

// the key's three fields must fit 63 bits
int gene_key_layout(const char* fn, int64_t G, int64_t C, int64_t n_samples, int* sample_bits)
{
    DIG_REQUIRE_IN(fn, G >= 0 && C >= 1 && n_samples >= 0, "G >= 0, C >= 1, n_samples >= 0");
    DIG_REQUIRE_IN(fn, G < ((int64_t)1 << 31) - 2 && C < ((int64_t)1 << 31) && n_samples < ((int64_t)1 << 31),
                   "G + 2, C and the sample count below 2^31");
    *sample_bits = key_bits_for(n_samples);
    DIG_REQUIRE_IN(fn, key_bits_for(C * (G + 2)) + *sample_bits + 3 <= 63,
                   "the key (cohort (G + 2) + gene, global sample, class) does not fit 63 bits: fewer cohorts per call");
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_gene_row_keys(const int32_t* gene, const int32_t* sample, const uint8_t* annot, const int32_t* cohort, const int64_t* sample_off,
                      int64_t n, int64_t G, int64_t C, int64_t n_samples, int64_t* keys, int32_t* sample_total, void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int sb = 0;
    if (int rc = gene_key_layout(__func__, G, C, n_samples, &sb)) return rc;
    DIG_REQUIRE(sample_off && (n_samples == 0 || sample_total), "non-null sample_off, sample_total");
    hipStream_t s = (hipStream_t)stream;
    if (n_samples) DIG_HIP_TRY(hipMemsetAsync(sample_total, 0, (size_t)n_samples * sizeof(int32_t), s));
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(gene && sample && annot && cohort && keys, "non-null pointers");
    const GeneKeyArgs a{gene, sample, cohort, annot, sample_off, n, G, C, sb, keys, sample_total};
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n, kGeneCountBlock, &blocks)) return rc;
    hipLaunchKernelGGL(gene_row_keys_kernel, dim3(blocks), dim3(kGeneCountBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_gene_counts(const int64_t* keys_sorted, int64_t n, const int32_t* sample_total, int64_t n_samples, double max_muts_per_sample,
                    double max_muts_per_gene_per_sample, int64_t tp53, int64_t G, int64_t C, int32_t* obs, int32_t* n_samp,
                    int32_t* extra, int64_t* n_syn, uint8_t* blacklisted, int32_t* scratch, void* stream)
{
    DIG_REQUIRE(n >= 0, "n >= 0");
    int sb = 0;
    if (int rc = gene_key_layout(__func__, G, C, n_samples, &sb)) return rc;
    DIG_REQUIRE(tp53 >= 0 && tp53 <= G + 1, "tp53: a gene id, G + 1 when the model has no TP53 row");
    DIG_REQUIRE(!(max_muts_per_sample != max_muts_per_sample) && !(max_muts_per_gene_per_sample != max_muts_per_gene_per_sample),
                "limits that are numbers");
    DIG_REQUIRE(n_syn && (G == 0 || (obs && n_samp && extra && scratch)) && (n_samples == 0 || (sample_total && blacklisted)),
                "non-null pointers");
    hipStream_t s = (hipStream_t)stream;
    const size_t GC = (size_t)G * C;
    DIG_HIP_TRY(hipMemsetAsync(n_syn, 0, (size_t)C * sizeof(int64_t), s));
    if (GC) {
        DIG_HIP_TRY(hipMemsetAsync(obs, 0, GC * 5 * sizeof(int32_t), s));
        DIG_HIP_TRY(hipMemsetAsync(n_samp, 0, GC * 6 * sizeof(int32_t), s));
        DIG_HIP_TRY(hipMemsetAsync(extra, 0, GC * 2 * sizeof(int32_t), s));
        DIG_HIP_TRY(hipMemsetAsync(scratch, 0, GC * 5 * sizeof(int32_t), s));
    }
    if (n) {
        DIG_REQUIRE(keys_sorted, "non-null keys");
        unsigned blocks = 0;
        if (int rc = row_blocks(__func__, n, kGeneCountBlock, &blocks)) return rc;
        const GeneCountArgs a{keys_sorted, n, sample_total, n_samples, max_muts_per_sample, max_muts_per_gene_per_sample, G, C, tp53, sb,
                              obs, n_samp, extra, scratch, reinterpret_cast<unsigned long long*>(n_syn)};
        hipLaunchKernelGGL(gene_counts_kernel, dim3(blocks), dim3(kGeneCountBlock), 0, s, a);
        DIG_HIP_TRY(hipGetLastError());
    }
    const int64_t m = std::max<int64_t>((int64_t)GC * 5, n_samples);
    if (m) {
        hipLaunchKernelGGL(gene_counts_finish_kernel, dim3(grid_for(m, kGeneCountBlock, 8)), dim3(kGeneCountBlock), 0, s, obs, scratch,
                           (int64_t)GC * 5, max_muts_per_gene_per_sample, sample_total, blacklisted, n_samples, max_muts_per_sample);
        DIG_HIP_TRY(hipGetLastError());
    }
    return DIG_OK;
}

}  // extern "C"
