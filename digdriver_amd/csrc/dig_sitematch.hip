// dig_sitematch.hip -- the sites route's observed counts for MANY cohorts: mutations that hit a listed (position, substitution)
// site EXACTLY, the one tabulation of the project that is an equality and not an interval overlap (dig_overlap_join_* cannot serve it).
//
// Reference, per cohort (mutation_tools.py:233-281 tabulate_nonc_mutations_at_sites):
//   df_mut.merge(df_sites, on=[CHROM, START, END, REF, ALT, GENE, ANNOT, MUT_TYPE, CONTEXT], how='inner')   one row per (mutation
//                                      row, site row) with all nine columns equal: a site row listed twice counts twice
//   groupby('ELT').agg(len(set(SAMPLE)), len)          OBS_SAMPLES = distinct samples, OBS_SNV = merged rows, per element
// Here the nine columns are three integers -- pos = chrom << 40 | START, END, and attr, an injective code of the six labels formed
// on the host from the sites file's own dictionaries (data_tools/sites.py; negative: a label the sites file does not hold) -- the
// site table is sorted by pos, and the chain is three kernels around one cumulative sum and one key sort by the caller:
//   site_match_kernel<false>   one thread per mutation row: a lower-bound binary search for the first site with the row's pos, then a
//                              walk over the equal-position run (short: three substitutions times the elements that list the
//                              position) counting the sites with equal END and attr
//   -- the caller forms the exclusive prefix sum of the counts (the two-call protocol of the interval join) --
//   site_match_kernel<true>    the same search; match q of row i writes keys[offsets[i] + q] =
//                              (cohort E + element) << sb | global sample, sb the bits of n_samples - 1
//   -- the caller sorts the keys --
//   site_counts_kernel         one thread per sorted key: obs_snv[element, cohort] += 1, and obs_samples[element, cohort] += 1 when the
//                              left neighbour -- read from global memory: it may lie in the previous wave or workgroup -- is another
//                              key.  Both sums go through segment_count of dig_keyruns.hpp: one integer atomic per run of lanes
//                              with one destination.
// A row outside the tables (cohort, sample) and a site row whose element is outside [0, E) match nothing here; the host twins refuse
// them.  Integer atomics only: the result does not depend on the order.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kSiteBlock = 256;

// the key's two fields must fit 63 bits
int site_key_layout(const char* fn, int64_t E, int64_t C, int64_t n_samples, int* sample_bits)
{
    DIG_REQUIRE_IN(fn, E >= 0 && C >= 1 && n_samples >= 0, "E >= 0, C >= 1, n_samples >= 0");
    DIG_REQUIRE_IN(fn, E < ((int64_t)1 << 31) && C < ((int64_t)1 << 31) && n_samples < ((int64_t)1 << 31),
                   "E, C and the sample count below 2^31");
    *sample_bits = key_bits_for(n_samples);
    DIG_REQUIRE_IN(fn, key_bits_for(C * E) + *sample_bits <= 63,
                   "the key (cohort E + element, global sample) does not fit 63 bits: fewer cohorts per call");
    return DIG_OK;
}

struct SiteMatchArgs {
    const int64_t *site_pos, *site_end, *site_attr;      // [S], site_pos ascending
    const int32_t* site_elt;                             // [S]
    int64_t S, E;
    const int64_t *row_pos, *row_end, *row_attr;         // [n]
    const int32_t *row_sample, *row_cohort;              // [n]: global sample, cohort
    const int64_t* sample_off;                           // [C + 1]
    int64_t n, C;
    int sample_bits;
    int32_t* counts;                                     // [n]                      (count)
    const int64_t* offsets;                              // [n]                      (fill)
    int64_t total;
    int64_t* keys;                                       // [total]                  (fill)
};

template <bool FILL>
__global__ __launch_bounds__(kSiteBlock) void site_match_kernel(SiteMatchArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kSiteBlock + threadIdx.x;
    if (i >= a.n) return;
    const int64_t pos = a.row_pos[i], end = a.row_end[i], attr = a.row_attr[i];
    const int64_t c = a.row_cohort[i], gs = a.row_sample[i];
    int32_t found = 0;
    if (attr >= 0 && c >= 0 && c < a.C && gs >= a.sample_off[c] && gs < a.sample_off[c + 1]) {
        int64_t lo = 0, hi = a.S;                        // the first site with site_pos >= pos
        while (lo < hi) {
            const int64_t mid = lo + ((hi - lo) >> 1);
            if (a.site_pos[mid] < pos)
                lo = mid + 1;
            else
                hi = mid;
        }
        int64_t o = FILL ? a.offsets[i] : 0;
        for (int64_t j = lo; j < a.S && a.site_pos[j] == pos; ++j) {
            if (a.site_end[j] != end || a.site_attr[j] != attr) continue;
            const int64_t e = a.site_elt[j];
            if (e < 0 || e >= a.E) continue;
            if (FILL) {
                if (o >= 0 && o < a.total) a.keys[o] = ((c * a.E + e) << a.sample_bits) | gs;     // (offsets the caller got wrong write nowhere)
                ++o;
            }
            ++found;
        }
    }
    if (!FILL) a.counts[i] = found;
}

struct SiteCountArgs {
    const int64_t* keys;                                 // [total] ascending
    int64_t total, E, C;
    int sample_bits;
    int32_t *obs_snv, *obs_samples;                      // [E, C]
};

__global__ __launch_bounds__(kSiteBlock) void site_counts_kernel(SiteCountArgs a)
{
    const int64_t i = (int64_t)blockIdx.x * kSiteBlock + threadIdx.x;
    int64_t slot = -1;                                   // cohort E + element; -1: no key here, or a key dig_site_match_keys did not make
    bool distinct = false;
    if (i < a.total) {
        const int64_t key = a.keys[i];
        if (key >= 0) {
            slot = key >> a.sample_bits;
            if (slot >= a.E * a.C)
                slot = -1;
            else
                distinct = i == 0 || a.keys[i - 1] != key;
        }
    }
    const int rows = segment_count(slot, true), samples = segment_count(slot, distinct);
    if (!rows) return;
    const int64_t c = slot / a.E, e = slot - c * a.E, at = e * a.C + c;
    atomicAdd(&a.obs_snv[at], rows);
    if (samples) atomicAdd(&a.obs_samples[at], samples);
}

// the checks and the launch the two search entry points share
template <bool FILL>
int site_match(const char* fn, SiteMatchArgs a, int64_t n_samples, hipStream_t s)
{
    DIG_REQUIRE_IN(fn, a.S >= 0 && a.n >= 0 && a.total >= 0, "S, n, total >= 0");
    DIG_REQUIRE_IN(fn, a.S < ((int64_t)1 << 31), "fewer than 2^31 site rows (a row's count is 32-bit)");
    if (int rc = site_key_layout(fn, a.E, a.C, n_samples, &a.sample_bits)) return rc;
    if (FILL) {
        DIG_REQUIRE_IN(fn, a.total == 0 || a.keys, "non-null keys");
        if (a.total) DIG_HIP_TRY(hipMemsetAsync(a.keys, 0xff, (size_t)a.total * sizeof(int64_t), s));      // -1: counted nowhere
        if (a.total == 0) return DIG_OK;
    }
    if (a.n == 0) return DIG_OK;
    DIG_REQUIRE_IN(fn, a.row_pos && a.row_end && a.row_attr && a.row_sample && a.row_cohort && a.sample_off, "non-null row arrays, sample_off");
    DIG_REQUIRE_IN(fn, FILL ? a.offsets != nullptr : a.counts != nullptr, FILL ? "non-null offsets" : "non-null counts");
    if (a.S == 0) {
        if (!FILL) DIG_HIP_TRY(hipMemsetAsync(a.counts, 0, (size_t)a.n * sizeof(int32_t), s));
        return DIG_OK;
    }
    DIG_REQUIRE_IN(fn, a.site_pos && a.site_end && a.site_attr && a.site_elt, "non-null site arrays");
    unsigned blocks = 0;
    if (int rc = row_blocks(fn, a.n, kSiteBlock, &blocks)) return rc;
    hipLaunchKernelGGL(site_match_kernel<FILL>, dim3(blocks), dim3(kSiteBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_site_match_count(const int64_t* site_pos, const int64_t* site_end, const int64_t* site_attr, const int32_t* site_elt, int64_t S,
                         int64_t E, const int64_t* row_pos, const int64_t* row_end, const int64_t* row_attr, const int32_t* row_sample,
                         const int32_t* row_cohort, const int64_t* sample_off, int64_t n, int64_t C, int64_t n_samples, int32_t* counts,
                         void* stream)
{
    const SiteMatchArgs a{site_pos, site_end, site_attr, site_elt, S, E, row_pos, row_end, row_attr, row_sample, row_cohort, sample_off,
                          n, C, 0, counts, nullptr, 0, nullptr};
    return site_match<false>(__func__, a, n_samples, (hipStream_t)stream);
}

int dig_site_match_keys(const int64_t* site_pos, const int64_t* site_end, const int64_t* site_attr, const int32_t* site_elt, int64_t S,
                        int64_t E, const int64_t* row_pos, const int64_t* row_end, const int64_t* row_attr, const int32_t* row_sample,
                        const int32_t* row_cohort, const int64_t* sample_off, int64_t n, int64_t C, int64_t n_samples,
                        const int64_t* offsets, int64_t total, int64_t* keys, void* stream)
{
    const SiteMatchArgs a{site_pos, site_end, site_attr, site_elt, S, E, row_pos, row_end, row_attr, row_sample, row_cohort, sample_off,
                          n, C, 0, nullptr, offsets, total, keys};
    return site_match<true>(__func__, a, n_samples, (hipStream_t)stream);
}

int dig_site_counts(const int64_t* keys_sorted, int64_t total, int64_t E, int64_t C, int64_t n_samples, int32_t* obs_snv,
                    int32_t* obs_samples, void* stream)
{
    DIG_REQUIRE(total >= 0, "total >= 0");
    int sb = 0;
    if (int rc = site_key_layout(__func__, E, C, n_samples, &sb)) return rc;
    if (E == 0) return DIG_OK;
    DIG_REQUIRE(obs_snv && obs_samples, "non-null outputs");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(obs_snv, 0, (size_t)E * C * sizeof(int32_t), s));
    DIG_HIP_TRY(hipMemsetAsync(obs_samples, 0, (size_t)E * C * sizeof(int32_t), s));
    if (total == 0) return DIG_OK;
    DIG_REQUIRE(keys_sorted, "non-null keys");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, total, kSiteBlock, &blocks)) return rc;
    const SiteCountArgs a{keys_sorted, total, E, C, sb, obs_snv, obs_samples};
    hipLaunchKernelGGL(site_counts_kernel, dim3(blocks), dim3(kSiteBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
