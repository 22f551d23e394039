// dig_seqcounts.hip -- the sufficient statistic of the sequence model for MANY cohorts: per cohort the K integer counts of
// (MUT_TYPE, CONTEXT) over the rows that lie in a whitelisted window, behind the interval join (dig_overlap_join_*) of all cohorts'
// rows with the windows.
//
// Reference, per cohort (scripts/DigPretrain.py:179-208, sequence_tools.py:321-354, mutation_tools.py:8-30):
//   restrict_mutations_by_bed(unique=True)   one row per (row, overlapping window) clipped to the overlap, whole-row duplicates dropped:
//                                            a one-base row counts once when at least one window holds it, however many do
//   groupby(['MUT_TYPE', 'CONTEXT']).size()  merged into the K rows of mk_mutation_context; other label pairs count nowhere
// Here a row carries its table row (row_type, K = no table entry) and its cohort, the join lists a row's pairs consecutively
// (mutation-major), and
//   sequence_counts_kernel   one thread per pair; a pair counts when its left neighbour belongs to another row (the
//                            de-duplication: the first pair of a row stands for the row) and the row's type is < K:
//                            counts[cohort, type] += 1.
// A few types hold a fifth and more of a real cohort's rows, so the counts are privatised: a workgroup keeps K 32-bit counters
// in LDS for ONE cohort, its home -- the cohort of the row of its first pair -- and adds them to the result at the end, one 64-bit
// integer atomic per non-zero counter.  Rows of a cohort are contiguous, so a workgroup sees one cohort or a few; at a cohort
// boundary inside a workgroup the pairs of the other cohorts add straight to the result, one integer atomic each (at most one
// workgroup's worth of pairs per boundary).  Nothing relies on that order: rows of cohorts in any order give the same counts, only
// more of them take the direct route.  The left neighbour is read from global memory, so a row's pairs may span waves and
// workgroups.  Integer atomics only: the result does not depend on the order.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kSeqBlock = 1024;

struct SeqCountArgs {
    const int32_t* pair_row;                // [P], a row's pairs consecutive
    int64_t P;
    const int32_t *row_type, *row_cohort;   // [n]
    int64_t n, C;
    int K;
    unsigned long long* counts;             // [C, K]
};

__global__ __launch_bounds__(kSeqBlock) void sequence_counts_kernel(SeqCountArgs a)
{
    __shared__ uint32_t hist[kSeqMaxK];
    __shared__ int64_t home_s;
    for (int t = threadIdx.x; t < a.K; t += kSeqBlock) hist[t] = 0;
    const int64_t first = (int64_t)blockIdx.x * kSeqBlock;
    if (threadIdx.x == 0) {
        const int64_t r = a.pair_row[first];                     // (first < P: the grid holds no empty workgroup)
        const int64_t c = r >= 0 && r < a.n ? a.row_cohort[r] : -1;
        home_s = c >= 0 && c < a.C ? c : -1;
    }
    __syncthreads();
    const int64_t home = home_s;
    const int64_t i = first + threadIdx.x;
    if (i < a.P) {
        const int64_t r = a.pair_row[i];
        if (r >= 0 && r < a.n && (i == 0 || a.pair_row[i - 1] != r)) {
            const int64_t t = a.row_type[r], c = a.row_cohort[r];
            if (t >= 0 && t < a.K && c >= 0 && c < a.C) {        // (a row outside the tables counts nowhere; the twin refuses it)
                if (c == home)
                    atomicAdd(&hist[t], 1u);
                else
                    atomicAdd(&a.counts[c * a.K + t], 1ull);
            }
        }
    }
    __syncthreads();
    if (home < 0) return;
    for (int t = threadIdx.x; t < a.K; t += kSeqBlock) {
        const uint32_t v = hist[t];
        if (v) atomicAdd(&a.counts[home * a.K + t], (unsigned long long)v);
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_sequence_counts(const int32_t* pair_row, int64_t n_pairs, const int32_t* row_type, const int32_t* row_cohort, int64_t n,
                        int64_t K, int64_t C, int64_t* counts, void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && n >= 0, "n_pairs, n >= 0");
    DIG_REQUIRE(K >= 1 && K <= kSeqMaxK, "K within [1, 3072] (the workgroup's LDS counters)");
    DIG_REQUIRE(C >= 1 && C < ((int64_t)1 << 31), "C within [1, 2^31)");
    DIG_REQUIRE(counts, "non-null counts");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)C * K * sizeof(int64_t), s));
    if (n_pairs == 0 || n == 0) return DIG_OK;
    DIG_REQUIRE(pair_row && row_type && row_cohort, "non-null pointers");
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, n_pairs, kSeqBlock, &blocks)) return rc;
    const SeqCountArgs a{pair_row, n_pairs, row_type, row_cohort, n, C, (int)K, reinterpret_cast<unsigned long long*>(counts)};
    hipLaunchKernelGGL(sequence_counts_kernel, dim3(blocks), dim3(kSeqBlock), 0, s, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
