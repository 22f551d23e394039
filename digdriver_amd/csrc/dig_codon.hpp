// dig_codon.hpp -- the device functions of the genic annotation that the per-gene counts of possible substitutions need as
// well: (gene, CDS index) -> genome position and the effect class of a codon change under the standard genetic code (one
// base of the 2-bit genome: genome2_base, dig_genome2.hpp).
#pragma once
#include "dig_genome2.hpp"

namespace dig {

// index of the last element <= key of the ascending a[lo, hi); lo - 1 when there is none
__device__ __forceinline__ int64_t codon_last_le(const int64_t* __restrict__ a, int64_t lo, int64_t hi, int64_t key)
{
    while (lo < hi) {
        const int64_t mid = (lo + hi) >> 1;
        if (a[mid] <= key) lo = mid + 1; else hi = mid;
    }
    return lo - 1;
}

// The CDS of one gene: blocks [b0, b1) of the table (ascending, disjoint, 1-based closed), the CDS length in front of each in
// genome order, the whole length and the strand.
struct GeneCds {
    const int64_t* __restrict__ blk_start;
    const int64_t* __restrict__ cds_off;
    int64_t b0, b1, len;
    bool minus;
};

// genome position (1-based) of CDS index `idx` (1-based, transcript direction) of the gene; 0 when idx is outside [1, len]
__device__ __forceinline__ int64_t cds_to_genome(const GeneCds& g, int64_t idx)
{
    if (idx < 1 || idx > g.len) return 0;
    const int64_t f = (g.minus ? g.len - idx : idx - 1);             // 0-based, genome order
    const int64_t b = codon_last_le(g.cds_off, g.b0, g.b1, f);       // cds_off[b0] == 0: b >= b0
    return g.blk_start[b] + (f - g.cds_off[b]);
}

// amino acid of a codon on the coding strand, codon = 16 b0 + 4 b1 + b2 with A C G T = 0 1 2 3 (the standard code, '*' = stop)
__device__ __forceinline__ char codon_amino_acid(unsigned codon)
{
    static constexpr char kCode[65] = "KNKNTTTTRSRSIIMI" "QHQHPPPPRRRRLLLL" "EDEDAAAAGGGGVVVV" "*Y*YSSSS*CWCLFLF";
    return kCode[codon & 63u];
}

// effect class (DIG_MF_SYN / _MIS / _NONS / _STOP_LOSS) of writing base `alt` at position `at` (0, 1, 2) of `codon`
__device__ __forceinline__ unsigned classify_codon_change(unsigned codon, int at, unsigned alt)
{
    const int sh = 2 * (2 - at);
    const unsigned changed = (codon & ~(3u << sh)) | ((alt & 3u) << sh);
    const char old_aa = codon_amino_acid(codon), new_aa = codon_amino_acid(changed);
    if (new_aa == old_aa) return DIG_MF_SYN;
    if (new_aa == '*') return DIG_MF_NONS;
    return old_aa != '*' ? DIG_MF_MIS : DIG_MF_STOP_LOSS;
}

}  // namespace dig
