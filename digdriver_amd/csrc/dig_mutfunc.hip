// dig_mutfunc.hip -- the genic function of every (mutation, gene) pair of a mutation file (DigPreprocess.py addMutationFunction).
//
// Reference (scripts/mutationFunction.R, an R loop per coding mutation over the gene's expanded CDS string from refcds_hg19.rda):
//   an SNV on an essential-splice position of the gene is Essential_Splice; otherwise its index in the CDS read in transcript
//   direction (chr2cds), the codon around it and the codon with ALT in place are translated with the standard code:
//   Synonymous / Nonsense / Missense / Stop_loss; a REF that is not the CDS base marks the row as wrong_ref.  An indel or MNV
//   gets the count, minimum and maximum of the CDS indices of its positions.
// Here the CDS string is never built: the gene is its CDS blocks with the CDS length in front of each, and the codon's three
// bases are read from the HBM-resident 2-bit genome of dig_count_contexts2.  One lane per pair: a binary search over the gene's
// splice positions and one over its blocks, then the (at most three) genome words of the codon and the walk over the non-ACGT
// run list from each base's bucket; a codon inside one block, the usual case, needs no further search.  Pairs whose codon or
// base touches a non-ACGT run are left to the host (DIG_MF_HOST), which knows the letters.  Short dependent gathers:
// latency-bound, like dig_mutation_contexts and the join.
#include "dig_codon.hpp"

namespace dig {

constexpr int kMfBlock = 256;
__global__ __launch_bounds__(kMfBlock) void mutation_function_kernel(
    Genome2 G, const int32_t* __restrict__ gene_chrom, const uint8_t* __restrict__ gene_minus, const int64_t* __restrict__ blk_ptr,
    const int64_t* __restrict__ blk_start, const int64_t* __restrict__ blk_end, const int64_t* __restrict__ cds_off,
    const int64_t* __restrict__ spl_ptr, const int64_t* __restrict__ spl_pos, int64_t n_genes,
    const int32_t* __restrict__ pair_gene, const int64_t* __restrict__ pair_start, const int64_t* __restrict__ pair_end,
    const uint8_t* __restrict__ pair_kind, const uint8_t* __restrict__ pair_ref, const uint8_t* __restrict__ pair_alt, int64_t n_pairs,
    uint8_t* __restrict__ impact, uint8_t* __restrict__ status, int32_t* __restrict__ n_cds, int32_t* __restrict__ cds_min,
    int32_t* __restrict__ cds_max)
{
    const int64_t stride = (int64_t)gridDim.x * kMfBlock;
    for (int64_t i = (int64_t)blockIdx.x * kMfBlock + threadIdx.x; i < n_pairs; i += stride) {
        const int64_t gi = pair_gene[i];
        const int64_t s = pair_start[i], e = pair_end[i];
        const unsigned kind = pair_kind[i];
        unsigned imp = DIG_MF_NONE, stt = DIG_MF_OK;
        int64_t n = 0, mn = 0, mx = 0;
        const int64_t b0 = gi >= 0 && gi < n_genes ? blk_ptr[gi] : 0, b1 = gi >= 0 && gi < n_genes ? blk_ptr[gi + 1] : 0;
        if (b1 <= b0) {
            stt = DIG_MF_OUTSIDE;                                    // no such gene, or a gene without a block
        } else {
            const bool minus = gene_minus[gi] != 0;
            const int64_t len = cds_off[b1 - 1] + blk_end[b1 - 1] - blk_start[b1 - 1] + 1;
            if (kind == DIG_MF_KIND_SNV) {
                const int ch = gene_chrom[gi];
                const bool ch_ok = ch >= 0 && ch < G.n_chrom;
                const int64_t off = ch_ok ? kGenome2PadBases + G.chrom_off[ch] : 0, clen = ch_ok ? G.chrom_len[ch] : 0;
                const unsigned ref = pair_ref[i], alt = pair_alt[i] & 3u;
                const int64_t q0 = spl_ptr[gi], q1 = spl_ptr[gi + 1];
                const int64_t q = codon_last_le(spl_pos, q0, q1, s);
                const int64_t b = codon_last_le(blk_start, b0, b1, s);
                const unsigned base = genome2_base(G, off, clen, s);
                bool host = base > 3u;
                if (q >= q0 && spl_pos[q] == s) {
                    imp = DIG_MF_SPLICE;
                } else if (b < b0 || s > blk_end[b]) {
                    stt = DIG_MF_OUTSIDE;
                } else {
                    const int64_t bs = blk_start[b], co = cds_off[b], bsz = blk_end[b] - bs + 1;
                    const int64_t f = co + (s - bs);                 // 0-based CDS index in genome order
                    const int64_t pos_ind = minus ? len - f : f + 1;
                    const int64_t k = (pos_ind + 2) / 3;             // ceil(pos_ind / 3)
                    const int at = (int)(pos_ind - 3 * (k - 1)) - 1; // 0, 1, 2 inside the codon
                    n = 1, mn = mx = pos_ind;
                    if (3 * k > len) {
                        stt = DIG_MF_OUTSIDE;                        // (a CDS that is not whole codons: the caller's table is wrong)
                    } else {
                        const GeneCds gene = {blk_start, cds_off, b0, b1, len, minus};
                        unsigned codon = 0;
#pragma unroll
                        for (int j = 0; j < 3; ++j) {
                            unsigned c = base;
                            if (j != at) {
                                const int64_t fj = minus ? f + (at - j) : f + (j - at);      // the neighbour, genome order
                                const int64_t p = fj >= co && fj < co + bsz ? bs + (fj - co) : cds_to_genome(gene, 3 * (k - 1) + j + 1);
                                c = genome2_base(G, off, clen, p);
                            }
                            host |= c > 3u;
                            codon = (codon << 2) | ((minus ? 3u - c : c) & 3u);
                        }
                        imp = classify_codon_change(codon, at, minus ? 3u - alt : alt);
                    }
                }
                if (stt == DIG_MF_OK) stt = host ? DIG_MF_HOST : (base != ref ? DIG_MF_WRONG_REF : DIG_MF_OK);
                if (stt == DIG_MF_HOST) imp = DIG_MF_NONE;           // (the 2-bit form stores such a letter as A: no class from it)
            } else {
                const int64_t lo = kind == DIG_MF_KIND_INS ? s - 1 : s, hi = e;
                int64_t fmin = INT64_MAX, fmax = -1;
                // the first block that ends at or after lo: blocks are disjoint and ascending, so their ends ascend too
                int64_t b = codon_last_le(blk_end, b0, b1, lo - 1) + 1;
                for (; b < b1; ++b) {
                    const int64_t bs = blk_start[b];
                    if (bs > hi) break;
                    const int64_t a = max(lo, bs), z = min(hi, blk_end[b]);
                    if (a <= z) {
                        n += z - a + 1;
                        fmin = min(fmin, cds_off[b] + (a - bs));
                        fmax = max(fmax, cds_off[b] + (z - bs));
                    }
                }
                if (n > 0) {
                    mn = minus ? len - fmax : fmin + 1;
                    mx = minus ? len - fmin : fmax + 1;
                }
            }
        }
        impact[i] = (uint8_t)imp;
        status[i] = (uint8_t)stt;
        n_cds[i] = (int32_t)n;
        cds_min[i] = (int32_t)mn;
        cds_max[i] = (int32_t)mx;
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_mutation_function(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                          const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                          const int32_t* gene_chrom, const uint8_t* gene_minus, const int64_t* blk_ptr, const int64_t* blk_start,
                          const int64_t* blk_end, const int64_t* cds_off, const int64_t* spl_ptr, const int64_t* spl_pos, int64_t n_genes,
                          const int32_t* pair_gene, const int64_t* pair_start, const int64_t* pair_end, const uint8_t* pair_kind,
                          const uint8_t* pair_ref, const uint8_t* pair_alt, int64_t n_pairs, uint8_t* impact, uint8_t* status,
                          int32_t* n_cds, int32_t* cds_min, int32_t* cds_max, void* stream)
{
    DIG_REQUIRE(n_pairs >= 0 && n_genes >= 0, "n_pairs, n_genes >= 0");
    const Genome2 G = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, G, n_pairs)) return rc;
    if (n_pairs == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len, "non-null genome arrays");
    DIG_REQUIRE(n_genes == 0 || (gene_chrom && gene_minus && blk_start && blk_end && cds_off), "non-null gene table");
    DIG_REQUIRE(blk_ptr && spl_ptr, "non-null blk_ptr, spl_ptr (n_genes + 1 entries)");
    DIG_REQUIRE(pair_gene && pair_start && pair_end && pair_kind && pair_ref && pair_alt, "non-null pair arrays");
    DIG_REQUIRE(impact && status && n_cds && cds_min && cds_max, "non-null outputs");
    hipLaunchKernelGGL(mutation_function_kernel, dim3(grid_for(n_pairs, kMfBlock)), dim3(kMfBlock), 0, (hipStream_t)stream, G,
                       gene_chrom, gene_minus, blk_ptr, blk_start, blk_end, cds_off, spl_ptr, spl_pos,
                       n_genes, pair_gene, pair_start, pair_end, pair_kind, pair_ref, pair_alt, n_pairs, impact, status, n_cds,
                       cds_min, cds_max);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
