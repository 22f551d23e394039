// dig_genesites.hip -- the possible single-base substitutions of every gene by effect class and substitution type: the L of the
// gene container (window_{w}/genes/L, [G, 4, 192]; the reference's L_data, which it takes from dNdScv's refcds_hg19.rda and has
// no code for).
//
// Rule: every CDS base of the gene and each of its three alternates is classified on its codon exactly as dig_mutation_function
// classifies an observed SNV (classify_codon_change, dig_codon.hpp): silent / missense / nonsense add one to class 0 / 1 / 2, a
// stop-loss to no class (mutationFunction.R:174-175 gives it no impact index) -- it is counted in n_stop_loss; every essential-splice
// position adds its three alternates to class 3.  The substitution type is the trinucleotide of the GENOME around the base (the
// flanks at an exon edge are intron bases), read in transcript direction, and the alternate on the gene's strand: column
// 3 (16 X + 4 Y + Z) + rank of the alternate among the three bases other than Y, the position of "XYZ>XaZ" in the sorted
// substitution index.  The denominators of the gene route count the same thing: genomic trinucleotides of the overlapped windows
// on the gene's strand (si_by_regions, sequence_tools.py:396-425).
//
// Shape: one workgroup per gene, its 768 counters and the stop-loss counter in LDS (3 KB, ds_add_u32), one lane per codon: the
// block of the codon's first base by binary search, the usual codon inside one block then takes its five genome bases (the codon
// and a flank on either side) from one window read and one look at the run list; 9 classifications, 9 LDS adds.  Every row of the
// output is written by its workgroup with coalesced stores: no global atomics, nothing to zero beforehand.  A gene in which any
// base read is a letter other than ACGT (or lies outside the chromosome) leaves with a zero row and DIG_GS_HOST: the caller
// knows the letters.  Integer counts: any order of summation gives the same bits.
#include "dig_codon.hpp"

namespace dig {

constexpr int kGsBlock = 256;
constexpr int kGsCounters = 4 * 192 + 1;                             // [class][type] and the stop-loss count

// the three alternates of the base at `at` of `codon` (transcript strand) whose trinucleotide is `ctx` = 16 X + 4 Y + Z
__device__ __forceinline__ void gene_sites_add_cds(uint32_t* cnt, unsigned codon, int at, unsigned ctx)
{
    const unsigned y = (ctx >> 2) & 3u;
#pragma unroll
    for (unsigned a = 0; a < 4; ++a) {
        if (a == y) continue;
        const unsigned cls = classify_codon_change(codon, at, a);
        const unsigned col = 3u * ctx + a - (a > y ? 1u : 0u);
        atomicAdd(&cnt[cls == DIG_MF_STOP_LOSS ? 4u * 192u : cls * 192u + col], 1u);
    }
}

// 16 X + 4 Y + Z in transcript direction from the genome's bases left, centre, right of a position
__device__ __forceinline__ unsigned gene_sites_ctx(unsigned l, unsigned c, unsigned r, bool minus)
{
    return minus ? 16u * (3u - r) + 4u * (3u - c) + (3u - l) : 16u * l + 4u * c + r;
}

__global__ __launch_bounds__(kGsBlock) void gene_site_counts_kernel(
    Genome2 G, const int32_t* __restrict__ gene_chrom, const uint8_t* __restrict__ gene_minus, const int64_t* __restrict__ blk_ptr,
    const int64_t* __restrict__ blk_start, const int64_t* __restrict__ blk_end, const int64_t* __restrict__ cds_off,
    const int64_t* __restrict__ spl_ptr, const int64_t* __restrict__ spl_pos, int64_t n_genes, int32_t* __restrict__ L,
    int32_t* __restrict__ n_stop_loss, uint8_t* __restrict__ status)
{
    __shared__ uint32_t cnt[kGsCounters];
    __shared__ uint32_t other;                                       // a base read was not ACGT
    const int tid = threadIdx.x;
    for (int64_t gi = blockIdx.x; gi < n_genes; gi += gridDim.x) {
        for (int i = tid; i < kGsCounters; i += kGsBlock) cnt[i] = 0;
        if (tid == 0) other = 0;
        __syncthreads();
        const int64_t b0 = blk_ptr[gi], b1 = blk_ptr[gi + 1];
        const bool minus = gene_minus[gi] != 0;
        const int ch = gene_chrom[gi];
        const bool ch_ok = ch >= 0 && ch < G.n_chrom;
        const int64_t off = ch_ok ? kGenome2PadBases + G.chrom_off[ch] : 0, clen = ch_ok ? G.chrom_len[ch] : 0;
        const int64_t len = b1 > b0 ? cds_off[b1 - 1] + blk_end[b1 - 1] - blk_start[b1 - 1] + 1 : 0;
        const GeneCds gene = {blk_start, cds_off, b0, b1, len, minus};
        bool host = false;
        for (int64_t k = tid; k < len / 3; k += kGsBlock) {
            const int64_t f0 = minus ? len - 1 - 3 * k : 3 * k;      // the codon's first base (transcript), 0-based in genome order
            const int64_t b = codon_last_le(cds_off, b0, b1, f0);
            const int64_t bs = blk_start[b], co = cds_off[b], bsz = blk_end[b] - bs + 1;
            const int64_t f2 = minus ? f0 - 2 : f0 + 2;
            if (f2 >= co && f2 < co + bsz) {
                // the codon inside one block: genome positions lo .. lo + 2 and one flank on either side
                const int64_t lo = bs + ((minus ? f2 : f0) - co);
                if (lo - 1 < 1 || lo + 3 > clen) { host = true; continue; }
                const int64_t q = off + lo - 2;                      // array base of the left flank
                if (G.n_int > 0) {
                    const int64_t j = genome2_first_run(G, q);
                    if (j < G.n_int && G.nint_start[j] < q + 5) { host = true; continue; }
                }
                const uint32_t w = genome2_window(G.words, q, 5);
                const unsigned x0 = (w >> 2) & 3u, x1 = (w >> 4) & 3u, x2 = (w >> 6) & 3u;        // the codon in genome order
                const unsigned codon = minus ? 16u * (3u - x2) + 4u * (3u - x1) + (3u - x0) : 16u * x0 + 4u * x1 + x2;
#pragma unroll
                for (int at = 0; at < 3; ++at) {
                    const uint32_t tri = w >> (2 * (minus ? 2 - at : at));            // left flank, base, right flank from bit 0 on
                    gene_sites_add_cds(cnt, codon, at, gene_sites_ctx(tri & 3u, (tri >> 2) & 3u, (tri >> 4) & 3u, minus));
                }
            } else {
                unsigned l[3], c[3], r[3], bad = 0;
#pragma unroll
                for (int at = 0; at < 3; ++at) {
                    const int64_t p = cds_to_genome(gene, 3 * k + at + 1);
                    l[at] = genome2_base(G, off, clen, p - 1);
                    c[at] = genome2_base(G, off, clen, p);
                    r[at] = genome2_base(G, off, clen, p + 1);
                    bad |= (l[at] | c[at] | r[at]) & 4u;
                }
                if (bad) { host = true; continue; }
                const unsigned codon = minus ? 16u * (3u - c[0]) + 4u * (3u - c[1]) + (3u - c[2]) : 16u * c[0] + 4u * c[1] + c[2];
#pragma unroll
                for (int at = 0; at < 3; ++at) gene_sites_add_cds(cnt, codon, at, gene_sites_ctx(l[at], c[at], r[at], minus));
            }
        }
        for (int64_t q = spl_ptr[gi] + tid; q < spl_ptr[gi + 1]; q += kGsBlock) {
            const int64_t p = spl_pos[q];
            const unsigned l = genome2_base(G, off, clen, p - 1), c = genome2_base(G, off, clen, p), r = genome2_base(G, off, clen, p + 1);
            if ((l | c | r) & 4u) { host = true; continue; }
            const unsigned ctx = gene_sites_ctx(l, c, r, minus);
#pragma unroll
            for (unsigned rank = 0; rank < 3; ++rank) atomicAdd(&cnt[3u * 192u + 3u * ctx + rank], 1u);
        }
        if (host) atomicOr(&other, 1u);
        __syncthreads();
        const bool to_host = other != 0;
        int32_t* row = L + gi * (4 * 192);
        for (int i = tid; i < 4 * 192; i += kGsBlock) row[i] = to_host ? 0 : (int32_t)cnt[i];
        if (tid == 0) {
            n_stop_loss[gi] = to_host ? 0 : (int32_t)cnt[4 * 192];
            status[gi] = to_host ? DIG_GS_HOST : DIG_GS_OK;
        }
        __syncthreads();                                             // (the counters are zeroed for the next gene)
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_gene_site_counts(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                         const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                         const int32_t* gene_chrom, const uint8_t* gene_minus, const int64_t* blk_ptr, const int64_t* blk_start,
                         const int64_t* blk_end, const int64_t* cds_off, const int64_t* spl_ptr, const int64_t* spl_pos, int64_t n_genes,
                         int32_t* L, int32_t* n_stop_loss, uint8_t* status, void* stream)
{
    DIG_REQUIRE(n_genes >= 0, "n_genes >= 0");
    const Genome2 G = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, G, n_genes)) return rc;
    if (n_genes == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len, "non-null genome arrays");
    DIG_REQUIRE(gene_chrom && gene_minus && blk_ptr && spl_ptr, "non-null gene_chrom, gene_minus, blk_ptr, spl_ptr");
    DIG_REQUIRE(L && n_stop_loss && status, "non-null outputs");
    const int64_t cap = (int64_t)cu_count() * 64;                    // (a workgroup takes the genes blockIdx, blockIdx + grid, ...;
                                                                     //  past the cap: test_gene_site_counts_past_one_pass_of_the_grid, tests/test_gpu_grid_wrap.py)
    hipLaunchKernelGGL(gene_site_counts_kernel, dim3((unsigned)(n_genes < cap ? n_genes : cap)), dim3(kGsBlock), 0, (hipStream_t)stream,
                       G, gene_chrom, gene_minus, blk_ptr, blk_start, blk_end, cds_off, spl_ptr, spl_pos, n_genes, L, n_stop_loss,
                       status);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
