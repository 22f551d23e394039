// dig_mutctx.hip -- the sequence context of every mutation of a file (DigPreprocess.py addMutationContext).
//
// Reference (sequence_tools.py:130-222, one pool worker per chromosome, a Python loop per row over the whole chromosome string):
//   a row matches when seq[START] == REF; its CONTEXT is seq[START - n_up : START + n_down + 1] when every row from the head of
//   its run (the maximal block of consecutive rows with the same START) up to and including it matches, "" otherwise (the
//   mismatch test and the START == prev_start copy at :145-157); a window holding an N becomes "" (seq_to_context :42-57);
//   collapse = True reverse-complements a window whose centre is G or A.
//
// Two launches over the rows in the caller's (chromosome-grouped) order:
//   * lookup: one lane per row -- the centre base and the window from the HBM-resident 2-bit genome of dig_count_contexts2 (one
//     64-bit gather: a window of at most 16 bases is one 32-bit code) and a walk over the non-ACGT run list from the row's
//     bucket.  Per row it writes three flags (matches, heads a run, needs the host) into `status` and the window code; per wave
//     of 64 rows the index of its last run head and of its last mismatching row (two ballots) into the workspace;
//   * resolve: the run rule as a max-scan -- a row is kept iff the last mismatch at or before it lies in front of the last run
//     head at or before it.  Inside a wave both come from ballots; a wave whose first row continues a run looks back over the
//     per-wave pairs, 64 waves per step, to the nearest wave holding a head (rows of a run are rarely more than a few waves
//     apart, so that is one step).  `status` is rewritten in place with the final code.
// Rows whose window touches a non-ACGT run (the 2-bit form stores N, R, M, ... all as A), starts before the chromosome or is cut
// short at its end are left to the host (DIG_MC_HOST), which knows the letters; their match test is still exact here, since
// the centre base's run membership is looked up.  The work is one short gather per row: latency-bound.
#include "dig_genome2.hpp"

namespace dig {

constexpr int kMcBlock = 256;
constexpr unsigned kMcMatch = 1u, kMcHead = 2u, kMcNeedsHost = 4u;

__device__ __forceinline__ uint64_t mc_upto(int lane)           // lanes 0 .. lane
{
    return ~0ull >> (63 - lane);
}

__device__ __forceinline__ int64_t mc_last(uint64_t mask, int64_t base)      // index of the highest set lane, -1 if none
{
    return mask ? base + 63 - __builtin_clzll(mask) : -1;
}

__global__ __launch_bounds__(kMcBlock) void mutctx_lookup_kernel(
    Genome2 G, const int32_t* __restrict__ row_chrom, const int64_t* __restrict__ row_start, const uint8_t* __restrict__ row_ref,
    int64_t N, int n_up, int n_down, int collapse, uint8_t* __restrict__ status, uint32_t* __restrict__ context,
    int32_t* __restrict__ wave_last)
{
    const int64_t i = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const bool have = i < N;
    bool match = false, head = false, host = false;
    uint32_t code = 0;
    if (have) {
        const int ch = row_chrom[i];
        const int64_t s = row_start[i];
        head = i == 0 || row_chrom[i - 1] != ch || row_start[i - 1] != s;
        const int64_t len = G.chrom_len[ch];
        if (s < 0 || s >= len) {
            host = true;                                             // the caller rejects these; nothing is read
        } else {
            const int W = n_up + n_down + 1;
            const int64_t off = kGenome2PadBases + G.chrom_off[ch];
            const int64_t g = off + s;                               // the centre in array bases
            host = s < n_up || s + n_down + 1 > len;
            const int64_t lo = max(g - n_up, off), hi = min(g + n_down + 1, off + len);      // the window inside the chromosome
            bool centre_other = false;
            if (G.n_int > 0) {                                       // the runs of non-ACGT letters that touch [lo, hi)
                for (int64_t j = genome2_first_run(G, lo); j < G.n_int && G.nint_start[j] < hi; ++j) {
                    host = true;
                    centre_other |= G.nint_start[j] <= g && g < G.nint_end[j];
                }
            }
            const unsigned centre = genome2_code(G.words, g);
            const unsigned ref = row_ref[i];
            match = ref == 4u || (ref < 4u && !centre_other && centre == ref);       // 4: the caller matched a non-ACGT letter
            if (!host) {
                code = genome2_window(G.words, g - n_up, W);         // base k of the window in bits 2 k, 2 k + 1
                if (collapse && (centre == 0u || centre == 2u)) {    // A / G centre: the reverse complement
                    uint32_t r = __builtin_bitreverse32(code);
                    r = ((r >> 1) & 0x55555555u) | ((r & 0x55555555u) << 1);
                    code = (r >> (32 - 2 * W)) ^ genome2_mask(W);
                }
            }
        }
        status[i] = (uint8_t)((match ? kMcMatch : 0u) | (head ? kMcHead : 0u) | (host ? kMcNeedsHost : 0u));
        context[i] = code;
    }
    const uint64_t heads = __ballot(have && head), bad = __ballot(have && !match);
    if (lane == 0 && i < N) {
        const int64_t w = i >> 6;
        wave_last[2 * w] = (int32_t)mc_last(heads, i);
        wave_last[2 * w + 1] = (int32_t)mc_last(bad, i);
    }
}

__device__ __forceinline__ int32_t mc_wave_max(int32_t v)
{
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) v = max(v, __shfl_xor(v, d, 64));
    return v;
}

__global__ __launch_bounds__(kMcBlock) void mutctx_resolve_kernel(const int32_t* __restrict__ wave_last, int64_t N,
                                                                   uint8_t* __restrict__ status)
{
    const int64_t i = (int64_t)blockIdx.x * kMcBlock + threadIdx.x;
    const int lane = threadIdx.x & 63;
    const int64_t w = i >> 6, base = i - lane;
    if (base >= N) return;                                           // (wave-uniform)
    const bool have = i < N;
    const unsigned f = have ? status[i] : 0u;
    const uint64_t heads = __ballot(have && (f & kMcHead)), bad = __ballot(have && !(f & kMcMatch));
    int64_t H = mc_last(heads & mc_upto(lane), base), B = mc_last(bad & mc_upto(lane), base);
    if (!(heads & 1ull)) {                                           // the wave's first row continues a run of earlier waves
        int32_t cH = -1, cB = -1;
        for (int64_t w0 = w - 1; w0 >= 0; w0 -= 64) {                // row 0 heads a run: the walk ends at wave 0 at the latest
                                                                     // (more than one step: test_mutation_context_runs_that_span_many_waves, tests/test_gpu_grid_wrap.py)
            const int64_t ww = w0 - lane;
            const int32_t ah = ww >= 0 ? wave_last[2 * ww] : -1, ab = ww >= 0 ? wave_last[2 * ww + 1] : -1;
            const uint64_t m = __ballot(ah >= 0);
            const int first = m ? __builtin_ctzll(m) : 64;          // the nearest wave with a head
            cB = max(cB, mc_wave_max(lane <= first ? ab : -1));
            if (m) {
                cH = __shfl(ah, first, 64);
                break;
            }
        }
        H = max(H, (int64_t)cH);
        B = max(B, (int64_t)cB);
    }
    if (!have) return;
    uint8_t out;
    if (!(f & kMcMatch)) out = DIG_MC_MISMATCH;
    else if (B >= H) out = DIG_MC_DROPPED;                           // a row of its run in front of it did not match
    else out = (f & kMcNeedsHost) ? DIG_MC_HOST : DIG_MC_KEPT;
    status[i] = out;
}

}  // namespace dig

using namespace dig;

extern "C" {

int64_t dig_mutation_contexts_workspace(int64_t n_rows)
{
    return n_rows > 0 ? 8 * ((n_rows + 63) / 64) : 0;
}

int dig_mutation_contexts(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                          const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                          const int32_t* row_chrom, const int64_t* row_start, const uint8_t* row_ref, int64_t n_rows, int n_up, int n_down,
                          int collapse, uint8_t* status, uint32_t* context, void* workspace, int64_t workspace_bytes, void* stream)
{
    DIG_REQUIRE(n_rows >= 0 && n_rows <= INT32_MAX, "0 <= n_rows < 2^31");
    DIG_REQUIRE(n_up >= 0 && n_down >= 0 && n_up + n_down + 1 <= 16, "n_up, n_down >= 0 and n_up + n_down + 1 <= 16");
    const Genome2 G = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, G, n_rows)) return rc;
    if (n_rows == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && row_chrom && row_start && row_ref && status && context && workspace,
                "non-null pointers");
    DIG_REQUIRE(workspace_bytes >= dig_mutation_contexts_workspace(n_rows), "workspace of dig_mutation_contexts_workspace bytes");
    DIG_REQUIRE(((uintptr_t)workspace & 3u) == 0, "workspace 4-byte aligned");
    const int grid = (int)((n_rows + kMcBlock - 1) / kMcBlock);
    int32_t* wave_last = static_cast<int32_t*>(workspace);
    hipLaunchKernelGGL(mutctx_lookup_kernel, dim3(grid), dim3(kMcBlock), 0, (hipStream_t)stream, G, row_chrom, row_start, row_ref,
                       n_rows, n_up, n_down, collapse, status, context, wave_last);
    DIG_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(mutctx_resolve_kernel, dim3(grid), dim3(kMcBlock), 0, (hipStream_t)stream, wave_last, n_rows, status);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
