// dig_eltcontext.hip -- the strand-aware trinucleotide counts of bed12 ELEMENTS straight from the 2-bit genome: the L of
// quickDriver's ad-hoc elements (driver_model/onthefly_tools.py: one dig_count_contexts2 row per block, a 192-column frame
// keyed by 'chr{}:{}-{}' strings and np.add.at per element on the host) for 10^5 - 10^6 elements in one pass.
//
// Definition: out[e] = the sum over the blocks b of element e of the row dig_count_contexts2 gives for
// (elt_chrom[e], blk_start[b], blk_end[b], elt_minus[e]) -- centres max(start, 1) .. min(end, chrom_len - 1) - 1, a triplet that
// touches a letter other than ACGT skipped, the reverse complement for a '-' element.  Integer counts: any order of summation
// gives the same bits.
//
// Mapping.  The unit of work is the BLOCK, not the element: an element of a thousand ten-base blocks is a thousand units, spread
// over as many waves as the grid has, and a block of megabases is cut across 1 024 waves.
//   elt_context_kernel        a wave takes a tile of 16 consecutive blocks: lanes 0..15 find their block's owner (an upper-bound
//                             search of blk_ptr, 16 searches for the latency of one) and its clamped range, then the wave walks
//                             the 16 blocks, lane = one 16-base word of the block per step (words w - 1, w, w + 1 give the 16
//                             triplets centred in word w; centres outside the range are masked in the first and last word).
//                             The counters are the wave's own LDS histogram, 64 codes x 16 copies (copy = lane mod 16: no
//                             same-address serialisation on AAA / TTT runs), so a base costs one LDS add and no global atomic.
//                             Centres whose window touches a non-ACGT run -- stored as A -- are taken back in the same histogram
//                             (genome2_take_back, the runs of a block strided over the lanes).  Consecutive blocks of one element
//                             share the histogram; when the owner changes (and at the tile's end) lane = context adds its total to
//                             out[e] with ONE integer atomic per non-zero context.  A block of more than kEcLongBases centres is
//                             not counted here: its (element, block) goes to a list in the workspace.
//   elt_context_long_kernel   the listed blocks, grid (kEcSplit workgroups) x (list entries): the 4 kEcSplit waves of an entry take
//                             the block's words 64 at a time, strided; wave 0 of the entry takes the runs back; every wave adds
//                             its 64 totals to out[e].  An empty list costs one launch of workgroups that return at once.
// Both grids are capped and wrap (grid-stride over tiles / list entries / words).  out is zeroed first (hipMemsetAsync): an
// element without blocks, an empty or inverted block and a chromosome id outside the genome add nothing.
// Measured on MI355X (tools/quick_cohorts_bench.py; DESIGN.md, Ad-hoc elements of many cohorts): 10^5 elements of 1 to 3 blocks of
// 200 to 3 000 bp 0.184 ms = 0.60 TB/s of the bytes read (bound by the LDS adds and the flush, not by HBM); one 5 Mb block 0.039 ms,
// of which 0.024 ms are the call's floor (two memsets, two launches) -- the cut into 1 024 waves that all add to one 256-byte row is
// too fine for a single block.
#include "dig_genome2.hpp"

namespace dig {

constexpr int kEcBlock = 256;
constexpr int kEcWaves = kEcBlock / 64;
constexpr int kEcCopies = 16;                  // histogram copies per wave (lane mod kEcCopies)
constexpr int kEcTile = 16;                    // consecutive blocks per wave and step
constexpr int kEcPerCu = 8;                    // workgroups per CU the first grid is capped at
constexpr int64_t kEcLongBases = 32768;        // a block with more centres than this is cut across waves
constexpr int kEcSplit = 256;                  // workgroups that share one long block
constexpr int kEcLongRows = 64;                // long blocks in flight (grid.y cap)
constexpr int64_t kEcListOffset = 16;          // workspace: the list's length (u32) in front, the entries from byte 16 on

struct EcLong {
    int32_t elt, blk;
};

__device__ __forceinline__ int ec_revcomp(int c)                       // context 16 b0 + 4 b1 + b2 of the reverse complement
{
    return ((3 - (c & 3)) << 4) | ((3 - ((c >> 2) & 3)) << 2) | (3 - (c >> 4));
}

__device__ __forceinline__ void ec_wave_sync()                         // LDS operations of one wave complete in order
{
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

__device__ __forceinline__ void ec_zero(uint32_t* hist, int lane)
{
#pragma unroll
    for (int i = 0; i < 64 * kEcCopies / 4 / 64; ++i) reinterpret_cast<uint4*>(hist)[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
}

// centres [gs, ge) (array bases, gs < ge) of the words first_word + lane, + word_stride, ... counted as they are stored, by CODE
// (left base in the low bits) in column `col` of the wave's histogram
__device__ __forceinline__ void ec_count_words(const uint32_t* __restrict__ words, int64_t gs, int64_t ge, int64_t first_word,
                                               int64_t word_stride, uint32_t* col, int lane)
{
    const int64_t w1 = (ge - 1) >> 4;
    int64_t w = first_word + lane;
    uint32_t prev = 0, cur = 0, next = 0;
    if (w <= w1) prev = words[w - 1], cur = words[w], next = words[w + 1];
    while (w <= w1) {
        const int64_t wn = w + word_stride;                             // the next step's words are requested before this one is counted
        uint32_t nprev = 0, ncur = 0, nnext = 0;
        if (wn <= w1) nprev = words[wn - 1], ncur = words[wn], nnext = words[wn + 1];
        // bases 16 w - 1 .. 16 w + 16: centre k of the word has its triplet at bits 2 k .. 2 k + 5
        const uint64_t x = (uint64_t)(prev >> 30) | ((uint64_t)cur << 2) | ((uint64_t)(next & 3u) << 34);
        const int64_t g0 = w << 4;
        const int k0 = gs > g0 ? (int)(gs - g0) : 0, k1 = ge - g0 < 16 ? (int)(ge - g0) : 16;
        if (k0 == 0 && k1 == 16) {
#pragma unroll
            for (int k = 0; k < 16; ++k) atomicAdd(&col[((unsigned)(x >> (2 * k)) & 63u) * kEcCopies], 1u);
        } else {
#pragma unroll
            for (int k = 0; k < 16; ++k)
                if (k >= k0 && k < k1) atomicAdd(&col[((unsigned)(x >> (2 * k)) & 63u) * kEcCopies], 1u);
        }
        prev = nprev, cur = ncur, next = nnext;
        w = wn;
    }
}

// the centres of [gs, ge) whose window touches a non-ACGT run, taken back from the histogram: the runs strided over the lanes
__device__ __forceinline__ void ec_take_back(const Genome2& G, int64_t gs, int64_t ge, uint32_t* col, int lane)
{
    if (G.n_int <= 0) return;
    const int64_t jf = genome2_first_run(G, gs - 1);                    // first run that ends behind the widened range's first base
    if (jf >= G.n_int || G.nint_start[jf] >= ge + 1) return;
    genome2_take_back<1>(G, jf + lane, 64, gs, ge, [&](int64_t n) { atomicAdd(&col[0], (uint32_t)0 - (uint32_t)n); },
                         [&](unsigned code) { atomicAdd(&col[code * kEcCopies], 0xffffffffu); });
}

// lane = context: the histogram's total of the context (of its reverse complement for a '-' element) added to row[lane]; the
// histogram is left zeroed
__device__ __forceinline__ void ec_flush(uint32_t* hist, int32_t* __restrict__ row, bool minus, int lane)
{
    ec_wave_sync();
    const int ctx = minus ? ec_revcomp(lane) : lane;
    const int code = ((ctx >> 4) & 3) | (ctx & 12) | ((ctx & 3) << 4);
    uint32_t total = 0;
#pragma unroll
    for (int j = 0; j < kEcCopies; ++j) total += hist[code * kEcCopies + ((j + lane) & (kEcCopies - 1))];
    if (total) atomicAdd(&row[lane], (int32_t)total);
    ec_wave_sync();
    ec_zero(hist, lane);
    ec_wave_sync();
}

// centres [gs, ge) in array bases of block b of an element on chromosome ch; false: nothing to count
__device__ __forceinline__ bool ec_range(const Genome2& G, int ch, int64_t s, int64_t e, int64_t& gs, int64_t& ge)
{
    if (ch < 0 || ch >= G.n_chrom) return false;
    const int64_t len = G.chrom_len[ch], off = G.chrom_off[ch] + kGenome2PadBases;
    if (s < 1) s = 1;                                                   // fetch_sequence: START == 0 -> 1
    if (e > len - 1) e = len - 1;                                       // the fetch is truncated: the last centre is len - 2
    if (e <= s) return false;
    gs = off + s;
    ge = off + e;
    return true;
}

__global__ __launch_bounds__(kEcBlock) void elt_context_kernel(Genome2 G, const int32_t* __restrict__ elt_chrom,
                                                               const uint8_t* __restrict__ elt_minus,
                                                               const int64_t* __restrict__ blk_ptr,
                                                               const int64_t* __restrict__ blk_start,
                                                               const int64_t* __restrict__ blk_end, int64_t E, int64_t n_blocks,
                                                               int32_t* __restrict__ out, uint32_t* __restrict__ n_long,
                                                               EcLong* __restrict__ longs)
{
    __shared__ alignas(16) uint32_t hist_all[kEcWaves][64 * kEcCopies];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* hist = hist_all[wave];
    uint32_t* col = hist + (lane & (kEcCopies - 1));
    ec_zero(hist, lane);
    ec_wave_sync();
    const int64_t n_tiles = (n_blocks + kEcTile - 1) / kEcTile;
    for (int64_t t = (int64_t)blockIdx.x * kEcWaves + wave; t < n_tiles; t += (int64_t)gridDim.x * kEcWaves) {
        // lanes 0 .. kEcTile - 1: the owner and the range of block t kEcTile + lane
        int64_t my_e = -1, my_gs = 0, my_ge = 0;
        const int64_t my_b = t * kEcTile + lane;
        if (lane < kEcTile && my_b < n_blocks) {
            int64_t lo = 0, hi = E + 1;                                 // the first index whose blk_ptr lies behind the block
            while (lo < hi) {
                const int64_t mid = (lo + hi) >> 1;
                if (blk_ptr[mid] > my_b) hi = mid; else lo = mid + 1;
            }
            const int64_t e = lo - 1;
            if (e >= 0 && e < E && ec_range(G, elt_chrom[e], blk_start[my_b], blk_end[my_b], my_gs, my_ge)) my_e = e;
        }
        int64_t cur = -1;                                               // the element whose counts the histogram holds
        for (int i = 0; i < kEcTile; ++i) {
            const int64_t e = __shfl(my_e, i);
            if (e < 0) continue;                                        // (wave-uniform)
            const int64_t gs = __shfl(my_gs, i), ge = __shfl(my_ge, i);
            if (ge - gs > kEcLongBases) {
                if (lane == 0) {
                    const uint32_t at = atomicAdd(n_long, 1u);
                    if ((int64_t)at < n_blocks) longs[at] = EcLong{(int32_t)e, (int32_t)(t * kEcTile + i)};
                }
                continue;
            }
            if (cur >= 0 && cur != e) ec_flush(hist, out + cur * 64, elt_minus[cur] != 0, lane);
            cur = e;
            ec_count_words(G.words, gs, ge, gs >> 4, 64, col, lane);
            ec_take_back(G, gs, ge, col, lane);
        }
        if (cur >= 0) ec_flush(hist, out + cur * 64, elt_minus[cur] != 0, lane);
    }
}

__global__ __launch_bounds__(kEcBlock) void elt_context_long_kernel(Genome2 G, const int32_t* __restrict__ elt_chrom,
                                                                    const uint8_t* __restrict__ elt_minus,
                                                                    const int64_t* __restrict__ blk_start,
                                                                    const int64_t* __restrict__ blk_end, int64_t E, int64_t n_blocks,
                                                                    int32_t* __restrict__ out, const uint32_t* __restrict__ n_long,
                                                                    const EcLong* __restrict__ longs)
{
    __shared__ alignas(16) uint32_t hist_all[kEcWaves][64 * kEcCopies];
    const int64_t listed = *n_long;
    const int64_t n = listed < n_blocks ? listed : n_blocks;
    if ((int64_t)blockIdx.y >= n) return;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* hist = hist_all[wave];
    uint32_t* col = hist + (lane & (kEcCopies - 1));
    ec_zero(hist, lane);
    ec_wave_sync();
    const int64_t wi = (int64_t)blockIdx.x * kEcWaves + wave, nw = (int64_t)gridDim.x * kEcWaves;
    for (int64_t i = blockIdx.y; i < n; i += gridDim.y) {
        const EcLong item = longs[i];
        const int64_t e = item.elt, b = item.blk;
        int64_t gs = 0, ge = 0;
        if (e < 0 || e >= E || b < 0 || b >= n_blocks || !ec_range(G, elt_chrom[e], blk_start[b], blk_end[b], gs, ge)) continue;
        ec_count_words(G.words, gs, ge, (gs >> 4) + wi * 64, nw * 64, col, lane);
        if (wi == 0) ec_take_back(G, gs, ge, col, lane);
        ec_flush(hist, out + e * 64, elt_minus[e] != 0, lane);
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int64_t dig_element_context_counts_workspace(int64_t n_blocks)
{
    return kEcListOffset + (int64_t)sizeof(EcLong) * (n_blocks > 0 ? n_blocks : 0);
}

int dig_element_context_counts(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                               const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len,
                               int n_chrom, const int32_t* elt_chrom, const uint8_t* elt_minus, const int64_t* blk_ptr,
                               const int64_t* blk_start, const int64_t* blk_end, int64_t E, int64_t n_blocks, int32_t* out,
                               void* workspace, int64_t workspace_bytes, void* stream)
{
    DIG_REQUIRE(E >= 0 && n_blocks >= 0, "E, n_blocks >= 0");
    DIG_REQUIRE(E < ((int64_t)1 << 31) && n_blocks < ((int64_t)1 << 31), "E, n_blocks < 2^31");
    const Genome2 G = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, G, E)) return rc;
    if (E == 0) return DIG_OK;
    DIG_REQUIRE(out, "non-null out");
    DIG_REQUIRE(((uintptr_t)out & 3) == 0, "out 4-byte aligned");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(out, 0, (size_t)E * 64 * sizeof(int32_t), s));
    if (n_blocks == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len, "non-null genome arrays");
    DIG_REQUIRE(((uintptr_t)words2 & 15) == 0, "words2 16-byte aligned");
    DIG_REQUIRE(elt_chrom && elt_minus && blk_ptr && blk_start && blk_end, "non-null elt_chrom, elt_minus, blk_ptr, blk_start, blk_end");
    DIG_REQUIRE(workspace && workspace_bytes >= dig_element_context_counts_workspace(n_blocks),
                "workspace of dig_element_context_counts_workspace(n_blocks) bytes");
    DIG_REQUIRE(((uintptr_t)workspace & 7) == 0, "workspace 8-byte aligned");
    uint32_t* n_long = static_cast<uint32_t*>(workspace);
    EcLong* longs = reinterpret_cast<EcLong*>(static_cast<char*>(workspace) + kEcListOffset);
    DIG_HIP_TRY(hipMemsetAsync(n_long, 0, kEcListOffset, s));
    const int64_t n_tiles = (n_blocks + kEcTile - 1) / kEcTile;
    const int grid = grid_for(n_tiles * 64, kEcBlock, kEcPerCu);        // a wave per tile; past the cap the waves take further tiles
    hipLaunchKernelGGL(elt_context_kernel, dim3(grid), dim3(kEcBlock), 0, s, G, elt_chrom, elt_minus, blk_ptr, blk_start, blk_end, E,
                       n_blocks, out, n_long, longs);
    DIG_HIP_TRY(hipGetLastError());
    const unsigned rows = (unsigned)(n_blocks < kEcLongRows ? n_blocks : kEcLongRows);       // past the cap a row takes further entries
    hipLaunchKernelGGL(elt_context_long_kernel, dim3(kEcSplit, rows), dim3(kEcBlock), 0, s, G, elt_chrom, elt_minus, blk_start, blk_end,
                       E, n_blocks, out, n_long, longs);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
