// dig_context5.hip -- penta-nucleotide (n_up = n_down = 2) context counting over the 2-bit genome of dig_count_contexts2.
//
// Reference (one pysam fetch + a Python loop per region, the default n_up = n_down = 2):
//   sequence_tools.py:21-29   fetch_sequence      region widened by two bases on either side, START == 0 -> 2,
//                                                 truncated at the chromosome end, upper-cased
//   sequence_tools.py:42-55   seq_to_context      a window holding 'N' is skipped (here: any letter other than ACGT)
//   sequence_tools.py:65-80   count_sequence_context   1 024 counts of the centre positions
//   sequence_tools.py:527-566 nonc_elt_context_count   '-' strand: the sequence is reverse-complemented first
// Centres of a region run over [s, e), s = 2 if START == 0 else START, e = min(END, chrom_len - 2).
//
// The 64-bin kernel (dig_count_contexts2) gives each lane a column of 256 sixteen-bit counters; 1 024 bins do not fit that
// shape.  Here a WAVE owns a region and a 4 KB histogram of 1 024 thirty-two-bit counters in LDS (no counter can wrap:
// a whole chromosome is one region), and every centre is one ds_add_u32:
//   * a lane takes two consecutive words of the 2-bit genome per step (32 centres, one 8-byte load plus the word in
//     front and the word behind), the wave 2 048 bases per step, the next step's loads issued before the current one is
//     counted;
//   * with the neighbouring bases joined in, the 64-bit string (hi:lo) holds base 16 w + j at bit 6 + 2 j, so the byte
//     offset of centre k's bin (4 x its 10-bit code, left base in the low bits) is one v_alignbit and one and-or away;
//   * a letter other than ACGT is stored as A: the scan counts a run's windows as they are stored, and the lanes then
//     take back, one run per lane, every centre whose window touches a run -- a run's interior as AAAAA, its up to four
//     edge centres on either side looked up; a region whose windows all lie inside one run is not scanned at all;
//   * the output stage reads bin code(ctx) for context ctx (ctx = 256 b0 + 64 b1 + 16 b2 + 4 b3 + b4, code = the same
//     digits in reverse order); a '-' strand region reads bin 1023 - ctx, which is code(revcomp(ctx)).
#include "dig_genome2.hpp"

namespace dig {

constexpr int kC5Block = 256;               // four waves, one region per wave at a time

typedef __attribute__((address_space(3))) unsigned lds5_u32;

#define DIG_C5_ADD(addr, val) \
    __hip_atomic_fetch_add(reinterpret_cast<lds5_u32*>(static_cast<uintptr_t>(addr)), (unsigned)(val), __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP)

// the centres k = lo .. hi - 1 of word w (array bases 16 w + k); prev / cur / next = words w - 1, w, w + 1; hist_addr = LDS
// byte address of the wave's 4 KB-aligned histogram.  kFull: all 16 centres, no range test.
template <bool kFull>
__device__ __forceinline__ void c5_count_word(uint32_t prev, uint32_t cur, uint32_t next, unsigned hist_addr, int lo, int hi)
{
    // bases 16 w - 3 .. 16 w + 28 at bits 0 .. 63 of (b:a); centre k's window starts at bit 2 + 2 k
    const uint32_t a = (cur << 6) | (prev >> 26);
    const uint32_t b = (cur >> 26) | (next << 6);
    unsigned addr[16];
#pragma unroll
    for (int k = 0; k < 16; ++k) addr[k] = (__builtin_amdgcn_alignbit(b, a, 2 * k) & 0xffcu) | hist_addr;
#pragma unroll
    for (int k = 0; k < 16; ++k)
        if (kFull || (k >= lo && k < hi)) DIG_C5_ADD(addr[k], 1u);
}

__device__ __forceinline__ int c5_rev_digits(int ctx)      // the five base-4 digits in reverse order
{
    return ((ctx & 3) << 8) | ((ctx & 12) << 4) | (ctx & 48) | ((ctx >> 4) & 12) | ((ctx >> 8) & 3);
}

__global__ __launch_bounds__(kC5Block) void context_count5_kernel(
    Genome2 G, const int32_t* __restrict__ reg_chrom, const int64_t* __restrict__ reg_start, const int64_t* __restrict__ reg_end,
    const uint8_t* __restrict__ reg_minus, int64_t R, int32_t* __restrict__ out)
{
    const uint32_t* __restrict__ words = G.words;
    const int64_t n_int = G.n_int;
    __shared__ alignas(4096) uint32_t hist_all[kC5Block / 64][1024];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    uint32_t* hist = hist_all[wave];
    uint4* hist4 = reinterpret_cast<uint4*>(hist);
    const unsigned hist_addr = (unsigned)(uintptr_t)(lds5_u32*)hist;        // a multiple of 4 096: the bin offset is or-ed in
#pragma unroll
    for (int i = 0; i < 4; ++i) hist4[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
    __builtin_amdgcn_wave_barrier();
    const int64_t nwaves = (int64_t)gridDim.x * (kC5Block / 64);
    for (int64_t r = (int64_t)blockIdx.x * (kC5Block / 64) + wave; r < R; r += nwaves) {
        const int ch = reg_chrom[r];
        const int minus = reg_minus[r];
        const int64_t len = G.chrom_len[ch], off = G.chrom_off[ch] + kGenome2PadBases;
        int64_t s = reg_start[r], e = reg_end[r];
        if (s < 2) s = 2;                                   // START == 0 -> 2 (fetch_sequence :25-26); the callers refuse 0 < START < 2
        if (e > len - 2) e = len - 2;                       // the fetch is truncated: the last centre is len - 3
        const int64_t gs = off + s, ge = off + e;           // centres [gs, ge) in array bases
        bool scan = ge > gs;
        int64_t jf = n_int;                                 // first run that overlaps the widened region [gs - 2, ge + 2)
        if (scan && n_int > 0) {
            const int64_t x0 = gs - 2, x1 = ge + 2;
            jf = genome2_first_run(G, x0);
            if (jf < n_int && G.nint_start[jf] <= x0 && G.nint_end[jf] >= x1) scan = false;    // every window lies inside one run
        }
        if (scan) {
            // word pairs v (words 2 v, 2 v + 1) from the pair of the first centre to the pair of the last
            const int64_t W0 = gs >> 4, W1 = (ge - 1) >> 4, V1 = W1 >> 1;
            int64_t v = (W0 >> 1) + lane;
            uint2 cur = make_uint2(0u, 0u);
            uint32_t before = 0, after = 0;
            if (v <= V1) {
                cur = *reinterpret_cast<const uint2*>(words + 2 * v);
                before = words[2 * v - 1];
                after = words[2 * v + 2];
            }
            while (v <= V1) {
                const int64_t vn = v + 64;
                uint2 nxt = make_uint2(0u, 0u);
                uint32_t nb = 0, na = 0;
                if (vn <= V1) {
                    nxt = *reinterpret_cast<const uint2*>(words + 2 * vn);
                    nb = words[2 * vn - 1];
                    na = words[2 * vn + 2];
                }
                const uint32_t wd[4] = {before, cur.x, cur.y, after};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    const int64_t b0 = 16 * (2 * v + j);                     // array base of centre k = 0
                    const int lo = gs > b0 ? (gs - b0 < 16 ? (int)(gs - b0) : 16) : 0;
                    const int hi = ge - b0 < 16 ? (ge - b0 > 0 ? (int)(ge - b0) : 0) : 16;
                    if (lo == 0 && hi == 16)
                        c5_count_word<true>(wd[j], wd[j + 1], wd[j + 2], hist_addr, 0, 16);
                    else
                        c5_count_word<false>(wd[j], wd[j + 1], wd[j + 2], hist_addr, lo, hi);
                }
                cur = nxt;
                before = nb;
                after = na;
                v = vn;
            }
            // ---- centres whose window touches a non-ACGT run: taken back, one run per lane ----
            // (a run's interior counts as AAAAA, code 0; its edge centres are looked up)
            genome2_take_back<2>(G, jf + lane, 64, gs, ge, [&](int64_t n) { DIG_C5_ADD(hist_addr, 0u - (unsigned)n); },
                                 [&](unsigned code) { DIG_C5_ADD(hist_addr + 4u * code, 0xffffffffu); });
        }
        // (one wave owns this histogram: LDS operations of a wave complete in order, no barrier needed)
        __builtin_amdgcn_wave_barrier();
        int32_t* row = out + r * 1024;
#pragma unroll
        for (int t = 0; t < 4; ++t) {
            const int ctx0 = 4 * (lane + 64 * t);
            int32_t val[4];
#pragma unroll
            for (int i = 0; i < 4; ++i) val[i] = (int32_t)hist[minus ? 1023 - (ctx0 + i) : c5_rev_digits(ctx0 + i)];
            *reinterpret_cast<int4*>(row + ctx0) = make_int4(val[0], val[1], val[2], val[3]);
        }
        __builtin_amdgcn_wave_barrier();
#pragma unroll
        for (int i = 0; i < 4; ++i) hist4[i * 64 + lane] = make_uint4(0u, 0u, 0u, 0u);
        __builtin_amdgcn_wave_barrier();
    }
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_count_contexts5(const uint32_t* words2, int64_t n_words2, const int64_t* nint_start, const int64_t* nint_end, int64_t n_int,
                        const int32_t* nint_bucket, int64_t n_buckets, const int64_t* chrom_off, const int64_t* chrom_len, int n_chrom,
                        const int32_t* reg_chrom, const int64_t* reg_start, const int64_t* reg_end, const uint8_t* reg_minus, int64_t R,
                        int32_t* out, void* stream)
{
    const Genome2 G = {words2, n_words2, nint_start, nint_end, n_int, nint_bucket, n_buckets, chrom_off, chrom_len, n_chrom};
    if (int rc = genome2_check(__func__, G, R, true)) return rc;
    if (R == 0) return DIG_OK;
    DIG_REQUIRE(words2 && chrom_off && chrom_len && reg_chrom && reg_start && reg_end && reg_minus && out, "non-null pointers");
    DIG_REQUIRE(((uintptr_t)words2 & 15) == 0 && ((uintptr_t)out & 15) == 0, "words2 and out 16-byte aligned");
    const int grid = grid_for(R * 64, kC5Block, 8);     // one wave per region, 16 KB of LDS per workgroup
    hipLaunchKernelGGL(context_count5_kernel, dim3(grid), dim3(kC5Block), 0, (hipStream_t)stream, G, reg_chrom, reg_start,
                       reg_end, reg_minus, R, out);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
