// dig_tiles.hpp -- what the kernels of the per-base route (dig_tiles.hip, dig_tiles_rows.hip, dig_tilesamples.hip, dig_tilesparse.hip, dig_tilesparsewindows.hip)
// and their host twins (dig_host.hip) share: the view of the 4-bit genome and the region table (TileGenome) with a region's positions,
// the packed-word window of a base range and its staging, the two nibble squeezes, the cohort operands of the matrix kernels, the
// tile a mutation row counts in (tile_slot), and on the host the argument block of the entry points that take the genome (TileArgs:
// launch, check_tile_args) and the DIG_TILES_FORM switch.
#pragma once
#include <stdlib.h>

#include <type_traits>

#include "dig_common.hpp"

namespace dig {

// ---- the 4-bit genome and the region table ----
constexpr int kCtxMaxPos = 16384;       // positions of the longest penta-nucleotide region that is evaluated (engine.TILE_CTX_MAX_POSITIONS)
constexpr int tile_contexts(int n_up) { return 1 << (2 * (2 * n_up + 1)); }      // rows of a cohort's table: 64 (n_up 1) or 1024 (2)

// The nine genome and region arguments of an entry point, in their order; the sparse kernels take it by value.
struct TileGenome {
    const uint32_t* words;
    int64_t n_words;
    const int64_t *chrom_off, *chrom_len;
    int n_chrom;
    const int32_t* reg_chrom;
    const int64_t *reg_start, *reg_end;
    int64_t R;
};

struct TileRegion {
    int64_t first;      // first position (chromosome coordinates)
    int64_t n_pos;      // number of positions
    int64_t g0;         // global base index of position `first` (counted from word 1 of the genome array)
};

// fetch_sequence (sequence_tools.py:21-29) with n_up = n_down = U: START == 0 becomes U; the fetch is widened by U bases on
// either side and cut at the chromosome end, so the last position with a full window is len - U - 1.  (len, off: the
// chromosome's row of the genome tables.)
__device__ __forceinline__ TileRegion region_positions(int U, int64_t len, int64_t off, int64_t start, int64_t end)
{
    TileRegion t;
    t.first = start == 0 ? U : start;
    const int64_t stop = end < len - U ? end : len - U;       // one past the last position
    t.n_pos = stop > t.first ? stop - t.first : 0;
    t.g0 = off + t.first;
    return t;
}

// region r of the view, with a chromosome id outside the table read as a region without positions; too_long: a penta-nucleotide
// region of more than kCtxMaxPos positions, which no kernel evaluates
template <int U>
__device__ __forceinline__ TileRegion sparse_region(const TileGenome& g, int64_t r, bool* too_long)
{
    const int chrom = g.reg_chrom[r];
    const int64_t start = g.reg_start[r], end = g.reg_end[r];
    TileRegion q{start == 0 ? U : start, 0, 0};
    if ((unsigned)chrom < (unsigned)g.n_chrom) q = region_positions(U, g.chrom_len[chrom], g.chrom_off[chrom], start, end);
    *too_long = U == 2 && q.n_pos > kCtxMaxPos;
    return q;
}

// ---- the tile a mutation row counts in ----
// A row (START `start`, cohort c) paired with region r (first_pos, n_valid: the region's entries of the tables the probability kernels
// and the census write): the slot (c R + r) n_tiles + t of its tile, or -1 for a row that counts nowhere -- START in front of the region
// (nb_model.py:160-163), a tile at or past n_valid (<= 0: a region without tiles) or n_tiles, a cohort outside [0, C), in this order.
__device__ __forceinline__ int64_t tile_slot(int64_t start, int64_t c, int64_t first_pos, int64_t n_valid, int binsize, int64_t n_tiles,
                                             int64_t R, int64_t C, int64_t r)
{
    const int64_t off = start - first_pos;
    if (off < 0) return -1;
    const int64_t t = off / binsize;
    if (t >= n_valid || t >= n_tiles) return -1;
    if ((uint64_t)c >= (uint64_t)C) return -1;
    return (c * R + r) * n_tiles + t;
}

// ---- the packed words of a base range (eight 4-bit codes per word; word 0 of the array is the leading pad word) ----
__device__ __forceinline__ int64_t word_of_base(int64_t g) { return (g >> 3) + 1; }      // array word = genome word + 1

struct WordWindow {
    int64_t w0;         // array word of the leftmost base
    int sh;             // nibble of the leftmost base in that word
    int64_t nw;         // words that cover the range, exactly: a caller that reads past the range adds its own margin
    int64_t g_lds0;     // global base index of nibble 0 of word w0 (LDS word 0 of a staged window)
};
__device__ __forceinline__ WordWindow word_window(int64_t ga, int64_t n_bases)
{
    WordWindow v;
    v.w0 = word_of_base(ga);
    v.sh = (int)(ga & 7);
    v.nw = ((v.sh + n_bases - 1) >> 3) + 1;
    v.g_lds0 = ga - v.sh;
    return v;
}

// array word w, clamped to the trailing pad word (NT: a non-temporal load)
template <bool NT = false>
__device__ __forceinline__ uint32_t load_word(const uint32_t* __restrict__ words, int64_t n_words, int64_t w)
{
    const uint32_t* p = &words[w < n_words ? w : n_words - 1];
    return NT ? __builtin_nontemporal_load(p) : *p;
}

// 4-bit code of global base g: out of staged words, and straight from the packed array
__device__ __forceinline__ unsigned tile_base(const uint32_t* s_words, int64_t g, int64_t g_lds0)
{
    const int64_t r = g - g_lds0;                               // base index inside the staged words
    return (s_words[r >> 3] >> (4 * (int)(r & 7))) & 15u;
}
__device__ __forceinline__ unsigned tile_base_global(const uint32_t* __restrict__ words, int64_t n_words, int64_t g)
{
    return (load_word(words, n_words, word_of_base(g)) >> (4 * (int)(g & 7))) & 15u;
}

// Staging nw <= PER * BLOCK words from array word w0 on, thread tid of BLOCK: all loads of a thread are issued before its first
// LDS write -- the plain loop `s_words[i] = words[...]` waits for every load in turn (one memory round trip per BLOCK words
// instead of one per region).  The halves are separate for the kernels that keep the registers across a region's walk.
template <int PER, int BLOCK, bool NT = false>
__device__ __forceinline__ void stage_load(uint32_t (&tmp)[PER], const uint32_t* __restrict__ words, int64_t n_words, int64_t w0,
                                           int64_t nw, int tid)
{
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t i = tid + (int64_t)j * BLOCK;
        tmp[j] = i < nw ? load_word<NT>(words, n_words, w0 + i) : 0u;
    }
}
template <int PER, int BLOCK>
__device__ __forceinline__ void stage_store(uint32_t* s_words, const uint32_t (&tmp)[PER], int64_t nw, int tid)
{
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int64_t i = tid + (int64_t)j * BLOCK;
        if (i < nw) s_words[i] = tmp[j];
    }
}
template <int PER, int BLOCK>
__device__ __forceinline__ void stage_words(uint32_t* s_words, const uint32_t* __restrict__ words, int64_t n_words, int64_t w0,
                                            int64_t nw, int tid)
{
    uint32_t tmp[PER];
    stage_load<PER, BLOCK>(tmp, words, n_words, w0, nw, tid);
    stage_store<PER, BLOCK>(s_words, tmp, nw, tid);
}

// ---- the eight nibbles of a packed word, squeezed ----
__device__ __forceinline__ uint32_t squeeze_bases(uint32_t w)       // 2-bit bases: base n at bits 2 n
{
    uint32_t x = w & 0x33333333u;
    x = (x | (x >> 2)) & 0x0F0F0F0Fu;
    x = (x | (x >> 4)) & 0x00FF00FFu;
    return (x | (x >> 8)) & 0xFFFFu;
}
__device__ __forceinline__ uint32_t nonacgt_flags(uint32_t w)       // base n is not A, C, G or T: bit n
{
    uint32_t f = ((w >> 2) | (w >> 3)) & 0x11111111u;
    f = (f | (f >> 3)) & 0x03030303u;
    f = (f | (f >> 6)) & 0x000F000Fu;
    return (f | (f >> 12)) & 0xFFu;
}

// ---- the sparse routes (dig_tilesparse.hip, dig_tilesparsewindows.hip) ----
constexpr int kSparseBlock = 256;
constexpr int64_t kSparseNoKey = INT64_MAX;          // a pair that counts nowhere: sorts behind every real key

// The windows of consecutive positions, one base at a time: ref is the table index of the last W bases (the leftmost base counts
// highest, as itertools.product orders the contexts), good the bases since the last letter other than ACGT.
template <int U>
struct WindowWalk {
    static constexpr int W = 2 * U + 1, K = 1 << (2 * W);
    const uint32_t* words;
    int64_t n_words, cw;
    uint32_t word;
    unsigned ref;
    int good;

    __device__ __forceinline__ WindowWalk(const uint32_t* w, int64_t nw) : words(w), n_words(nw), cw(-1), word(0), ref(0), good(0) {}
    __device__ __forceinline__ void push(int64_t g)
    {
        int64_t w = word_of_base(g);
        w = w < 0 ? 0 : (w < n_words ? w : n_words - 1);           // (never outside the array, whatever the region table holds)
        if (w != cw) {
            cw = w;
            word = words[w];
        }
        const unsigned b = (word >> (4 * (int)(g & 7))) & 15u;
        ref = ((ref << 2) | (b & 3u)) & (unsigned)(K - 1);
        good = b < 4u ? good + 1 : 0;
    }
    // in front of the first position p (global base g): the W - 1 bases to the left of its window's last one
    __device__ __forceinline__ void start(int64_t g)
    {
        for (int i = -U; i < U; ++i) push(g + i);
    }
    // position at global base g: true when its window is all ACGT (ref is then its context)
    __device__ __forceinline__ bool step(int64_t g)
    {
        push(g + U);
        return good >= W;
    }
};

// dig_tilesparse.hip: the cohort masks of the census, [ceil(C / 64)][4^W] words (tile_census_workspace_bytes, dig_keyruns.hpp) into
// `mask`: per context the cohorts of a pass whose table entry is positive
void launch_tile_census_mask(const double* s_prob, int64_t C, int n_up, uint64_t* mask, hipStream_t stream);

// ---- the cohort operands of the matrix kernels ----
// A[m][ks]: lane 16 k + i holds S[c0 + 16 m + i][context of histogram row 4 ks + k] (v_mfma_f64_16x16x4); Aq[q][ks]: A[i][k] of
// every 4x4 block b sits in lane 16 k + 4 b + i (v_mfma_f64_4x4x4).  The histogram rows are in the order the walk produces them
// (first base in the low bits: b0 + 4 b1 + 16 b2), the table's contexts are 16 b0 + 4 b1 + b2.  A lane that is not `active`
// (and a cohort at or beyond C) holds zeros.
template <int MT, int NQ>
__device__ __forceinline__ void load_cohort_operands(double (&A)[MT > 0 ? MT : 1][16], double (&Aq)[NQ > 0 ? NQ : 1][16],
                                                     const double* __restrict__ s_prob, int c0, int64_t C, int lane, bool active)
{
    constexpr int MTA = MT > 0 ? MT : 1, NQA = NQ > 0 ? NQ : 1;
    const int li = lane & 15, lk = lane >> 4;
#pragma unroll
    for (int ks = 0; ks < 16; ++ks) {
        const int row = 4 * ks + lk;
        const int ctx = ((row & 3) << 4) | (row & 12) | (row >> 4);
#pragma unroll
        for (int m = 0; m < MTA; ++m) {
            const int64_t c = c0 + 16 * m + li;
            A[m][ks] = (active && m < MT && c < C) ? s_prob[c * 64 + ctx] : 0.0;
        }
#pragma unroll
        for (int q = 0; q < NQA; ++q) {
            const int64_t c = c0 + 16 * MT + 4 * q + (lane & 3);
            Aq[q][ks] = (active && q < NQ && c < C) ? s_prob[c * 64 + ctx] : 0.0;
        }
    }
}

// ---- host side ----
// The 14 arguments the entry points that walk the genome begin with (n_up = 1 for dig_base_tile_probs, which has none) and the three
// outputs of the probability kernels.  Those kernels keep their own parameter lists (and their __restrict__): `launch` puts the genome,
// the regions and the table in front of a kernel's own arguments, the outputs behind them, and returns the call that takes the rest.
struct TileArgs {
    TileGenome g;
    const double* s_prob;
    int64_t C;
    int n_up, binsize;
    int64_t n_tiles;
    double* pt;
    int64_t* first_pos;
    int32_t* n_valid;
    hipStream_t stream;

    template <class Kernel, class... Own>
    auto launch(Kernel kernel, int grid, int block, Own... own) const
    {
        return [=, a = *this](auto... last) {
            hipLaunchKernelGGL(kernel, dim3(grid), dim3(block), 0, a.stream, a.g.words, a.g.n_words, a.g.chrom_off, a.g.chrom_len,
                               a.g.reg_chrom, a.g.reg_start, a.g.reg_end, a.g.R, a.s_prob, own..., a.pt, a.first_pos, a.n_valid, last...);
        };
    }
};

// What entry point `fn` requires of the 14 arguments; R == 0 passes with the sizes checked alone.  dense: the probability entries,
// whose three outputs belong to the block; the sparse entries check their own outputs, and their keys need the sizes below 2^31.
inline int check_tile_args(const char* fn, const TileArgs& a, bool dense)
{
    DIG_REQUIRE_IN(fn, a.n_up == 1 || a.n_up == 2, "n_up = n_down = 1 (trinucleotide) or 2 (penta-nucleotide)");
    DIG_REQUIRE_IN(fn, a.g.R >= 0 && a.C >= 0 && a.g.n_words >= 2 && a.g.n_chrom >= 0 && a.n_tiles >= 0,
                   "non-negative sizes, n_words >= 2 (pad words)");
    DIG_REQUIRE_IN(fn, a.binsize >= 1, "binsize >= 1");
    const int64_t lim = (int64_t)1 << 31;
    DIG_REQUIRE_IN(fn, dense || (a.g.R < lim && a.C < lim && a.n_tiles < lim), "C, R and n_tiles below 2^31");
    if (a.g.R == 0) return DIG_OK;
    const bool tables = a.g.words && a.g.chrom_off && a.g.chrom_len && a.g.reg_chrom && a.g.reg_start && a.g.reg_end;
    DIG_REQUIRE_IN(fn, dense || tables, "non-null genome and region tables");
    if (!dense) return DIG_OK;
    DIG_REQUIRE_IN(fn, tables && a.first_pos && a.n_valid, "non-null pointers");
    DIG_REQUIRE_IN(fn, a.C == 0 || a.n_tiles == 0 || (a.s_prob && a.pt), "s_prob and pt");
    return DIG_OK;
}

// DIG_TILES_FORM (developer switch, read once, by its first letter): "one-role" / "two-role" force either matrix kernel of
// dig_base_tile_probs; "general" sends dig_base_tile_probs_ctx to the general kernel for every region, n_up = 1 too; "rows"
// sends it to the row walk for n_up = 1 too (both cross-check the trinucleotide kernels).  Anything else: no wish.
enum class TilesForm { kAuto, kOneRole, kTwoRole, kGeneral, kRows };
inline TilesForm tiles_form()
{
    static const TilesForm form = []() {
        const char* e = getenv("DIG_TILES_FORM");
        switch (e ? e[0] : '\0') {
        case 'o': return TilesForm::kOneRole;
        case 't': return TilesForm::kTwoRole;
        case 'g': return TilesForm::kGeneral;
        case 'r': return TilesForm::kRows;
        default: return TilesForm::kAuto;
        }
    }();
    return form;
}

// f(std::integral_constant<int, V>) for the V of Vs that equals v; false when none does
template <int... Vs, class F>
inline bool dispatch_const(int v, F&& f)
{
    return ((v == Vs ? (f(std::integral_constant<int, Vs>{}), true) : false) || ...);
}

// dig_tiles_rows.hip: the row walk of the tile probabilities, one launch per cohort pass; regions it does not take are left with
// n_valid = -2 for the general kernel (dig_tiles.hip)
int launch_tile_probs_rows(const TileArgs& a);

}  // namespace dig
