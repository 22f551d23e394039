// dig_genome2.hpp -- the 2-bit genome that dig_count_contexts2, dig_count_contexts5, dig_mutation_contexts and
// dig_mutation_function read (include/dig_hip.h): the one place that knows its layout.  The struct that carries it, the
// device functions every kernel reads it through, and the checks of its ten arguments.
//
// Layout: A=0 C=1 G=2 T=3 at 2 bits per base, every other letter stored as A, 16 bases per 32-bit word, base 0 in the low
// bits; array base = kGenome2PadBases + chrom_off + position; at least kGenome2PadWordsBehind words behind the last
// chromosome (a lane of the counting kernel reads whole 16-word steps).  Next to it the sorted list of the maximal runs of
// letters other than ACGT, [nint_start, nint_end) in array bases, and the list's bucket index: per 2^kGenome2BucketShift
// array bases the first run that ends behind the bucket's first base.  PackedGenome.two_bit packs it (PAD2_BASES and
// BUCKET_SHIFT there are these constants: tests/test_abi_and_host.py compares them).
#pragma once
#include "dig_common.hpp"

namespace dig {

constexpr int kGenome2PadBases = 64;           // bases in front of chromosome data (one 4-word group)
constexpr int kGenome2PadWordsBehind = 24;
constexpr int kGenome2BasesPerWord = 16;
constexpr int kGenome2BucketShift = 12;
constexpr int64_t kGenome2MinWords = kGenome2PadBases / kGenome2BasesPerWord + kGenome2PadWordsBehind;

// The ten genome arguments of an entry point, in their order; a kernel takes it by value.
struct Genome2 {
    const uint32_t* __restrict__ words;
    int64_t n_words;
    const int64_t* __restrict__ nint_start;
    const int64_t* __restrict__ nint_end;
    int64_t n_int;
    const int32_t* __restrict__ nint_bucket;
    int64_t n_buckets;
    const int64_t* __restrict__ chrom_off;
    const int64_t* __restrict__ chrom_len;
    int n_chrom;
};

// index of the first run that ends behind array base x, n_int when there is none (n_int > 0)
__device__ __forceinline__ int64_t genome2_first_run(const Genome2& G, int64_t x)
{
    int64_t b = x >> kGenome2BucketShift;
    if (b >= G.n_buckets) b = G.n_buckets - 1;
    int64_t j = G.nint_bucket[b];
    while (j < G.n_int && G.nint_end[j] <= x) ++j;
    return j;
}

__device__ __forceinline__ uint32_t genome2_mask(int W)              // the low 2 W bits, W <= 16
{
    return W == 16 ? 0xffffffffu : ((1u << (2 * W)) - 1u);
}

// the W <= 16 bases from array base q on as one code: base k of the window in bits 2 k, 2 k + 1
__device__ __forceinline__ uint32_t genome2_window(const uint32_t* __restrict__ w, int64_t q, int W)
{
    const uint64_t x = (uint64_t)w[q >> 4] | ((uint64_t)w[(q >> 4) + 1] << 32);
    return (uint32_t)(x >> (2 * (int)(q & 15))) & genome2_mask(W);
}

// the code of the context centred at array base c with kUp bases on either side (the left-most base in the low bits)
template <int kUp>
__device__ __forceinline__ unsigned genome2_context(const uint32_t* __restrict__ w, int64_t c)
{
    return genome2_window(w, c - kUp, 2 * kUp + 1);
}

__device__ __forceinline__ unsigned genome2_code(const uint32_t* __restrict__ w, int64_t g)     // array base g as stored
{
    return (w[g >> 4] >> (2 * (int)(g & 15))) & 3u;
}

// code 0-3 of position p (1-based) of a chromosome at array offset `off` (pad included) of length `len`; 4 for a letter other
// than ACGT or a position outside the chromosome (nothing is read then)
__device__ __forceinline__ unsigned genome2_base(const Genome2& G, int64_t off, int64_t len, int64_t p)
{
    if (p < 1 || p > len) return 4u;
    const int64_t g = off + p - 1;
    const unsigned code = genome2_code(G.words, g);
    if (G.n_int > 0) {
        const int64_t j = genome2_first_run(G, g);
        if (j < G.n_int && G.nint_start[j] <= g) return 4u;
    }
    return code;
}

// The centres of [gs, ge) whose context (kUp bases either side) touches a run, for a scan that has counted them as they
// are stored: walks the runs first, first + stride, ... up to the first that starts at or behind ge + kUp (the list is
// sorted: nothing further can touch).  A centre that sees two runs (they are fewer than 2 kUp bases apart) belongs to the
// earlier one.  Per run it calls interior(n) for the n centres whose whole context lies inside the run -- stored as all
// A, code 0 -- and edge(code) for each of the up to kUp centres at either end with the context as it is stored.
template <int kUp, typename Interior, typename Edge>
__device__ __forceinline__ void genome2_take_back(const Genome2& G, int64_t first, int64_t stride, int64_t gs, int64_t ge,
                                                  Interior interior, Edge edge)
{
    const int64_t x1 = ge + kUp;
    for (int64_t j = first; j < G.n_int; j += stride) {
        const int64_t ns = G.nint_start[j], ne = G.nint_end[j];
        if (ns >= x1) break;
        int64_t lo = ns - kUp > gs ? ns - kUp : gs;
        if (j > 0 && G.nint_end[j - 1] + kUp > lo) lo = G.nint_end[j - 1] + kUp;
        const int64_t hi = ne + kUp < ge ? ne + kUp : ge;
        if (hi <= lo) continue;
        const int64_t i0 = lo > ns + kUp ? lo : ns + kUp, i1 = hi < ne - kUp ? hi : ne - kUp;
        if (i1 > i0) interior(i1 - i0);
        const int64_t l1 = hi < ns + kUp ? hi : ns + kUp;                   // left edge centres [lo, l1)
        int64_t e0 = ne - kUp > ns + kUp ? ne - kUp : ns + kUp;             // right edge centres [e0, hi)
        if (e0 < lo) e0 = lo;
        for (int64_t c = lo; c < l1; ++c) edge(genome2_context<kUp>(G.words, c));
        for (int64_t c = e0; c < hi; ++c) edge(genome2_context<kUp>(G.words, c));
    }
}

// What entry point `fn` requires of the genome arguments; n is its own count (regions, rows, pairs: with n == 0 nothing is
// read and the run list's pointers may be NULL), which the counting entries (n_is_R) have reported in the same message.
inline int genome2_check(const char* fn, const Genome2& G, int64_t n, bool n_is_R = false)
{
    static_assert(kGenome2MinWords == 28, "the messages below");
    DIG_REQUIRE_IN(fn, n >= 0 && G.n_words >= kGenome2MinWords && G.n_chrom >= 0 && G.n_int >= 0,
                   n_is_R ? "R, n_int, n_chrom >= 0, n_words2 >= 28 (pad words)" : "n_int, n_chrom >= 0, n_words2 >= 28 (pad words)");
    DIG_REQUIRE_IN(fn, n == 0 || G.n_int == 0 || (G.nint_start && G.nint_end && G.nint_bucket && G.n_buckets >= 1),
                   "interval list with its bucket index");
    return DIG_OK;
}

// What a `_host` twin verifies in addition, on host arrays that genome2_check and its own non-null test have passed
inline int genome2_check_host(const char* fn, const Genome2& G)
{
    const int64_t n_bases = (G.n_words - kGenome2PadWordsBehind) * kGenome2BasesPerWord;
    for (int c = 0; c < G.n_chrom; ++c)
        DIG_REQUIRE_IN(fn, G.chrom_off[c] >= 0 && G.chrom_off[c] + G.chrom_len[c] + kGenome2PadBases <= n_bases, "chromosomes inside the genome array");
    for (int64_t j = 0; j < G.n_int; ++j)
        DIG_REQUIRE_IN(fn, G.nint_start[j] < G.nint_end[j] && (j == 0 || G.nint_end[j - 1] < G.nint_start[j]), "intervals sorted, disjoint, not touching");
    return DIG_OK;
}

}  // namespace dig
