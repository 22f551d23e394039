// dig_rowhits.hip -- the calls of the element route: the entries of a score plane [rows, n] (a row = one p-value column of one cohort,
// n = the elements) that pass the row's cut, taken out as ragged lists and put back.  dig_tilehits.hip does this for the [C, R, T]
// planes of the per-base route with one wave per (cohort, region) row in its fill: rows of a few hundred tiles.  A row of this plane
// is 10^5 elements and there are 10^2 of them, so the unit of work is not the row but a CHUNK of it.
//
// Rule: element (r, e) is selected when score[r, e] <= cut[r].  A NaN on either side compares false: a NaN score or a NaN cut selects
// nothing, cut = +inf takes every score that is a number.
//
// A row is cut into chunks of kRowSelectChunk consecutive elements (the last one shorter); chunk w = r * chunks + c of the plane
// belongs to ONE wave, in all three kernels, and every kernel makes the same walk over it (row_chunk_walk):
//   a chunk that starts at 8 (mod 16) has a LEAD element that stands alone; then 16-byte aligned pairs, kRowLoads of them in flight
//   per lane (a step of the wave: 64 * kRowLoads pairs, issued before any is looked at); an odd rest leaves one TAIL element.
//   Within a load the lanes' pairs are consecutive, so the selected elements below one -- the ballots of the two halves, masked to the
//   lanes below, its own first half for a second half -- number the selected elements of the chunk in ascending order.
//   row_count_kernel    the number of selected elements of the chunk -> counts[w]: every slot written once by its owner, no atomics,
//                       no zero-fill.
//   -- the caller forms the exclusive prefix sum of the counts --
//   row_fill_kernel     selected element number h of chunk w -> slot offsets[w] + h, as its index in the row and its score: row-major,
//                       ascending within a row, no sort.  A chunk whose slots [offsets[w], offsets[w + 1]) are empty returns at once
//                       (almost every chunk at a real cut); a slot is written only inside that range and inside [0, total).
//   row_scatter_kernel  the inverse: out[r, e] = values[slot] where (r, e) is selected (and its slot lies in the chunk's range), `fill`
//                       elsewhere; every element of out is written, as 16-byte stores where out lies as score does (mod 16).
// One wave per chunk and no cap on the grid: rows * chunks < 2^31 waves are fewer than 2^29 workgroups.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kRowBlock = 256;                           // four waves, a chunk each
constexpr int kRowLoads = 4;                             // 16-byte loads a lane has in flight
constexpr int kRowStep = 64 * kRowLoads;                 // pairs per step of a wave (4 KiB)
static_assert(kRowSelectChunk % (2 * kRowStep) == 0, "a chunk is whole steps");

enum RowMode { kRowCount, kRowFill, kRowScatter };

struct RowSelectArgs {
    const double* score;                                 // [rows, n]
    const double* cut;                                   // [rows]
    int64_t n, waves;                                    // waves = rows * chunks
    uint32_t chunks;                                     // per row
    int32_t* counts;                                     // [waves]                  (count)
    const int64_t* offsets;                              // [waves]                  (fill, scatter)
    int64_t total;
    int32_t* hit_index;                                  // [total] or NULL          (fill)
    double* hit_score;
    const double* values;                                // [total]                  (scatter)
    double fill;
    double* out;                                         // [rows, n]
};

template <int MODE>
__device__ __forceinline__ void row_chunk_walk(const RowSelectArgs& a)
{
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * (kRowBlock / 64) + __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
    if (w >= a.waves) return;
    // o: the slot of the chunk's next selected element (count: their number so far); [o, end): the chunk's own slots
    int64_t o = 0, end = 0;
    if (MODE != kRowCount) {
        o = a.offsets[w];
        end = w + 1 < a.waves ? a.offsets[w + 1] : a.total;
        if (end > a.total) end = a.total;
        if (o < 0 || o >= end) {
            if (MODE == kRowFill) return;                // no slot of its own: almost every chunk at a real cut
            o = end = 0;                                 // (scatter: `fill` everywhere)
        }
    }
    const uint32_t r = (uint32_t)w / a.chunks, c = (uint32_t)w - r * a.chunks;
    const int64_t e0 = (int64_t)c * kRowSelectChunk, at0 = (int64_t)r * a.n + e0;
    const int len = (int)(a.n - e0 < kRowSelectChunk ? a.n - e0 : kRowSelectChunk);          // >= 1: the chunk exists
    const double* __restrict__ base = a.score + at0;
    const double cut = a.cut[r];
    const int lead = (int)(((uintptr_t)base >> 3) & 1), n_pairs = (len - lead) >> 1;
    const unsigned long long below = (1ull << lane) - 1;
    double* outp = MODE == kRowScatter ? a.out + at0 : nullptr;
    const bool wide = MODE == kRowScatter && (((uintptr_t)(outp + lead)) & 15) == 0;          // out lies as score does
    // one element that stands alone (the same for every lane; lane 0 places it)
    auto single = [&](int e) {
        const double v = base[e];
        const bool h = v <= cut;
        if (MODE == kRowFill && lane == 0 && h && o < end) {
            if (a.hit_index) a.hit_index[o] = (int32_t)(e0 + e);
            if (a.hit_score) a.hit_score[o] = v;
        }
        if (MODE == kRowScatter && lane == 0) outp[e] = h && o < end ? a.values[o] : a.fill;
        o += h;
    };
    if (lead) single(0);
    const double2* __restrict__ pair = reinterpret_cast<const double2*>(base + lead);
    for (int p0 = 0; p0 < n_pairs && (MODE != kRowFill || o < end); p0 += kRowStep) {
        // every load of the step is issued before one is looked at; a lane past the last pair loads pair 0, which the loop's
        // condition says exists, and `in` keeps it out of the selection
        double2 v[kRowLoads];
#pragma unroll
        for (int j = 0; j < kRowLoads; ++j) {
            const int i = p0 + j * 64 + lane;
            v[j] = pair[i < n_pairs ? i : 0];
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kRowLoads; ++j) {
            const int i = p0 + j * 64 + lane;
            const bool in = i < n_pairs, hx = in & (v[j].x <= cut), hy = in & (v[j].y <= cut);
            const unsigned long long bx = __ballot(hx), by = __ballot(hy);
            if (MODE != kRowCount) {
                const int e = lead + 2 * i;
                const int64_t ax = o + __popcll(bx & below) + __popcll(by & below), ay = ax + hx;
                if (MODE == kRowFill) {
                    if (hx && ax < end) {
                        if (a.hit_index) a.hit_index[ax] = (int32_t)(e0 + e);
                        if (a.hit_score) a.hit_score[ax] = v[j].x;
                    }
                    if (hy && ay < end) {
                        if (a.hit_index) a.hit_index[ay] = (int32_t)(e0 + e + 1);
                        if (a.hit_score) a.hit_score[ay] = v[j].y;
                    }
                } else if (in) {
                    const double x = hx && ax < end ? a.values[ax] : a.fill, y = hy && ay < end ? a.values[ay] : a.fill;
                    if (wide)
                        *reinterpret_cast<double2*>(outp + e) = double2{x, y};
                    else
                        outp[e] = x, outp[e + 1] = y;
                }
            }
            o += __popcll(bx) + __popcll(by);
        }
    }
    if ((len - lead) & 1) single(len - 1);
    if (MODE == kRowCount && lane == 0) a.counts[w] = (int32_t)o;
}

__global__ __launch_bounds__(kRowBlock) void row_count_kernel(RowSelectArgs a) { row_chunk_walk<kRowCount>(a); }
__global__ __launch_bounds__(kRowBlock) void row_fill_kernel(RowSelectArgs a) { row_chunk_walk<kRowFill>(a); }
__global__ __launch_bounds__(kRowBlock) void row_scatter_kernel(RowSelectArgs a) { row_chunk_walk<kRowScatter>(a); }

// the size checks the three entry points (and their host twins) share: nothing is read before them
int row_select_sizes(const char* fn, int64_t rows, int64_t n, int64_t* chunks)
{
    DIG_REQUIRE_IN(fn, rows >= 0 && n >= 0, "rows, n >= 0");
    DIG_REQUIRE_IN(fn, n < ((int64_t)1 << 31), "fewer than 2^31 elements per row (an element index is 32-bit)");
    const int64_t ch = (n + kRowSelectChunk - 1) / kRowSelectChunk;
    DIG_REQUIRE_IN(fn, rows < ((int64_t)1 << 31) && rows * ch < ((int64_t)1 << 31),
                   "rows * chunks below 2^31 (a chunk per wave, numbered in 32 bits): fewer rows per call");
    *chunks = ch;
    return DIG_OK;
}

static RowSelectArgs row_args(const double* score, const double* cut, int64_t rows, int64_t n, int64_t chunks)
{
    RowSelectArgs a{};
    a.score = score, a.cut = cut, a.n = n, a.waves = rows * chunks, a.chunks = (uint32_t)chunks;
    return a;
}

template <class K>
static int row_launch(K kernel, const RowSelectArgs& a, void* stream)
{
    const unsigned blocks = (unsigned)((a.waves + kRowBlock / 64 - 1) / (kRowBlock / 64));         // waves < 2^31
    hipLaunchKernelGGL(kernel, dim3(blocks), dim3(kRowBlock), 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int64_t dig_row_select_chunk(void) { return kRowSelectChunk; }

int64_t dig_row_select_counts_size(int64_t rows, int64_t n)
{
    int64_t chunks = 0;
    return row_select_sizes(__func__, rows, n, &chunks) ? -1 : rows * chunks;
}

int dig_row_select_count(const double* score, const double* cut, int64_t rows, int64_t n, int32_t* counts, void* stream)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    if (rows * chunks == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && counts, "non-null score, cut, counts");
    RowSelectArgs a = row_args(score, cut, rows, n, chunks);
    a.counts = counts;
    return row_launch(row_count_kernel, a, stream);
}

int dig_row_select_fill(const double* score, const double* cut, int64_t rows, int64_t n, const int64_t* offsets, int64_t total,
                        int32_t* hit_index, double* hit_score, void* stream)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    if (rows * chunks == 0 || total == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && offsets, "non-null score, cut, offsets");
    RowSelectArgs a = row_args(score, cut, rows, n, chunks);
    a.offsets = offsets, a.total = total, a.hit_index = hit_index, a.hit_score = hit_score;
    return row_launch(row_fill_kernel, a, stream);
}

int dig_row_scatter(const double* score, const double* cut, int64_t rows, int64_t n, const int64_t* offsets, int64_t total,
                    const double* values, double fill, double* out, void* stream)
{
    int64_t chunks = 0;
    if (int rc = row_select_sizes(__func__, rows, n, &chunks)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    if (rows * chunks == 0) return DIG_OK;
    DIG_REQUIRE(score && cut && offsets && out && (values || total == 0), "non-null score, cut, offsets, out, values");
    RowSelectArgs a = row_args(score, cut, rows, n, chunks);
    a.offsets = offsets, a.total = total, a.values = values, a.fill = fill, a.out = out;
    return row_launch(row_scatter_kernel, a, stream);
}

}  // extern "C"
