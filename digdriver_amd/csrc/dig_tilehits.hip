// dig_tilehits.hip -- the hits of the per-base route: the (cohort, region, tile) entries of a score plane [C, R, T] (the p-values of
// dig_tiled_nb_test) that pass a per-cohort cut, picked out in the row order of the reference's frame (nb_model.py:188-234 appends
// one block per region, tiles ascending; one frame per cohort) without the frame ever being built.
//
// Hit rule: tile (c, r, t) is a hit when t < n_valid[r] and score[c, r, t] <= cut[c].  A NaN on either side compares false, so a
// NaN score (a tile without an ACGT window: Pi = 0) or a NaN cut never hits; cut = +inf takes every existing tile with a number.
//
// The two-call protocol of the interval join (dig_join.hip):
//   tile_count_kernel   one streaming pass over the flat plane with 16-byte loads, two of them in flight per lane: a plane that
//                       starts at 8 (mod 16) is read as pairs from its second element on; the one or two elements outside the
//                       pairs are looked at by one lane.  A wave in which no score passes its cohort's cut goes on to its next
//                       loads at once.  Otherwise the per-(c, r) sums go through segment_count of dig_keyruns.hpp -- once for the
//                       lanes' first element, once for their second -- and a run of lanes adds to its row only when it holds a
//                       hit: counts is zeroed first, and at a cut that few tiles pass the pass is 8 C R T bytes of reads and next
//                       to no atomics.  (cohort, region, tile) of a lane's element are formed by division once and then stepped
//                       by the grid's stride, in 32 bits.
//   -- the caller forms the exclusive prefix sum of the counts --
//   tile_fill_kernel    a wave per (c, r) row.  A row whose slots [offsets[row], offsets[row + 1]) are empty returns at once (almost
//                       every row at a real cut); another walks its existing tiles 64 at a time and places the hits by a ballot and
//                       the count of hit lanes below: tiles ascending, no sort.  A slot is written only inside the row's own range
//                       and inside [0, total): offsets that are not the prefix sum write nowhere else.
// Integer atomics only; the result does not depend on the order.
#include "dig_keyruns.hpp"

namespace dig {

constexpr int kTileHitBlock = 256;

struct TileSelectArgs {
    const double* score;                                 // [C, R, T]
    const int32_t* n_valid;                              // [R]
    const double* cut;                                   // [C]
    int64_t C, R, T;
    int32_t* counts;                                     // [C R]                    (count)
    const int64_t* offsets;                              // [C R]                    (fill)
    int64_t total;
    const double *pt, *exp_in;                           // [C, R, T] or NULL        (fill)
    const int32_t* k;
    int32_t *hit_region, *hit_tile;                      // [total] or NULL          (fill)
    double *hit_score, *hit_pt, *hit_exp;
    int32_t* hit_k;
};

// where an element lies, e = (c R + r) T + t, and a stride of the grid in the same form (r < R, t < T); 32-bit and unsigned: every
// field stays below 2^31 and a sum of two below 2^32
struct TilePos {
    uint32_t c, r, t;
};

__host__ __device__ inline TilePos tile_pos_of(int64_t e, int64_t R, int64_t T)
{
    const int64_t row = e / T, c = row / R;
    return {(uint32_t)c, (uint32_t)(row - c * R), (uint32_t)(e - row * T)};
}

__device__ __forceinline__ void tile_pos_advance(TilePos& p, const TilePos& step, uint32_t R, uint32_t T)
{
    p.t += step.t;
    if (p.t >= T) p.t -= T, ++p.r;
    p.r += step.r;
    if (p.r >= R) p.r -= R, ++p.c;
    p.c += step.c;
}

// the cuts of the cohorts of elements e1 - 1 and e1, e1 lying at q (a lane without a pair holds an index past the table: clamped into it)
__device__ __forceinline__ double2 tile_pair_cuts(const TileSelectArgs& a, const TilePos& q)
{
    const uint32_t C = (uint32_t)a.C, c1 = q.c, c0 = q.r == 0 && q.t == 0 ? c1 - 1 : c1;       // e1 the first of its cohort: e1 - 1 belongs to the one in front
    return {a.cut[c0 < C ? c0 : C - 1], a.cut[c1 < C ? c1 : C - 1]};
}

// one pair of a lane: v = the scores of elements e1 - 1 and e1 (anything when the lane has no pair: `in` false), cut = their cohorts'
// cuts, q = where e1 lies.  Only a wave that holds a score that passes -- one in a hundred at a real cut -- looks at n_valid and counts.
__device__ __forceinline__ void tile_count_pair(const TileSelectArgs& a, bool in, const TilePos& q, double2 v, double2 cut)
{
    const uint32_t R = (uint32_t)a.R, T = (uint32_t)a.T;
    bool h0 = in & (v.x <= cut.x), h1 = in & (v.y <= cut.y);
    if (!__any(h0 || h1)) return;                                    // (the same for every lane of the wave)
    const uint32_t t0 = q.t ? q.t - 1 : T - 1, r0 = q.t ? q.r : (q.r ? q.r - 1 : R - 1), c0 = q.t || q.r ? q.c : q.c - 1;
    h0 = h0 && (int64_t)t0 < a.n_valid[r0];
    h1 = h1 && (int64_t)q.t < a.n_valid[q.r];
    const int64_t row0 = in ? (int64_t)c0 * R + r0 : -1, row1 = in ? (int64_t)q.c * R + q.r : -1;
    const int n0 = segment_count(row0, h0), n1 = segment_count(row1, h1);
    if (n0) atomicAdd(&a.counts[row0], n0);
    if (n1) atomicAdd(&a.counts[row1], n1);
}

// an element that belongs to no aligned pair (the first of a plane at 8 (mod 16), the last of an odd rest): at most two per call
__device__ __forceinline__ void tile_count_single(const TileSelectArgs& a, int64_t e)
{
    const TilePos p = tile_pos_of(e, a.R, a.T);
    if (a.score[e] <= a.cut[p.c] && (int64_t)p.t < a.n_valid[p.r]) atomicAdd(&a.counts[(int64_t)p.c * a.R + p.r], 1);
}

// The plane as `lead` single elements (1 when it starts at 8 (mod 16), else 0), n_pairs 16-byte aligned pairs and, for an odd rest,
// one single element.  Lane g of the grid holds, per trip, pair g of one block of `stride` pairs and pair g of the next block: two
// 16-byte loads in flight.  step / step2: one block and one trip (two blocks) of elements as a TilePos.
__global__ __launch_bounds__(kTileHitBlock) void tile_count_kernel(TileSelectArgs a, int64_t n, int lead, TilePos step, TilePos step2)
{
    const uint32_t R = (uint32_t)a.R, T = (uint32_t)a.T;
    const int64_t stride = (int64_t)gridDim.x * kTileHitBlock, n_pairs = (n - lead) >> 1;
    const int64_t g0 = (int64_t)blockIdx.x * kTileHitBlock + threadIdx.x;
    if (g0 == 0) {
        if (lead) tile_count_single(a, 0);
        if ((n - lead) & 1) tile_count_single(a, n - 1);
    }
    const double2* __restrict__ pair = reinterpret_cast<const double2*>(a.score + lead);
    TilePos q = tile_pos_of(lead + 2 * g0 + 1, a.R, a.T);            // where the second element of the lane's pair lies
    // the trips are counted from the wave's first lane, so that every lane of a wave makes the same number (__any, segment_count)
    int64_t g = g0;
    for (int64_t w = g0 - (threadIdx.x & 63); w < n_pairs; w += 2 * stride, g += 2 * stride) {
        const bool in_a = g < n_pairs, in_b = g + stride < n_pairs;
        TilePos qb = q;
        tile_pos_advance(qb, step, R, T);
        // The cuts first, then both score loads, and nothing waits before all are issued (loads return in order: a compare then
        // waits for its own pair, not for a table entry queued behind the other one).  A lane past the last pair loads pair 0,
        // which the loop's condition says exists; `in` keeps it out of the hits.
        const double2 ca = tile_pair_cuts(a, q), cb = tile_pair_cuts(a, qb);
        const double2 va = pair[in_a ? g : 0], vb = pair[in_b ? g + stride : 0];
        __builtin_amdgcn_sched_barrier(0);
        tile_count_pair(a, in_a, q, va, ca);
        tile_count_pair(a, in_b, qb, vb, cb);
        tile_pos_advance(q, step2, R, T);
    }
}

__global__ __launch_bounds__(kTileHitBlock) void tile_fill_kernel(TileSelectArgs a, int64_t rows)
{
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * (kTileHitBlock / 64) + (threadIdx.x >> 6);
    if (row >= rows) return;
    int64_t o = a.offsets[row];
    int64_t end = row + 1 < rows ? a.offsets[row + 1] : a.total;
    if (end > a.total) end = a.total;
    if (o < 0 || o >= end) return;                       // no slot of its own: almost every row
    const int64_t c = row / a.R, r = row - c * a.R;
    int64_t nv = a.n_valid[r];
    if (nv > a.T) nv = a.T;
    const double cut = a.cut[c];
    const int64_t base = row * a.T;
    for (int64_t t0 = 0; t0 < nv && o < end; t0 += 64) {
        const int64_t t = t0 + lane;
        const double s = t < nv ? a.score[base + t] : 0.0;
        const bool h = t < nv && s <= cut;
        const unsigned long long hits = __ballot(h);
        const int64_t at = o + __popcll(hits & ((1ull << lane) - 1));
        if (h && at < end) {
            if (a.hit_region) a.hit_region[at] = (int32_t)r;
            if (a.hit_tile) a.hit_tile[at] = (int32_t)t;
            if (a.hit_score) a.hit_score[at] = s;
            if (a.hit_pt && a.pt) a.hit_pt[at] = a.pt[base + t];
            if (a.hit_exp && a.exp_in) a.hit_exp[at] = a.exp_in[base + t];
            if (a.hit_k && a.k) a.hit_k[at] = a.k[base + t];
        }
        o += __popcll(hits);
    }
}

// the size checks the two entry points (and their host twins) share: nothing is read before them
int tile_select_sizes(const char* fn, int64_t C, int64_t R, int64_t T)
{
    DIG_REQUIRE_IN(fn, C >= 0 && R >= 0 && T >= 0, "C, R, T >= 0");
    DIG_REQUIRE_IN(fn, T < ((int64_t)1 << 31), "fewer than 2^31 tiles per region (a tile index is 32-bit)");
    DIG_REQUIRE_IN(fn, C < ((int64_t)1 << 31) && R < ((int64_t)1 << 31) && C * R < ((int64_t)1 << 31),
                   "C R below 2^31 (a row's count and a region index are 32-bit): fewer cohorts per call");
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_tile_select_count(const double* score, const int32_t* n_valid, const double* cut, int64_t C, int64_t R, int64_t T,
                          int32_t* counts, void* stream)
{
    if (int rc = tile_select_sizes(__func__, C, R, T)) return rc;
    const int64_t rows = C * R, n = rows * T;
    if (rows == 0) return DIG_OK;
    DIG_REQUIRE(counts, "non-null counts");
    hipStream_t s = (hipStream_t)stream;
    DIG_HIP_TRY(hipMemsetAsync(counts, 0, (size_t)rows * sizeof(int32_t), s));
    if (n == 0) return DIG_OK;
    DIG_REQUIRE(score && n_valid && cut, "non-null score, n_valid, cut");
    const int lead = (int)(((uintptr_t)score >> 3) & 1);                        // a plane at 8 (mod 16): its first element stands alone
    const int grid = grid_for((n - lead) >> 1, kTileHitBlock);                  // (past the cap: test_tile_select_past_one_trip_of_the_grid, tests/test_gpu_grid_wrap.py)
    const int64_t block = 2 * (int64_t)grid * kTileHitBlock;                    // elements of one block of pairs; a trip is two
    TileSelectArgs a{};
    a.score = score, a.n_valid = n_valid, a.cut = cut, a.C = C, a.R = R, a.T = T, a.counts = counts;
    hipLaunchKernelGGL(tile_count_kernel, dim3(grid), dim3(kTileHitBlock), 0, s, a, n, lead, tile_pos_of(block, R, T),
                       tile_pos_of(2 * block, R, T));
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

int dig_tile_select_fill(const double* score, const int32_t* n_valid, const double* cut, int64_t C, int64_t R, int64_t T,
                         const int64_t* offsets, int64_t total, const double* pt, const double* exp_in, const int32_t* k,
                         int32_t* hit_region, int32_t* hit_tile, double* hit_score, double* hit_pt, double* hit_exp, int32_t* hit_k,
                         void* stream)
{
    if (int rc = tile_select_sizes(__func__, C, R, T)) return rc;
    DIG_REQUIRE(total >= 0, "total >= 0");
    const int64_t rows = C * R;
    if (rows == 0 || T == 0 || total == 0) return DIG_OK;
    DIG_REQUIRE(score && n_valid && cut && offsets, "non-null score, n_valid, cut, offsets");
    TileSelectArgs a{};
    a.score = score, a.n_valid = n_valid, a.cut = cut, a.C = C, a.R = R, a.T = T, a.offsets = offsets, a.total = total;
    a.pt = pt, a.exp_in = exp_in, a.k = k;
    a.hit_region = hit_region, a.hit_tile = hit_tile, a.hit_score = hit_score, a.hit_pt = hit_pt, a.hit_exp = hit_exp, a.hit_k = hit_k;
    unsigned blocks = 0;
    if (int rc = row_blocks(__func__, rows, kTileHitBlock / 64, &blocks)) return rc;
    hipLaunchKernelGGL(tile_fill_kernel, dim3(blocks), dim3(kTileHitBlock), 0, (hipStream_t)stream, a, rows);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // extern "C"
