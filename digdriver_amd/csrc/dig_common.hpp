// dig_common.hpp -- error plumbing and launch helpers shared by the .hip translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <hip/hip_ext.h>
#include <stdint.h>
#include <stdio.h>

#include <string>
#include <type_traits>

#include "../../include/dig_hip.h"

namespace dig {

std::string& last_error_ref();
int set_error(int code, const char* fmt, ...);

#define DIG_HIP_TRY(expr)                                                                              \
    do {                                                                                               \
        hipError_t _e = (expr);                                                                        \
        if (_e != hipSuccess)                                                                          \
            return ::dig::set_error(DIG_EHIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e),   \
                                    __FILE__, __LINE__);                                               \
    } while (0)

// (fn: the entry point's name, for a check that a helper makes on its behalf)
#define DIG_REQUIRE_IN(fn, cond, msg)                                                           \
    do {                                                                                        \
        if (!(cond)) return ::dig::set_error(DIG_EINVAL, "%s: requirement failed: %s", fn, msg); \
    } while (0)
#define DIG_REQUIRE(cond, msg) DIG_REQUIRE_IN(__func__, cond, msg)

// number of CUs of the current device (cached per device)
int cu_count();

// i / C with a host-computed magic multiplier: e = hi64(i * ceil(2^64 / C)), exact while
// i * C < 2^64 (the per-pair int64 division the flat [E, C] index would otherwise need costs
// more than a whole recurrence step).
struct FastDiv {
    uint64_t magic;   // ceil(2^64 / d), d >= 2
};
inline FastDiv make_fastdiv(int64_t d)
{
    FastDiv f;
    f.magic = (d >= 2) ? (~(uint64_t)0 / (uint64_t)d) + 1 : 0;
    return f;
}
__device__ __forceinline__ int64_t fastdiv(int64_t i, const FastDiv& f)
{
    return (int64_t)__umul64hi((uint64_t)i, f.magic);
}

// A stage timer (dig_stage_timer_*, include/dig_hip.h): two events that the next launch of a stage's kernel on the arming
// thread fills with the kernel's own begin and end (hipExtLaunchKernelGGL: taken from the dispatch, no packet added to the stream).
struct StageTimer {
    hipEvent_t start = nullptr, stop = nullptr;
    int launched = 0;
};
StageTimer* take_armed_timer(int stage);
void disarm_stage_timers();                    // end of a dig_element_pipeline call: nothing stays armed       // the timer armed for `stage` by this thread, or NULL; disarms it
// launch `kernel` as hipLaunchKernelGGL does, through the armed timer of `stage` if there is one
#define DIG_LAUNCH_STAGE(stage, kernel, grid, block, lds, stream, ...)                                                   \
    do {                                                                                                                 \
        if (::dig::StageTimer* _t = ::dig::take_armed_timer(stage)) {                                                    \
            hipExtLaunchKernelGGL(kernel, grid, block, lds, stream, _t->start, _t->stop, 0, __VA_ARGS__);                \
            _t->launched = 1;                                                                                            \
        } else                                                                                                           \
            hipLaunchKernelGGL(kernel, grid, block, lds, stream, __VA_ARGS__);                                           \
    } while (0)

inline int grid_for(int64_t n, int block, int max_blocks_per_cu = 8)
{
    int64_t want = (n + block - 1) / block;
    int64_t cap = (int64_t)cu_count() * max_blocks_per_cu;
    if (want < 1) want = 1;
    return (int)(want < cap ? want : cap);
}

// How the (at most 48) cohort columns of a chunk are cut: full 16-column tiles for v_mfma_f64_16x16x4, and, when what is
// left over is 1..8 columns, one or two QUADS of four columns for v_mfma_f64_4x4x4 (four 4x4 blocks = the same sixteen
// elements; a quad costs a quarter of a tile's matrix-pipe time, so 37 cohorts pay for 40 columns instead of 48).
// (the dot kernels of dig_accumulate.hip and the matrix kernels of dig_tiles.hip)
constexpr int kCutChunk = 48;                 // cohorts per chunk
struct ChunkCut {
    int nt, nq;      // full tiles, tail quads
};
__host__ __device__ inline ChunkCut chunk_cut(int C, int chunk)
{
    const int rem = C - chunk * kCutChunk < kCutChunk ? C - chunk * kCutChunk : kCutChunk;
    const int full = rem >> 4, r = rem & 15;
    if (r == 0) return {full, 0};
    if (r <= 8) return {full, (r + 3) >> 2};
    return {full + 1, 0};
}
// f(std::integral_constant<int, NT>{}, std::integral_constant<int, NQ>{}) -> int for the nine cuts a chunk with a cohort in
// it can have; any other pair is refused
template <class F>
inline int dispatch_cut(ChunkCut cut, F&& f)
{
#define DIG_CUT_CASE(NT, NQ) \
    case NT * 3 + NQ: return f(std::integral_constant<int, NT>{}, std::integral_constant<int, NQ>{})
    switch (cut.nq >= 0 && cut.nq <= 2 ? cut.nt * 3 + cut.nq : -1) {
        DIG_CUT_CASE(0, 1);
        DIG_CUT_CASE(0, 2);
        DIG_CUT_CASE(1, 0);
        DIG_CUT_CASE(1, 1);
        DIG_CUT_CASE(1, 2);
        DIG_CUT_CASE(2, 0);
        DIG_CUT_CASE(2, 1);
        DIG_CUT_CASE(2, 2);
        DIG_CUT_CASE(3, 0);
    default: return set_error(DIG_EINVAL, "dispatch_cut: no kernel for %d tiles + %d quads", cut.nt, cut.nq);
    }
#undef DIG_CUT_CASE
}

}  // namespace dig
