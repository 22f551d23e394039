// dig_groupfisher.hip -- the meta-cohorts of the element route: the p-values of GROUPS of cohorts combined per element by Fisher's
// method, and the group sums of the counts that stand beside them.  Input planes are [R, C, E] (R stacked columns, C cohorts, E
// elements, E contiguous: the layout of the element route's S planes), membership is member u8 [M, C] (non-zero: cohort c belongs to
// group g), outputs are [R, M, E].  C <= 64, M <= 32 per launch.
//
// One walk serves both entry points (group_walk<MODE, MACC>):
//   A row of E elements is cut into chunks of kGroupChunk = 128 elements, chunk w = r * chunks + k belongs to ONE wave, and lane l
//   owns the same PAIR of elements (e, e + 1), e = 128 k + 2 l, in every one of the C cohort rows -- its group accumulators are that
//   pair's.  The row of cohort c starts at p + (r C + c) E: where that address + e lies at 0 (mod 16) the pair is one 16-byte load,
//   where it lies at 8 (an odd E puts the rows at 0 and at 8 in turn; so does a plane that itself starts at 8) it is two 8-byte
//   loads of the same 16 bytes -- the same cache lines either way, and the branch is wave-uniform.  (Not the lead / pairs / tail form
//   of dig_rowhits.hip: there a lane may own different elements in different rows, here its registers belong to one pair.)  An odd E
//   leaves the last lane of a row one element: it is loaded alone, nothing is read behind a row's end.
//   The cohorts are walked in ascending c, kGroupLoads = 4 rows' loads issued before the first is looked at.  Every value is read
//   once, its -log taken once, and added to the accumulator of every group that cohort c belongs to: lane c holds the groups of
//   cohort c as a 32-bit list (read from member once per wave), a row's list is read into a scalar register, so the branches on its
//   bits are uniform.  The accumulators are MACC x 2 doubles in registers; MACC = 8 or 32 is chosen by M at the launch
//   (gfx950: fisher 112 / 208 VGPRs, sums 76 / 172, no scratch, no spill: 4 / 2 and 6 / 2 waves per SIMD).  The groups are
//   finished one after the other in a loop that is NOT unrolled (the Fisher value is long code): group g's accumulators are taken
//   from slot 0 and the rest move down a slot, all with compile-time indices, which keeps them in registers.
//   fisher: a lane keeps the 64-bit mask of its non-NaN cohorts per element; m = popcount(valid & mask_g) is out_n, and
//             m = 0   NaN
//             m = 1   the member's p, re-read at ctz(valid & mask_g): its bits
//             m = 2   fisher_combine_fast(p_a, p_b), a < b re-read: the bits of dig_fisher
//             m >= 3  Q(m, s) = e^-s sum_{j<m} s^j / j! as exp(log(r) - s), r = 1 + s/1 (1 + s/2 (... (1 + s/(m-1)))) by Horner
//                     (one exponential of a difference, as fisher_combine; m <= 64 and s <= 745 m keep r below 1e210);
//                     s < 0 -> 1, s = +inf -> 0, NaN s -> NaN
//   sums:   out = the sum of x[r, c, e] over the members in ascending c, one IEEE addition each, from +0.0; with a gate only the
//           members whose gate[r, c, e] is not NaN (the others add +0.0, which changes no bit of an accumulator that began at +0.0).
// No atomics: every output slot is written once, by the lane that owns the element.  No LDS beyond the logarithm table of
// fisher_combine_fast.
#include "dig_keyruns.hpp"
#include "dig_math.hpp"

namespace dig {

constexpr int kGroupBlock = 64;                          // one wave, one chunk
constexpr int kGroupChunk = 128;                         // elements of a chunk: a pair per lane
constexpr int kGroupLoads = 4;                           // cohort rows a lane has in flight

enum GroupMode { kGroupFisher, kGroupSums };

struct GroupArgs {
    const double* x;                                     // [R, C, E]: p (fisher), x (sums)
    const double* gate;                                  // [R, C, E] or NULL           (sums)
    const uint8_t* member;                               // [M, C]
    int64_t E, waves;                                    // waves = R * chunks
    uint32_t chunks;                                     // per row
    int C, M;
    double* out;                                         // [R, M, E]
    int32_t* out_n;                                      // [R, M, E] or NULL           (fisher)
};

typedef double GroupPair __attribute__((ext_vector_type(2)));

// the pair (e, e + 1) of a row -> (x, y); in_x / in_y: the element exists (NaN otherwise).  A lane past the row's end reads nothing.
__device__ __forceinline__ void group_load_pair(const double* __restrict__ row, int64_t e, bool in_x, bool in_y, double& x, double& y)
{
    x = y = dnan();
    if (((uintptr_t)(row + e) & 15) == 0 && in_y) {
        const GroupPair t = *reinterpret_cast<const GroupPair*>(row + e);
        x = t.x, y = t.y;
    } else {
        if (in_x) x = row[e];
        if (in_y) y = row[e + 1];
    }
}

// Fisher's method over the members `vm` (the non-NaN ones) of one element: col = &p[r, 0, e], s their sum of -ln p
__device__ __forceinline__ double group_fisher_value(const double* __restrict__ col, int64_t E, double s, unsigned long long vm)
{
    const int m = __popcll(vm);
    if (m == 0) return dnan();
    const int a = __ffsll((long long)vm) - 1;
    if (m == 1) return col[(int64_t)a * E];
    if (m == 2) return fisher_combine_fast(col[(int64_t)a * E], col[(int64_t)(63 - __clzll((long long)vm)) * E]);
    if (isnan(s)) return dnan();
    if (s < 0.0) return 1.0;
    if (isinf(s)) return 0.0;
    double r = 1.0;
    for (int j = m - 1; j >= 1; --j) r = 1.0 + s / (double)j * r;
    return exp(log(r) - s);
}

template <int MODE, int MACC>
__device__ __forceinline__ void group_walk(const GroupArgs& a)
{
    if (MODE == kGroupFisher) nb_tables_init();          // (the table of fisher_combine_fast; every lane of the block arrives)
    const int lane = threadIdx.x & 63;
    const int64_t w = blockIdx.x;
    if (w >= a.waves) return;
    const uint32_t r = (uint32_t)w / a.chunks, k = (uint32_t)w - r * a.chunks;
    const int64_t E = a.E, e = (int64_t)k * kGroupChunk + 2 * lane;
    const bool in_x = e < E, in_y = e + 1 < E;
    const int C = a.C, M = a.M;
    // lane c holds the groups of cohort c as a bit list: bit g = cohort c belongs to group g.  A row's list is read into a scalar
    // register (readlane at the uniform c), so the branches on its bits are uniform
    uint32_t groups_of = 0;
    if (lane < C)
        for (int g = 0; g < M; ++g) groups_of |= (uint32_t)(a.member[g * C + lane] != 0) << g;
    const double* __restrict__ x0 = a.x + (int64_t)r * C * E;
    const double* __restrict__ g0 = MODE == kGroupSums && a.gate ? a.gate + (int64_t)r * C * E : nullptr;
    double sx[MACC], sy[MACC];
#pragma unroll
    for (int g = 0; g < MACC; ++g) sx[g] = sy[g] = 0.0;
    unsigned long long valid_x = 0, valid_y = 0;
    for (int c0 = 0; c0 < C; c0 += kGroupLoads) {
        // every load of the step is issued before one is looked at; a row past the last one loads the last one again
        double vx[kGroupLoads], vy[kGroupLoads], qx[kGroupLoads], qy[kGroupLoads];
#pragma unroll
        for (int j = 0; j < kGroupLoads; ++j) {
            const int c = c0 + j < C ? c0 + j : C - 1;
            group_load_pair(x0 + (int64_t)c * E, e, in_x, in_y, vx[j], vy[j]);
            if (MODE == kGroupSums && g0) group_load_pair(g0 + (int64_t)c * E, e, in_x, in_y, qx[j], qy[j]);
        }
        __builtin_amdgcn_sched_barrier(0);
#pragma unroll
        for (int j = 0; j < kGroupLoads; ++j) {
            const int c = c0 + j;
            if (c < C) {
                double tx, ty;
                if (MODE == kGroupFisher) {
                    const bool ok_x = !isnan(vx[j]), ok_y = !isnan(vy[j]);
                    valid_x |= (unsigned long long)ok_x << c, valid_y |= (unsigned long long)ok_y << c;
                    tx = ok_x ? -log(vx[j]) : 0.0, ty = ok_y ? -log(vy[j]) : 0.0;
                } else if (g0) {
                    tx = isnan(qx[j]) ? 0.0 : vx[j], ty = isnan(qy[j]) ? 0.0 : vy[j];
                } else {
                    tx = vx[j], ty = vy[j];
                }
                const uint32_t in_groups = (uint32_t)__builtin_amdgcn_readlane((int)groups_of, c);
#pragma unroll
                for (int g = 0; g < MACC; ++g)
                    if ((in_groups >> g) & 1) sx[g] += tx, sy[g] += ty;
            }
        }
    }
    // The groups one after the other, NOT unrolled (the Fisher value is long code): group g's accumulators are taken from slot 0 and
    // the others move down one slot, all with compile-time indices, so that the accumulators stay in registers
#pragma unroll 1
    for (int g = 0; g < M; ++g) {
        const double s_x = sx[0], s_y = sy[0];
#pragma unroll
        for (int i = 0; i + 1 < MACC; ++i) sx[i] = sx[i + 1], sy[i] = sy[i + 1];
        const unsigned long long members = __ballot((groups_of >> g) & 1);
        if (in_x) {
            const int64_t at = ((int64_t)r * M + g) * E + e;
            double ox = s_x, oy = s_y;
            if (MODE == kGroupFisher) {
                const unsigned long long mx = valid_x & members, my = valid_y & members;
                // (x, then y, through one copy of the code)
#pragma unroll 1
                for (int h = 0; h < (in_y ? 2 : 1); ++h) {
                    const double v = group_fisher_value(x0 + e + h, E, h ? s_y : s_x, h ? my : mx);
                    if (h) oy = v; else ox = v;
                }
                if (a.out_n) {
                    int32_t* n = a.out_n + at;
                    n[0] = __popcll(mx);
                    if (in_y) n[1] = __popcll(my);
                }
            }
            double* o = a.out + at;
            if (in_y && ((uintptr_t)o & 15) == 0)
                *reinterpret_cast<GroupPair*>(o) = GroupPair{ox, oy};
            else {
                o[0] = ox;
                if (in_y) o[1] = oy;
            }
        }
    }
}

template <int MACC>
__global__ __launch_bounds__(kGroupBlock) void group_fisher_kernel(GroupArgs a) { group_walk<kGroupFisher, MACC>(a); }
template <int MACC>
__global__ __launch_bounds__(kGroupBlock) void group_sums_kernel(GroupArgs a) { group_walk<kGroupSums, MACC>(a); }

// the size checks the two entry points (and their host twins) share: nothing is read before them
int group_sizes(const char* fn, int64_t R, int64_t C, int64_t E, int64_t M, int64_t* chunks)
{
    DIG_REQUIRE_IN(fn, R >= 0 && C >= 0 && E >= 0 && M >= 0, "R, C, E, M >= 0");
    DIG_REQUIRE_IN(fn, C <= 64, "C <= 64 cohorts (a lane's mask of testable cohorts is 64-bit)");
    DIG_REQUIRE_IN(fn, M <= 32, "M <= 32 groups per call (the accumulators of a lane): fewer groups per call");
    DIG_REQUIRE_IN(fn, E < ((int64_t)1 << 31), "fewer than 2^31 elements per row");
    const int64_t ch = (E + kGroupChunk - 1) / kGroupChunk;
    DIG_REQUIRE_IN(fn, R < ((int64_t)1 << 31) && R * ch < ((int64_t)1 << 31),
                   "R * chunks below 2^31 (a chunk per workgroup): fewer stacked columns per call");
    *chunks = ch;
    return DIG_OK;
}

template <class K8, class K32>
static int group_launch(K8 k8, K32 k32, GroupArgs& a, int64_t R, int64_t C, int64_t E, int64_t M, int64_t chunks, void* stream)
{
    a.E = E, a.waves = R * chunks, a.chunks = (uint32_t)chunks, a.C = (int)C, a.M = (int)M;
    const dim3 grid((unsigned)a.waves), block(kGroupBlock);
    if (M <= 8)
        hipLaunchKernelGGL(k8, grid, block, 0, (hipStream_t)stream, a);
    else
        hipLaunchKernelGGL(k32, grid, block, 0, (hipStream_t)stream, a);
    DIG_HIP_TRY(hipGetLastError());
    return DIG_OK;
}

}  // namespace dig

using namespace dig;

extern "C" {

int dig_group_fisher(const double* p, const uint8_t* member, int64_t R, int64_t C, int64_t E, int64_t M, double* out_p, int32_t* out_n,
                     void* stream)
{
    int64_t chunks = 0;
    if (int rc = group_sizes(__func__, R, C, E, M, &chunks)) return rc;
    if (R * M * E == 0) return DIG_OK;
    DIG_REQUIRE(out_p && (C == 0 || (p && member)), "non-null p, member, out_p");
    GroupArgs a{};
    a.x = p, a.member = member, a.out = out_p, a.out_n = out_n;
    return group_launch(group_fisher_kernel<8>, group_fisher_kernel<32>, a, R, C, E, M, chunks, stream);
}

int dig_group_sums(const double* x, const double* gate, const uint8_t* member, int64_t R, int64_t C, int64_t E, int64_t M, double* out,
                   void* stream)
{
    int64_t chunks = 0;
    if (int rc = group_sizes(__func__, R, C, E, M, &chunks)) return rc;
    if (R * M * E == 0) return DIG_OK;
    DIG_REQUIRE(out && (C == 0 || (x && member)), "non-null x, member, out");
    GroupArgs a{};
    a.x = x, a.gate = gate, a.member = member, a.out = out;
    return group_launch(group_sums_kernel<8>, group_sums_kernel<32>, a, R, C, E, M, chunks, stream);
}

}  // extern "C"
